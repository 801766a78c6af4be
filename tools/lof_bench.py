"""LOFOutlierErrorDetector on one continuous column: the code-space evaluation on the device -- `Table.count_codes` on the resident
column plus `HipEngine.lof_codes` (rgbm_lof_1d, csrc/rgbm_lof.hip), wall clock with the upload of the dictionary and the copy of the
scores and flag words included -- against scikit-learn's `LocalOutlierFactor(novelty=False).fit_predict` on the same column in value
space, which is what the value-space detector (repair/errors.py) runs.  Two tie-free columns of normal doubles:

  * N = 1M rows, D = 1M distinct values;
  * N = 10M rows, D = 2.5M distinct values (every value drawn once, the other rows uniformly among them).

The flagged rows of the two are compared before any time is reported.  `--sklearn-max-rows`: columns above it are not given to
scikit-learn (the figure is then reported as not measured).

    python tools/lof_bench.py [--reps 3] [--sklearn-max-rows 10000000] [--out profiles/lof_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N                                                   # noqa: E402
from repair.engine import HipEngine                                               # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def column(n, d, seed):
    """(values [d] ascending, codes int32 [n]): every code occurs."""
    rng = np.random.default_rng(seed)
    values = np.unique(rng.normal(size=d + d // 100 + 16))[:d]
    assert len(values) == d
    codes = np.concatenate([np.arange(d), rng.integers(0, d, n - d)]).astype(np.int32)
    rng.shuffle(codes)
    return values, codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000000:1000000,10000000:2500000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--sklearn-max-rows", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = HipEngine(0)
    res = dict(k=a.k, columns=[])
    for shape in a.shapes.split(","):
        n, d = (int(x) for x in shape.split(":"))
        values, codes = column(n, d, seed=n % 1000 + 3)
        tab = N.Table(codes.reshape(1, n), [d])

        def device():
            counts = tab.count_codes(0)[0]
            return eng.lof_codes(values, counts, a.k)
        best, med, (score, bad, n_ties, n_near) = timed(device, a.reps)
        cb, _, _ = timed(lambda: tab.count_codes(0), a.reps)
        col = dict(rows=n, distinct=d, device_ms_best=best * 1e3, device_ms_median=med * 1e3, count_codes_ms_best=cb * 1e3,
                   n_ties=n_ties, n_near=n_near, codes_flagged=int(bad.sum()), rows_flagged=int(bad[codes].sum()))
        if n <= a.sklearn_max_rows:
            from sklearn.neighbors import LocalOutlierFactor
            x = values[codes].reshape(-1, 1)
            est = LocalOutlierFactor(n_neighbors=a.k, novelty=False)
            t = time.perf_counter()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                pred = est.fit_predict(x)
            sk = time.perf_counter() - t
            ref = -est.negative_outlier_factor_
            col.update(sklearn_ms=sk * 1e3, sklearn_runs=1, speedup_vs_sklearn=sk / best, flags_equal=bool(np.array_equal(pred < 0, bad[codes])),
                       max_relative_deviation=float(np.max(np.abs(score[codes] - ref) / np.abs(ref))))
            assert col["flags_equal"] or n_ties + n_near > 0, "flags differ on a column the lowering would accept"
        else:
            col.update(sklearn_ms=None, note="scikit-learn not measured at this size")
        res["columns"].append(col)
        print(json.dumps(col), flush=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
