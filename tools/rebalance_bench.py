"""`Table.smoten` (rgbm_table_smoten, csrc/rgbm_smoten.hip) against the host loop it restates (`repair.train.smoten_resample`) at the
class sizes of the reference's default 10 000-row sample: one grown class of m = 2 000 / 5 000 / 10 000 rows beside 15 other classes
(K = 16), F = 15 features of 8 codes each, 1 000 new rows.

  device_ms   wall-clock of the whole `Table.smoten` call on a table that is resident already -- gather, counts, P, pair tables, the
              all-pairs neighbour search, merge, emit and the final synchronise (the call returns after it) -- best and median of `--reps`
              after a warm-up call;  knn_pair_features_per_second = m^2 x F / device_ms_best (the whole call, not the kernel alone)
  host_ms     one `smoten_resample` call on the same rows as a pandas frame (one repetition: it takes seconds to minutes)
The synthetic rows of both are compared first; a difference ends the run.

    python tools/rebalance_bench.py [--sizes 2000,5000,10000] [--reps 5] [--out profiles/FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N                                   # noqa: E402
from repair.train import smoten_resample                          # noqa: E402

F, V, K, OTHERS, N_NEW = 15, 8, 16, 200, 1000


def table(m, seed):
    rng = np.random.default_rng(seed)
    y = rng.permutation(np.concatenate([np.zeros(m, np.int64), np.repeat(np.arange(1, K), OTHERS)]))
    cols = []
    for _ in range(F):
        shift, noise = rng.integers(0, V, K), rng.integers(0, V, len(y))
        cols.append(np.where(rng.random(len(y)) < 0.5, (shift[y] + noise % 2) % V, noise))
    return np.asarray(cols + [y], np.int32), np.asarray([V] * F + [K], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000,5000,10000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("rebalance_bench: no HIP device")
    res = dict(features=F, codes_per_feature=V, classes=K, new_rows=N_NEW, k=5)
    for m in [int(s) for s in a.sizes.split(",")]:
        codes, n_codes = table(m, m)
        n = codes.shape[1]
        picks = np.random.RandomState(42).choice(np.arange(m), size=N_NEW, replace=True)
        tab = N.Table(codes, n_codes)
        call = lambda: tab.smoten(F, list(range(F)), np.arange(n), [0], [0, N_NEW], picks, k=5)     # noqa: E731
        got = call()
        synth = np.stack([got.read_column(j) for j in range(F + 1)]).T
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter(); call().close(); ts.append(time.perf_counter() - t)
        X = pd.DataFrame({"f%02d" % j: codes[j].astype(object) for j in range(F)})
        t = time.perf_counter()
        Xn, yn = smoten_resample(X, pd.Series(codes[F], name="t"), {0: m + N_NEW}, k_neighbors=5, random_state=42)
        host = time.perf_counter() - t
        same = bool((Xn.iloc[n:].to_numpy().astype(np.int64) == synth[:, :F]).all() and (yn.iloc[n:].to_numpy() == synth[:, F]).all())
        r = dict(fit_rows=n, device_ms_best=1e3 * min(ts), device_ms_median=1e3 * float(np.median(ts)), host_ms=1e3 * host,
                 host_over_device=host / min(ts), knn_pair_features_per_second=float(m) * m * F / min(ts), same_rows=same)
        res["m_%d" % m] = r
        print("m = %d: %s" % (m, json.dumps(r)), flush=True)
        if not same:
            raise SystemExit("rebalance_bench: the device rows differ from smoten_resample's at m = %d" % m)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
