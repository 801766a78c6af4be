"""`Table.distinct_rows()` (rgbm_table_distinct_rows, csrc/rgbm_distinct.hip) on the bench table shape (synthetic 10M rows x 16 columns, 1 % NULLs)
against yardsticks measured in the same process --

  * the host statement `repair.pipeline.distinct_rows` (numpy.unique over mixed-radix keys) on the same code matrix;
  * the stream floor: rows x columns x 4 B (the table read once) over the 6.29 TB/s copy ceiling DESIGN.md uses.

The device result is first compared with the host's: the same (row, multiplicity) multiset, `distinct[:, inverse]` the table itself, the
groups in order of first occurrence.  Then wall-clock per call (the copy of `inverse` to the host included; a second timing leaves it
out), best of `--reps` after a warm-up call.

    python tools/distinct_bench.py [--rows 10000000] [--cols 16] [--reps 5] [--out profiles/FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N              # noqa: E402
from repair.pipeline import distinct_rows    # noqa: E402
from tests.synth import make_table           # noqa: E402

COPY_CEILING = 6.29e12                       # B/s, DESIGN.md


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    dirty, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    tab = N.Table(dirty, cards)
    t = time.perf_counter(); hd, hm, hi = distinct_rows(dirty, cards); t_host = time.perf_counter() - t
    # the check: the device table against the host's, up to the order of the groups (the host's come in key order)
    d, inv = tab.distinct_rows(want_inverse=True)
    dd = np.stack([d.read_column(j) for j in range(c)])
    dm = d.row_multiplicity()
    assert dd.shape == hd.shape, (dd.shape, hd.shape)
    assert np.array_equal(dd[:, inv], dirty) and int(dm.astype(np.int64).sum()) == n
    heads, first = np.unique(inv, return_index=True)             # first copies of the groups and their first rows, which ascend
    assert (np.diff(first) > 0).all() and np.array_equal(dd[:, heads], dirty[:, first])
    order_d = np.lexsort(np.vstack([dm[None].astype(np.int32), dd])[::-1])
    order_h = np.lexsort(np.vstack([hm[None].astype(np.int32), hd])[::-1])
    assert np.array_equal(dd[:, order_d], hd[:, order_h]) and np.array_equal(dm[order_d], hm[order_h])
    del dd, hd, d
    best, med, _ = timed(lambda: tab.distinct_rows(want_inverse=True)[0].close(), a.reps)
    best_ni, med_ni, _ = timed(lambda: tab.distinct_rows().close(), a.reps)
    floor = n * c * 4 / COPY_CEILING
    res = dict(rows=n, cols=c, distinct=int(len(hm)), groups=int(len(heads)), host_numpy_ms=t_host * 1e3,
               ms_best=best * 1e3, ms_median=med * 1e3, ms_best_without_inverse=best_ni * 1e3, ms_median_without_inverse=med_ni * 1e3,
               speedup_over_host=t_host / best, stream_floor_ms=floor * 1e3, ratio_to_stream_floor=best_ni / floor)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
