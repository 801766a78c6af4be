"""Column statistics of a resident table: ONE call of `Table.column_stats` (rgbm_table_column_stats, csrc/rgbm_colstats.hip: the per-code
counts stay on the device) against one call of `Table.count_codes` per column (rgbm_table_count_codes: the counts of every column come to
the host, n_codes x 8 B each), which is what a caller had before the entry existed.  Wall clock around calls that end in a stream
synchronise, result copies included; the two are timed alternately in the same process, best and median of `--reps` after a warm-up.
`column_stats` is timed with a length LUT per column (as `describe` calls it for string columns: n_codes x 4 B go to the device), without any,
and column by column without any, next to the `count_codes` call of the same column.
The device result is compared with the statement (`repair.table_stats.column_stats`) before any time is reported; the time numpy would
then need to reduce the fetched counts to the same numbers is NOT part of the `count_codes` figure.

    python tools/column_stats_bench.py [--rows 10000000] [--codes 2,8,64,1000,8192,8193,100000,0] [--reps 5] [--bins 8] [--out profiles/column_stats_bench.json]

A code count of 0 stands for a row-id-like column: as many codes as rows, each held once."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N                                                   # noqa: E402
from repair import table_stats as T                                               # noqa: E402


def make_table(n, n_codes, seed=1, null=0.02):
    rng = np.random.default_rng(seed)
    codes = np.empty((len(n_codes), n), np.int32)
    for j, d in enumerate(n_codes):
        codes[j] = rng.permutation(n).astype(np.int32) if d == n else rng.integers(0, d, n, dtype=np.int32)
        codes[j][rng.random(n) < null] = -1
    return codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--codes", default="2,8,64,1000,8192,8193,100000,0")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bins", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n_codes = [int(x) or a.rows for x in a.codes.split(",")]
    cols = list(range(len(n_codes)))
    codes = make_table(a.rows, n_codes)
    rng = np.random.default_rng(2)
    luts = [rng.integers(0, 30, d).astype(np.int32) for d in n_codes]
    tab = N.Table(codes, n_codes)

    def one_call():
        return tab.column_stats(cols, len_luts=luts, n_bins=a.bins)

    def per_column():
        return [tab.count_codes(c) for c in cols]

    got, counts = one_call(), per_column()                    # warm-up of both, and the check
    want = T.column_stats(codes, n_codes, cols, len_luts=luts, n_bins=a.bins)
    for f in T.FIELDS + ("edges",):
        assert np.array_equal(got[f], want[f]), "column_stats differs from its statement in %s" % f
    for c in cols:
        ok = codes[c] >= 0
        assert np.array_equal(counts[c][0], np.bincount(codes[c][ok], minlength=n_codes[c])) and counts[c][1] == int((~ok).sum())
    for c in cols:
        tab.column_stats([c], n_bins=a.bins)                  # (warm-up of the single-column shape)
    t_one, t_bare, t_per, t_each, t_each_cs = [], [], [], np.zeros((a.reps, len(cols))), np.zeros((a.reps, len(cols)))
    for r in range(a.reps):                                   # alternating
        t = time.perf_counter(); one_call(); t_one.append(time.perf_counter() - t)
        t = time.perf_counter(); tab.column_stats(cols, n_bins=a.bins); t_bare.append(time.perf_counter() - t)
        for c in cols:
            t = time.perf_counter(); tab.column_stats([c], n_bins=a.bins); t_each_cs[r, c] = time.perf_counter() - t
        t0 = time.perf_counter()
        for c in cols:
            t = time.perf_counter(); tab.count_codes(c); t_each[r, c] = time.perf_counter() - t
        t_per.append(time.perf_counter() - t0)
    res = dict(rows=a.rows, n_codes=n_codes, n_bins=a.bins, reps=a.reps, length_luts=True,
               column_stats_one_call_ms=dict(best=min(t_one) * 1e3, median=float(np.median(t_one)) * 1e3),
               column_stats_one_call_without_luts_ms=dict(best=min(t_bare) * 1e3, median=float(np.median(t_bare)) * 1e3,
                                                          best_of_each_column_alone=[float(x) * 1e3 for x in t_each_cs.min(axis=0)]),
               count_codes_per_column_ms=dict(best=min(t_per) * 1e3, median=float(np.median(t_per)) * 1e3,
                                              best_of_each_column=[float(x) * 1e3 for x in t_each.min(axis=0)]),
               bytes_to_host=dict(column_stats=len(cols) * (6 * 8 + (a.bins + 1) * 4), count_codes=int(sum(n_codes)) * 8 + 8 * len(cols)),
               stream_floor_ms=a.rows * len(cols) * 4 / 6.29e12 * 1e3,
               note="wall clock, host side included; no kernel trace was taken")
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
