"""The value detectors on the bench table shape (synthetic 10M rows x 16 columns, 1 % NULLs): `Table.detect_cells`
(rgbm_table_detect_cells, csrc/rgbm_prep.hip) on all columns --

  * `null_only`:      the synthetic table, an all-zero bitset per column (staged into LDS, tested for every cell) and NULLs as errors: the
                      cell list of `detect_nulls` itself, so the two calls differ by the predicate alone;
  * `bitset_lds_4k`:  2 % of the codes flagged on a table of 4096-code columns (64-word bitsets in LDS), NULLs are errors;
  * `bitset_lds_max`: the same with as many codes as the LDS stage takes (the bound of the source: the most staging per row tile);
  * `bitset_global`:  the same with 2^20-code columns (bitsets beyond the bound: read from global memory);
  * `range_only`:     a kept code range that leaves 2 % of the codes outside on the 2^20-code columns (the outlier detector on continuous
                      columns), no bitset, NULLs are errors;

each next to `Table.detect_nulls` on the same table and columns (it moves the same bytes), to the stream floor (rows x columns x 4 B
over the 6.29 TB/s copy ceiling DESIGN.md uses), and (unless --no-host) to the value-space detectors of repair/errors.py on
`--host-cols` columns of the same data as a frame (regex per row, `np.percentile` of the column), scaled to all columns.  The wall
clock of a call includes the copy of its cell list (12 B per cell): compare configurations with their `cells` in view.

Wall-clock per call (uploads of the predicates and the copy of the cell list included), best of `--reps` after a warm-up call.  Every
device result is compared with the numpy restatement (tests/detector_restatements.py) before any time is reported.

    python tools/detect_bench.py [--rows 10000000] [--cols 16] [--reps 5] [--host-cols 1] [--out profiles/FILE.json]
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

from repair import _native as N                                                   # noqa: E402
from repair import detect_codes as DC                                             # noqa: E402
from repair.errors import GaussianOutlierErrorDetector, RegExErrorDetector       # noqa: E402
from tests import detector_restatements as R                                     # noqa: E402
from tests.helpers import csrc_constant                                          # noqa: E402
from tests.synth import make_table                                                # noqa: E402

COPY_CEILING = 6.29e12                       # B/s, DESIGN.md
WIDE = 1 << 20                               # codes per column of the wide table


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def finish(res, out):
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-cols", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    rng = np.random.default_rng(3)
    dirty, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    wide = rng.integers(0, WIDE, (c, n), dtype=np.int32)
    wide[:, rng.random(n) < 0.01] = -1
    every = list(range(c))
    floor = n * c * 4 / COPY_CEILING
    res = dict(rows=n, cols=c, stream_floor_ms=floor * 1e3, lds_bound_codes=None)
    lds_max = csrc_constant("DET_LDS_WORDS") * 64
    res["lds_bound_codes"] = lds_max

    def narrowed(k):
        return np.where(wide >= 0, wide % k, -1).astype(np.int32)

    def flagged(k):
        return [DC.pack_bits(rng.random(k) < 0.02) for _ in range(c)]

    configs = {}
    configs["null_only"] = (lambda: dirty, cards, [1] * c, [0] * c, [-1] * c, [DC.pack_bits(np.zeros(int(k), bool)) for k in cards])
    configs["bitset_lds_4k"] = (lambda: narrowed(4096), [4096] * c, [1] * c, [0] * c, [-1] * c, flagged(4096))
    configs["bitset_lds_max"] = (lambda: narrowed(lds_max), [lds_max] * c, [1] * c, [0] * c, [-1] * c, flagged(lds_max))
    configs["bitset_global"] = (lambda: wide, [WIDE] * c, [1] * c, [0] * c, [-1] * c, flagged(WIDE))
    configs["range_only"] = (lambda: wide, [WIDE] * c, [1] * c, [WIDE // 100] * c, [WIDE - WIDE // 100 - 1] * c, None)
    for name, (make, n_codes, null, lo, hi, bits) in configs.items():
        codes = make()
        tab = N.Table(codes, n_codes)
        nb, nm, nul = timed(lambda: tab.detect_nulls(every), a.reps)
        nulls = dict(ms_best=nb * 1e3, ms_median=nm * 1e3, cells=int(len(nul[0])), ratio_to_stream_floor=nb / floor)
        best, med, got = timed(lambda: tab.detect_cells(every, null, lo, hi, bits), a.reps)
        want = R.detect_cells(codes, every, null, lo, hi, bits)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        if name == "null_only":
            assert np.array_equal(got[0], nul[0]) and np.array_equal(got[1], nul[1])
        res[name] = dict(n_codes_max=int(max(n_codes)), cells=int(len(got[0])), ms_best=best * 1e3, ms_median=med * 1e3, detect_nulls=nulls,
                         ratio_to_detect_nulls=best / nb, ratio_to_stream_floor=best / floor)
        del tab
    if a.no_host:
        return finish(res, a.out)
    # the value-space detectors on the same data as a frame: a string column for the regex, a float column for the fences
    k = max(1, min(a.host_cols, c))
    host = {}
    frame = pd.DataFrame({"tid": np.arange(n)})
    for j in range(k):
        v = dirty[j]
        frame["s%d" % j] = pd.Series(np.where(v >= 0, v, 0)).map(lambda x: "v%d" % x).where(v >= 0, None)
        w = wide[j].astype(np.float64)
        w[wide[j] < 0] = np.nan
        frame["x%d" % j] = w
    attrs = [cn for cn in frame.columns if cn != "tid"]
    t = time.perf_counter()
    for j in range(k):
        keep = "^v(%s)$" % "|".join(str(x) for x in range(1, int(cards[j])))          # every value but v0
        cells = RegExErrorDetector("s%d" % j, keep).setUp("tid", frame, [], attrs).detect()
        assert len(cells) == int((dirty[j] <= 0).sum())
    host["regex_ms_per_column"] = (time.perf_counter() - t) * 1e3 / k
    t = time.perf_counter()
    cells = GaussianOutlierErrorDetector().setUp("tid", frame, ["x%d" % j for j in range(k)], attrs).detect()
    host["outlier_ms_per_column"] = (time.perf_counter() - t) * 1e3 / k
    host["columns_measured"] = k
    host["regex_ms_all_columns"] = host["regex_ms_per_column"] * c
    host["outlier_ms_all_columns"] = host["outlier_ms_per_column"] * c
    res["value_space"] = host
    res["speedup_regex_vs_bitset_lds_4k"] = host["regex_ms_all_columns"] / res["bitset_lds_4k"]["ms_best"]
    res["speedup_outlier_vs_range_only"] = host["outlier_ms_all_columns"] / res["range_only"]["ms_best"]
    finish(res, a.out)


if __name__ == "__main__":
    main()
