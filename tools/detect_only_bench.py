"""Error detection alone on a resident 10M x 16 synthetic table (repair/synth.py): the detectors' cells merged on the host against the
table's cell set (csrc/rgbm_cellset.hip) -- the same build, the same table, the same run.

Detectors: the NULL detector over all 16 attributes, one `X -> Y` constraint and one order constraint by sort and scan.

  * host   `pipeline.detect_error_cells(on_device=False)` -- every detector's cells fetched, `np.unique` over int64 keys on the host --
           followed by `Table.read_cells` of the merged cells (uploaded again) for their current codes;
  * device `pipeline.detect_error_cells(on_device=True)`: every detector followed by `Table.cellset_add`, one `Table.cellset_emit`.

Wall clock of the whole call, best / median of `--reps` rounds after a warm-up call each, the two routes taking turns; the two cell lists
and code lists are compared.

Then the OR pass alone (`Table.cellset_add`, launch to synchronise) on sorted results -- every cell of one column (10M cells), then of all
16 columns (160M) -- with the in-wave combine (RGBM_CELLSET_COMBINE unset) and without it (=0: one atomic per lane), taking turns, the set
zeroed again before every timed call.

    python tools/detect_only_bench.py [--rows 10000000] [--reps 3] [--out profiles/FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N                                   # noqa: E402
from repair.pipeline import detect_error_cells                    # noqa: E402
from repair.synth import make_table_parallel                      # noqa: E402


def alternating(fns, reps, before=None):
    """{name: (best, median, last result)} of the callables, warmed up once each and then timed in turn, `reps` rounds (the spread of a shared
    host falls on all of them alike); `before` runs ahead of every timed call, outside the clock."""
    for fn in fns.values():
        if before is not None:
            before()
        fn()
    ts, out = {k: [] for k in fns}, {}
    for _ in range(reps):
        for k, fn in fns.items():
            if before is not None:
                before()
            t = time.perf_counter(); out[k] = fn(); ts[k].append(time.perf_counter() - t)
    return {k: (min(v), float(np.median(v)), out[k]) for k, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, 16
    codes, _, n_codes = make_table_parallel(n, c, seed=3, null_ratio=0.01)
    tab = N.Table(codes, n_codes)
    targets = list(range(c))
    fd = ([4, 8, 9], 10)                                                                     # X -> Y: the 10 % noise breaks it in most groups
    order = dict(kind="dc_scan", preds=[("EQ", 5, 5, None, None), ("EQ", 11, 11, None, None), ("EQ", 12, 12, None, None),
                                        ("GT", 6, 6, None, None), ("LT", 7, 7, None, None)], refs=[5, 6, 7])
    cons = [fd, order]

    def host():
        rows, cols = detect_error_cells(tab, targets, cons, True)
        return rows, cols, tab.read_cells(rows, cols)

    def device():
        return detect_error_cells(tab, targets, cons, True, on_device=True)

    parts = dict(nulls=len(tab.detect_nulls(targets)[0]), fd=len(tab.detect_constraint(fd[0], fd[1], cell_cols=[4, 8, 9, 10])[0]),
                 order=len(tab.detect_dc_scan(order["preds"], cell_cols=[5, 6, 7])[0]))
    r = alternating(dict(host=host, device=device), a.reps)
    (hb, hm, hres), (db, dm, dres) = r["host"], r["device"]
    assert all(np.array_equal(x, y) for x, y in zip(hres, dres)), "the two routes differ"
    res = dict(rows=n, columns=c, detector_cells=parts, merged_cells=int(len(hres[0])), host_ms_best=hb * 1e3, host_ms_median=hm * 1e3,
               device_ms_best=db * 1e3, device_ms_median=dm * 1e3, host_over_device=hb / db)
    del hres, dres, r

    # the OR pass alone, launch to synchronise, on sorted results: every cell of column 0 (10M cells), then of all 16 columns
    big = 2 ** 31 - 1

    def add_with(env):
        def call():
            if env is None:
                os.environ.pop("RGBM_CELLSET_COMBINE", None)
            else:
                os.environ["RGBM_CELLSET_COMBINE"] = env
            tab.cellset_add()
        return call

    for label, cols in (("1_column", [0]), ("16_columns", targets)):
        k = len(cols)

        def reopen():
            tab.cellset_open(cols)
            assert tab.detect_cells(cols, [1] * k, [big] * k, [big] * k, None, fetch=False) == n * k
        r = alternating(dict(combine=add_with(None), no_combine=add_with("0")), max(a.reps, 10), before=reopen)
        assert tab.cellset_emit(fetch=False).tolist() == [n] * k
        res["or_pass_" + label] = dict(cells=n * k, combine_ms_best=r["combine"][0] * 1e3, combine_ms_median=r["combine"][1] * 1e3,
                                       no_combine_ms_best=r["no_combine"][0] * 1e3, no_combine_ms_median=r["no_combine"][1] * 1e3)
    os.environ.pop("RGBM_CELLSET_COMBINE", None)
    tab.cellset_close()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
