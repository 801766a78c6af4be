"""Phases 1 and 2 of a resident REPAIR run -- detect, prune the weak labels, NULL the error cells, find the dirty rows -- on a 10M x 16
synthetic table (repair/synth.py), on the host route against the table's cell set (csrc/rgbm_cellset.hip): the same build, the
same table, the same run.

Detectors (those of tools/detect_only_bench.py): the NULL detector over all 16 attributes, one `X -> Y` constraint and one order constraint
by sort and scan; the cell-domain analysis is on, so the weak-labelled cells are pruned before the null-out (`error.*` defaults but for
`error.max_attrs_to_compute_pairwise_stats` = 16 and `error.domain_threshold_beta` = 0.5: see `main`).

  * host   `pipeline._detect_and_prune` + `pipeline._null_and_merge`: every detector's cells fetched and merged with `np.unique`, the weak
           flags of `Table.cell_domains` fetched per target, then `Table.read_cells`, `Table.null_cells` and `Table.rows_of_cells`, each with
           the cells uploaded again;
  * set    `pipeline._cells_on_set`: every detector followed by `Table.cellset_add`, one `Table.cellset_drop_weak` per target, one fetching
           `Table.cellset_emit`, `Table.cellset_null`, `Table.cellset_rows`.

Wall clock of the whole of both phases, best / median of `--reps` rounds after a warm-up call each, the two routes taking turns.  Both routes
NULL their cells: ahead of every call, outside the clock, the cells of the call before are written back (`Table.write_cells`) and the whole
table is compared with the original once at the end.  The two routes' cells, currents, dirty rows, pruned-cell lists and domain summaries
are compared for equality inside the run.

    python tools/cellrun_bench.py [--rows 10000000] [--reps 5] [--out profiles/FILE.json]
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
from repair import pipeline as P                                  # noqa: E402
from repair.synth import make_table_parallel                      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
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
    # the table's uniform noise fills every cell of every joint table: the reference's candidate filter (non-empty cells / all cells < 0.05, applied
    # when an attribute has more than `max_attrs_to_compute_pairwise_stats` = 3 candidates) would leave no correlated attribute and nothing
    # would be pruned.  With 16 candidates allowed the filter does not apply and the two attributes of least conditional entropy are used.
    options = {"error.max_attrs_to_compute_pairwise_stats": 16, "error.domain_threshold_beta": 0.5}
    analysis = dict(options=options, discrete_thres=int(max(n_codes)) + 1, domain_stats=[int(v) for v in n_codes], continuous={})
    nulled = [None]                                                                           # what the call before left NULL

    def restore():
        if nulled[0] is not None:
            tab.write_cells(*nulled[0])
            nulled[0] = None

    def host():
        det_rows, det_cols, kept, info, _, _ = P._detect_and_prune(tab, targets, cons, True, None, False, analysis, None, None)
        rows, cols, current, _, dirty = P._null_and_merge(None, tab, kept, det_rows, det_cols, None)
        return rows, cols, current, dirty, info

    def on_set():
        res = P._cells_on_set(None, tab, targets, cons, True, None, False, analysis, None, None, None)
        return res[6], res[7], res[8], res[10], res[3]

    fns, ts, out = dict(host=host, set=on_set), dict(host=[], set=[]), {}
    assert P.set_route_refusal(tab, targets) is None
    for rep in range(a.reps + 1):                                                             # round 0 warms up
        for k, fn in fns.items():
            restore()
            t = time.perf_counter(); out[k] = fn(); dt = time.perf_counter() - t
            nulled[0] = out[k][:3]
            if rep:
                ts[k].append(dt)
    restore()
    h, s = out["host"], out["set"]
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(h[:4], s[:4])), "the two routes differ"
    assert h[4] == s[4], "the two routes' domain summaries differ"
    assert all(np.array_equal(tab.read_column(j), codes[j]) for j in range(c)), "the table was not restored"
    res = dict(rows=n, columns=c, reps=a.reps, noisy_cells=int(h[4]["noisy_cells"]), weak_cells=int(h[4]["weak_cells"]), error_cells=int(len(h[0])),
               dirty_rows=int(len(h[3])), routes_equal=True,
               host_ms_best=min(ts["host"]) * 1e3, host_ms_median=float(np.median(ts["host"])) * 1e3,
               set_ms_best=min(ts["set"]) * 1e3, set_ms_median=float(np.median(ts["set"])) * 1e3,
               host_over_set_best=min(ts["host"]) / min(ts["set"]), host_over_set_median=float(np.median(ts["host"]) / np.median(ts["set"])))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
