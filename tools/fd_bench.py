"""`Table.fd_measures` and `RepairMisc.discoverFunctionalDeps` on the bench table shape (synthetic 10M rows x 16 columns, 1 % NULLs), against
yardsticks measured in the same process on the same host:

  * the numpy statement `repair.fd_codes.fd_measures` (the reference here, timed once per case: it takes seconds),
  * for single-column left-hand sides, the way that existed before the entry: one `Table.pair_counts` call for the pairs (x, y) plus the
    host reduction of its dense joint tables to the same four integers.

Left-hand sides of 1, 2 and 3 columns with 1 and 15 right-hand sides on each route; the hash route is reached on the same codes by
declaring the dictionary of the first left-hand column 8192 codes wide (a table's n_codes are only numbers).  Wall-clock per call (upload
of the lists and the copy of the result included), warm: median, min and max of `--reps` calls after one warm-up call.  Every device
result is compared with the statement before any time is reported.

    python tools/fd_bench.py [--rows 10000000] [--cols 16] [--reps 7] [--no-discover] [--out profiles/FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N          # noqa: E402
from repair import fd_codes              # noqa: E402
from repair.synth import make_table      # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return dict(ms_median=float(np.median(ts)) * 1e3, ms_min=min(ts) * 1e3, ms_max=max(ts) * 1e3, reps=reps), out


def same(a, b):
    return int(a["groups"]) == int(b["groups"]) and all(np.array_equal(a[f], b[f]) for f in ("kept", "violating", "xy_groups"))


def reduce_pair_counts(dense):
    """The four integers from the dense joint tables [x + NULL][y + NULL] of `Table.pair_counts`."""
    kept, viol, xy = [], [], []
    for d in dense:
        size, distinct = d.sum(axis=1), (d > 0).sum(axis=1)
        kept.append(int(d.max(axis=1).sum())); viol.append(int(size[distinct >= 2].sum())); xy.append(int(distinct.sum()))
    return dict(groups=np.int64(int((dense[0].sum(axis=1) > 0).sum())), kept=np.asarray(kept, np.int64), violating=np.asarray(viol, np.int64),
                xy_groups=np.asarray(xy, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-discover", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    codes, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    wide = cards.copy(); wide[0] = max(int(wide[0]), 8192)
    tabs = {"lds": (N.Table(codes, cards), cards), "hash": (N.Table(codes, wide), wide)}
    res = dict(rows=n, cols=c, n_codes=[int(v) for v in cards], limits=N.fd_measures_limits(), cases=[])
    for n_lhs in (1, 2, 3):
        lhs = list(range(n_lhs))
        rest = [j for j in range(c) if j not in lhs]
        for rhs in (rest[-1:], rest[-15:] if len(rest) >= 15 else rest):
            t = time.perf_counter(); want = fd_codes.fd_measures(codes, cards, lhs, rhs); host_ms = (time.perf_counter() - t) * 1e3
            case = dict(n_lhs=n_lhs, n_rhs=len(rhs), statement_ms=host_ms)
            for route, (tab, n_codes) in tabs.items():
                tm, got = timed(lambda: tab.fd_measures(lhs, rhs), a.reps)
                routes = tab.fd_measures_report()["routes"]
                assert same(got, want), (route, lhs, rhs)             # (every code lies inside the narrower dictionaries: one statement for both)
                case[route] = dict(tm, routes=routes, speedup_on_statement=host_ms / tm["ms_median"])
            if n_lhs == 1:                 # the way before the entry: dense pair counts on the device, reduced on the host
                tab = tabs["lds"][0]
                tm, got = timed(lambda: reduce_pair_counts(tab.pair_counts([(lhs[0], y) for y in rhs])), a.reps)
                assert same(got, want), (lhs, rhs)
                case["pair_counts_plus_host_reduction"] = tm
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
    if not a.no_discover:
        import pandas as pd
        from repair.api import Delphi
        from repair.misc import RepairMisc
        from repair.engine import HipEngine
        df = pd.DataFrame({"c%d" % j: np.where(codes[j] >= 0, codes[j], np.nan) for j in range(c)})

        class Counting:
            def __init__(self):
                self.engine, self.calls, self.seconds = HipEngine(0), 0, 0.0

            def upload_dictionaries(self, indices, remaps):
                return self.engine.upload_dictionaries(indices, remaps)

            def fd_measures(self, table, lhs, rhs):
                t = time.perf_counter(); out = self.engine.fd_measures(table, lhs, rhs)
                self.calls += 1; self.seconds += time.perf_counter() - t
                return out

        Delphi.register_table("fd_bench", df)
        runs = []
        for _ in range(1 + min(a.reps, 5)):
            m = RepairMisc().options({"table_name": "fd_bench", "max_lhs_size": "2", "max_error": "0.0"})
            m._engine_override = eng = Counting()
            t = time.perf_counter(); out = m.discoverFunctionalDeps(); runs.append((time.perf_counter() - t, eng.calls, eng.seconds))
        warm = runs[1:]
        possible = c + c * (c - 1) // 2
        res["discover"] = dict(max_lhs_size=2, max_error="0.0", dependencies=len(out), measure_calls=warm[0][1], level0_calls=1,
                               possible_lhs=possible, lhs_left_out=possible - (warm[0][1] - 1),
                               end_to_end_ms_median=float(np.median([r[0] for r in warm])) * 1e3, end_to_end_ms_min=min(r[0] for r in warm) * 1e3,
                               end_to_end_ms_max=max(r[0] for r in warm) * 1e3, in_measure_calls_ms_median=float(np.median([r[2] for r in warm])) * 1e3,
                               reps=len(warm))
        print(json.dumps(res["discover"]), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
