"""`Table.detect_dc` (rgbm_table_detect_dc, csrc/rgbm_dc.hip) on synthetic tables in the three regimes of the pair kernel --

  * fd_like     n = 1M rows in groups of 3: millions of tiny groups, the cost is the grouping;
  * groups_1000 n = 1M rows in groups of ~1000: EQ + GT + LT, early exit at work;
  * one_group   n = 200k rows in ONE group and two predicates no pair satisfies (LT and GT of one attribute): every lane walks the whole
                group, the no-early-exit worst case; one_group_16 is the same on 100k rows with 15 pair predicates.  Their pairs per second
                size DC_DEFAULT_MAX_PAIRS and DC_LAUNCH_PAIRS.
  * groups_3_order       the 1M rows in groups of 3 with EQ + GT + LT: tiny groups, where the pairs route has next to nothing to do;
  * one_group_two_attrs  the 200k rows in one group with GT of one attribute and LT of another (early exit at work);
  * one_group_10m        n = 10M rows, no EQ predicate: ONE group of 10^14 pairs, which the pairs route refuses.

Every shape that is an order constraint (`repair.dc_codes.scan_eligible`) is answered by `Table.detect_dc_scan` (sort and scan, no pairs) as
well, on the same table in the same run, and the two row lists compared: `scan_ms_best` / `scan_ms_median` next to `ms_best` / `ms_median`.

`pairs` is the sum of |group|^2 (what `max_pairs` bounds); pairs per second = pairs / wall-clock of the whole call (grouping, pair launches,
compaction and the copy of the rows to the host), best of `--reps` after a warm-up call.  The device rows of a sample of groups are
compared with the numpy restatement (tests/dc_restatement.py) first.

Then the 20 000-row frame -- the largest `errors._violating_rows` accepts for such a constraint: the host loop against lowering +
device call on the same frame, same rows.

    python tools/dc_bench.py [--reps 3] [--out profiles/FILE.json]
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
from repair.dc_codes import lower_constraint, scan_eligible       # noqa: E402
from repair.errors import _violating_rows, parse_constraint       # noqa: E402
from repair.pipeline import encode_frame                          # noqa: E402
from tests import dc_restatement as R                             # noqa: E402
from tests.dc_scan_cases import scan_statement                    # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def shape(name, rng):
    if name == "fd_like":
        n = 1_000_000
        g = rng.permutation(np.arange(n) // 3)
        preds = [("EQ", 0, 0, None, None), ("IQ", 1, 1, None, None), ("IQ", 2, 2, None, None)]
    elif name == "groups_1000":
        n = 1_000_000
        g = rng.permutation(np.arange(n) // 1000)
        preds = [("EQ", 0, 0, None, None), ("GT", 1, 1, None, None), ("LT", 2, 2, None, None)]
    elif name == "groups_3_order":
        n = 1_000_000
        g = rng.permutation(np.arange(n) // 3)
        preds = [("EQ", 0, 0, None, None), ("GT", 1, 1, None, None), ("LT", 2, 2, None, None)]
    elif name == "one_group_two_attrs":
        n = 200_000
        g = np.zeros(n, np.int64)
        preds = [("EQ", 0, 0, None, None), ("GT", 1, 1, None, None), ("LT", 2, 2, None, None)]
    elif name == "one_group_10m":
        n = 10_000_000
        g = np.zeros(n, np.int64)
        preds = [("GT", 1, 1, None, None), ("LT", 2, 2, None, None)]
    elif name == "one_group":
        n = 200_000
        g = np.zeros(n, np.int64)
        preds = [("EQ", 0, 0, None, None), ("LT", 1, 1, None, None), ("GT", 1, 1, None, None)]
    else:                            # the same with 15 pair predicates, the most a call takes next to one EQ
        n = 100_000
        g = np.zeros(n, np.int64)
        preds = [("EQ", 0, 0, None, None)] + [("IQ", 1 + k % 2, 1 + k % 2, None, None) for k in range(13)] + [("LT", 1, 1, None, None), ("GT", 1, 1, None, None)]
    codes = np.stack([g, rng.integers(0, 1000, n), rng.integers(0, 1000, n)]).astype(np.int32)
    codes[1:][rng.random((2, n)) < 0.01] = -1
    return codes, [int(g.max()) + 1, 1000, 1000], preds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(7)
    res = {}
    for name in ("fd_like", "groups_1000", "one_group", "one_group_16", "groups_3_order", "one_group_two_attrs", "one_group_10m"):
        codes, n_codes, preds = shape(name, rng)
        n = codes.shape[1]
        tab = N.Table(codes, n_codes)
        pairs = int((np.bincount(codes[0]).astype(np.int64) ** 2).sum())
        if name == "one_group_10m":
            # the pairs route refuses it at its default bound; the scan route against the numpy statement of the tests
            try:
                tab.detect_dc(preds)
                raise AssertionError("the pairs route accepted 10^14 pairs")
            except N.RepairGbmError as e:
                assert e.code == -2
            best, med, rows = timed(lambda: tab.detect_dc_scan(preds), a.reps)
            assert np.array_equal(rows, scan_statement(codes, n_codes, preds))
            res[name] = dict(rows=n, groups=1, pairs=pairs, predicates=[p[0] for p in preds], violating_rows=int(len(rows)), pairs_route="refused (-2)",
                             scan_ms_best=best * 1e3, scan_ms_median=med * 1e3)
            continue
        best, med, rows = timed(lambda: tab.detect_dc(preds, max_pairs=pairs), a.reps)
        # the check: a sample of whole groups against the restatement
        mask = np.zeros(n, bool); mask[rows] = True
        pick = np.flatnonzero(np.isin(codes[0], rng.choice(n_codes[0], min(n_codes[0], 20), replace=False)))[:5000] if not name.startswith("one_group") else np.arange(0)
        if len(pick):
            sub = codes[:, pick]
            keep = np.isin(sub[0], [gid for gid, c in zip(*np.unique(sub[0], return_counts=True)) if c == (codes[0] == gid).sum()])
            sub, pick = sub[:, keep], pick[keep]
            assert np.array_equal(np.flatnonzero(mask[pick]), R.detect_dc(sub, n_codes, preds)), name
        elif name != "one_group_two_attrs":
            assert len(rows) == 0
        scan = {}
        if scan_eligible(preds):
            sbest, smed, srows = timed(lambda: tab.detect_dc_scan(preds), a.reps)
            assert np.array_equal(srows, rows), name
            scan = dict(scan_ms_best=sbest * 1e3, scan_ms_median=smed * 1e3, pairs_over_scan=best / sbest)
        res[name] = dict(scan, rows=n, groups=int(n_codes[0]), pairs=pairs, predicates=[p[0] for p in preds], violating_rows=int(len(rows)),
                         ms_best=best * 1e3, ms_median=med * 1e3, pairs_per_second=pairs / best)
    # the largest frame the host loop accepts
    n = 20000
    salary = rng.integers(20, 200, n).astype(np.float64) * 500
    tax = np.round(salary * 0.2)
    odd = rng.random(n) < 0.01
    tax[odd] = rng.integers(0, 40000, int(odd.sum()))
    df = pd.DataFrame({"State": np.array(["s%03d" % (i % 400) for i in range(n)], object), "Salary": salary, "Tax": tax})
    cols = list(df.columns)
    preds = parse_constraint("t1&t2&EQ(t1.State,t2.State)&GT(t1.Salary,t2.Salary)&LT(t1.Tax,t2.Tax)")
    t = time.perf_counter(); want = np.flatnonzero(_violating_rows(df, preds)); t_host = time.perf_counter() - t
    t = time.perf_counter()
    idx, remaps, dicts = encode_frame(df, cols)
    prog = lower_constraint(preds, cols, dicts, {c: df[c].dtype for c in cols})
    t_lower = time.perf_counter() - t
    tab = N.Table.from_dictionaries(idx, remaps)
    best, med, rows = timed(lambda: tab.detect_dc(prog["preds"]), a.reps)
    assert np.array_equal(rows, want)
    sbest, smed, srows = timed(lambda: tab.detect_dc_scan(prog["preds"]), a.reps)
    assert scan_eligible(prog["preds"]) and np.array_equal(srows, want)
    res["frame_20000"] = dict(scan_ms_best=sbest * 1e3, scan_ms_median=smed * 1e3, pairs_over_scan=best / sbest, rows=n, violating_rows=int(len(want)), host_violating_rows_ms=t_host * 1e3, encode_and_lower_ms=t_lower * 1e3,
                              device_ms_best=best * 1e3, device_ms_median=med * 1e3, host_over_device=t_host / best,
                              host_over_device_with_encoding=t_host / (best + t_lower))
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
