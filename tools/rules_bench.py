"""Rule-based repairs on the bench table shape (synthetic 10M rows x 16 columns, 1 % NULLs): the three device entries of
csrc/rgbm_rules.hip (rgbm_table_fd_map, rgbm_table_rule_fill, rgbm_nearest_values) against yardsticks measured in the same process --

  * `fd_map`: pandas `RepairModel._build_rule_model` on the same two columns, and the stream floor: rows x 8 B (two int32 columns read
    once) over the 6.29 TB/s copy ceiling DESIGN.md uses;
  * `rule_fill`: the stream floor of its 12 B per row (x and y read, the labels written);
  * `nearest_values`: `--current` distinct current values against a `--domain`-value domain, against the host loop of
    `RepairModel._repair_by_nearest_values` (measured on `--host-values` of them and scaled).

Wall-clock per call (uploads and the copy of the result included), best of `--reps` after a warm-up call.  Every device result is compared
with the host's before any time is reported.

    python tools/rules_bench.py [--rows 10000000] [--cols 16] [--reps 5] [--current 100000] [--domain 1000] [--host-values 200] [--out profiles/FILE.json]
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

from repair import _native as N              # noqa: E402
from repair.costs import Levenshtein         # noqa: E402
from repair.model import RepairModel         # noqa: E402
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
    ap.add_argument("--current", type=int, default=100_000)
    ap.add_argument("--domain", type=int, default=1000)
    ap.add_argument("--host-values", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    dirty, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    tab = N.Table(dirty, cards)
    res = dict(rows=n, cols=c)
    # fd_map: the pair with the largest source domain, and a derived column that really depends on it
    x = int(np.argmax(cards))
    y = (x + 1) % c
    floor = n * 8 / COPY_CEILING
    out = {}
    for name, ycol in (("random_pair", dirty[y]), ("dependent_pair", np.where(dirty[x] >= 0, dirty[x] % int(cards[y]), -1).astype(np.int32))):
        codes = np.stack([dirty[x], ycol])
        t2 = N.Table(codes, [cards[x], cards[y]])
        best, med, got = timed(lambda: t2.fd_map(0, 1), a.reps)
        df = pd.DataFrame({"x": codes[0], "y": codes[1]}).astype("float64").where(lambda d: d >= 0)
        t = time.perf_counter(); fm = RepairModel()._build_rule_model(df, "x", "y").fd_map; th = time.perf_counter() - t
        want = np.array([int(fm.get(float(k), -1)) for k in range(int(cards[x]))], np.int32)
        assert np.array_equal(got, want), name
        out[name] = dict(n_codes_x=int(cards[x]), mapped=int((got >= 0).sum()), ms_best=best * 1e3, ms_median=med * 1e3, pandas_ms=th * 1e3,
                         speedup=th / best, stream_floor_ms=floor * 1e3, ratio_to_stream_floor=best / floor)
    res["fd_map"] = out
    # rule_fill over every row (a fresh table per call would time the upload: the fill is idempotent, so the same table is reused)
    lut = tab.fd_map(x, y)
    lut = np.where(lut >= 0, lut, np.arange(len(lut)) % int(cards[y])).astype(np.int32)
    want = dirty[y].copy()
    pred = np.where(dirty[x] >= 0, lut[np.maximum(dirty[x], 0)], -1)
    want = np.where((want < 0) & (pred >= 0), pred, want)
    best, med, lab = timed(lambda: tab.rule_fill(y, x, lut), a.reps)
    assert np.array_equal(lab, pred) and np.array_equal(tab.read_column(y), want)
    best_nl, _, _ = timed(lambda: tab.rule_fill(y, x, lut, want_labels=False), a.reps)
    res["rule_fill"] = dict(ms_best=best * 1e3, ms_median=med * 1e3, ms_best_without_labels=best_nl * 1e3, stream_floor_ms=n * 12 / COPY_CEILING * 1e3)
    # nearest values: 8-character words, the current values one or two edits away from a domain word
    rng = np.random.default_rng(1)
    abc = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    dom = sorted({"".join(w) for w in abc[rng.integers(0, 26, (a.domain * 2, 8))]})[:a.domain]
    cur = []
    for i in range(a.current):
        w = list(dom[int(rng.integers(0, len(dom)))])
        for _ in range(int(rng.integers(1, 3))):
            w[int(rng.integers(0, 8))] = abc[int(rng.integers(0, 26))]
        cur.append("".join(w) + ("%d" % i if i % 7 == 0 else ""))
    cur = list(dict.fromkeys(cur))
    best, med, near = timed(lambda: N.nearest_values(cur, dom, threshold=2.0), max(1, a.reps // 2))
    cf = Levenshtein()
    k = min(a.host_values, len(cur))
    t = time.perf_counter()
    for i in range(k):
        costs = sorted((cf.compute(cur[i], v), j) for j, v in enumerate(dom))
        w = costs[0][1] if costs[0][0] <= 2.0 and (len(costs) == 1 or costs[0][0] < costs[1][0]) else -1
        assert w == int(near[i]), i
    th = (time.perf_counter() - t) * len(cur) / k
    res["nearest_values"] = dict(current_values=len(cur), domain_values=len(dom), merged=int((near >= 0).sum()), ms_best=best * 1e3,
                                 ms_median=med * 1e3, host_loop_ms=th * 1e3, host_values_measured=k, speedup=th / best)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
