"""Cell-domain analysis on the bench table shape (synthetic 10M rows x 16 columns, 1 % NULLs, 16 targets -> 120 column pairs):
pair counting and cell domains on the device (csrc/rgbm_domain.hip) against two yardsticks measured in the same process --

  * the host path of repair/domain.py (sparse counting with numpy, the same cell-domain arithmetic), and
  * the stream floor: the bytes of the columns read ONCE (rows x columns x 4 B) over the 6.29 TB/s copy ceiling DESIGN.md uses.

Wall-clock per call (upload of the descriptors and the copy of the result included), best of `--reps` after a warm-up call; kernel-level
times come from running this under `rocprofv3 --kernel-trace --stats`.  The device and host results are compared before any time is reported.

    python tools/domain_bench.py [--rows 10000000] [--cols 16] [--reps 5] [--host-pairs 120] [--out profiles/FILE.json]
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
from repair import domain as D           # noqa: E402
from tests.synth import make_table       # noqa: E402

COPY_CEILING = 6.29e12                   # B/s, DESIGN.md


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
    ap.add_argument("--host-pairs", type=int, default=120, help="pairs the host yardstick counts (scaled to all pairs when fewer)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    dirty, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    tab = N.Table(dirty, cards)
    view = D.discretised_view(cards, cards, {}, 80)
    pairs = D.all_pairs(list(range(c)), view.cols)
    res = dict(rows=n, cols=c, pairs=len(pairs), dense_cells=int(sum((cards[x] + 1) * (cards[y] + 1) for x, y in pairs)))
    best, med, dense = timed(lambda: tab.pair_counts(pairs), a.reps)
    floor = n * c * 4 / COPY_CEILING
    res["pair_counts_device"] = dict(ms_best=best * 1e3, ms_median=med * 1e3, stream_floor_ms=floor * 1e3, ratio_to_stream_floor=best / floor)
    host = D.HostBackend(dirty, view)
    hp = pairs[:max(1, min(a.host_pairs, len(pairs)))]
    t = time.perf_counter(); hj = host.pair_counts(hp); th = time.perf_counter() - t
    for p, j, d in zip(hp, hj, dense):
        assert np.array_equal(j.dense(), d), p
    res["pair_counts_host"] = dict(ms=th * 1e3 * len(pairs) / len(hp), pairs_measured=len(hp), speedup=th * len(pairs) / len(hp) / best)
    # cell domains: the NULL-free 1 % sample of every target's cells, two correlated attributes each (the reference's default)
    ptab = D.PairTable(pairs, [D.Joint.from_dense(d) for d in dense])
    rng = np.random.default_rng(0)
    rows = np.sort(rng.choice(n, n // 100, replace=False)).astype(np.int64)
    td = thh = 0.0
    cells = 0
    for t_col in range(c):
        corr = [(t_col + 1) % c, (t_col + 5) % c]
        ok = ptab.single(t_col)[:int(cards[t_col])] > 0
        pidx = [ptab.index[frozenset((x, t_col))] for x in corr]
        b, _, dev = timed(lambda: tab.cell_domains(t_col, rows, pidx, [0, 0], ok, 0.7, n), a.reps)
        t0 = time.perf_counter(); hst = host.cell_domains(t_col, rows, corr, ptab, [0, 0], ok, 0.7, n); thh += time.perf_counter() - t0
        assert np.array_equal(dev[0], hst[0]) and np.array_equal(dev[1], hst[1]) and dev[2].tobytes() == hst[2].tobytes(), t_col
        td += b; cells += len(rows)
    res["cell_domains"] = dict(cells=cells, device_ms=td * 1e3, host_ms=thh * 1e3, speedup=thh / td)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
