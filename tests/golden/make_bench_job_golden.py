#!/usr/bin/env python3
"""Generates tests/golden/bench_job_digests.json: the CPU oracle's model of the BENCHMARKED job, pinned past iteration 2.

VERDICT r3 ("What's weak" 2): the 10M x 16 job of bench.py was compared with the oracle for two boosting iterations only, while an
intermediate build had once produced a second K = 64 model that was identical up to iteration 43 and different from 44 on.  This script
trains the oracle (OpenMP, bit-identical for any thread count) on the targets bench.py trains -- the K = 64 target c10 and the binary
target c0 of BASELINE configs[2] (make_table(10_000_000, 16, seed=42), the reference's fixed parameters, python/repair/train.py:102-131,
+ LightGBM defaults) -- for `--iters` iterations and stores one md5 per boosting iteration (tests/numerics_bound.py::iteration_digests).
tests/test_gpu_bench_shapes.py trains the same targets on the HIP engine WITH FIVE OTHER TARGETS IN FLIGHT (the bench's schedule) and
compares every iteration; tools/job_determinism.py repeats that across processes.

    python tests/golden/make_bench_job_golden.py [--iters 60] [--threads 8] [--targets 10,0]

Takes about an hour of host time for the K = 64 target on 8 cores (64 class trees x 10M rows per iteration).  Needs no reference files.

The other files of tests/golden/bench_*_digests.json come from the same script (tests/bench_golden_expect.py lists what each must hold;
an existing file's other targets are kept when table, --iters and the numerics version match):
    bench_shard_digests.json      --rows 12500000 --cols 32 --seed 43 --targets 0,7 --iters 30 --out bench_shard_digests.json
    bench_whole_digests.json      --rows 100000000 --cols 32 --seed 43 --parallel --targets 0,1 --iters 5 --out bench_whole_digests.json
    bench_big_index_digests.json  --rows 35000000 --cols 32 --seed 43 --targets 10 --iters 2 --out bench_big_index_digests.json
                                  (K x n_train = 2.22e9 > 2^31; the oracle holds 24 bytes per (row, class): 60 GB of peak memory)
Every entry records the host time, the thread count and the peak resident memory of the run that made it.
"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle import oracle as O  # noqa: E402
from repair.synth import balanced_weights, make_table  # noqa: E402
from tests.numerics_bound import iteration_digests  # noqa: E402

NUMERICS_VERSION = 220     # rgbm_version() of the library the digests pin (numerics v2.2: a fixed-point grid per class tree and iteration)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_job_digests.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--threads", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--targets", default="10,0")
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--iters-for", default="", help="per-target iteration counts that override --iters, e.g. 0:300,11:300 (the cheap targets pinned end to end)")
    ap.add_argument("--parallel", action="store_true", help="draw the table with make_table_parallel (the chunked generator bench.py uses for --config 100m32: "
                                                            "the WHOLE-table pin of configs[3] is made with --rows 100000000 --cols 32 --seed 43 --parallel --out bench_whole_digests.json)")
    ap.add_argument("--out", default=OUT, help="bench_job_digests.json (10M x 16) or bench_shard_digests.json (--rows 12500000 --cols 32 --seed 43)")
    a = ap.parse_args()
    OUT_ = a.out if os.path.isabs(a.out) else os.path.join(os.path.dirname(os.path.abspath(__file__)), a.out)
    if a.parallel:
        from repair.synth import make_table_parallel
        dirty, _, cards = make_table_parallel(a.rows, a.cols, seed=a.seed, threads=max(1, a.threads))
    else:
        dirty, clean, cards = make_table(a.rows, a.cols, seed=a.seed)
        del clean
    doc = {"table": dict({"rows": a.rows, "cols": a.cols, "seed": a.seed, "null_ratio": 0.01}, **({"generator": "make_table_parallel"} if a.parallel else {})), "iters": a.iters,
           "numerics_version": NUMERICS_VERSION, "generator": "tests/golden/make_bench_job_golden.py", "targets": {}}
    if os.path.exists(OUT_):
        old = json.load(open(OUT_))
        if old.get("table") == doc["table"] and old.get("iters") == a.iters and old.get("numerics_version") == NUMERICS_VERSION:
            doc["targets"] = old["targets"]
    O.lib().orc_set_threads(a.threads)
    iters_for = {int(x.split(":")[0]): int(x.split(":")[1]) for x in a.iters_for.split(",") if x}
    for t in [int(x) for x in a.targets.split(",")]:
        feats = [c for c in range(a.cols) if c != t]
        K = int(cards[t])
        rows = dirty[t] >= 0
        cw = balanced_weights(dirty[t], K)
        n_it = iters_for.get(t, a.iters)      # (a target's own count: the test trains it for len(digests) iterations)
        kw = dict(objective=0 if K == 2 else 1, num_class=max(K, 2), n_estimators=n_it)
        t0 = time.time()
        X = np.empty((len(feats), int(rows.sum())), np.int32)          # (column by column: a fancy-indexed copy of a 100M-row table would hold it twice)
        for j, f in enumerate(feats):
            X[j] = dirty[f][rows]
        blob = O.train(X, cards[feats], dirty[t][rows], K, class_weight=cw, **kw).save()
        del X
        doc["targets"]["c%d" % t] = {"K": K, "train_rows": int(rows.sum()), "digests": iteration_digests(blob),
                                      "oracle_seconds": round(time.time() - t0, 1), "threads": a.threads,
                                      "peak_rss_gb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2.0 ** 20, 1)}   # (of the process so far: table + oracle state)
        with open(OUT_, "w") as f:
            json.dump(doc, f, indent=1)
        print("c%d (K=%d): %d iterations in %.0f s" % (t, K, n_it, time.time() - t0), flush=True)


if __name__ == "__main__":
    main()
