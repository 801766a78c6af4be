"""-m gpu: the BENCHMARKED shapes under the parity gate -- the HIP trainer against the CPU oracle, model bytes identical.

bench.py quotes its numbers on BASELINE configs[2] (10M rows x 16 columns) and, per GPU of the 8-GPU job, on a row shard of configs[3]
(100M x 32: 12.5M rows x 32 columns -> two 16-feature chunks, the two-chunk wave-specialised level pass).  The other parity tests stop
at 2.5M rows.  Exactly this is pinned here:

  whole models, oracle trained in the test (2 boosting iterations)
    10M x 16     c10 (K = 64), c0 (K = 2)
    12.5M x 32   c7 (K = 24)
  the oracle's per-iteration tree digests, committed under tests/golden/ (tests/golden/make_bench_job_golden.py; never from the HIP library)
    bench_job_digests.json        10M x 16     all 16 targets, 60 iterations each, c0 / c11 / c1 / c12 for all 300; six targets in flight
    bench_shard_digests.json      12.5M x 32   c0 (K = 2) and c7 (K = 24), 30 iterations, both in flight
    bench_whole_digests.json      100M x 32    c0 (K = 2) and c1 (K = 3), 5 iterations (the table of bench.py --config 100m32)
    bench_big_index_digests.json  35M x 32     c10 (K = 64), 2 iterations: K x n_train = 2.22e9, the only pin above 2^31 ELEMENTS

The largest K x n_train held to the oracle is that last one (2.22e9 > 2^31 = 2.15e9: every per-(row, class) buffer -- (g, h), scores, node
ids -- is indexed beyond 2^31, through k_grad_mc and the two-chunk level pass).  NOT pinned: a many-class target of the whole 100M x 32
table (c7 there is 2.4e9 elements on 100M-row class trees; the oracle would need about 105 GB), which stays on bench.py's models_md5.

tests/bench_golden_expect.py names the targets, K values and digest counts every file must hold; each digest test asserts them BEFORE it
trains (a missing target is a failure, never a skip), and tests/test_golden_manifest.py asserts the same without a GPU.
"""
import os

import numpy as np
import pytest

from tests import bench_golden_expect as E
from tests.synth import make_table, balanced_weights

pytestmark = pytest.mark.gpu


def _gold(name):
    """The committed oracle digests `name`, held to tests/bench_golden_expect.py (expected targets, K, digest counts, the library's numerics
    version) before anything trains.  Returns (parsed file, {target column: iterations to train})."""
    from repair import _native as N
    gold = E.load(name)
    return gold, E.check(name, gold, N.lib().rgbm_version())


def _compare(what, gold, blobs, counts):
    from tests.numerics_bound import iteration_digests
    assert set(blobs) == set(counts)
    for t, n in counts.items():
        g = gold["targets"]["c%d" % t]
        got = iteration_digests(blobs[t])
        assert len(got) == len(g["digests"]) == n, "%s, target c%d: %d iterations trained, %d digests" % (what, t, len(got), len(g["digests"]))
        bad = [i for i, (a, b) in enumerate(zip(got, g["digests"])) if a != b]
        assert not bad, "%s, target c%d (K=%d): iterations %s of %d differ from the oracle (first at %d)" % (what, t, g["K"], bad[:8], len(got), bad[0])


def _both(dirty, cards, target, iters):
    from oracle import oracle as O
    from repair import _native as N
    cols = dirty.shape[0]
    feats = [c for c in range(cols) if c != target]
    K = int(cards[target])
    cw = balanced_weights(dirty[target], K)
    kw = dict(objective=0 if K == 2 else 1, num_class=max(K, 2), n_estimators=iters)       # everything else: the reference's defaults
    mg = N.Table(dirty, cards).train(target, feats, class_weight=cw, **kw).save()           # resident-table path, rows with a NULL target skipped on the device
    rows = dirty[target] >= 0
    O.lib().orc_set_threads(min(32, os.cpu_count() or 1))
    try:
        mo = O.train(np.ascontiguousarray(dirty[feats][:, rows]), cards[feats], dirty[target][rows], K, class_weight=cw, **kw).save()
    finally:
        O.lib().orc_set_threads(1)
    return mg, mo


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("target", [10, 0])
def test_config2_shape_10m_x_16(target):
    dirty, clean, cards = make_table(10_000_000, 16, seed=42)
    del clean
    assert int(cards[target]) == (64 if target == 10 else 2)
    mg, mo = _both(dirty, cards, target, iters=2)
    assert mg == mo, "10M x 16, target c%d: HIP model differs from the oracle" % target


@pytest.mark.timeout(1800)
def test_config3_per_gpu_shape_12_5m_x_32():
    dirty, clean, cards = make_table(12_500_000, 32, seed=43)
    del clean
    target = 7
    assert int(cards[target]) == 24
    mg, mo = _both(dirty, cards, target, iters=2)
    assert mg == mo, "12.5M x 32 (two feature chunks), target c7: HIP model differs from the oracle"


def _train(tab, dirty, cards, gold, target, iters):
    """One target on the resident table with the reference's fixed parameters; the golden entry must describe THIS column."""
    g = gold["targets"]["c%d" % target]
    K = int(cards[target])
    assert g["K"] == K and g["train_rows"] == int(np.count_nonzero(dirty[target] >= 0)), "golden entry c%d is not of this table" % target
    feats = [c for c in range(dirty.shape[0]) if c != target]
    return tab.train(target, feats, class_weight=balanced_weights(dirty[target], K), objective=0 if K == 2 else 1, num_class=max(K, 2), n_estimators=iters).save()


@pytest.mark.timeout(1800)
def test_bench_job_60_iterations_with_six_targets_in_flight_match_the_oracle_digests():
    """engine.run_job's schedule: the six most expensive targets of the 10M x 16 job train concurrently (one HIP stream each, host
    threads); then the binary target next to five small ones.  Digest of EVERY boosting iteration == the committed oracle digests.
    Expected before training (tests/bench_golden_expect.py): all 16 targets, at least 60 digests each, 300 each for c0, c11, c1 and c12."""
    from concurrent.futures import ThreadPoolExecutor
    from repair import _native as N
    gold, counts = _gold("bench_job_digests.json")
    assert set(counts) == set(range(16)) and min(counts.values()) >= 60 and all(counts[t] == 300 for t in (0, 11, 1, 12))
    dirty, clean, cards = make_table(gold["table"]["rows"], gold["table"]["cols"], seed=gold["table"]["seed"])
    del clean
    tab = N.Table(dirty, cards)
    # a target trains for as many iterations as the golden file holds for it: 60 for most, ALL 300 of the reference's job for the cheap ones
    waves = ([10, 9, 8, 7, 6, 5], [0, 11, 1, 12, 2, 13], [3, 4, 14, 15])
    assert sorted(t for w in waves for t in w) == sorted(counts)            # every target of the file is trained and compared
    for wave in waves:
        with ThreadPoolExecutor(len(wave)) as ex:
            blobs = dict(zip(wave, ex.map(lambda t: _train(tab, dirty, cards, gold, t, counts[t]), wave)))
        _compare("10M x 16", gold, blobs, {t: counts[t] for t in wave})


@pytest.mark.timeout(1800)
def test_config3_shard_30_iterations_match_the_oracle_digests():
    """The per-GPU shape of BASELINE configs[3] -- a 12.5M x 32 row shard, two 16-feature chunks, the two-chunk wave-specialised level pass
    in its DEFAULT form -- past iteration 2.  tests/golden/bench_shard_digests.json (tests/golden/make_bench_job_golden.py --rows 12500000
    --cols 32 --seed 43 --targets 0,7 --iters 30 --out bench_shard_digests.json: 10 minutes of host time) holds the oracle's digest of every
    one of 30 iterations for the binary target c0 AND the K = 24 target c7 (k_grad_mc, 24 class trees per iteration, each on its own
    fixed-point grid: numerics v2.2).  Exactly {c0, c7} with K = 2 / 24 and 30 digests each is asserted before training -- the file once
    lost c7 in a regeneration and this test went on passing on c0 alone.  The HIP trainer trains both next to each other (two streams)
    and every iteration must match."""
    from concurrent.futures import ThreadPoolExecutor
    from repair import _native as N
    gold, counts = _gold("bench_shard_digests.json")
    assert counts == {0: 30, 7: 30} and gold["targets"]["c0"]["K"] == 2 and gold["targets"]["c7"]["K"] == 24
    dirty, clean, cards = make_table(gold["table"]["rows"], gold["table"]["cols"], seed=gold["table"]["seed"])
    del clean
    tab = N.Table(dirty, cards)
    targets = list(counts)
    with ThreadPoolExecutor(len(targets)) as ex:
        blobs = dict(zip(targets, ex.map(lambda t: _train(tab, dirty, cards, gold, t, counts[t]), targets)))
    _compare("12.5M x 32 shard", gold, blobs, counts)


@pytest.mark.timeout(1800)
def test_config3_whole_table_100m_x_32_matches_the_oracle_digests():
    """The N = 1 base of the north-star scaling curve: the WHOLE 100M x 32 table of BASELINE configs[3] on one GPU.  tests/golden/
    bench_whole_digests.json (make_bench_job_golden.py --rows 100000000 --cols 32 --seed 43 --parallel --targets 0,1 --iters 5 --out
    bench_whole_digests.json: the table bench.py --config 100m32 draws) holds the oracle's digest of every iteration of exactly {c0 (K = 2),
    c1 (K = 3)}, asserted before training.  What this reaches: 100M-row class trees on the real 100M-row fixed-point grid through the
    two-chunk wave-specialised level pass, and BYTE offsets above 2^32 in the bin records (3.2 GB per chunk).  What it does not: with
    K <= 3, K x n_train is 3.0e8 ELEMENTS, so no (g, h), score or node-id index comes near 2^31 -- that is
    test_two_chunk_k64_35m_x_32_indexes_beyond_2_to_31_elements below; the many-class targets of this table are pinned by no oracle."""
    from concurrent.futures import ThreadPoolExecutor
    from repair import _native as N
    from repair.synth import make_table_parallel
    gold, counts = _gold("bench_whole_digests.json")
    assert counts == {0: 5, 1: 5} and gold["table"]["generator"] == "make_table_parallel"
    dirty, _, cards = make_table_parallel(gold["table"]["rows"], gold["table"]["cols"], seed=gold["table"]["seed"], threads=min(32, os.cpu_count() or 1))
    tab = N.Table(dirty, cards)
    targets = list(counts)
    with ThreadPoolExecutor(len(targets)) as ex:
        blobs = dict(zip(targets, ex.map(lambda t: _train(tab, dirty, cards, gold, t, counts[t]), targets)))
    _compare("100M x 32", gold, blobs, counts)


@pytest.mark.timeout(1800)
def test_two_chunk_k64_35m_x_32_indexes_beyond_2_to_31_elements():
    """The only oracle comparison whose per-(row, class) element index exceeds 2^31: make_table(35_000_000, 32, seed=43), target c10 (K = 64),
    2 boosting iterations (the second one's gradients come from scores the first one updated).  31 features -> two 16-feature chunks ->
    k_level_mt<2, ...>; 64 class trees -> k_grad_mc; K x n_train = 64 x 34 649 311 = 2.218e9 = 1.033 x 2^31, so (g, h), scores and node
    ids are all indexed beyond 2^31 -- where `row * K + k` or `k * N + row` in 32-bit arithmetic would wrap.  bench.py --config 100m32
    trains such targets (c7: 2.4e9) under models_md5 only, which compares the library with itself.
    tests/golden/bench_big_index_digests.json: make_bench_job_golden.py --rows 35000000 --cols 32 --seed 43 --targets 10 --iters 2 --out
    bench_big_index_digests.json -- 78 s of host time on 16 threads and 60 GB of peak memory (24 bytes of oracle state per (row, class))."""
    from repair import _native as N
    gold, counts = _gold("bench_big_index_digests.json")
    assert counts == {10: 2}
    g = gold["targets"]["c10"]
    assert g["K"] * g["train_rows"] > 2 ** 31, "K x train_rows = %d: the pin no longer crosses 2^31 elements" % (g["K"] * g["train_rows"])
    assert 17 <= gold["table"]["cols"] - 1 <= 32                          # nchunk == 2
    dirty, clean, cards = make_table(gold["table"]["rows"], gold["table"]["cols"], seed=gold["table"]["seed"])
    del clean
    tab = N.Table(dirty, cards)
    blobs = {10: _train(tab, dirty, cards, gold, 10, counts[10])}
    print("35M x 32, c10: K x train_rows = %d = %.4f x 2^31" % (g["K"] * g["train_rows"], g["K"] * g["train_rows"] / 2.0 ** 31))
    _compare("35M x 32", gold, blobs, counts)
