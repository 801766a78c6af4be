"""-m gpu: the HIP tree growers (level-synchronous streaming grower, leaf-wise index-list grower) against the CPU oracle and
against each other, bit-exact.

The level grower (csrc/rgbm_level.h) is used for 1 <= max_depth <= 7 and F <= 255, everything else takes the leaf-wise grower
(csrc/rgbm_kernels.h); RGBM_GROWER=level|leafwise forces one of them.  The level pass (k_level_mt) shares a workgroup between as
many class trees as the LDS holds and takes further launches per level when it does not hold one class tree's built nodes; the
switches RGBM_MT_TREES (cap on the class trees per workgroup), RGBM_LV_LDS (smaller LDS pool: several built-slot windows per level)
and RGBM_MT_BLOCKS (row blocks) run the same configuration through those shapes here.
"""
import os

import numpy as np
import pytest

from tests.synth import make_table, balanced_weights

pytestmark = pytest.mark.gpu


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# the same fit through: the level grower as configured by default; one class tree per workgroup; a small LDS pool (several built-slot
# windows per level) with odd row-block counts; the leaf-wise grower
VARIANTS = [("level", dict(RGBM_GROWER="level")),
            ("level, 1 class tree per workgroup", dict(RGBM_GROWER="level", RGBM_MT_TREES=1)),
            ("level, 2 class trees, small LDS, 24 row blocks", dict(RGBM_GROWER="level", RGBM_MT_TREES=2, RGBM_LV_LDS=99000, RGBM_MT_BLOCKS=24, RGBM_LV_BLOCKS=24)),
            ("leafwise", dict(RGBM_GROWER="leafwise"))]


def _three_way(X, n_codes, y, K, obj, cw=None, yv=None, variants=None, **kw):
    from oracle import oracle as O
    from repair import _native as N
    params = dict(objective=obj, num_class=max(K, 2), **kw)
    mo = O.train(X, n_codes, y, K, y_value=yv, class_weight=cw, **params)
    bo = mo.save()
    first = None
    for name, env in (variants or VARIANTS):
        with _env(**env):
            m = N.train(X, n_codes, y, K, y_value=yv, class_weight=cw, **params)
        assert m.save() == bo, "%s: differs from the oracle" % name
        first = first or m
    assert np.array_equal(mo.predict(X), first.predict(X))
    return mo


def _xy(n, cols, tgt, seed, null_ratio=0.01):
    dirty, clean, cards = make_table(n, cols, seed=seed, null_ratio=null_ratio)
    feats = [c for c in range(cols) if c != tgt]
    rows = dirty[tgt] >= 0
    return np.ascontiguousarray(dirty[feats][:, rows]), cards[feats], dirty[tgt][rows], int(cards[tgt])


@pytest.mark.parametrize("depth,leaves", [(1, 31), (2, 31), (3, 5), (5, 31), (7, 2), (7, 100), (6, 64)])
def test_depth_and_leaf_budgets(depth, leaves):
    X, nc, y, K = _xy(20011, 8, 5, seed=31)
    _three_way(X, nc, y, K, 1, cw=balanced_weights(y, K), n_estimators=6, learning_rate=0.3, max_depth=depth, num_leaves=leaves)


@pytest.mark.parametrize("n", [1, 7, 63, 2047, 2049, 4100])
def test_row_counts_around_tile_edges(n):
    X, nc, y, K = _xy(max(n * 2, 40), 6, 3, seed=37)
    X = np.ascontiguousarray(X[:, :n]); y = y[:n]
    _three_way(X, nc, y, K, 1, cw=balanced_weights(y, K) if len(np.unique(y)) > 1 else None, n_estimators=4, learning_rate=0.3, min_data_in_leaf=2)


def test_binary_and_regression_three_way():
    X, nc, y, K = _xy(30000, 8, 0, seed=41)   # column 0 is binary
    assert K == 2
    _three_way(X, nc, y, K, 0, cw=balanced_weights(y, K), n_estimators=12, learning_rate=0.2)
    rng = np.random.default_rng(43)
    dirty, clean, cards = make_table(9000, 6, seed=43)
    vals = np.sort(rng.normal(size=30))
    _three_way(np.ascontiguousarray(dirty[:5]), cards[:5], (clean[5] % 30).astype(np.int32), 30, 2, yv=vals, n_estimators=10, learning_rate=0.1, lambda_l2=1.0)


def test_many_bins_force_histogram_groups():
    """16 features x ~250 bins: one node's histogram is ~64 KB of LDS, so every level beyond the first takes several launches
    (windows of one built slot each) -- with the full LDS pool (a smaller one does not hold a node of this table at all)."""
    rng = np.random.default_rng(47)
    n = 60000
    z = rng.integers(0, 250, n)
    X = np.stack([((z * (j + 3) + rng.integers(0, 40, n)) % 250).astype(np.int32) for j in range(16)])
    X[3][rng.random(n) < 0.03] = -1
    y = ((z // 25 + (X[0] > 120)) % 6).astype(np.int32)
    _three_way(np.ascontiguousarray(X), [250] * 16, y, 6, 1, cw=balanced_weights(y, 6), variants=[VARIANTS[0], VARIANTS[1], VARIANTS[3]],
               n_estimators=4, learning_rate=0.3, min_data_in_leaf=5)


def test_two_chunks_with_many_bins():
    rng = np.random.default_rng(53)
    n = 25000
    z = rng.integers(0, 120, n)
    X = np.stack([((z * (j + 1) + rng.integers(0, 9, n)) % (20 + 11 * j)).astype(np.int32) for j in range(23)])
    y = ((z // 10 + X[20] % 3) % 5).astype(np.int32)
    _three_way(np.ascontiguousarray(X), [20 + 11 * j for j in range(23)], y, 5, 1, cw=balanced_weights(y, 5), n_estimators=5, learning_rate=0.3)


@pytest.mark.parametrize("kw", [
    dict(bagging_fraction=0.6, bagging_freq=2),
    dict(feature_fraction=0.4, lambda_l1=0.3, min_gain_to_split=0.02),
    dict(min_data_in_leaf=400, min_sum_hessian_in_leaf=5.0),
])
def test_sampling_constraints_three_way(kw):
    X, nc, y, K = _xy(15000, 9, 6, seed=59, null_ratio=0.03)
    _three_way(X, nc, y, K, 1, cw=balanced_weights(y, K), n_estimators=8, learning_rate=0.2, **kw)


def test_many_classes():
    """K = 64 class trees grown in lock step (the expensive shape of the synthetic workload)."""
    X, nc, y, K = _xy(40000, 16, 10, seed=61)
    assert K == 64
    _three_way(X, nc, y, K, 1, cw=balanced_weights(y, K), n_estimators=3, learning_rate=0.3)


def test_unseen_and_constant_columns():
    rng = np.random.default_rng(67)
    n = 5000
    a = rng.integers(0, 4, n).astype(np.int32)
    b = np.zeros(n, np.int32)                      # constant -> trivial feature
    c = np.full(n, -1, np.int32)                   # all NULL
    d = rng.integers(0, 9, n).astype(np.int32)
    y = ((a + d) % 3).astype(np.int32)
    _three_way(np.ascontiguousarray(np.stack([a, b, c, d])), [4, 1, 5, 9], y, 3, 1, cw=balanced_weights(y, 3), n_estimators=6, learning_rate=0.3)


def test_random_configurations_stress():
    """Irregular gains (noise features, tiny leaves, heavy leaf-budget pruning): the speculative expansion bound and the
    best-first replay must reproduce the oracle's leaf-wise tree for every draw."""
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(20260922)
    for trial in range(24):
        n = int(rng.integers(300, 9000))
        F = int(rng.integers(2, 12))
        cards = rng.integers(2, 40, F)
        X = np.stack([rng.integers(0, c, n) for c in cards]).astype(np.int32)
        if rng.random() < 0.5:
            X[rng.integers(0, F)][rng.random(n) < 0.1] = -1
        K = int(rng.choice([2, 3, 5, 9]))
        signal = (X[0] % K + (X[min(1, F - 1)] > cards[min(1, F - 1)] // 2)) % K
        y = np.where(rng.random(n) < rng.uniform(0.2, 0.9), rng.integers(0, K, n), signal).astype(np.int32)
        kw = dict(objective=0 if K == 2 else 1, num_class=max(K, 2), n_estimators=int(rng.integers(2, 7)), learning_rate=float(rng.uniform(0.05, 0.5)),
                  num_leaves=int(rng.integers(2, 41)), max_depth=int(rng.integers(1, 8)), min_data_in_leaf=int(rng.integers(1, 60)),
                  min_sum_hessian_in_leaf=float(10 ** rng.uniform(-3, 0.5)), lambda_l2=float(rng.choice([0.0, 0.5, 3.0])),
                  min_gain_to_split=float(rng.choice([0.0, 0.0, 0.05])), feature_fraction=float(rng.choice([1.0, 1.0, 0.6])))
        cw = balanced_weights(y, K)
        mo = O.train(X, cards.astype(np.int32), y, K, class_weight=cw, **kw)
        for g, env in (VARIANTS[0], VARIANTS[1 + trial % 2]):
            with _env(**env):
                mg = N.train(X, cards.astype(np.int32), y, K, class_weight=cw, **kw)
            assert mo.save() == mg.save(), "trial %d differs (%s): n=%d F=%d K=%d %r" % (trial, g, n, F, K, kw)


def test_random_configurations_stress_wide_and_sampled():
    """Second stress family: two feature chunks (F up to 24), bagging / feature sub-sampling, regression targets."""
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(777)
    for trial in range(18):
        n = int(rng.integers(500, 12000))
        F = int(rng.integers(14, 25))
        cards = rng.integers(2, 70, F)
        z = rng.integers(0, 48, n)
        X = np.stack([np.where(rng.random(n) < 0.7, (z * (j + 1)) % c, rng.integers(0, c, n)) for j, c in enumerate(cards)]).astype(np.int32)
        X[rng.integers(0, F)][rng.random(n) < 0.05] = -1
        reg = trial % 5 == 4
        kw = dict(n_estimators=int(rng.integers(2, 6)), learning_rate=float(rng.uniform(0.05, 0.4)), num_leaves=int(rng.integers(2, 64)),
                  max_depth=int(rng.integers(2, 8)), min_data_in_leaf=int(rng.integers(1, 40)), lambda_l2=float(rng.choice([0.0, 1.0])))
        if trial % 3 == 0:
            kw.update(bagging_fraction=float(rng.uniform(0.5, 0.95)), bagging_freq=int(rng.integers(1, 4)))
        if trial % 4 == 1:
            kw.update(feature_fraction=float(rng.uniform(0.3, 0.9)))
        if reg:
            vals = np.sort(rng.normal(size=25))
            y = ((z + X[1]) % 25).astype(np.int32)
            args, kws = (X, cards.astype(np.int32), y, 25), dict(y_value=vals, objective=2, num_class=2, **kw)
        else:
            K = int(rng.choice([2, 4, 7, 17]))
            y = np.where(rng.random(n) < 0.3, rng.integers(0, K, n), (z + X[2]) % K).astype(np.int32)
            args, kws = (X, cards.astype(np.int32), y, K), dict(class_weight=balanced_weights(y, K), objective=0 if K == 2 else 1, num_class=max(K, 2), **kw)
        mo = O.train(*args, **kws)
        for g, env in (VARIANTS[0], VARIANTS[1 + trial % 2]):
            with _env(**env):
                mg = N.train(*args, **kws)
            assert mo.save() == mg.save(), "trial %d differs (%s): n=%d F=%d %r" % (trial, g, n, F, kw)


@pytest.mark.parametrize("lds,trees,blocks", [(None, None, None), (99000, None, 16), (97000, 1, 8), (None, 3, 40)])
def test_level_pass_shapes_stay_bit_exact(lds, trees, blocks):
    """Binary (the largest gradients), K = 24 and a two-chunk regression table through several shapes of the level pass: class trees
    per workgroup, LDS pool (built-slot windows), row blocks."""
    from oracle import oracle as O
    from repair import _native as N
    env = dict(RGBM_GROWER="level", RGBM_LV_LDS=lds, RGBM_MT_TREES=trees, RGBM_MT_BLOCKS=blocks, RGBM_LV_BLOCKS=blocks)
    cases = []
    X, nc, y, K = _xy(30000, 8, 0, seed=101)                       # binary
    cases.append((X, nc, y, K, dict(objective=0, num_class=2, n_estimators=5, learning_rate=0.3), balanced_weights(y, K), None))
    X, nc, y, K = _xy(26000, 10, 7, seed=103, null_ratio=0.03)     # K = 24
    cases.append((X, nc, y, K, dict(objective=1, num_class=K, n_estimators=3, learning_rate=0.3, min_data_in_leaf=5), balanced_weights(y, K), None))
    rng = np.random.default_rng(107)                               # two chunks, regression
    z = rng.integers(0, 90, 21000)
    X = np.stack([((z * (j + 1) + rng.integers(0, 5, 21000)) % (9 + 7 * j)).astype(np.int32) for j in range(19)])
    vals = np.sort(rng.normal(size=30) * 50.0)
    cases.append((np.ascontiguousarray(X), np.asarray([9 + 7 * j for j in range(19)], np.int32), (z % 30).astype(np.int32), 30,
                  dict(objective=2, num_class=2, n_estimators=4, learning_rate=0.2), None, vals))
    for X, nc, y, K, kw, cw, yv in cases:
        mo = O.train(X, nc, y, K, y_value=yv, class_weight=cw, **kw)
        with _env(**env):
            mg = N.train(X, nc, y, K, y_value=yv, class_weight=cw, **kw)
        assert mo.save() == mg.save(), "objective %d differs (lds=%r trees=%r blocks=%r)" % (kw["objective"], lds, trees, blocks)


@pytest.mark.parametrize("tgt", [0, 3])
def test_millions_of_rows_against_the_oracle(tgt):
    """2.5M rows: every workgroup streams many wave tiles, the rings wrap many times, and the per-workgroup partials are summed by
    k_level_reduce.  (100M rows: tools/big_rows_check.py.)"""
    X, nc, y, K = _xy(2_500_000, 8, tgt, seed=109)
    from oracle import oracle as O
    from repair import _native as N
    kw = dict(objective=0 if K == 2 else 1, num_class=max(K, 2), n_estimators=3, learning_rate=0.3)
    cw = balanced_weights(y, K)
    mo = O.train(X, nc, y, K, class_weight=cw, **kw)
    mg = N.train(X, nc, y, K, class_weight=cw, **kw)
    assert mo.save() == mg.save()


def test_three_and_more_feature_chunks():
    """F = 40 and F = 70: more than two 16-feature chunks (the split feature of a node may live in any record)."""
    rng = np.random.default_rng(131)
    for F, n in ((40, 9000), (70, 5000)):
        z = rng.integers(0, 50, n)
        cards = [int(c) for c in rng.integers(2, 30, F)]
        X = np.stack([np.where(rng.random(n) < 0.6, (z * (j + 2)) % c, rng.integers(0, c, n)) for j, c in enumerate(cards)]).astype(np.int32)
        X[rng.integers(0, F)][rng.random(n) < 0.05] = -1
        y = ((z + X[F - 1] + X[17]) % 6).astype(np.int32)
        _three_way(np.ascontiguousarray(X), cards, y, 6, 1, cw=balanced_weights(y, 6), n_estimators=4, learning_rate=0.3)


@pytest.mark.parametrize("K", [113, 219])
def test_hundreds_of_classes(K):
    """The reference's logs show targets with 52..219 classes; the gradient kernel switches layout above 112."""
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(K)
    n = 30000
    z = rng.integers(0, K, n)
    X = np.stack([(z * (j + 1) + rng.integers(0, 3, n)) % (20 + 13 * j) for j in range(6)]).astype(np.int32)
    y = np.where(rng.random(n) < 0.2, rng.integers(0, K, n), z).astype(np.int32)
    cards = [20 + 13 * j for j in range(6)]
    kw = dict(objective=1, num_class=K, n_estimators=2, learning_rate=0.3)
    cw = balanced_weights(y, K)
    mo = O.train(X, cards, y, K, class_weight=cw, **kw)
    mg = N.train(X, cards, y, K, class_weight=cw, **kw)
    assert mo.save() == mg.save()
    assert np.array_equal(mo.predict(X[:, :2000]), mg.predict(X[:, :2000]))


def test_regression_with_thousands_of_distinct_targets_and_small_max_bin():
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(137)
    n = 40000
    X = np.stack([rng.integers(0, c, n) for c in (700, 40, 9, 300)]).astype(np.int32)
    vals = np.sort(rng.normal(size=3000) * 10.0)
    y = ((X[0] * 3 + X[1]) % 3000).astype(np.int32)
    for max_bin in (15, 63, 255):
        kw = dict(objective=2, num_class=2, n_estimators=6, learning_rate=0.2, max_bin=max_bin)
        mo = O.train(X, [700, 40, 9, 300], y, 3000, y_value=vals, **kw)
        mg = N.train(X, [700, 40, 9, 300], y, 3000, y_value=vals, **kw)
        assert mo.save() == mg.save(), "max_bin=%d" % max_bin


@pytest.mark.parametrize("rows,cols,tgt", [(600, 4, 2), (40000, 11, 10)])
def test_sparse_sweep_of_the_level_pass_changes_nothing(rows, cols, tgt, monkeypatch):
    """k_level_mt sweeps class trees whose expanded parents hold few rows through their node ids only (RGBM_MT_SPARSE, default on):
    same routing, same built rows -- the model bytes (leaf counts included) must not depend on it.  A many-class target (deep levels
    with a few per cent live rows next to dense class trees in the same workgroup) and a tiny table."""
    from repair import _native as N
    from tests.synth import make_table, balanced_weights
    dirty, clean, cards = make_table(rows, cols, seed=29)
    feats = [c for c in range(cols) if c != tgt]
    r = dirty[tgt] >= 0
    X = np.ascontiguousarray(dirty[feats][:, r]); y = dirty[tgt][r]; K = int(cards[tgt])
    for kw in (dict(), dict(bagging_fraction=0.7, bagging_freq=1), dict(num_leaves=60, min_data_in_leaf=3)):
        blobs = []
        for v in ("0", "1"):
            monkeypatch.setenv("RGBM_MT_SPARSE", v)
            blobs.append(N.train(X, cards[feats], y, K, class_weight=balanced_weights(y, K), objective=0 if K == 2 else 1, num_class=max(K, 2),
                                 n_estimators=14, learning_rate=0.2, **kw).save())
        assert blobs[0] == blobs[1], kw


@pytest.mark.parametrize("rows,cols,tgt", [(600, 4, 2), (30000, 11, 10), (30000, 11, 5), (50000, 6, 0)])
def test_grid_sums_out_of_the_gradient_kernels_equal_a_pass_of_their_own(rows, cols, tgt, monkeypatch):
    """Numerics v2.2: every class tree of an iteration gets its fixed-point grid from the coarse sums of its (g, h).  By default the gradient
    kernels leave those sums per workgroup (k_grad_mc: K = 64, the 64-rows x 4-waves layout; k_grad_mc_rows: K = 4 / 12, thread per row;
    k_grad<0> / <2>: binary / L2) and k_fx_reduce adds them up; RGBM_FX_MEASURE=separate takes them from a pass of its own over the (g, h)
    array (k_fx_measure).  Same integer sums, so the model bytes must not depend on it -- with NULL target cells in the table (rows that
    never take part), bagging (out-of-bag rows carry (0, 0)), deep trees and one-iteration jobs -- and both equal the oracle's model."""
    from oracle import oracle as O
    from repair import _native as N
    from tests.synth import make_table, balanced_weights
    dirty, clean, cards = make_table(rows, cols, seed=31, null_ratio=0.03)
    feats = [c for c in range(cols) if c != tgt]
    K = int(cards[tgt])
    tab = N.Table(dirty, cards)
    yv = np.arange(K, dtype=np.float64) * 0.75 - 1.0
    cases = [dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=balanced_weights(dirty[tgt], K), n_estimators=9, learning_rate=0.2),
             dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=balanced_weights(dirty[tgt], K), n_estimators=6, learning_rate=0.2, bagging_fraction=0.6, bagging_freq=2),
             dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=None, n_estimators=2, num_leaves=90, min_data_in_leaf=2),
             dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=None, n_estimators=1),
             dict(objective=2, y_value=yv, class_weight=None, n_estimators=7, learning_rate=0.3, num_leaves=50, min_data_in_leaf=5)]
    r = dirty[tgt] >= 0
    for ci, kw in enumerate(cases):
        blobs = []
        for v in ("fused", "separate"):
            monkeypatch.setenv("RGBM_FX_MEASURE", v)
            blobs.append(tab.train(tgt, feats, **kw).save())
        monkeypatch.delenv("RGBM_FX_MEASURE")
        assert blobs[0] == blobs[1], {k: v for k, v in kw.items() if k not in ("class_weight", "y_value")}
        if ci in (0, 1, 4):
            mo = O.train(np.ascontiguousarray(dirty[feats][:, r]), cards[feats], dirty[tgt][r], K, **kw).save()
            assert blobs[0] == mo, {k: v for k, v in kw.items() if k not in ("class_weight", "y_value")}


@pytest.mark.parametrize("rows,cols,tgt", [(600, 4, 2), (30000, 11, 10), (30000, 11, 5), (50000, 6, 0), (20000, 20, 7)])
def test_score_update_pass_matches_the_oracle_in_every_case(rows, cols, tgt):
    """AddScore of the level grower is a pass of its own after every iteration (k_level_final: the last routing step, the deepest counts and the
    score update in one).  Every model equals the oracle's -- binary / few-class / many-class / L2 targets, NULL target cells (rows that never
    take part), bagging (out-of-bag rows are routed and scored too), trees without a split, a one-iteration job, two chunks.  (The variant that
    folded the update into the next iteration's gradient kernel was measured slower and removed; its shapes and cases stay.)"""
    from oracle import oracle as O
    from repair import _native as N
    from tests.synth import make_table, balanced_weights
    dirty, clean, cards = make_table(rows, cols, seed=37, null_ratio=0.03)
    feats = [c for c in range(cols) if c != tgt]
    K = int(cards[tgt])
    tab = N.Table(dirty, cards)
    yv = np.arange(K, dtype=np.float64) * 0.75 - 1.0
    base = dict(objective=0 if K == 2 else 1, num_class=max(K, 2))
    cases = [dict(base, class_weight=balanced_weights(dirty[tgt], K), n_estimators=9, learning_rate=0.2),
             dict(base, class_weight=balanced_weights(dirty[tgt], K), n_estimators=7, learning_rate=0.2, bagging_fraction=0.6, bagging_freq=2),
             dict(base, class_weight=None, n_estimators=5, min_data_in_leaf=rows),          # no tree can split
             dict(base, class_weight=None, n_estimators=1),
             dict(objective=2, y_value=yv, class_weight=None, n_estimators=7, learning_rate=0.3, num_leaves=50, min_data_in_leaf=5)]
    r = dirty[tgt] >= 0
    for kw in cases:
        blob = tab.train(tgt, feats, **kw).save()
        mo = O.train(np.ascontiguousarray(dirty[feats][:, r]), cards[feats], dirty[tgt][r], K, **kw).save()
        assert blob == mo, {k: v for k, v in kw.items() if k not in ("class_weight", "y_value")}


@pytest.mark.parametrize("rows,cols,tgt", [(40000, 11, 10), (30000, 11, 8), (25000, 24, 7), (60000, 16, 10), (40000, 32, 7)])
def test_feature_rotation_of_the_level_pass_changes_nothing(rows, cols, tgt, monkeypatch):
    """The histogram updates of a level pass in rotated form (lane l works on feature (j + l) mod 16: rgbm_level.h, MT_ROT) -- chosen per launch
    where the LDS holds fewer than eight copies of the level's histograms (RGBM_MT_ROT=-1, the default; three until round 6), never (0) or for every pass that has the
    instantiation (1) -- are the same exact integer sums in another order of atomics: the model bytes must not depend on it.  Many-class targets on
    one 16-byte record (deep levels rotate by default) and a two-chunk table (the wave-specialised pass: both records rotated), also with bagging
    and with a small LDS pool (several built-slot windows per level)."""
    from repair import _native as N
    from tests.synth import make_table, balanced_weights
    dirty, clean, cards = make_table(rows, cols, seed=37)
    feats = [c for c in range(cols) if c != tgt]
    K = int(cards[tgt])
    tab = N.Table(dirty, cards)
    for kw, env in ((dict(), {}), (dict(bagging_fraction=0.7, bagging_freq=1), {}), (dict(num_leaves=60, min_data_in_leaf=3), {"RGBM_LV_LDS": "99000"})):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        blobs = []
        for v in ("0", "-1", "1"):
            monkeypatch.setenv("RGBM_MT_ROT", v)
            blobs.append(tab.train(tgt, feats, class_weight=balanced_weights(dirty[tgt], K), objective=1, num_class=K, n_estimators=8, learning_rate=0.2, **kw).save())
        for k_ in env:
            monkeypatch.delenv(k_)
        assert blobs[0] == blobs[1] == blobs[2], (kw, env)
        #  the DEFAULT per-launch policy only rotates chunks that fill >= 12 of their 16 feature slots: the 16-column table (15 features, K = 64:
        # levels 2-6 hold fewer than eight copies) and the 32-column one (16 + 15 features, wave-specialised two-chunk pass) are the shapes where "-1" really
        # rotates some launches and not others -- held to the oracle as well
        if cols in (16, 32) and not kw:
            from oracle import oracle as O
            r = dirty[tgt] >= 0
            mo = O.train(np.ascontiguousarray(dirty[feats][:, r]), cards[feats], dirty[tgt][r], K, class_weight=balanced_weights(dirty[tgt], K), objective=1, num_class=K,
                         n_estimators=8, learning_rate=0.2).save()
            assert blobs[1] == mo


def test_joint_codes_in_the_root_pass_change_nothing(monkeypatch):
    """The root pass accumulates joint histograms of feature groups (one byte of the joint record per group of up to 256 joint bins); every real
    feature's histogram is the exact marginal, so the model bytes are those of the plain record (RGBM_JOINT_ROOT=0)."""
    from repair import _native as N
    from tests.synth import make_table, balanced_weights
    dirty, clean, cards = make_table(300000, 16, seed=41)       # K * N >= 2^21: the joint root pass is on
    tgt = 10
    feats = [c for c in range(16) if c != tgt]
    K = int(cards[tgt])
    tab = N.Table(dirty, cards)
    blobs = []
    for env in ({"RGBM_JOINT_ROOT": "0"}, {}):
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        blobs.append(tab.train(tgt, feats, class_weight=balanced_weights(dirty[tgt], K), objective=1, num_class=K, n_estimators=4, learning_rate=0.2).save())
        for k_ in env:
            monkeypatch.delenv(k_)
    assert blobs[0] == blobs[1]
