"""-m gpu: k_level_step (csrc/rgbm_level.h) -- one workgroup per expanded parent sums the built child's partials, derives the sibling, scans
both children with the packed threshold scan and leaves each child's best split in its node -- and the register form of k_level_replay's
selection loop.  Model bytes against the CPU oracle (3 iterations, learning_rate 0.3, level grower, no distinct-row view) on the smallest
tables where these can go wrong:

  * wide and narrow features in one lane map: a 224-bin feature (56 lanes of a wave) next to one-lane features, NULLs in three columns; also
    with masked features (feature_fraction 0.5) and with children that are not searched (min_data_in_leaf 2500);
  * F = 1: one lane-map row, one candidate per child;
  * two chunks: seventeen one-lane features and a 56-lane feature that has to move to the next wave;
  * ties: equal gains between two leaves and between a feature and its copy -- leaf order and feature order come from the tie rules alone.

Each table under: the defaults; fewer / more workgroup partials per class tree than the step kernel sums itself (more: k_level_reduce runs
in front); the plain root pass; a small LDS pool for the passes; the scan out of the pool instead of LDS; row multiplicities (against the
oracle on the expanded table); the collective path with a world of one.  The oracle's models are computed once per table and shared."""
import functools

import numpy as np
import pytest

from tests.test_gpu_growers import _env
from tests.test_gpu_level_setup import _mult

pytestmark = pytest.mark.gpu

BASE = dict(n_estimators=3, learning_rate=0.3)
STEP_MAX_GX = 256     # LevelGrower::step_max_gx (csrc/rgbm.hip): the most workgroup partials per class tree k_level_step sums itself


def _with_nulls(col, rng, ratio):
    col = col.copy()
    col[rng.random(col.shape[0]) < ratio] = -1
    return col


def wide_narrow():
    """20 000 rows, K = 3, cardinalities 255, 2, 3, 3, 3, 3, 200, 4, 65, 129; 5 % NULLs in columns 0, 2 and 8"""
    rng = np.random.default_rng(1401)
    n = 20000
    cards = np.asarray([255, 2, 3, 3, 3, 3, 200, 4, 65, 129], np.int32)
    z = rng.integers(0, 240, n)
    y = ((z // 7 + rng.integers(0, 2, n)) % 3).astype(np.int32)
    X = np.empty((10, n), np.int32)
    for j, c in enumerate(cards):
        sig = (z * (j + 1) + (y << (j % 2))) % c
        X[j] = np.where(rng.random(n) < 0.75, sig, rng.integers(0, c, n))
    # column 0 holds 224 of its 255 codes: 224 value bins (56 lanes of the scan) + the NaN bin
    X[0] = np.minimum(X[0], 223)
    for j in (0, 2, 8):
        X[j] = _with_nulls(X[j], rng, 0.05)
    return np.ascontiguousarray(X), cards, y, 3


def one_feature():
    """one 37-code feature, K = 3"""
    rng = np.random.default_rng(1409)
    n = 20000
    # eight of the codes sit in two rows each (below min_data_in_bin: no bin of their own), the other 29 get a bin each; the class
    # probabilities follow the bits of a code's rank, the top bit strongest, so that best-first growth stays inside max_depth
    rare = np.arange(37)[2::4][:8]
    freq = np.setdiff1d(np.arange(37), rare)
    r = rng.integers(0, len(freq), n)
    x = freq[r].astype(np.int32)
    x[rng.permutation(n)[:16]] = np.repeat(rare, 2)
    S = rng.normal(size=(5, 3))
    logit = sum(2.0 ** (b - 4) * 2 * S[b][None, :] * ((r >> b) & 1)[:, None] for b in range(5))
    pr = np.exp(logit)
    pr /= pr.sum(axis=1, keepdims=True)
    y = (rng.random(n)[:, None] > np.cumsum(pr, axis=1)).sum(axis=1).clip(0, 2).astype(np.int32)
    return np.ascontiguousarray(x[None, :]), np.asarray([37], np.int32), y, 3


def two_chunks():
    """seventeen 3-bin features followed by a 255-code one, K = 4"""
    rng = np.random.default_rng(1423)
    n = 20000
    cards = np.asarray([3] * 17 + [255], np.int32)
    z = rng.integers(0, 224, n)
    y = ((z // 5 + rng.integers(0, 2, n)) % 4).astype(np.int32)
    X = np.empty((18, n), np.int32)
    for j in range(17):
        X[j] = np.where(rng.random(n) < 0.7, (z // (1 + j % 5) + y * (j % 3)) % 3, rng.integers(0, 3, n))
    X[17] = z
    return np.ascontiguousarray(X), cards, y, 4


def ties():
    """24 000 rows: A in {0, 1} x B in {0..3} x D in {0, 1, 2}, 1000 rows per cell; the label is 1 in round(p 1000) rows of a cell; columns A, B, B, D"""
    p0, p1 = (0.1, 0.1, 0.5, 0.5), (0.9, 0.9, 0.5, 0.5)
    cols, ys = [], []
    for a in range(2):
        for b in range(4):
            for d in range(3):
                ones = int(round((p1 if a else p0)[b] * 1000))
                cols.append(np.tile(np.asarray([[a], [b], [b], [d]], np.int32), (1, 1000)))
                ys.append((np.arange(1000) < ones).astype(np.int32))
    return np.ascontiguousarray(np.concatenate(cols, axis=1)), np.asarray([2, 4, 4, 3], np.int32), np.concatenate(ys), 2


# table -> (generator, extra parameters, check of the oracle's tree sizes [iteration][class tree])
TABLES = {
    "wide+narrow": (wide_narrow, dict(), lambda L: (L == 31).all()),
    "wide+narrow, masked features": (wide_narrow, dict(feature_fraction=0.5), lambda L: (L > 8).all()),
    "wide+narrow, unsearched children": (wide_narrow, dict(min_data_in_leaf=2500), lambda L: (L >= 5).all() and (L <= 7).all()),
    "F = 1": (one_feature, dict(), lambda L: (L >= 26).all() and (L <= 29).all()),
    "two chunks": (two_chunks, dict(), lambda L: (L == 31).all()),
    "ties": (ties, dict(), lambda L: (L >= 3).all()),
}


def _kw(K, extra):
    return dict(BASE, objective=0 if K == 2 else 1, num_class=max(K, 2), **extra)


def _leaves(blob):
    from repair import _native as N
    K, n_iter, trees = N.model_trees(blob)
    nt = 1 if K == 2 else K            # (a binary model has one tree per iteration)
    return np.asarray([len(t["leaf_value"]) for t in trees]).reshape(n_iter, -1)[:, :nt]


@functools.lru_cache(maxsize=None)
def _case(table, with_mult):
    """the table, its multiplicities (or None) and the oracle's model bytes -- of the EXPANDED table when the rows carry multiplicities"""
    from oracle import oracle as O
    gen, extra, sizes_ok = TABLES[table]
    X, cards, y, K = gen()
    mult = _mult(X.shape[1], seed=1427) if with_mult else None
    Xe, ye = (np.ascontiguousarray(np.repeat(X, mult, axis=1)), np.repeat(y, mult)) if with_mult else (X, y)
    ref = O.train(Xe, cards, ye, K, **_kw(K, extra)).save()
    if not with_mult:
        assert sizes_ok(_leaves(ref)), "the oracle's trees are not the sizes this table is meant to give: %s" % _leaves(ref).tolist()
    return X, cards, y, K, mult, ref


def _train(table, env, with_mult=False, collective=False):
    from repair import _native as N
    X, cards, y, K, mult, ref = _case(table, with_mult)
    kw = _kw(K, TABLES[table][1])
    F = X.shape[0]
    tab_codes = np.ascontiguousarray(np.concatenate([X, y[None, :]], axis=0))
    with _env(RGBM_GROWER="level", RGBM_DISTINCT="0", **env):
        tab = N.Table(tab_codes, np.append(cards, K).astype(np.int32))
        if mult is not None:
            tab.set_row_multiplicity(mult)
        if not collective:
            return tab.train(F, list(range(F)), **kw).save(), ref
        N.comm_init(N.comm_unique_id(), 0, 1, 0)
        try:
            return tab.train(F, list(range(F)), row_sharded=True, **kw).save(), ref
        finally:
            N.comm_finalize()


SETTINGS = [
    ("defaults", dict()),
    ("partials below the threshold", dict(RGBM_MT_BLOCKS=24, RGBM_LV_BLOCKS=24)),
    ("partials above the threshold", dict(RGBM_MT_BLOCKS=STEP_MAX_GX + 8, RGBM_LV_BLOCKS=STEP_MAX_GX + 8)),
    ("plain root pass", dict(RGBM_JOINT_ROOT=0)),
    ("small LDS pool", dict(RGBM_LV_LDS=70000)),
    ("scan out of the pool", dict(RGBM_STEP_READBACK=1)),
]


@pytest.mark.parametrize("name,env", SETTINGS, ids=[s[0] for s in SETTINGS])
@pytest.mark.parametrize("table", list(TABLES))
def test_step_kernel_gives_the_oracle_model(table, name, env):
    got, ref = _train(table, env)
    assert got == ref, "%s, %s" % (table, name)


@pytest.mark.parametrize("table", list(TABLES))
def test_step_kernel_with_row_multiplicities(table):
    got, ref = _train(table, dict(), with_mult=True)
    assert got == ref, table


@pytest.mark.parametrize("table", list(TABLES))
def test_step_kernel_on_the_collective_path_world_of_one(table):
    got, ref = _train(table, dict(), collective=True)
    assert got == ref, table


def test_ties_first_tree_is_decided_by_the_tie_rules():
    """gains 3840, 1920, 1920: a tie between two leaves (the smaller leaf index goes first) and between feature 1 and its copy 2 (never 2)"""
    from repair import _native as N
    X, cards, y, K, mult, ref = _case("ties", False)
    _, _, trees = N.model_trees(ref)
    t0 = trees[0]
    assert np.allclose(t0["gain"][:3], [3840.0, 1920.0, 1920.0], rtol=1e-9), t0["gain"].tolist()
    assert t0["feat"][0] == 0 and (t0["feat"][1:3] == 1).all()
    assert all((t["feat"] != 2).all() for t in trees)
