"""-m gpu: what a workgroup of the level passes does before its first row and after its last one (csrc/rgbm_level.h: the layout tables the
host builds once per fit, the route-table fill in parallel over the class trees, the 16-byte zeroing, the flush through the bin -> feature map),
model bytes against the CPU oracle on the smallest shapes where that set-up can go wrong:

  * K = 40 on eight features of at most 8 bins: the LDS holds every class tree of the target, so a workgroup gets 40 class trees at level 2 --
    the fill wraps around the 16 waves twice -- and groups of 16, 16, 8 (a short last group) with RGBM_MT_TREES=16; replicated and rotated form;
  * one class of 10 rows (its tree has nothing to split: finished at the root) and one of 0.5 % of the rows (swept sparsely at the deep levels)
    next to 38 dense ones: finished, sparse and dense class trees share a workgroup, with the sparse sweep on and off;
  * RGBM_LV_LDS=70000: several built-slot windows per level, so the table and the flush of the later launches of a level;
  * 3 000 rows in 24 row blocks: 12 wave tiles, so half of the workgroups see no row and still have to flush zeros;
  * each of these with row multiplicities (the multiplicity takes byte 15 of the record: the ring carries a slot array, the LDS budget differs);
  * a 20-feature table: the both-chunk form shares the prologue.
The oracle's models are computed once per table and shared by the cases."""
import functools
import struct

import numpy as np
import pytest

from tests.test_gpu_growers import _env

pytestmark = pytest.mark.gpu

K40 = 40
CARDS8 = np.asarray([8, 8, 7, 6, 8, 5, 8, 4], np.int32)
# min_sum_hessian_in_leaf = 8: the tree of the 10-row class (hessians of about 10 in all) cannot split, the tree of the 0.5 % class (about 150) can
KW = dict(objective=1, num_class=K40, n_estimators=3, learning_rate=0.3, min_sum_hessian_in_leaf=8.0)
KW_SMALL = dict(objective=1, num_class=K40, n_estimators=3, learning_rate=0.3)


def make_k40(n, seed):
    """(X [8][n], y [n]): class 0 has 10 rows whose features say nothing about it, class 1 about 0.5 % of the rows, classes 2..39 the rest."""
    rng = np.random.default_rng(seed)
    y = rng.integers(2, K40, n).astype(np.int32)
    pos = rng.permutation(n)
    n1 = max(15, n // 200)
    y[pos[:10]] = 0
    y[pos[10:10 + n1]] = 1
    X = np.empty((8, n), np.int32)
    for j, c in enumerate(CARDS8):
        sig = (y * (2 * j + 3) + (y >> (j % 3))) % c
        noise = rng.integers(0, c, n)
        X[j] = np.where(rng.random(n) < 0.7, sig, noise)
    X[:, pos[:10]] = np.stack([rng.integers(0, c, 10) for c in CARDS8])
    return np.ascontiguousarray(X), y


def _mult(n, seed):
    rng = np.random.default_rng(seed)
    m = np.ones(n, np.uint8)
    idx = rng.permutation(n)
    m[idx[: n // 5]] = 2
    m[idx[n // 5: n // 4]] = rng.integers(3, 9, n // 4 - n // 5)
    m[idx[n // 4: n // 4 + 3]] = 255
    return m


def tree_leaves(model_bytes):
    """leaf count of every tree of a saved model, [iteration][class tree]"""
    hdr = struct.unpack_from("<7i", model_bytes, 0)
    version, K, n_iter, F = hdr[1], hdr[4], hdr[5], hdr[6]
    p = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("<3i", model_bytes, p)
        p += 12 + 4 * V
        if version == 2:
            p += 4 + 4 * struct.unpack_from("<i", model_bytes, p)[0]
    out = []
    for _ in range(n_iter * K):
        L = struct.unpack_from("<i", model_bytes, p)[0]
        p += 4 + (L - 1) * 28 + L * 12
        out.append(L)
    assert p == len(model_bytes)
    return np.asarray(out).reshape(n_iter, K)


@functools.lru_cache(maxsize=None)
def _case(n, with_mult):
    """the table, its multiplicities (or None) and the oracle's model bytes -- of the EXPANDED table when the rows carry multiplicities"""
    from oracle import oracle as O
    X, y = make_k40(n, seed=211)
    mult = _mult(n, seed=223) if with_mult else None
    Xe, ye = (np.ascontiguousarray(np.repeat(X, mult, axis=1)), np.repeat(y, mult)) if with_mult else (X, y)
    ref = O.train(Xe, CARDS8, ye, K40, **KW).save()
    leaves = tree_leaves(ref)
    assert (leaves[:, 0] == 1).all(), "class 0 is meant to be finished at the root"
    assert (leaves[:, 2:] > 16).all() and (leaves[:, 1] > 4).all(), "the other class trees are meant to grow"
    return X, y, mult, ref


def _train(X, y, mult, env, kw=KW):
    from repair import _native as N
    table = np.ascontiguousarray(np.concatenate([X, y[None, :]], axis=0))
    with _env(RGBM_GROWER="level", RGBM_DISTINCT="0", **env):
        tab = N.Table(table, np.append(CARDS8, K40).astype(np.int32))
        if mult is not None:
            tab.set_row_multiplicity(mult)
        return tab.train(8, list(range(8)), **kw).save()


SETUPS = [
    ("40 class trees in one workgroup", dict()),
    ("groups of 16, 16, 8", dict(RGBM_MT_TREES=16)),
    ("replicated form everywhere", dict(RGBM_MT_ROT=0)),
    ("rotated form everywhere", dict(RGBM_MT_ROT=1)),
    ("rotated, groups of 16, 16, 8", dict(RGBM_MT_ROT=1, RGBM_MT_TREES=16)),
    ("no sparse sweep", dict(RGBM_MT_SPARSE=0)),
    ("sparse sweep, one class tree per workgroup", dict(RGBM_MT_SPARSE=1, RGBM_MT_TREES=1)),
    ("small LDS: several windows per level", dict(RGBM_LV_LDS=70000)),
    ("small LDS, rotated", dict(RGBM_LV_LDS=70000, RGBM_MT_ROT=1)),
]


@pytest.mark.parametrize("with_mult", [False, True], ids=["rows", "multiplicities"])
@pytest.mark.parametrize("name,env", SETUPS, ids=[s[0] for s in SETUPS])
def test_many_and_mixed_class_trees_per_workgroup(name, env, with_mult):
    X, y, mult, ref = _case(30000, with_mult)
    assert _train(X, y, mult, env) == ref, name


@pytest.mark.parametrize("with_mult", [False, True], ids=["rows", "multiplicities"])
@pytest.mark.parametrize("env", [dict(), dict(RGBM_MT_ROT=1), dict(RGBM_LV_LDS=70000)], ids=["default", "rotated", "small LDS"])
def test_empty_row_blocks_flush_zeros(env, with_mult):
    """3 000 rows are 12 wave tiles; 24 row blocks per class tree leave half of the workgroups without a row"""
    from oracle import oracle as O
    X, y = make_k40(3000, seed=227)
    mult = _mult(3000, seed=229) if with_mult else None
    Xe, ye = (np.ascontiguousarray(np.repeat(X, mult, axis=1)), np.repeat(y, mult)) if with_mult else (X, y)
    ref = O.train(Xe, CARDS8, ye, K40, **KW_SMALL).save()
    assert tree_leaves(ref).max() > 8
    assert _train(X, y, mult, dict(RGBM_MT_BLOCKS=24, RGBM_LV_BLOCKS=24, **env), KW_SMALL) == ref


@pytest.mark.parametrize("env", [dict(), dict(RGBM_MT_ROT=1), dict(RGBM_MT_ACC2=0), dict(RGBM_LV_LDS=70000)], ids=["default", "rotated", "one pass per chunk", "small LDS"])
def test_two_chunk_forms_share_the_prologue(env):
    """20 features, 20 000 rows, K = 5: the wave-specialised both-chunk pass (768 threads, two layout rows per feature index) and the pass per chunk"""
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(233)
    n = 20000
    y = rng.integers(0, 5, n).astype(np.int32)
    cards = np.asarray([3 + (5 * j) % 17 for j in range(20)], np.int32)
    X = np.ascontiguousarray(np.stack([np.where(rng.random(n) < 0.6, (y * (j + 2) + (y >> 1)) % c, rng.integers(0, c, n)).astype(np.int32) for j, c in enumerate(cards)]))
    kw = dict(objective=1, num_class=5, n_estimators=3, learning_rate=0.3)
    ref = O.train(X, cards, y, 5, **kw).save()
    with _env(RGBM_GROWER="level", **env):
        assert N.train(X, cards, y, 5, **kw).save() == ref
