"""-m gpu: the last level pass (k_level_final, csrc/rgbm_level.h) at every row-count residue and score alignment.

The scores are [K][N] with stride N, so class tree k's scores start at 8 mod 16 bytes when N and k are both odd: those class trees take the
8 + 16 + 8 byte load form, the others the 16 + 16 one, and only the last, incomplete group of four rows the scalar path.  Rows with
multiplicities take the routing bin and the multiplicity out of ONE record fetch when the split feature lives in the last chunk, out of two
loads otherwise.  Every case trains max_depth = 7 trees for five iterations (a wrong score of iteration t changes the trees of t + 1) and must
give the oracle's model byte for byte; every case also asserts that the oracle's model has a leaf at depth 7 in a tree of an ODD class index,
i.e. that the pass really routed rows of a misaligned class tree (the binary target, one tree and always aligned, is the control).
Reference semantics pinned: the model of python/repair/train.py:102-131 (LightGBM: Tree::Split of the last level + ScoreUpdater::AddScore)."""
import struct

import numpy as np
import pytest

from tests.synth import make_table, balanced_weights

pytestmark = pytest.mark.gpu

PARAMS = dict(n_estimators=5, learning_rate=0.2, max_depth=7, num_leaves=48, min_data_in_leaf=3)
T_BINARY, T_FEW, T_MANY = 0, 1, 6           # cardinalities 2, 3, 16 (repair.synth.CARDS): k_grad<0>, k_grad_mc_rows, k_grad_mc
N_MAX = 12292
_tables, _oracle = {}, {}


def _env(monkeypatch, distinct="0"):
    monkeypatch.setenv("RGBM_SMALL_ROWS", "0")
    monkeypatch.setenv("RGBM_GROWER", "level")
    monkeypatch.setenv("RGBM_DISTINCT", distinct)


def _table(cols):
    """the first N rows of ONE table per column count serve every row count"""
    if cols not in _tables:
        dirty, _, cards = make_table(N_MAX, cols, seed=1201, null_ratio=0.01)
        _tables[cols] = (dirty, cards)
    return _tables[cols]


def _kw(dirty, cards, t, **over):
    K = int(cards[t])
    return dict(dict(PARAMS, objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=balanced_weights(dirty[t], K)), **over)


def _oracle_blob(key, dirty, cards, t, kw):
    if key not in _oracle:
        from oracle import oracle as O
        feats = [c for c in range(dirty.shape[0]) if c != t]
        r = dirty[t] >= 0
        _oracle[key] = O.train(np.ascontiguousarray(dirty[feats][:, r]), cards[feats], dirty[t][r], int(cards[t]), **kw).save()
    return _oracle[key]


def parse_trees(blob):
    """(K, [tree dict]) of a saved model: the layout of rgbm_model_save (tests/tree_walk.py `blob` writes the same one)"""
    magic, ver, _, _, K, n_iter, F = struct.unpack_from("<7i", blob, 0)
    assert magic == 0x4D424752 and ver in (1, 2)
    o = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("<3i", blob, o)
        o += 12 + 4 * V
        if ver == 2:
            o += 4 + 4 * struct.unpack_from("<i", blob, o)[0]
    trees = []
    for _ in range(K * n_iter):
        L = struct.unpack_from("<i", blob, o)[0]
        o += 4
        n = L - 1
        t = {}
        for name in ("feat", "theta", "dleft", "left", "right"):
            t[name] = np.frombuffer(blob, "<i4", n, o)
            o += 4 * n
        o += 8 * n + 8 * L + 4 * L              # gain, leaf_value, leaf_count
        t["L"] = L
        trees.append(t)
    assert o == len(blob)
    return K, trees


def last_level_splits(t, depth=7):
    """the split features of the nodes at depth - 1 that have a LEAF child (at `depth`): the nodes the last routing step routes"""
    out = []
    if t["L"] <= 1:
        return out
    stack = [(0, 0)]
    while stack:
        j, d = stack.pop()
        for ch in (int(t["left"][j]), int(t["right"][j])):
            if ch >= 0:
                stack.append((ch, d + 1))
            elif d + 1 == depth:
                out.append(int(t["feat"][j]))
    return out


def routed_features(blob, odd_only=True):
    """split features of the last routing step over the class trees of odd index (every tree of a one-tree model)"""
    K, trees = parse_trees(blob)
    return [f for i, t in enumerate(trees) if (K == 1 or not odd_only or (i % K) % 2 == 1) for f in last_level_splits(t)]


def _check(tab, dirty, cards, t, key, whole=None, need_chunks=(), **over):
    kw = _kw(dirty, cards, t, **over)
    feats = [c for c in range(dirty.shape[0]) if c != t]
    ref = _oracle_blob(key, dirty, cards, t, kw)
    fs = routed_features(ref)
    assert fs, "the case no longer routes a row of an odd class tree at the last level"
    for ch in need_chunks:
        assert any(f >> 4 == ch for f in fs), "no last-level split on a feature of chunk %d" % ch
    got = tab.train(t, feats, **kw).save()
    if whole is not None:
        assert got == whole.train(t, feats, **kw).save(), "distinct rows with multiplicities differ from the whole table"
    assert got == ref, "HIP model differs from the oracle"


@pytest.mark.parametrize("target", [T_BINARY, T_FEW, T_MANY])
@pytest.mark.parametrize("rows", [12289, 12290, 12291, 12292])
def test_row_count_residues(rows, target, monkeypatch):
    from repair import _native as N
    _env(monkeypatch)
    dirty, cards = _table(16)
    dirty = np.ascontiguousarray(dirty[:, :rows])
    _check(N.Table(dirty, cards), dirty, cards, target, ("rows", rows, target))


def _with_repeats(cols, rows, rep):
    """`rows` rows (odd) of which the last `rep` repeat earlier ones; an ODD number of distinct rows"""
    from repair import _native as N
    from repair.pipeline import distinct_rows
    base, cards = _table(cols)
    for drop in (0, 1):
        dirty = np.ascontiguousarray(np.concatenate([base[:, :rows - rep - drop], base[:, 100:100 + rep + drop]], axis=1))
        dist, mult, inv = distinct_rows(dirty, cards)
        if dist.shape[1] % 2 == 1:
            break
    assert dirty.shape[1] == rows and rows % 2 == 1 and dist.shape[1] % 2 == 1 and dist.shape[1] < rows
    assert int(mult.sum()) == rows and np.array_equal(dist[:, inv], dirty)
    tab = N.Table(dist, cards)
    tab.set_row_multiplicity(mult)
    return dirty, cards, tab


@pytest.mark.parametrize("target", [T_FEW, T_MANY])
def test_multiplicities_at_an_odd_distinct_row_count(target, monkeypatch):
    from repair import _native as N
    _env(monkeypatch)
    dirty, cards, tab = _with_repeats(16, 12291, 3000)
    _check(tab, dirty, cards, target, ("mult", 16, target), whole=N.Table(dirty, cards))


@pytest.mark.parametrize("target", [T_FEW, T_MANY])
def test_two_chunks_at_odd_n(target, monkeypatch):
    from repair import _native as N
    _env(monkeypatch)
    dirty, cards = _table(24)
    dirty = np.ascontiguousarray(dirty[:, :12291])
    _check(N.Table(dirty, cards), dirty, cards, target, ("chunks", target), need_chunks=(0, 1))


@pytest.mark.parametrize("target", [T_FEW, T_MANY])
def test_two_chunks_with_multiplicities_at_odd_n(target, monkeypatch):
    from repair import _native as N
    _env(monkeypatch)
    dirty, cards, tab = _with_repeats(24, 12291, 3000)          # 23 features: the multiplicity rides in the second record, splits come from both
    _check(tab, dirty, cards, target, ("mult", 24, target), whole=N.Table(dirty, cards), need_chunks=(0, 1))


@pytest.mark.parametrize("target", [T_FEW, T_MANY])
def test_bagging_at_odd_n(target, monkeypatch):
    from repair import _native as N
    _env(monkeypatch)
    dirty, cards = _table(16)
    dirty = np.ascontiguousarray(dirty[:, :12291])
    _check(N.Table(dirty, cards), dirty, cards, target, ("bag", target), bagging_fraction=0.5, bagging_freq=1)
