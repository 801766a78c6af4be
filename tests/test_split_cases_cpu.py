"""The tables of tests/split_cases.py on the CPU alone: the oracle's first tree (every class tree of iteration 0) equals the plain restatement
of LightGBM's rules (tests/split_restatement.py) node for node -- feature, threshold, default direction, links, the gain's bits, the leaf
counts, and for regression the leaf values bit for bit; `holds` says that the tie or limit a case is named after decides that tree; and
the model's bins are one per code.  tests/test_gpu_split_edges.py then holds every device route to the oracle's bytes on these tables."""
import functools

import numpy as np
import pytest

from tests import batch_cases as B
from tests import split_cases as S
from tests import split_restatement as R

NAMES = [c.name for c in S.cases()]


@functools.lru_cache(maxsize=None)
def _oracle_blob(name):
    return S.by_name(name).oracle().save()


def _trees(name):
    from repair import _native as N
    return N.model_trees(_oracle_blob(name))[2]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64).tolist()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_tree_equals_the_restatement_and_the_edge_decides_it(name):
    c = S.by_name(name)
    trees = _trees(name)
    for k in range(c.class_trees()):
        g, h = c.gh(k)
        tree, trace = R.grow(c.bins(), c.feats(), g, h, used=c.used, **c.grower_params())
        o = trees[k]
        for field in ("feat", "theta", "dleft", "left", "right", "leaf_count"):
            assert o[field].tolist() == tree[field], "%s, class tree %d: %s" % (name, k, field)
        assert _bits(o["gain"]) == _bits(tree["gain"]), "%s, class tree %d: gains %r / %r" % (name, k, o["gain"].tolist(), tree["gain"])
        if c.K == 0 and len(tree["feat"]):
            # Shrinkage: output * learning_rate; the initial score of these tables is exactly 0, so no bias is added
            assert _bits(o["leaf_value"]) == _bits([v * c.params["learning_rate"] for v in tree["leaf_value"]]), name
        if k == 0:
            assert c.holds(c, tree, trace), "%s: the edge does not decide the tree: root candidates %r, picks %r" % (
                name, trace["searches"][0]["best"][:8], trace["picks"][:8])


@pytest.mark.parametrize("name", NAMES)
def test_a_code_is_a_bin(name):
    c = S.by_name(name)
    blob = _oracle_blob(name)
    assert B.blob_bins(blob) == c.feats()
    for f, card in enumerate(c.cards):
        assert B.blob_upper_bounds(blob, f)[:-1].tolist() == list(range(int(card) - 1)), (name, f)


def test_the_two_fits_of_a_limit_give_different_trees():
    assert len(S.LIMIT_PAIRS) >= 12
    for a, b in S.LIMIT_PAIRS:
        ta, tb = _trees(a)[0], _trees(b)[0]
        same = all(ta[k].tolist() == tb[k].tolist() for k in ("feat", "theta", "dleft", "left", "right", "leaf_count"))
        assert not same, "%s / %s" % (a, b)


def test_every_group_of_the_issue_has_its_cases():
    names = set(NAMES)
    assert len(NAMES) == 65
    for V in (5, 9, 130, 254):
        assert "end isolating V=%d alone" % V in names and "end isolating V=%d moved to the next wave" % V in names
    for i, j in S.PAIRS:
        for kind in ("copy", "mirror", "mirror first"):
            assert "feature %d and its %s at %d" % (i, kind, j) in names
    for nl in (64, 65, 100, 128):
        assert "symmetric 7 levels, num_leaves %d" % nl in names
    weighted = [c.name for c in S.cases() if c.weights is not None]
    assert len(weighted) == 2 and all(n.startswith("count estimate") for n in weighted)
    assert all(c.single_fit() for c in S.cases())
    assert [c.name for c in S.cases() if not c.batch()] == weighted
    # routes a case is not eligible for: per-row weights (resident-table routes), more than 32 features (row multiplicities)
    assert [c.name for c in S.cases() if not c.multiplicities()] == [c.name for c in S.cases() if len(c.cards) > 32] + weighted
    assert len(S.gpu_node_ids()) == 3 * 65 + (65 - 9 - 2) + 2
