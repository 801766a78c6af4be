"""-m gpu: the comparison rules of the split search and of the best-first order -- which of two equal gains wins, and on which side of `<`
every limit lies -- on the tables of tests/split_cases.py, where a tie or a limit decides the tree (tests/test_split_cases_cpu.py shows
that on the CPU oracle and a plain restatement of LightGBM's rules).  Every case: 3 iterations at learning_rate 0.5; the model bytes must
equal the CPU oracle's, no tolerance.

The rules are written out several times on the device (scan_child and reduce_leaf_best / tree_step_pick in csrc/rgbm_kernels.h,
scan_child_packed in csrc/rgbm_small.h, k_level_step and k_level_replay's selection loop in csrc/rgbm_level.h, the 2 min_data_in_leaf
gates on the host and the device), so every case runs on every route it is eligible for:

  leafwise                       RGBM_GROWER=leafwise (k_split_find: one wave per feature)
  level                          RGBM_GROWER=level (k_level_step: packed scan out of LDS; k_level_replay)
  level, scan out of the pool    level with RGBM_STEP_READBACK=1
  level, row multiplicities      the table's distinct rows with their multiplicities; the oracle trains on the expanded table
  fused batch                    all cases in one train_batch call (k_small_tree, packed scan)
  fused batch, one wave a feature  the same call under RGBM_SMALL_PACKED=0 (scan_child)

The three routes that go through a resident table take no per-row weights: the two count-estimate cases run on the first three only.
A table with row multiplicities trains with at most 32 features (two chunks, the last not full): the nine feature-tie cases with 34 and
72 features are not eligible for that route.
The single-fit routes run without the distinct-row view (RGBM_DISTINCT=0); every case keeps max_depth in 1..7."""
import functools

import numpy as np
import pytest

from tests import split_cases as S
from tests.test_gpu_growers import _env

pytestmark = pytest.mark.gpu

HOST_ROUTES = S.HOST_ROUTES
HOST_NODES, MULT_NODES, BATCH_NAMES = S.host_nodes(), S.mult_nodes(), S.batch_names()       # eligible (route, case) combinations only


@functools.lru_cache(maxsize=None)
def _oracle(name):
    return S.by_name(name).oracle().save()


@functools.lru_cache(maxsize=None)
def _oracle_expanded(name):
    """the distinct rows, their multiplicities and the oracle's model of the expanded table"""
    c = S.by_name(name)
    T, mult = c.distinct_rows()
    E = np.ascontiguousarray(np.repeat(T, mult, axis=1))
    return T, mult, c.oracle(np.ascontiguousarray(E[:-1]), np.ascontiguousarray(E[-1])).save()


@pytest.mark.parametrize("route,name", HOST_NODES, ids=["%s-%s" % n for n in HOST_NODES])
def test_single_fit_route_gives_the_oracle_model(route, name):
    from repair import _native as N
    c = S.by_name(name)
    with _env(RGBM_DISTINCT="0", **dict(HOST_ROUTES)[route]):
        got = N.train(c.X, c.cards, c.y_code, c.n_y, y_value=c.y_value, sample_weight=c.weights, **c.params).save()
    assert got == _oracle(name), "%s, %s" % (name, route)


@pytest.mark.parametrize("name", MULT_NODES)
def test_level_grower_with_row_multiplicities_gives_the_oracle_model_of_the_expanded_table(name):
    from repair import _native as N
    c = S.by_name(name)
    T, mult, ref = _oracle_expanded(name)
    F = T.shape[0] - 1
    with _env(RGBM_GROWER="level", RGBM_DISTINCT="0"):
        tab = N.Table(T, c.table_codes()[1])
        tab.set_row_multiplicity(mult)
        got = tab.train(F, list(range(F)), y_value=c.y_value, **c.params).save()
    assert got == ref, name
    assert ref == _oracle(name), "%s: the expanded table is the case's table up to row order" % name


@pytest.mark.parametrize("packed", [True, False], ids=S.BATCH_IDS)
def test_fused_batch_gives_the_oracle_models(packed, monkeypatch):
    from repair import _native as N
    if not packed:
        monkeypatch.setenv("RGBM_SMALL_PACKED", "0")
    fits = [S.by_name(n) for n in BATCH_NAMES]
    specs = []
    for c in fits:
        T, cards = c.table_codes()
        F = T.shape[0] - 1
        specs.append(dict(table=N.Table(T, cards), target_col=F, feat_cols=list(range(F)), y_value=c.y_value, **c.params))
    out = N.train_batch(specs)
    rep = N.train_batch_report(len(fits))
    # first: every fit took the route this test is about
    for c, r in zip(fits, rep):
        assert r["route"] == 1 and (r["scan_waves"] > 0) == packed, "%s: the report says %r" % (c.name, r)
    wrong = []
    for c, res in zip(fits, out):
        assert not isinstance(res, Exception), "%s failed: %r" % (c.name, res)
        if res.save() != _oracle(c.name):
            wrong.append(c.name)
    assert not wrong, "the batched model differs from the oracle's: %r" % wrong
