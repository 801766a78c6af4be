"""-m gpu: every kernel of the predictor against a plain tree walk, on hand-built models that sit on its edges.  Every comparison is
exact: the float64 bits and the labels.

`predict_device` (csrc/rgbm.hip) launches one of ten kernel instantiations, chosen by `predict_form` from the model's table size: eight
fixed-stride scorers `k_predict_qs<MW, FMAX, TW, TBN>`, the dynamic-stride scorer with 8 .. 1 trees per LDS stage, or the walk
`k_predict_raw<one chunk | more>`; `k_softmax_argmax` and `k_fill_cells` finish.  Trained models (tests/test_gpu_predictor.py) cannot be
steered to the places where these can be wrong; the models of tests/predictor_form_cases.py are built there: stage loops at n_iter = 1, TBN,
TBN + 1, 2 TBN, 2 TBN + 1, 4 TBN + 3; table sizes on both sides of every turn-over of the rule, the silent fall to the walk included; exit
leaves 0, 31, 32, 63, 64 of chains and random shapes; every feature index 0 .. 32; theta = -1 and V - 1, V = 1 and 255, both default
directions on NULLs, out-of-dictionary codes and unseen categories; stumps; ties, raw 0 and saturating scores; 1 .. 1100 rows around the
256-row and 512-row ownership of a workgroup.  Each case first asserts that `Model.predict_form()` names the kernel it is built for.

The reference is tests/tree_walk.py, which tests/test_tree_walk_cpu.py holds to `OracleModel.predict` bit for bit on the same models: a
mismatch here is a fault of that form's kernel or of its table builder (`device_model`).
"""
import functools

import numpy as np
import pytest

from tests import predictor_form_cases as PC
from tests import tree_walk as W

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 511, 512, 513, 1100)
FORCED = ({"RGBM_QS_FIXED": "0"}, {"RGBM_PREDICTOR": "walk"})


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(blob, X, walk's output for all rows, its labels, its top probabilities): computed once per case; rows are independent, so the
    answer for the first n rows is the first n rows of the answer"""
    m, X = PC.BY_NAME[name].make()
    want = W.predict(m, X)
    lab, top = W.label_top(m, want)
    for a in (X, want, lab, top):
        a.setflags(write=False)
    return W.blob(m), X, want, lab, top


def _check_rows(model, X, want, what):
    for n in SIZES:
        got = model.predict(np.ascontiguousarray(X[:, :n]))
        assert got.shape == want[:n].shape
        bad = np.flatnonzero((_bits(got) != _bits(want[:n])).any(axis=1))
        assert bad.size == 0, "%s, n = %d: %d rows differ, the first at row %d: got %r, want %r" % (what, n, bad.size, bad[0], got[bad[0]][:4], want[bad[0]][:4])


def _check_labels(model, m_info, X, lab, top, what):
    """the chain's outputs for one model: label (first maximum) and its probability, and the NULL target column filled with the labels"""
    from repair import _native as N
    F, n = X.shape
    table = np.ascontiguousarray(np.vstack([X, np.full((1, n), -1, np.int32)]))
    ncls = m_info["num_class"] if m_info["objective"] != 2 else 0
    got_lab, got_top = N.repair_chain([model], [F], [list(range(F))], [list(range(ncls))], table)
    assert np.array_equal(got_lab[0], lab), what
    assert np.array_equal(_bits(got_top[0]), _bits(top)), what
    assert np.array_equal(table[F], lab if ncls else np.full(n, -1, np.int32)), what
    assert np.array_equal(table[:F], X), what


@pytest.mark.parametrize("name", [c.name for c in PC.CASES])
def test_predictor_form_gives_the_tree_walk_bits(name, monkeypatch):
    from repair import _native as N
    case = PC.BY_NAME[name]
    blob, X, want, lab, top = _reference(name)
    mg = N.Model.load(blob)
    pf = mg.predict_form()
    assert (pf["form"], pf["MW"], pf["TW"], pf["tb"]) == case.form           # the kernel this case is built for
    info = mg.info()
    _check_rows(mg, X, want, "default form %r" % (case.form,))
    _check_labels(mg, info, X, lab, top, "default form %r" % (case.form,))
    for env in FORCED:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        forced = mg.predict_form()
        assert forced["form"] == "walk" if "RGBM_PREDICTOR" in env else forced["form"] != "fixed"
        fresh = N.Model.load(blob)
        _check_rows(fresh, X, want, "forced %s (%s) on a fresh model" % (env, forced))
        _check_rows(mg, X, want, "forced %s (%s) on a model whose tables exist" % (env, forced))
        _check_labels(mg, info, X, lab, top, "forced %s" % env)
        for k in env:
            monkeypatch.delenv(k)
    assert mg.predict_form() == pf
    _check_rows(mg, X, want, "default form again")


# ---------------------------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("env", [{}] + list(FORCED), ids=["default", "dynamic", "walk"])
@pytest.mark.parametrize("row_begin", [0, 1, 257])
def test_chain_on_a_row_window_of_the_resident_table(row_begin, env, monkeypatch):
    """Table.repair_chain on rows [row_begin, row_begin + n_rows) of a longer table (k_pack_bins with row0 != 0 and Ntab != n), feature
    lists in no column order, the second model reading the column the first one fills: labels and top probabilities of the walk and of
    the oracle's chain; cells that held a value keep it; rows outside the window are untouched."""
    from oracle import oracle as O
    from repair import _native as N
    models, targets, feat_cols, class_codes, table = PC.chain_setup()
    n_rows = 700
    assert row_begin + n_rows < table.shape[1]
    window = np.ascontiguousarray(table[:, row_begin:row_begin + n_rows])
    by_walk, by_oracle = window.copy(), window.copy()
    lab_w, top_w = W.repair_chain(models, targets, feat_cols, class_codes, by_walk)
    lab_o, top_o = O.repair_chain([O.OracleModel.load(W.blob(m)) for m in models], targets, feat_cols, class_codes, by_oracle)
    assert np.array_equal(lab_w, lab_o) and np.array_equal(_bits(top_w), _bits(top_o)) and np.array_equal(by_walk, by_oracle)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gm = [N.Model.load(W.blob(m)) for m in models]
    tab = N.Table(table, [6, 2, 9, 7, 3, 5])
    lab_g, top_g = tab.repair_chain(gm, targets, feat_cols, row_begin=row_begin, n_rows=n_rows)
    assert np.array_equal(lab_g, lab_w) and np.array_equal(_bits(top_g), _bits(top_w))
    after = table.copy()
    after[:, row_begin:row_begin + n_rows] = by_walk
    for c in range(table.shape[0]):
        assert np.array_equal(tab.read_column(c), after[c]), c
    held = table >= 0
    assert np.array_equal(after[held], table[held]) and (after[4] != table[4]).any() and (after[1] != table[1]).any()


def test_chain_leaves_a_cell_null_when_its_label_has_no_class_code():
    from repair import _native as N
    models, targets, feat_cols, _, table = PC.chain_setup()
    cc = [[2, 0], [1, 0]]                                    # model 0 has three classes: label 2 has no code
    want_t, got_t = table.copy(), table.copy()
    lab_w, top_w = W.repair_chain(models, targets, feat_cols, cc, want_t)
    lab_g, top_g = N.repair_chain([N.Model.load(W.blob(m)) for m in models], targets, feat_cols, cc, got_t)
    assert np.array_equal(lab_g, lab_w) and np.array_equal(_bits(top_g), _bits(top_w)) and np.array_equal(got_t, want_t)
    no_code = (lab_w[0] == 2) & (table[4] < 0)
    assert no_code.any() and (got_t[4][no_code] == -1).all()
