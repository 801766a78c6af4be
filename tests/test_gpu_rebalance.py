"""-m gpu: rgbm_table_smoten / rgbm_table_concat (csrc/rgbm_smoten.hip) against the numpy statement repair/rebalance_codes.py -- neighbour
lists and synthetic rows are integers, so equality -- at the edges of the kernels' tiles, splits and routes, every refusal of the entry, and
`RepairModel.run()` with rebalancing on the resident table through the HIP engine against the value-space path."""
import numpy as np
import pandas as pd
import pytest

from repair.rebalance_codes import smoten_codes
from tests import rebalance_cases as RC
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

TABLE_CODES = csrc_constant("VDM_TABLE_CODES")
QUERY_TILE = csrc_constant("VDM_QUERY_TILE")
CAND_TILE = csrc_constant("VDM_CAND_TILE")
ERR_PARAM = -2


def _class_sized(seed, m, others, n_codes, K):
    """A random table whose class 0 has exactly m rows (the other classes share `others` rows), in random row order."""
    codes, nc = RC.random_table(seed, m + others, n_codes, K)
    rng = np.random.default_rng(seed + 1000)
    y = np.concatenate([np.zeros(m, np.int64), 1 + rng.integers(0, K - 1, others)])
    codes[-1] = rng.permutation(y)
    return codes, nc


def _read(tab):
    return np.stack([tab.read_column(j) for j in range(tab.c)])


def _check(codes, n_codes, classes, n_new, k=5, fit_rows=None, feat_cols=None, target_col=None, picks=None):
    """Device == statement: neighbour lists and synthetic rows.  Returns the statement's result."""
    from repair import _native as N
    c = codes.shape[0]
    target_col = c - 1 if target_col is None else target_col
    feat_cols = [j for j in range(c) if j != target_col] if feat_cols is None else list(feat_cols)
    fit_rows = np.arange(codes.shape[1]) if fit_rows is None else np.asarray(fit_rows, np.int64)
    y = codes[target_col, fit_rows]
    targets = {int(cl): int((y == cl).sum()) + int(nn) for cl, nn in zip(classes, n_new)}
    want = smoten_codes(codes, n_codes, target_col, feat_cols, fit_rows, targets, k=k, picks=picks)
    assert [r["klass"] for r in want] == [int(cl) for cl in classes]
    pick_off = np.concatenate([[0], np.cumsum(n_new)]).astype(np.int64)
    tab = N.Table(codes, n_codes)
    got, nn = tab.smoten(target_col, feat_cols, fit_rows, classes, pick_off, np.concatenate([r["picks"] for r in want]), k=k, want_nn=True)
    for r, g in zip(want, nn):
        bad = np.flatnonzero((r["nn"] != g).any(axis=1))
        assert len(bad) == 0, "class %d: %d of %d neighbour lists differ, e.g. row %d: %s, statement %s" % (
            r["klass"], len(bad), len(g), bad[0], g[bad[0]].tolist(), r["nn"][bad[0]].tolist())
    assert np.array_equal(_read(got).T, np.concatenate([r["synth"] for r in want]))
    assert got.n == int(pick_off[-1]) and got.c == c and np.array_equal(got.n_codes, n_codes)
    return want


@pytest.mark.parametrize("m", sorted({6, 63, 64, 65, CAND_TILE - 1, CAND_TILE, CAND_TILE + 1, QUERY_TILE - 1, QUERY_TILE, QUERY_TILE + 1}))
def test_class_sizes_at_the_tile_edges(m):
    codes, nc = _class_sized(m, m, 90, [4, 3, 5], 3)
    _check(codes, nc, [0], [9])


def test_candidate_split_merge_and_launch_split(monkeypatch):
    """m about 1 100: five query tiles, so the candidates are split by default; then a forced odd split, a single split, and one query tile
    per launch through the environment hook -- all the same lists."""
    codes, nc = _class_sized(7, 1100, 700, [5, 4, 6, 3], 4)
    _check(codes, nc, [0], [40])
    for splits, pairs in (("7", None), ("1", None), (None, "1"), ("3", "1")):
        if splits is not None:
            monkeypatch.setenv("RGBM_VDM_SPLITS", splits)
        else:
            monkeypatch.delenv("RGBM_VDM_SPLITS", raising=False)
        if pairs is not None:
            monkeypatch.setenv("RGBM_VDM_LAUNCH_PAIRS", pairs)
        else:
            monkeypatch.delenv("RGBM_VDM_LAUNCH_PAIRS", raising=False)
        _check(codes, nc, [0], [40])


@pytest.mark.parametrize("F", [1, 15, 16, 17, 31])
def test_feature_counts(F):
    codes, nc = _class_sized(F, 150, 200, [3 + j % 4 for j in range(F)], 3)
    _check(codes, nc, [0], [20])


def test_table_limit_and_single_code_features_in_one_table():
    """V_f = 1, 2, VDM_TABLE_CODES, VDM_TABLE_CODES + 1 and 300 in one table: pair tables and the pair-by-pair route side by side."""
    codes, nc = RC.large_v_table(TABLE_CODES)
    _check(codes, nc, [0, 2], [15, 15])


def test_both_routes_give_the_same_bits():
    """One feature, its dictionary declared at the table limit and one above it: the same codes go through the pair table and through the
    K-term evaluation, and give the same lists."""
    codes, nc = _class_sized(3, 300, 300, [TABLE_CODES], 5)
    a = _check(codes, nc, [0], [10])
    nc2 = nc.copy(); nc2[0] = TABLE_CODES + 1
    b = _check(codes, nc2, [0], [10])
    assert np.array_equal(a[0]["nn"], b[0]["nn"])


@pytest.mark.parametrize("F,V", [(3, 8), (3, TABLE_CODES), (6, TABLE_CODES)])
def test_pair_tables_in_lds_and_through_l2(F, V):
    """24 codes^2 fit the default LDS window, 3 x 64^2 doubles need the enlarged one, 6 x 64^2 doubles do not fit beside the tiles."""
    codes, nc = _class_sized(F * V, 200, 400, [V] * F, 4)
    _check(codes, nc, [0], [12])


@pytest.mark.parametrize("K", [2, 3, 64, 65])
def test_class_counts(K):
    codes, nc = _class_sized(K, 120, 6 * K + 100, [4, 70, 3], K)
    _check(codes, nc, [0], [11])


def test_a_class_code_without_rows_and_several_classes_in_one_call():
    codes, nc = RC.random_table(21, 500, [4, 5, 3, 6], 6, class_p=[0.3, 0.2, 0.0, 0.25, 0.15, 0.1])
    assert not (codes[-1] == 2).any()
    _check(codes, nc, [0, 1], [5, 17])
    _check(codes, nc, [1, 3, 5], [30, 1, 8])


def test_ties_and_identical_rows():
    codes, nc = RC.tie_table()
    _check(codes, nc, [0], [25])
    codes, nc = RC.identical_table()
    r, = _check(codes, nc, [0], [6])
    m = len(r["nn"])
    assert (r["nn"] == np.asarray([[j for j in range(7) if j != q][:5] for q in range(m)])).all()


@pytest.mark.parametrize("k", [1, 8, 9, 16])
def test_k_at_both_ends(k):
    codes, nc = _class_sized(k, 90, 120, [4, 3, 5, 2], 3)
    _check(codes, nc, [0], [14], k=k)
    codes, nc = _class_sized(k + 50, k + 1, 60, [4, 3], 3)              # m = k + 1: every other row is a neighbour
    _check(codes, nc, [0], [3], k=k)


def test_one_new_row_and_every_pick_the_same_row():
    codes, nc = _class_sized(5, 70, 100, [4, 3, 5], 3)
    _check(codes, nc, [0], [1])
    _check(codes, nc, [0], [13], picks={0: np.full(13, 69)})
    _check(codes, nc, [0], [4], picks={0: np.zeros(4, np.int64)})


def test_fit_rows_in_any_order_beside_rows_with_nulls():
    """The fit rows are a shuffled subset; the other rows hold NULLs, which the entry must never read as codes.  A column that is neither
    the target nor a feature comes out NULL."""
    codes, nc = RC.random_table(33, 900, [4, 5, 3, 6, 2], 4)
    rng = np.random.default_rng(34)
    dirty = rng.choice(900, 250, replace=False)
    codes[rng.integers(0, 6, 250), dirty] = -1
    codes[4] = -1                                                         # a column outside the call: all NULL
    fit = rng.permutation(np.setdiff1d(np.arange(900), dirty))
    assert not (np.diff(fit) > 0).all()
    want = _check(codes, nc, [0, 2], [20, 9], fit_rows=fit, feat_cols=[3, 0, 2], target_col=5)
    assert (want[0]["synth"][:, [1, 4]] == -1).all()


def test_five_thousand_fit_rows():
    codes, nc = RC.random_table(41, 5000, [6, 5, 4, 7, 3, 8], 4, class_p=[0.45, 0.25, 0.2, 0.1])
    _check(codes, nc, [2, 3], [50, 50])


def test_refusals_leave_the_table_usable():
    from repair import _native as N
    codes, nc = _class_sized(9, 40, 80, [4, 3], 4)
    codes[-1, np.flatnonzero(codes[-1] == 3)[4:]] = 2                       # class 3 keeps four rows
    tab = N.Table(codes, nc)
    fit = np.arange(codes.shape[1])
    ok = dict(target_col=2, feat_cols=[0, 1], fit_rows=fit, classes=[0], pick_off=[0, 2], picks=[0, 39], k=5)

    def refused(**kw):
        with pytest.raises(N.RepairGbmError) as e:
            tab.smoten(**dict(ok, **kw))
        assert e.value.code == ERR_PARAM, str(e.value)
        assert tab.smoten(**ok).n == 2                                     # the table goes on working

    refused(k=0)
    refused(k=17)
    refused(classes=[3], k=4)                                              # m = 4 <= k
    refused(classes=[3])
    refused(picks=[0, 40])
    refused(picks=[-1, 0])
    refused(feat_cols=[0, 0])
    refused(feat_cols=[0, 2])
    with_null = codes.copy(); with_null[0, 7] = -1; with_null[2, 11] = -1
    tab2 = N.Table(with_null, nc)
    for rows in (fit, np.setdiff1d(fit, [7]), np.setdiff1d(fit, [11])):
        with pytest.raises(N.RepairGbmError) as e:
            tab2.smoten(**dict(ok, fit_rows=rows))
        assert e.value.code == ERR_PARAM and "NULL" in str(e.value)
    assert tab2.smoten(**dict(ok, fit_rows=np.setdiff1d(fit, [7, 11]), picks=[0, 37])).n == 2
    big = N.Table(codes, np.asarray([1 << 20, 3, 1 << 9], np.int32))       # P of the first feature alone: 2^29 entries
    with pytest.raises(N.RepairGbmError) as e:
        big.smoten(**ok)
    assert e.value.code == ERR_PARAM and "2^28" in str(e.value)


def test_concat_is_np_concatenate_and_inherits_kinds_and_values():
    from repair import _native as N
    codes, nc = RC.random_table(51, 700, [4, 5, 3], 3)
    codes[1, ::7] = -1
    tab = N.Table(codes, nc)
    tab.set_column_kind(0, True)
    tab.set_column_values(2, [0.5, 1.5, 4.0])
    a, b, c = tab.gather_rows(np.arange(300, 700)), tab.gather_rows([5]), tab.gather_rows(np.arange(257))
    ab = N.Table.concat([a, b])
    assert np.array_equal(_read(ab), np.concatenate([codes[:, 300:700], codes[:, [5]]], axis=1))
    # the result carries the kinds and values of its parts: it concatenates with another table that does, and not with one that does not
    abc = N.Table.concat([ab, c, ab])
    assert np.array_equal(_read(abc), np.concatenate([_read(ab), codes[:, :257], _read(ab)], axis=1))
    assert np.array_equal(_read(N.Table.concat([c])), codes[:, :257])
    plain = N.Table(codes[:, :10], nc)
    other_codes = N.Table(codes[:, :10], nc + 1)
    narrow = N.Table(codes[:3, :10], nc[:3])
    for bad in (plain, other_codes, narrow):
        with pytest.raises(N.RepairGbmError) as e:
            N.Table.concat([ab, bad])
        assert e.value.code == ERR_PARAM
    assert N.Table.concat([b, b]).n == 2


def test_the_rebalanced_training_table_is_the_value_space_frame_encoded():
    from repair import _native as N
    from repair.pipeline import rebalanced_training_table
    from repair.train import rebalance_training_data
    for name in ("four_class", "numeric", "none_below", "none_above"):
        X, y = RC.VALUE_FRAMES[name]()
        Xr, yr = rebalance_training_data(X.copy(), y.copy(), "t")
        codes, nc, dicts, cols = RC.encode(X, y)
        out, _ = rebalanced_training_table(N.Table(codes, nc), len(cols) - 1)
        got, want = RC.decode(_read(out), dicts), RC.frame_values(Xr, yr)
        assert got.shape == want.shape and (got == want).all(), name


def _run_model(df, resident, **opts):
    from repair.errors import NullErrorDetector
    from repair.model import RepairModel
    m = RepairModel().setInput(df).setRowId("tid").setErrorDetectors([NullErrorDetector()]).setTargets(["y"])
    m = m.setTrainingDataRebalancingEnabled(True)
    for k, v in dict({"model.hp.max_evals": "1", "model.lgb.n_estimators": "10", "model.lgb.learning_rate": "0.2",
                      "model.rebalance.resident": "true" if resident else "false"}, **opts).items():
        m = m.option(k, str(v))
    return m


@pytest.mark.parametrize("max_rows", [10000, 300])
def test_run_with_rebalancing_on_the_resident_table(max_rows):
    """`setTrainingDataRebalancingEnabled(True)` through the HIP engine: with `model.rebalance.resident` the run stays on the resident path and
    gives the cells of the same run with the option off (the value-space path with the HIP estimators), with and without the row sample."""
    from repair.engine import HipEngine
    df = RC.skewed_run_frame()
    opts = {"model.max_training_row_num": max_rows}
    slow = _run_model(df, False, **opts)
    slow._engine_override = HipEngine(0)
    a = slow.run()
    assert getattr(slow, "_last_resident_info", None) is None
    fast = _run_model(df, True, **opts)
    fast._engine_override = HipEngine(0)
    b = fast.run()
    info = getattr(fast, "_last_resident_info", None)
    assert info is not None, "the run did not take the resident path"
    assert info["rebalanced"]["y"]["synthetic"] > 0
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(a.sort_values(key).reset_index(drop=True), b.sort_values(key).reset_index(drop=True))
    assert len(a) >= 40
