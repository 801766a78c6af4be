"""GPU: rgbm_table_detect_dc_scan (csrc/rgbm_dc.hip) -- the order constraints by sort and scan -- against the O(n^2) restatement
tests/dc_restatement.py::detect_dc, against the pairs route on the same table where n^2 is out of the restatement's reach, and a whole
`RepairModel.run()` with `error.constraints.order_scan` against the value-space path.  Tables and predicate sets: tests/dc_scan_cases.py."""
import numpy as np
import pandas as pd
import pytest

from tests import dc_restatement as R
from tests import dc_scan_cases as S
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

T = csrc_constant("DC_SCAN_TILE")                     # positions per workgroup of the segmented suffix-max scan
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1]


def _same(got, want):
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and got[0].dtype == np.int64 and got[1].dtype == np.int32
        return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got.dtype == np.int64 and np.array_equal(got, want)


@pytest.mark.parametrize("shape", S.SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_detect_dc_scan_equals_the_restatement(n, shape):
    from repair import _native as N
    codes, n_codes = S.make_table(n, shape, T, seed=3)
    tab = N.Table(codes, n_codes)
    for name, preds in S.pred_sets(n_codes, 3).items():
        want = R.detect_dc(codes, n_codes, preds)
        assert _same(tab.detect_dc_scan(preds), want), (name, n, shape)
        if name in S.NOBODY:
            assert len(want) == 0
        cells = np.tile(want, 2), np.repeat(np.asarray([S.B, S.G], np.int32), len(want))      # the rows x cell_cols, column-major
        assert _same(tab.detect_dc_scan(preds, cell_cols=[S.B, S.G]), cells), (name, n, shape, "cells")


def test_one_group_the_pairs_route_refuses():
    """4097 rows in one group with two order predicates: more pairs than the bound, and no pair is needed."""
    from repair import _native as N
    n = 4097
    codes, n_codes = S.make_table(n, "one", T, seed=5)
    preds = S.pred_sets(n_codes, 5)[S.TWO_ORDER]
    assert R.group_pairs(codes, n_codes, preds) == n * n
    tab = N.Table(codes, n_codes)
    with pytest.raises(N.RepairGbmError) as e:
        tab.detect_dc(preds, max_pairs=n * n - 1)
    assert e.value.code == -2
    want = R.detect_dc(codes, n_codes, preds)
    assert len(want) > 0 and _same(tab.detect_dc_scan(preds), want)


@pytest.mark.parametrize("shape", ["one", "mixed"])
def test_many_tiles_equal_the_numpy_statement_and_the_pairs_route(shape):
    """200 003 rows: the multi-block paths of the sort and of the scan, groups that straddle many tiles."""
    from repair import _native as N
    n = 200003
    codes, n_codes = S.make_table(n, shape, T, seed=7, values=1000)
    tab = N.Table(codes, n_codes)
    found = 0
    for name, preds in S.pred_sets(n_codes, 7).items():
        want = S.scan_statement(codes, n_codes, preds)
        assert _same(tab.detect_dc_scan(preds), want), (name, shape)
        if len(preds) >= 2:                               # (the pairs entry takes two predicates or more)
            assert _same(tab.detect_dc(preds), want), (name, shape, "pairs")
        found += len(want)
    assert found > 0
    cells = S.scan_statement(codes, n_codes, S.pred_sets(n_codes, 7)[S.TWO_ORDER], cell_cols=[S.B, S.G])
    assert _same(tab.detect_dc_scan(S.pred_sets(n_codes, 7)[S.TWO_ORDER], cell_cols=[S.B, S.G]), cells)


@pytest.mark.parametrize("shape", ["one", "three"])
def test_more_tiles_than_one_round_of_the_tile_carry(shape):
    """2 x 256 x T + 1 rows: the one workgroup that joins the tiles' runs takes 256 tiles per round, so these tables need three rounds,
    with groups that lie on both sides of every round's boundary; the one-predicate sets scan the groups' first positions the same way."""
    from repair import _native as N
    n = 2 * 256 * T + 1
    if shape == "three":
        assert S.straddles(S.three_sizes(n), 256 * T)
    codes, n_codes = S.make_table(n, shape, T, seed=9, values=1000)
    tab = N.Table(codes, n_codes)
    sets = S.pred_sets(n_codes, 9)
    found = 0
    for name in ("eq_gt_lt", "eq_gt_lt_ranked", "two_lt_no_eq", "eq_lt_across", "gt_across_alone", "two_eq_gt"):
        want = S.scan_statement(codes, n_codes, sets[name])
        assert _same(tab.detect_dc_scan(sets[name]), want), (name, shape)
        found += len(want)
    assert found > 0


def test_refusals_leave_the_previous_result():
    from repair import _native as N
    codes, n_codes = S.make_table(300, "mixed", T, seed=1)
    tab = N.Table(codes, n_codes)
    ra = S.rank_arrays(n_codes, 1)[0]
    eq, gt, lt, iq = ("EQ", S.G, S.G, None, None), ("GT", S.A, S.A, None, None), ("LT", S.B, S.B, None, None), ("IQ", S.G2, S.G2, None, None)
    before = tab.detect_nulls([S.A, S.B])
    assert len(before[0]) > 0

    def refused(preds, code, **kw):
        with pytest.raises(N.RepairGbmError) as e:
            tab.detect_dc_scan(preds, **kw)
        assert e.value.code == code, preds
        kept = tab._fetch_cells(len(before[0]), True)     # the table's previous result is intact
        assert np.array_equal(kept[0], before[0]) and np.array_equal(kept[1], before[1])

    refused([eq, iq, gt], -2)                             # RGBM_ERR_PARAM: an IQ present
    refused([iq, gt, lt], -2)
    refused([eq, ("EQ", S.G2, S.G2, None, None)], -2)     # no order predicate
    refused([eq, gt, lt, gt], -2)                         # three order predicates
    refused([], -1)                                       # RGBM_ERR_ARG, as rgbm_table_detect_dc gives them
    refused([gt] * 17, -1)
    refused([("EQ", S.A, S.B, None, None), gt], -1)       # EQ across two attributes
    refused([eq, ("IQ", S.A, S.A, ra, ra), gt], -1)       # IQ with rank arrays
    refused([eq, ("LT", S.A, 4, None, None)], -1)         # column out of range
    refused([eq, ("LT", -1, S.A, None, None)], -1)
    refused([eq, gt], -1, cell_cols=[4])
    assert _same(tab.detect_dc_scan([eq, gt, lt]), R.detect_dc(codes, n_codes, [eq, gt, lt]))


def test_run_with_order_scan_equals_the_value_space_run(monkeypatch):
    from repair.errors import ConstraintErrorDetector, NullErrorDetector
    from repair.model import RepairModel
    df = S.small_frame()

    def model(**opts):
        m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(80).setTargets(S.FRAME_TARGETS) \
            .setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints=S.FRAME_CONSTRAINT)])
        for k, v in dict({"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2"}, **opts).items():
            m = m.option(k, v)
        return m

    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = model().run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = model(**{"error.constraints.resident": "true", "error.constraints.order_scan": "true"})
    fast = fm.run()
    assert fm._last_detection_on_device is True and fm._last_resident_info["constraint_routes"] == ["dc_scan"]
    key = ["tid", "attribute"]
    assert len(slow) > 0 and {"Salary", "Tax"} & set(slow["attribute"])
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True), check_exact=True)
