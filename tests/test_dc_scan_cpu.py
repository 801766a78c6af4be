"""CPU: the order constraints that take sort and scan instead of pairs (`error.constraints.order_scan`).

The vectorised numpy statement of tests/dc_scan_cases.py is held to the O(n^2) restatement tests/dc_restatement.py::detect_dc on every
generator case, `repair.dc_codes.scan_eligible` to the forms rgbm_table_detect_dc_scan accepts and refuses, and whole runs on a CPU
engine whose table answers `detect_dc_scan` with the numpy statement to the value-space path."""
import logging

import numpy as np
import pandas as pd
import pytest

from repair import dc_codes as DC
from repair.errors import ConstraintErrorDetector, NullErrorDetector, parse_constraint
from repair.model import RepairModel
from tests import dc_restatement as R
from tests import dc_scan_cases as S
from tests.helpers import csrc_constant
from tests.test_constraints_resident_cpu import DcEngine, DcTable

T = csrc_constant("DC_SCAN_TILE")


@pytest.mark.parametrize("shape", S.SHAPES + ("three",))
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_numpy_statement_equals_the_restatement(n, shape):
    for seed in (0, 1):
        # a tile of 64 puts tile edges (and the groups of `mixed` sized by it) inside these small tables
        codes, n_codes = S.make_table(n, shape, tile=64, seed=seed)
        for name, preds in S.pred_sets(n_codes, seed).items():
            want = R.detect_dc(codes, n_codes, preds)
            got = S.scan_statement(codes, n_codes, preds)
            assert got.dtype == np.int64 and np.array_equal(got, want), (name, n, shape, seed)
            if name in S.NOBODY:
                assert len(want) == 0
            wr, wc = R.detect_dc(codes, n_codes, preds, cell_cols=[S.B, S.G])
            gr, gc = S.scan_statement(codes, n_codes, preds, cell_cols=[S.B, S.G])
            assert np.array_equal(gr, wr) and np.array_equal(gc, wc) and gc.dtype == np.int32


def test_the_cases_find_something():
    codes, n_codes = S.make_table(257, "mixed", tile=64)
    hits = {name: len(S.scan_statement(codes, n_codes, preds)) for name, preds in S.pred_sets(n_codes).items()}
    assert all(v > 0 for k, v in hits.items() if k not in S.NOBODY) and all(hits[k] == 0 for k in S.NOBODY), hits
    sizes, _ = S.group_sizes(200003, T)
    assert sizes == [T + 1, T, T - 1, 65, 64, 63, 2, 1]
    # `three`: whatever the order of the groups, one lies across each boundary between the rounds of the scan's tile carry
    assert S.straddles(S.three_sizes(2 * 256 * T + 1), 256 * T) and not S.straddles([256 * T, 256 * T, 1], 256 * T)


def test_scan_eligible():
    eq = lambda c: ("EQ", c, c, None, None)          # noqa: E731
    gt, lt, iq = ("GT", 1, 1, None, None), ("LT", 2, 3, np.zeros(4, np.int32), np.zeros(4, np.int32)), ("IQ", 4, 4, None, None)
    for preds in ([gt], [lt], [gt, lt], [eq(0), gt], [eq(0), gt, lt], [eq(0), eq(0), eq(5), lt, lt], [eq(c) for c in range(12)] + [gt, lt]):
        assert DC.scan_eligible(preds) is True, preds
    for preds in ([], [eq(0)], [eq(0), eq(5)], [iq, gt], [eq(0), iq, gt, lt], [iq, iq], [gt, lt, gt], [eq(0), gt, gt, gt],
                  [eq(c) for c in range(13)] + [gt], [eq(0)] * 16 + [gt], [("EQ", 0, 5, None, None), gt]):
        assert DC.scan_eligible(preds) is False, preds
    for name, preds in S.pred_sets(np.asarray([3, 5, 5, 3])).items():
        assert DC.scan_eligible(preds), name


def test_lowered_order_constraints_are_eligible_and_unchanged():
    df = S.small_frame()
    cols = [c for c in df.columns if c != "tid"]
    from repair.pipeline import encode_frame
    _, _, dicts = encode_frame(df, cols)
    dt = {c: df[c].dtype for c in cols}
    prog = DC.lower_constraint(parse_constraint(S.FRAME_CONSTRAINT), cols, dicts, dt)
    assert prog["kind"] == "dc" and DC.scan_eligible(prog["preds"])
    two_iq = DC.lower_constraint(parse_constraint("t1&t2&EQ(t1.State,t2.State)&IQ(t1.Kind,t2.Kind)&GT(t1.Tax,t2.Tax)"), cols, dicts, dt)
    assert two_iq["kind"] == "dc" and not DC.scan_eligible(two_iq["preds"])


# ---------------------------------------------------------------------------------------------- whole runs
class ScanTable(DcTable):
    """The CPU table of the resident-constraint tests with `detect_dc_scan`, answered by the numpy statement."""
    scan_calls = 0

    def detect_dc_scan(self, preds, cell_cols=()):
        ScanTable.scan_calls += 1
        if not DC.scan_eligible(preds):
            raise AssertionError("a program that is not an order constraint reached detect_dc_scan")
        return S.scan_statement(self.codes, self.n_codes, preds, cell_cols)


class ScanEngine(DcEngine):
    table_cls = ScanTable


class Refusal(Exception):
    code = -2


class RefusingScanTable(DcTable):
    def detect_dc_scan(self, preds, cell_cols=()):
        raise Refusal("rgbm_table_detect_dc_scan: refused by this table")


class RefusingScanEngine(DcEngine):
    table_cls = RefusingScanTable


OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "6", "model.lgb.learning_rate": "0.2"}
RESIDENT, SCAN = "error.constraints.resident", "error.constraints.order_scan"


def _model(df, engine=None, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(80).setTargets(S.FRAME_TARGETS) \
        .setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints=S.FRAME_CONSTRAINT)])
    for key, val in dict(OPTS, **opts).items():
        m = m.option(key, str(val))
    m._engine_override = engine
    return m


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


@pytest.fixture(scope="module")
def tax():
    return S.small_frame()


@pytest.fixture()
def value_space(tax, oracle_backend, monkeypatch):
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    frame = _model(tax).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    assert {"Salary", "Tax"} & set(frame["attribute"])
    return frame


def test_option_is_registered_and_off_by_default(tax):
    assert SCAN in RepairModel.option_keys
    assert RepairModel()._get_option_value(*RepairModel._opt_constraints_order_scan) is False
    plan = _model(tax, ScanEngine(), **{RESIDENT: "true"})._device_detection_plan(tax, [], False, False)
    assert plan is not None and "order_scan" not in plan
    plan = _model(tax, ScanEngine(), **{RESIDENT: "true", SCAN: "true"})._device_detection_plan(tax, [], False, False)
    assert plan["order_scan"] is True
    # the option alone does nothing: the constraint is not `X -> Y`, so the run stays with the pandas detectors
    assert _model(tax, ScanEngine(), **{SCAN: "true"})._device_detection_plan(tax, [], False, False) is None


def test_run_with_the_option_takes_the_scan_route(tax, value_space):
    pairs, scans = DcTable.calls, ScanTable.scan_calls
    m = _model(tax, ScanEngine(), **{RESIDENT: "true", SCAN: "true"})
    frame = m.run()
    assert m._last_detection_on_device is True and m._last_resident_info["constraint_routes"] == ["dc_scan"]
    assert ScanTable.scan_calls > scans and DcTable.calls == pairs
    pd.testing.assert_frame_equal(_sorted(value_space), _sorted(frame), check_exact=True)


def test_run_without_the_option_takes_pairs(tax, value_space):
    pairs, scans = DcTable.calls, ScanTable.scan_calls
    m = _model(tax, ScanEngine(), **{RESIDENT: "true"})
    frame = m.run()
    assert m._last_detection_on_device is True and m._last_resident_info["constraint_routes"] == ["dc"]
    assert ScanTable.scan_calls == scans and DcTable.calls > pairs
    pd.testing.assert_frame_equal(_sorted(value_space), _sorted(frame), check_exact=True)


def test_a_table_without_the_method_takes_pairs(tax, value_space):
    pairs = DcTable.calls
    m = _model(tax, DcEngine(), **{RESIDENT: "true", SCAN: "true"})
    frame = m.run()
    assert m._last_detection_on_device is True and m._last_resident_info["constraint_routes"] == ["dc"]
    assert DcTable.calls > pairs
    pd.testing.assert_frame_equal(_sorted(value_space), _sorted(frame), check_exact=True)


def test_a_refusing_table_lands_in_value_space(tax, value_space, caplog):
    m = _model(tax, RefusingScanEngine(), **{RESIDENT: "true", SCAN: "true"})
    with caplog.at_level(logging.INFO):
        frame = m.run()
    assert m._last_detection_on_device is False
    assert any("refused by this table" in r.getMessage() for r in caplog.records)
    pd.testing.assert_frame_equal(_sorted(value_space), _sorted(frame), check_exact=True)


def test_detect_error_cells_routes_the_marked_program():
    from repair.pipeline import NotResidentEligible, constraint_routes, detect_error_cells, route_order_constraints
    codes, n_codes = S.make_table(257, "mixed", tile=64)
    sets = S.pred_sets(n_codes)
    dc = dict(kind="dc", preds=sets["eq_gt_lt"], refs=[S.G, S.A, S.B])
    iq = dict(kind="dc", preds=[("EQ", S.G, S.G, None, None), ("IQ", S.A, S.A, None, None), ("GT", S.B, S.B, None, None)], refs=[S.G, S.A, S.B])
    fd = ([S.G], S.A)
    routed = route_order_constraints([fd, dc, iq], ScanTable(codes, n_codes))
    assert constraint_routes(routed) == ["fd", "dc_scan", "dc"] and dc["kind"] == "dc"
    assert constraint_routes(route_order_constraints([fd, dc, iq], DcTable(codes, n_codes))) == ["fd", "dc", "dc"]
    scans = ScanTable.scan_calls
    r, c = detect_error_cells(ScanTable(codes, n_codes), [S.A, S.B], constraints=[routed[1]], detect_nulls=False)
    assert ScanTable.scan_calls == scans + 1
    wr, wc = R.detect_dc(codes, n_codes, dc["preds"], cell_cols=[S.A, S.B])
    assert np.array_equal(r, wr) and np.array_equal(c, wc) and len(wr) > 0
    with pytest.raises(NotResidentEligible, match="refused by this table"):
        detect_error_cells(RefusingScanTable(codes, n_codes), [S.A], constraints=[routed[1]], detect_nulls=False)
