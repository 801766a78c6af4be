"""-m gpu: `Table.recode` (rgbm_table_recode, csrc/rgbm_recode.hip) against its numpy statement `repair.recode_codes.recode` on the cases
of tests/fitted_cases.py -- the same codes and the same unmapped counts, each case first asserting its routes through `recode_report()` --
its refusals, and a kept fit applied through the HIP engine."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from repair import recode_codes
from tests import fitted_cases as FC
from tests import fitted_restatement as FR

pytestmark = pytest.mark.gpu

# the nodes tests/test_fitted_gpu_guarded.py runs once more under guard zones and poison: the row edges up to 257, the refusals
GUARDED = ["tests/test_fitted_gpu.py::test_recode_equals_the_statement[r%dc%d]" % (n, c) for n in FC.ROWS if n <= FC.GUARDED_ROWS for c in FC.COLS] + \
          ["tests/test_fitted_gpu.py::test_recode_equals_the_statement[all_identity]", "tests/test_fitted_gpu.py::test_refusals_leave_everything_as_it_was"]


def _check_case(c):
    from repair import _native as N
    tab = N.Table(c["codes"], c["n_codes"])
    for j in range(tab.c):                                      # the source carries kinds and values: the result must not inherit them
        if j % 2:
            tab.set_column_kind(j, True)
        else:
            tab.set_column_values(j, np.arange(int(c["n_codes"][j]), dtype=np.float64))
    assert tab.recode_report()["routes"] == [-1] * tab.c
    out, unmapped = tab.recode(c["luts"], c["n_codes_out"])
    rep = tab.recode_report()
    assert rep["routes"] == c["routes"] and rep["lds_codes"] == FC.lds_codes() == N.recode_limits()["lds_codes"]
    want, want_un = recode_codes.recode(c["codes"], c["n_codes"], c["luts"], c["n_codes_out"])
    got = np.stack([out.read_column(j) for j in range(out.c)])
    assert (out.n, out.c) == (tab.n, tab.c) and np.array_equal(out.n_codes, c["n_codes_out"])
    assert np.array_equal(got, want) and np.array_equal(unmapped, want_un) and unmapped.dtype == np.int64
    assert np.array_equal(np.stack([tab.read_column(j) for j in range(tab.c)]), c["codes"])              # the source reads back unchanged
    assert np.array_equal(out.row_multiplicity(), np.ones(out.n, np.uint8))
    # no kinds, no values: `concat` takes parts of equal dictionaries only, and a fresh table of the same codes has neither
    both = N.Table.concat([out, N.Table(want, c["n_codes_out"])])
    assert both.n == 2 * out.n
    assert tab.recode(c["luts"], c["n_codes_out"], want_unmapped=False)[1] is None
    for t in (both, out, tab):
        t.close()


@pytest.mark.parametrize("cid", FC.case_ids())
def test_recode_equals_the_statement(cid):
    _check_case(FC.case(cid))


def test_recode_of_a_large_table_with_a_column_of_100000_codes():
    c = FC.big_case()
    assert c["codes"].shape == (6, 200003) and max(c["n_codes"]) > 100000 and sorted(set(c["routes"])) == [0, 1, 2]
    _check_case(c)


def _raw(tab, luts, n_codes_out, handle, counts):
    from repair import _native as N
    keep = [None if m is None else np.ascontiguousarray(m, np.int32) for m in (luts or [])]
    ptrs = (C.POINTER(C.c_int32) * max(len(keep), 1))(*[N._p(m, C.c_int32) for m in keep]) if luts is not None else None
    nco = None if n_codes_out is None else np.ascontiguousarray(n_codes_out, np.int32)
    rc = N.lib().rgbm_table_recode(tab.h if tab is not None else None, ptrs, N._p(nco, C.c_int32), C.byref(handle) if handle is not None else None,
                                   N._p(counts, C.c_int64))
    return rc, N.lib().rgbm_last_error().decode()


def test_refusals_leave_everything_as_it_was():
    from repair import _native as N
    rng = np.random.default_rng(5)
    codes = rng.integers(-1, 3, (3, 301)).astype(np.int32)
    tab = N.Table(codes, [3, 3, 3])
    good = [np.array([2, -1, 0], np.int32), None, np.array([0, 0, 1], np.int32)]
    out, un = tab.recode(good, [3, 3, 2])
    report = tab.recode_report()
    tab.cellset_open([0, 2])
    n_cells = tab.detect_nulls([0, 1, 2], fetch=False)
    tab.cellset_add()
    cells = tab._fetch_cells(n_cells, True)
    for luts, nco, code, why in (
            (None, [3, 3, 2], -1, "bad argument"), (good, None, -1, "bad argument"),
            (good, [3, 3, 0], -1, "column 2 has an output dictionary of 0 codes"),
            (good, [3, 4, 2], -1, "identity column 1 changes its dictionary size (3 -> 4)"),
            ([good[0], None, np.array([0, 2, 1], np.int32)], [3, 3, 2], -1, "column 2, LUT entry 1 = 2 is outside [-1, 2)"),
            ([np.array([0, -2, 1], np.int32), None, good[2]], [3, 3, 2], -1, "column 0, LUT entry 1 = -2 is outside [-1, 3)")):
        handle, counts = C.c_void_p(0x5A5A), np.full(3, 77, np.int64)
        rc, msg = _raw(tab, luts, nco, handle, counts)
        assert rc == code and why in msg and "rgbm_table_recode" in msg, (rc, msg)
        assert handle.value == 0x5A5A and list(counts) == [77, 77, 77]                 # *out and the counts as they were
        assert tab.recode_report() == report
    rc, msg = _raw(None, good, [3, 3, 2], C.c_void_p(), None)
    assert rc == -1 and "bad argument" in msg
    rc, msg = _raw(tab, good, [3, 3, 2], None, None)
    assert rc == -1 and "bad argument" in msg
    bad_report = np.zeros(8, np.int32)
    assert N.lib().rgbm_table_recode_report(tab.h, N._p(bad_report, C.c_int32), C.c_int32(2)) == -1      # c is not the table's columns
    assert tab.recode_report() == report
    # the cell list and the cell set: as the detect call and the add left them, after the refusals and after a successful call
    out2, un2 = tab.recode(good, [3, 3, 2])
    again = tab._fetch_cells(n_cells, True)
    assert np.array_equal(again[0], cells[0]) and np.array_equal(again[1], cells[1])
    rows, cols, held, counts = tab.cellset_emit()
    assert np.array_equal(cols, cells[1][np.isin(cells[1], [0, 2])]) and np.array_equal(rows, cells[0][np.isin(cells[1], [0, 2])]) and (held < 0).all()
    tab.cellset_close()
    assert np.array_equal(un, un2) and np.array_equal(out.read_column(0), out2.read_column(0))
    assert np.array_equal(np.stack([tab.read_column(j) for j in range(3)]), codes)
    for t in (out, out2, tab):
        t.close()


# ---------------------------------------------------------------------------------------------- whole runs through the HIP engine
def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


def test_hospital_fit_and_apply_on_the_same_frame_through_the_hip_engine():
    from repair.model import RepairModel
    from tests.test_fitted_cpu import OPTS
    from tests.test_quality import HOSPITAL_TARGETS, _hospital
    df, _, cells = _hospital()
    cells = cells[["tid", "attribute"]]

    def model(**extra):
        m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400).setTargets(HOSPITAL_TARGETS).setErrorCells(cells)
        for k, v in dict(OPTS, **extra).items():
            m = m.option(k, v)
        return m
    m = model(**{"model.fitted.keep": "true"})
    out = m.run()
    assert m._last_resident_info is not None and len(out) > 100
    fit = m.fittedModels()
    m2 = model().setFittedModels(fit)
    again = m2.run()
    info = m2._last_resident_info
    assert info["times"]["train"] == 0.0 and info["fitted"]["recode_seconds"] > 0 and not any(info["fitted"]["unmapped"].values())
    pd.testing.assert_frame_equal(_sorted(out), _sorted(again))
    data, again_data = model().run(repair_data=True), model().setFittedModels(fit).run(repair_data=True)
    pd.testing.assert_frame_equal(data.sort_values("tid").reset_index(drop=True), again_data.sort_values("tid").reset_index(drop=True))


def test_first_half_fit_applied_to_the_second_half_through_the_hip_engine():
    """The HIP engine fits boston's first half and applies the fit to the second; the restatement predicts with the HIP blobs loaded into
    the oracle's model (one serialisation format)."""
    from oracle import oracle as O
    from repair.engine import HipEngine
    from repair.fitted import FittedRepairModels
    from repair.pipeline import repair_frame
    from tests.test_fitted_cpu import PARAMS, _as_dict, _null_cells
    from tests.test_quality import _boston_frame
    df, _ = _boston_frame()
    a, b = df.iloc[:253].reset_index(drop=True), df.iloc[253:].reset_index(drop=True)
    eng = HipEngine(0)
    _, details = repair_frame(eng, a, "tid", targets=["CRIM", "RAD", "TAX", "LSTAT"], base_params=PARAMS,
                              continuous_columns=["CRIM", "TAX", "LSTAT"], want_details=True, keep_fit=True)
    fit = FittedRepairModels.from_pieces(details["fit"])
    cells = _null_cells(b, fit.chain)
    for resident in (False, True):
        got, info = repair_frame(eng, b, "tid", error_cells=cells, detect_nulls=False, want_details=True, fitted=fit, cells_resident=resident)
        want = FR.apply_loops(fit, b, "tid", list(cells.itertuples(index=False, name=None)), O.OracleModel.load)
        assert len(got) == len(cells) > 60 and _as_dict(got) == want
        assert info["fitted"]["unmapped"]["RAD"] > 0 and info["fitted"]["unmapped"]["CRIM"] == 0
