"""-m gpu: the four entries that carry a repair run on the table's cell set (csrc/rgbm_cellset.hip: rgbm_table_cellset_add_cells / _drop_weak /
_null / _rows) against the plain numpy statement tests/cellrun_restatement.py -- rows, columns, codes and counts exactly, the whole table read
back after every null-out -- and `RepairModel.run()` with `error.cells.resident` through the HIP engine against the same run without it.
The cases and the driver are tests/cellrun_cases.py (tests/test_cellrun_cpu.py holds every generator to its purpose without a device): one
sequence of calls runs on the device table and on the restated one, and the two records are compared entry by entry.  The weak flags of
`cellset_drop_weak` are also held to `Table.cell_domains` on the same rows, inside that sequence.
tests/test_cellrun_gpu_guarded.py runs the smallest of these cases once more under guard zones and poison (GUARDED below).

(The file is not named test_gpu_*.py: tests/guarded_runs.py lists every file of that pattern in its families, and it stays as it is.)"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tests import cellrun_cases as X
from tests.cellrun_restatement import CellrunTable
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu


def _both(case):
    """(the device's record, the restatement's record) of the case's whole sequence."""
    from repair import _native as N
    got = X.drive(N.Table(case["codes"], case["n_codes"]), case)
    want = X.drive(CellrunTable(case["codes"], case["n_codes"]), case)
    X.same(got, want)
    return got, want


def test_constants_are_what_the_cases_assume():
    assert csrc_constant("PB") * csrc_constant("PSUB") == X.PROWS              # rows per compaction block: 64 words of the set
    assert X.SIZES == [1, 63, 64, 65, 4095, 4096, 4097, 8193] and [len(s) for s in X.SETS.values()] == [1, 2, 16, 17]


@pytest.mark.parametrize("which", list(X.SETS))
@pytest.mark.parametrize("n", X.SIZES)
def test_the_four_entries_equal_the_restatement(n, which):
    got, _ = _both(X.generic_case(n, which))
    rec = dict(got)
    for t in [d["target"] for d in X.generic_case(n, which)["prune"]]:           # the kernel's flag against `Table.cell_domains` on the same rows
        assert rec["drop_weak %d.weak" % t] == int(rec["drop_weak %d.flags of cell_domains" % t].sum())


@pytest.mark.parametrize("kind", X.PRUNE_KINDS)
def test_drop_weak_prunes_what_cell_domains_calls_weak(kind):
    case = X.prune_case(kind)
    got, _ = _both(case)
    X.purpose(case, got)
    rec = dict(got)
    for d in case["prune"]:
        t = d["target"]
        flags, rows = rec["drop_weak %d.flags of cell_domains" % t].astype(bool), rec["drop_weak %d.rows" % t]
        after = rec["after drop_weak %d.rows" % t][rec["after drop_weak %d.cols" % t] == t]
        assert np.array_equal(after, rows[~flags])                                # exactly the weak cells left the column


@pytest.mark.parametrize("kind", ["empty", "every_row", "block_edges"])
def test_cellset_rows(kind):
    _both(X.rows_case(kind))


def test_many_blocks_three_overlapping_detectors_given_cells_and_pruning():
    case = X.many_blocks_case()
    got, _ = _both(case)
    rec = dict(got)
    assert rec["detected.counts"].sum() < rec["nulls"] + rec["cells"] + rec["constraint"]
    assert all(0 < rec["drop_weak %d.weak" % t] < rec["drop_weak %d.cells" % t] for t in (1, 2))


def test_the_codes_of_the_last_emit_are_what_the_cells_held_then():
    """`cellset_null` leaves the set, the cell list and the last emit's codes: the codes are still fetchable and are the values BEFORE the
    null-out; a second null-out finds the same cells and changes nothing."""
    from repair import _native as N
    case = X.generic_case(X.PROWS + 1, "sixteen")
    tab = N.Table(case["codes"], case["n_codes"])
    tab.cellset_open(case["set_cols"])
    tab.cellset_add_cells(*case["given"][0])
    rows, cols, codes, counts = tab.cellset_emit()
    assert (codes >= 0).any() and np.array_equal(codes, case["codes"][cols, rows])
    assert tab.cellset_null() == len(rows)
    got = tab._fetch_cells(len(rows), True)
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols) and np.array_equal(tab.cells_fetch_codes(len(rows)), codes)
    assert (tab.read_cells(rows, cols) == -1).all()
    table = np.stack([tab.read_column(j) for j in range(X.C)])
    assert tab.cellset_null() == len(rows) and np.array_equal(np.stack([tab.read_column(j) for j in range(X.C)]), table)
    again = tab.cellset_emit()
    assert np.array_equal(again[0], rows) and np.array_equal(again[1], cols) and (again[2] == -1).all() and np.array_equal(again[3], counts)
    tab.cellset_close()


def test_a_distinct_row_view_is_rebuilt_after_the_null_out(monkeypatch):
    from repair import _native as N
    from tests.test_gpu_distinct_view import CARDS8, _feats, _kw, _table
    monkeypatch.setenv("RGBM_DISTINCT_MIN_ROWS", "1")
    for name in ("RGBM_DISTINCT", "RGBM_DISTINCT_MAX_RATIO"):
        monkeypatch.delenv(name, raising=False)
    codes, cards = _table(CARDS8, seed=78, n=6000, pool=900, big=300)
    t, feats = 1, _feats(8, 1)
    tab = N.Table(codes, cards)

    def fresh(c):
        return N.Table(c, cards).train(t, feats, whole_table=True, **_kw(c, cards, t)).save()

    assert tab.train(t, feats, **_kw(codes, cards, t)).save() == fresh(codes)
    assert tab.distinct_view_info()["state"] == "built"
    rng = np.random.default_rng(2)
    rows, cols = rng.integers(0, codes.shape[1], 500), rng.choice([t, 4], 500).astype(np.int32)
    tab.cellset_open([4, t])
    tab.cellset_add_cells(rows, cols)
    assert tab.distinct_view_info()["state"] == "built"                          # the set alone writes no code
    cells = tab.cellset_null()
    assert tab.distinct_view_info()["state"] == "none"
    tab.cellset_close()
    nulled = codes.copy()
    nulled[cols, rows] = -1
    assert cells == len(set(zip(rows.tolist(), cols.tolist()))) and np.array_equal(np.stack([tab.read_column(j) for j in range(8)]), nulled)
    assert tab.train(t, feats, **_kw(nulled, cards, t)).save() == fresh(nulled)
    assert tab.distinct_view_info() == dict(tab.distinct_view_info(), state="built", builds=2)


def _refused(N, code, fn, *a, **kw):
    with pytest.raises(N.RepairGbmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)


def test_refusals_leave_the_set_the_cell_list_and_the_last_emits_codes():
    from repair import _native as N
    n = X.PROWS + 1
    codes, n_codes, _ = X.table(n, 4)
    tab = N.Table(codes, n_codes)
    lib = N.lib()
    ok, i64, i32, u8 = np.ones(X.K, np.uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    out = (C.c_int64 * 2)()
    one_row, one_col = np.zeros(1, np.int64), np.ones(1, np.int32)

    def raw_add(rows, cols, m):
        return lib.rgbm_table_cellset_add_cells(tab.h, rows.ctypes.data_as(i64) if rows is not None else None,
                                                cols.ctypes.data_as(i32) if cols is not None else None, C.c_int64(m))

    def raw_drop(target, pidx, k, min_cnt, single_ok, row_count, counts=True):
        p, m = np.asarray(pidx if pidx is not None else [0], np.int32), np.asarray(min_cnt if min_cnt is not None else [0], np.int64)
        return lib.rgbm_table_cellset_drop_weak(tab.h, C.c_int32(target), p.ctypes.data_as(i32) if pidx is not None else None, C.c_int32(k),
                                                m.ctypes.data_as(i64) if min_cnt is not None else None,
                                                single_ok.ctypes.data_as(u8) if single_ok is not None else None, C.c_double(0.5), C.c_int64(row_count),
                                                C.cast(C.byref(out, 0), i64) if counts else None, C.cast(C.byref(out, 8), i64) if counts else None)

    # ---- no open set: RGBM_ERR_PARAM from all four, and the detector's cell list stays
    want = tab.detect_nulls([2, 5])
    assert tab.detect_nulls([2, 5], fetch=False) == len(want[0]) > 0

    def cell_list_is(w):
        got = tab._fetch_cells(len(w[0]), True)
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])

    tab.pair_counts([(0, 1), (2, 0)], n_bins={j: X.K for j in range(X.C)})
    for fn, a in ((tab.cellset_add_cells, (one_row, one_col)), (tab.cellset_drop_weak, (1, [0], [0], ok, 0.5, n)), (tab.cellset_null, ()),
                  (tab.cellset_rows, ())):
        _refused(N, -2, fn, *a)
        cell_list_is(want)
    assert np.array_equal(np.stack([tab.read_column(j) for j in range(X.C)]), codes)

    # ---- an open set with an emit behind it
    set_cols = [5, 1, 2]
    tab.cellset_open(set_cols)
    tab.cellset_add()
    tab.cellset_add_cells(*X.given_cells(n, set_cols, 1))
    before = tab.cellset_emit()
    assert len(before[0]) > len(want[0])

    def intact():
        """The cell list and the last emit's codes (fetchable only while cell_version is that emit's), then the set itself."""
        cell_list_is(before[:2])
        assert np.array_equal(tab.cells_fetch_codes(len(before[0])), before[2])
        assert all(np.array_equal(g, w) for g, w in zip(tab.cellset_emit(), before))

    for rc in (raw_add(None, one_col, 1), raw_add(one_row, None, 1), raw_add(one_row, one_col, -1)):      # RGBM_ERR_ARG
        assert rc == -1 and b"rgbm_table_cellset_add_cells" in lib.rgbm_last_error()
        intact()
    assert raw_add(None, None, 0) == 0                                            # nothing to read: fine
    intact()
    # drop_weak, RGBM_ERR_ARG: the target outside the table, k < 0, a NULL array that is needed, row_count < 1, no place for the counts
    for rc in (raw_drop(X.C, [0], 1, [0], ok, n), raw_drop(-1, [0], 1, [0], ok, n), raw_drop(1, [0], -1, [0], ok, n), raw_drop(1, None, 1, [0], ok, n),
               raw_drop(1, [0], 1, None, ok, n), raw_drop(1, [0], 1, [0], None, n), raw_drop(1, [0], 1, [0], ok, 0), raw_drop(1, [0], 1, [0], ok, n, counts=False)):
        assert rc == -1 and b"rgbm_table_cellset_drop_weak" in lib.rgbm_last_error()
        intact()
    # drop_weak, RGBM_ERR_PARAM: more than 8 attributes, a pair index outside the call's pairs, a pair without the target, a target outside the set
    for a in ((1, [0] * 9, [0] * 9, ok, 0.5, n), (1, [2], [0], ok, 0.5, n), (1, [-1], [0], ok, 0.5, n), (1, [1], [0], ok, 0.5, n), (0, [0], [0], ok, 0.5, n)):
        _refused(N, -2, tab.cellset_drop_weak, *a)
        intact()
    lut = (np.arange(X.K) // 2).astype(np.int32)                                  # ... and a target that was counted through a LUT
    tab.pair_counts([(0, 1)], luts={1: lut}, n_bins={0: X.K, 1: 3})
    _refused(N, -2, tab.cellset_drop_weak, 1, [0], [0], np.ones(3, np.uint8), 0.5, n)
    intact()
    for rc in (lib.rgbm_table_cellset_null(tab.h, None), lib.rgbm_table_cellset_rows(tab.h, None), lib.rgbm_table_cellset_null(None, C.cast(C.byref(out, 0), i64))):
        assert rc == -1
        intact()
    assert np.array_equal(np.stack([tab.read_column(j) for j in range(X.C)]), codes)           # nothing wrote a code
    # ---- a fresh table: no pair_counts result
    tab2 = N.Table(codes, n_codes)
    tab2.cellset_open([1])
    tab2.cellset_add_cells(one_row, one_col)
    _refused(N, -2, tab2.cellset_drop_weak, 1, [0], [0], ok, 0.5, n)
    got = tab2.cellset_emit()
    assert got[0].tolist() == [0] and got[1].tolist() == [1]
    tab2.cellset_close()
    # ---- closed: all four refuse again
    tab.cellset_close()
    for fn, a in ((tab.cellset_add_cells, (one_row, one_col)), (tab.cellset_null, ()), (tab.cellset_rows, ())):
        _refused(N, -2, fn, *a)
    cell_list_is(before[:2])


def test_run_through_the_hip_engine_with_the_option_on_and_off():
    from tests.test_cellrun_cpu import ANALYSIS, SAME_DETAILS, _hospital, _hospital_detectors, _model, _sorted
    from tests.test_quality import HOSPITAL_TARGETS
    df = _hospital()
    off = _model(df, _hospital_detectors(), HOSPITAL_TARGETS, 80, None, False, **ANALYSIS)
    want = off.run()
    on = _model(df, _hospital_detectors(), HOSPITAL_TARGETS, 80, None, True, **ANALYSIS)
    got = on.run()
    assert off._last_detection_on_device is True and on._last_detection_on_device is True
    assert "cells_route" not in off._last_resident_info and on._last_resident_info["cells_route"] == "set"
    assert len(want) > 0 and on._last_resident_info["weak_cells"] > 0
    pd.testing.assert_frame_equal(_sorted(want), _sorted(got), check_exact=True)
    for key in SAME_DETAILS:
        assert on._last_resident_info.get(key) == off._last_resident_info.get(key), key


# what tests/test_cellrun_gpu_guarded.py runs once more under guard zones and poison: the row counts up to 4097 and the refusals
_HERE = "tests/test_cellrun_gpu.py::"
GUARDED = [_HERE + "test_the_four_entries_equal_the_restatement[%d-%s]" % (n, w) for w in X.SETS for n in X.SIZES if n <= X.PROWS + 1] + \
          [_HERE + "test_the_codes_of_the_last_emit_are_what_the_cells_held_then", _HERE + "test_refusals_leave_the_set_the_cell_list_and_the_last_emits_codes"]
