"""GPU: the table's cell set (csrc/rgbm_cellset.hip: rgbm_table_cellset_open / _add / _emit / _close, rgbm_table_cells_fetch_codes) against
the plain numpy statement tests/cellset_restatement.py -- rows, columns, codes and counts exactly -- at the edges of a 64-row word and of a
compaction block, for sets of 1, 2, 16 and all 17 columns in non-ascending order, and every refusal with what it must leave behind."""
import numpy as np
import pytest

from tests import cellset_restatement as CS
from tests import detector_restatements as DR
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

PROWS = csrc_constant("PB") * csrc_constant("PSUB")          # rows per compaction block
assert PROWS == 4096
SIZES = [1, 63, 64, 65, PROWS - 1, PROWS, PROWS + 1, 2 * PROWS + 1]
C, K = 17, 5
FIRST, LAST, BEYOND = 3, 4, 7                                 # columns: a 1 in the first row only / in the last row only / a code beyond the dictionary
SETS = {"one": [5], "two": [9, 2], "sixteen": [16, 0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7], "all": [8, 16, 0, 15, 1, 14, 2, 13, 3, 12, 4, 11, 5, 10, 6, 9, 7]}


def _table(n, seed=0):
    rng = np.random.default_rng(seed * 131 + n)
    codes = rng.integers(0, K, (C, n)).astype(np.int32)
    codes[rng.random((C, n)) < 0.2] = -1
    codes[[2, 5], 0] = -1                                      # a NULL in every set below, whatever the size
    codes[FIRST], codes[LAST] = 0, 0
    codes[FIRST, 0], codes[LAST, n - 1] = 1, 1
    codes[BEYOND, n // 2] = K + 3                              # returned as it lies
    return codes, np.full(C, K, np.int32)


def _nulls(codes, cols):
    k = len(cols)
    return DR.detect_cells(codes, cols, [1] * k, [0] * k, [-1] * k, None)


def _bits(*set_codes):
    w = np.zeros(1, np.uint64)
    for v in set_codes:
        w[0] |= np.uint64(1) << np.uint64(v)
    return w


class _Pair:
    """The device table and the restated set, driven together."""

    def __init__(self, n, set_cols, seed=0):
        from repair import _native as N
        self.N, self.n, self.set_cols = N, n, list(set_cols)
        self.codes, self.n_codes = _table(n, seed)
        self.tab = N.Table(self.codes, self.n_codes)
        self.tab.cellset_open(self.set_cols)
        self.keys = CS.new_set()

    def add(self, count, want):
        """The device holds `count` cells (the result `want` of the restated detector) in its cell list: add them on both sides."""
        assert count == len(want[0])
        self.tab.cellset_add()
        got = self.tab._fetch_cells(count, True)                # the cell list itself is left as it was
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        self.keys = CS.add(self.keys, self.set_cols, self.n, C, *want)

    def nulls(self, cols):
        self.add(self.tab.detect_nulls(cols, fetch=False), _nulls(self.codes, cols))

    def cells(self, cols, null, lo, hi, bits):
        self.add(self.tab.detect_cells(cols, null, lo, hi, bits, fetch=False), DR.detect_cells(self.codes, cols, null, lo, hi, bits))

    def check(self):
        got = self.tab.cellset_emit()
        want = CS.emit(self.keys, self.codes, self.set_cols)
        assert [a.dtype for a in got] == [np.int64, np.int32, np.int32, np.int64]
        for g, w, what in zip(got, want, ("rows", "cols", "codes", "counts")):
            assert np.array_equal(g, w), (what, self.n, self.set_cols)
        return got


@pytest.mark.parametrize("which", list(SETS))
@pytest.mark.parametrize("n", SIZES)
def test_cellset_equals_the_restatement(n, which):
    p = _Pair(n, SETS[which])
    assert len(p.check()[0]) == 0                                              # a fresh set
    p.cells([FIRST], [0], [0], [-1], [_bits(2)])                               # an empty result
    assert len(p.check()[0]) == 0
    p.cells([FIRST], [0], [0], [-1], [_bits(1)])                               # a cell in the first row only ...
    p.cells([LAST], [0], [0], [-1], [_bits(1)])                                # ... and in the last row only
    first = p.check()
    assert set(zip(first[0].tolist(), first[1].tolist())) == {(r, c) for r, c in ((0, FIRST), (n - 1, LAST)) if c in p.set_cols}
    p.nulls([2, 5, 9, BEYOND])                                                 # columns inside and outside the set
    p.check()
    p.nulls([2, 5, 9, BEYOND])                                                 # the same result twice
    p.check()
    p.cells([9, 5, 12], [1, 0, 1], [0, 0, 1], [-1, -1, 2], [_bits(0, 3), _bits(4), None])   # overlaps the NULL cells of 9, adds to 5, new in 12
    once = p.check()
    twice = p.check()                                                          # emit twice
    assert all(np.array_equal(a, b) for a, b in zip(once, twice))
    everything = list(range(C))
    p.cells(everything, [1] * C, [2 ** 31 - 1] * C, [2 ** 31 - 1] * C, None)   # add after emit: every cell of the table
    got = p.check()
    assert len(got[0]) == n * len(p.set_cols) and got[3].tolist() == [n] * len(p.set_cols)
    if BEYOND in p.set_cols:
        at = np.flatnonzero((got[1] == BEYOND) & (got[0] == n // 2))
        assert got[2][at].tolist() == [K + 3]                                  # beyond the dictionary, as it lies
    assert (got[2] == -1).any()                                                # and NULL as -1
    p.tab.cellset_open(p.set_cols)                                             # re-open clears
    p.keys = CS.new_set()
    assert len(p.check()[0]) == 0
    p.tab.cellset_close()


def _refused(N, code, fn, *a, **kw):
    with pytest.raises(N.RepairGbmError) as e:
        fn(*a, **kw)
    assert e.value.code == code, str(e.value)


def test_refusals_leave_the_cell_list_and_the_set_as_they_were():
    from repair import _native as N
    n = PROWS + 1
    codes, n_codes = _table(n)
    tab = N.Table(codes, n_codes)
    want = _nulls(codes, [2, 5])

    def cell_list_is(w):
        got = tab._fetch_cells(len(w[0]), True)
        assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])

    assert tab.detect_nulls([2, 5], fetch=False) == len(want[0])
    _refused(N, -2, tab.cellset_add)                                           # no open set
    _refused(N, -2, tab.cellset_emit)
    cell_list_is(want)
    for bad in ([], [1, 1], [-1], [C], list(range(C)) + [0]):                  # none, twice, out of range, more than the table has
        _refused(N, -1, tab.cellset_open, bad)
    _refused(N, -2, tab.cellset_add)                                           # still no set
    tab.cellset_open([5, 2])
    tab.cellset_add()
    keys = CS.add(CS.new_set(), [5, 2], n, C, *want)
    before = tab.cellset_emit()
    assert all(np.array_equal(g, w) for g, w in zip(before, CS.emit(keys, codes, [5, 2]))) and len(before[0]) > 0
    for bad in ([1, 1], [C]):                                                  # a refused open leaves the set
        _refused(N, -1, tab.cellset_open, bad)
    assert all(np.array_equal(g, w) for g, w in zip(tab.cellset_emit(), before))
    rows = tab.detect_constraint([0], 1, fetch=False)                          # a row list without columns
    assert rows > 0
    row_list = tab._fetch_cells(rows, False)
    _refused(N, -2, tab.cellset_add)
    assert np.array_equal(tab._fetch_cells(rows, False), row_list)             # the row list stays ...
    _refused(N, -2, tab.cells_fetch_codes, rows)                               # ... and it is not an emit's result
    again = tab.cellset_emit()                                                 # ... and so does the set
    assert all(np.array_equal(g, w) for g, w in zip(again, before))
    assert np.array_equal(tab.cells_fetch_codes(len(again[0])), before[2])
    tab.detect_nulls([2], fetch=False)                                         # a later detect call: the codes are no longer the cell list's
    _refused(N, -2, tab.cells_fetch_codes, len(again[0]))
    tab.cellset_close()
    _refused(N, -2, tab.cellset_add)
    tab.cellset_close()                                                        # closing twice is fine


def test_many_blocks_three_overlapping_detectors():
    from oracle import prep as P
    from repair import _native as N
    n = 200003
    rng = np.random.default_rng(11)
    codes = rng.integers(0, 40, (6, n)).astype(np.int32)
    codes[0] = rng.integers(0, 2000, n)
    codes[1] = codes[0] % 7
    flip = rng.random(n) < 0.01
    codes[1, flip] = (codes[1, flip] + 1) % 7                                   # 0 -> 1 broken in one row of a hundred
    codes[:, rng.random(n) < 0.05] = -1
    codes[2, rng.random(n) < 0.1] = -1
    n_codes = np.asarray([2000, 7, 40, 40, 40, 40], np.int32)
    set_cols = [4, 2, 1]
    tab = N.Table(codes, n_codes)
    tab.cellset_open(set_cols)
    keys = CS.new_set()
    a = _nulls(codes, [1, 2, 3])
    assert tab.detect_nulls([1, 2, 3], fetch=False) == len(a[0])
    tab.cellset_add()
    bits = np.zeros(1, np.uint64)
    bits[0] = np.uint64(0x5555555555)
    b = DR.detect_cells(codes, [2, 4], [1, 0], [0, 3], [-1, 30], [bits, None])
    assert tab.detect_cells([2, 4], [1, 0], [0, 3], [-1, 30], [bits, None], fetch=False) == len(b[0])
    tab.cellset_add()
    c = P.constraint_cells(codes, [0], 1, [1, 2])
    assert tab.detect_constraint([0], 1, cell_cols=[1, 2], fetch=False) == len(c[0]) > 0
    tab.cellset_add()
    for part in (a, b, c):
        keys = CS.add(keys, set_cols, n, 6, *part)
    got, want = tab.cellset_emit(), CS.emit(keys, codes, set_cols)
    for g, w, what in zip(got, want, ("rows", "cols", "codes", "counts")):
        assert np.array_equal(g, w), what
    assert len(got[0]) < len(a[0]) + len(b[0]) + len(c[0]) and got[3].min() > 0          # they do overlap
    tab.cellset_close()
