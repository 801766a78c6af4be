"""The plain numpy statement of the four entries that carry a REPAIR run on the table's cell set (include/rgbm.h: rgbm_table_cellset_add_cells /
_drop_weak / _null / _rows), shared by the CPU and the GPU tests; no code of the product but `repair.domain.cell_domains`, the value-space
statement the device's weak flag is held to.  On top of tests/cellset_restatement.py: the set is a sorted array of keys
position-in-the-set's-columns * n + row.  `CellrunTable` / `CellrunEngine` put the four methods on the CPU tables of the other test modules and
keep a CALL RECORD: the names of the table methods a run used, in order, over every table the engine made."""
import numpy as np

from tests import cellset_restatement as CS
from tests.cellset_restatement import CellsetEngine, CellsetTable, Refused
from tests.test_domain_analysis import _DomainTable


def add_cells(keys, set_cols, n, c, rows, cols):
    """keys | the given cells, in any order and with duplicates; cells outside the table or the set's columns are skipped."""
    return CS.add(keys, set_cols, n, c, rows, cols)


def column_rows(keys, set_cols, n, target):
    """Ascending rows of the set's cells of column `target`."""
    p = list(set_cols).index(int(target))
    keys = np.asarray(keys, np.int64)
    return np.sort(keys[keys // n == p] % n).astype(np.int64)


def drop_weak(keys, set_cols, n, target, weak_of_rows):
    """(keys without the weak cells of column `target`, the examined rows, cells cleared); weak_of_rows(rows) -> flags."""
    rows = column_rows(keys, set_cols, n, target)
    weak = np.asarray(weak_of_rows(rows), bool) if len(rows) else np.zeros(0, bool)
    p = list(set_cols).index(int(target))
    return np.setdiff1d(np.asarray(keys, np.int64), p * n + rows[weak]), rows, int(weak.sum())


def null(keys, codes, set_cols):
    """(the codes with NULL in every cell of the set -- every other code untouched --, the number of cells)"""
    out = np.array(codes, np.int32, copy=True)
    n = out.shape[1]
    keys = np.unique(np.asarray(keys, np.int64))
    if len(keys):
        out[np.asarray(set_cols, np.int64)[keys // n], keys % n] = -1
    return out, len(keys)


def rows_of(keys, n):
    """Ascending rows that hold at least one cell of the set."""
    return np.unique(np.asarray(keys, np.int64) % n).astype(np.int64)


RECORDED = ("read_cells", "null_cells", "write_cells", "rows_of_cells", "cell_domains", "pair_counts", "cellset_open", "cellset_add", "cellset_emit",
            "cellset_close", "cellset_add_cells", "cellset_drop_weak", "cellset_null", "cellset_rows")
# the calls that send error cells to the table
CELL_UPLOADS = ("read_cells", "null_cells", "write_cells", "rows_of_cells", "cell_domains", "cellset_add_cells")


class CellrunTable(CellsetTable):
    """`CellsetTable` with the four entries, stated by the functions above, and the call record."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = []

    def _fetch_cells(self, n, want_cols, fetch=True):
        """The table's cell list, as `_native.Table._fetch_cells` reads it."""
        rows, cols = self._cells
        assert n == len(rows)
        if not fetch:
            return n
        rows = np.asarray(rows, np.int64)
        return (rows, np.asarray(cols, np.int32)) if want_cols else rows

    def _need_set(self, who):
        if self._set is None:
            raise Refused("%s: no open cell set" % who)
        return self._set

    def cellset_add_cells(self, rows, cols):
        set_cols, keys = self._need_set("cellset_add_cells")
        rows, cols = np.asarray(rows, np.int64).reshape(-1), np.asarray(cols, np.int32).reshape(-1)
        if len(rows) != len(cols):
            raise ValueError("rows and cols must have the same length")
        self._set = (set_cols, add_cells(keys, set_cols, self.n, self.c, rows, cols))

    def cellset_drop_weak(self, target_col, pair_idx, min_cnt, single_ok, beta, row_count):
        set_cols, keys = self._need_set("cellset_drop_weak")
        if int(target_col) not in set_cols:
            raise Refused("cellset_drop_weak: the target is not a column of the cell set")
        flags = lambda rows: _DomainTable.cell_domains(self, int(target_col), rows, pair_idx, min_cnt, single_ok, beta, row_count)[0]  # noqa: E731
        keys, rows, weak = drop_weak(keys, set_cols, self.n, target_col, flags)
        self._set = (set_cols, keys)
        self._cells = (rows, np.full(len(rows), int(target_col), np.int32))
        return len(rows), weak

    def cellset_null(self):
        set_cols, keys = self._need_set("cellset_null")
        self.codes, m = null(keys, self.codes, set_cols)
        return m

    def cellset_rows(self, fetch=True):
        _, keys = self._need_set("cellset_rows")
        rows = rows_of(keys, self.n)
        self._cells = (rows, None)
        return rows if fetch else len(rows)


def _recorded(name):
    def call(self, *a, **kw):
        self.calls.append(name)
        return getattr(super(RecordingTable, self), name)(*a, **kw)
    call.__name__ = name
    return call


class RecordingTable(CellrunTable):
    """Every call of a `RECORDED` method is noted in `calls` (a list the engine shares among its tables) before it runs."""


for _name in RECORDED:
    setattr(RecordingTable, _name, _recorded(_name))


class CellrunEngine(CellsetEngine):
    """The oracle engine on `RecordingTable`s; `calls` is the record of all of them, `uploads` the tables made."""
    table_cls = RecordingTable

    def __init__(self):
        super().__init__()
        self.calls = []

    def _share(self, t):
        t.calls = self.calls
        return t

    def upload(self, codes, n_codes):
        return self._share(super().upload(codes, n_codes))

    def upload_dictionaries(self, indices, remaps):
        return self._share(super().upload_dictionaries(indices, remaps))

    def cell_uploads(self):
        return [c for c in self.calls if c in CELL_UPLOADS]


class _NoCellrunTable(CellsetTable):
    """A table of the previous library: the cell set without the four entries."""
    calls = None


class OldEngine(CellsetEngine):
    table_cls = _NoCellrunTable
