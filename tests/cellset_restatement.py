"""The plain numpy statement of the table's CELL SET (include/rgbm.h: rgbm_table_cellset_open / _add / _emit / _close), shared by the CPU
and the GPU tests; no code of the product.  The set is a set of keys  position-in-the-set's-columns * n + row ; emit is np.unique of
them plus codes[column, row].  `CellsetTable` / `CellsetEngine` put the four methods (and ``fetch=False`` on every detect method) on the
CPU tables of the other test modules, so that whole runs take the set's route without a device."""
import numpy as np

from tests import dc_scan_cases as S
from tests import detector_restatements as DR
from tests.helpers import OracleEngine
from tests.test_constraints_resident_cpu import DcTable
from tests.test_domain_analysis import _DomainTable


class Refused(Exception):
    """What `_native._check` raises for RGBM_ERR_PARAM."""
    code = -2


def new_set():
    return np.zeros(0, np.int64)


def add(keys, set_cols, n, c, rows, cols):
    """keys | the cells (rows, cols) whose column is in `set_cols` and that lie inside the n x c table."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    pos = np.full(c, -1, np.int64)
    pos[np.asarray(set_cols, np.int64)] = np.arange(len(set_cols))
    inside = (rows >= 0) & (rows < n) & (cols >= 0) & (cols < c)
    p = np.where(inside, pos[np.where(inside, cols, 0)], -1)
    keep = p >= 0
    return np.unique(np.concatenate([keys, p[keep] * n + rows[keep]]))


def emit(keys, codes, set_cols):
    """(rows int64, cols int32, codes int32, counts int64 [len(set_cols)]): by position in `set_cols`, then ascending row."""
    codes = np.asarray(codes, np.int32)
    n = codes.shape[1]
    keys = np.unique(np.asarray(keys, np.int64))
    rows, p = keys % n, keys // n
    cols = np.asarray(set_cols, np.int32)[p] if len(keys) else np.zeros(0, np.int32)
    return rows.astype(np.int64), cols.astype(np.int32), codes[cols.astype(np.int64), rows].astype(np.int32), \
        np.bincount(p, minlength=len(set_cols)).astype(np.int64)


class CellsetTable(DcTable, _DomainTable):
    """The CPU table of the resident tests with every detector entry, each taking ``fetch=False`` (the result stays as the table's cell
    list and the count is returned), and the cell set on top of the functions above."""
    set_calls = 0

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self._cells, self._set = (np.zeros(0, np.int64), np.zeros(0, np.int32)), None

    def _keep(self, res, fetch):
        self._cells = res if isinstance(res, tuple) else (res, None)          # a row list has no columns
        return res if fetch else len(self._cells[0])

    def detect_nulls(self, cols, fetch=True):
        return self._keep(super().detect_nulls(cols), fetch)

    def detect_cells(self, cols, null_is_error, keep_lo, keep_hi, flag_bits=None, fetch=True):
        return self._keep(DR.detect_cells(self.codes, cols, null_is_error, keep_lo, keep_hi, flag_bits), fetch)

    def detect_constraint(self, eq_cols, iq_col, cell_cols=(), fetch=True):
        return self._keep(super().detect_constraint(eq_cols, iq_col, cell_cols), fetch)

    def detect_dc(self, preds, cell_cols=(), max_pairs=0, fetch=True):
        return self._keep(super().detect_dc(preds, cell_cols, max_pairs), fetch)

    def detect_dc_scan(self, preds, cell_cols=(), fetch=True):
        return self._keep(S.scan_statement(self.codes, self.n_codes, preds, cell_cols), fetch)

    def detect_row_bits(self, cols, bits, cell_cols=(), fetch=True):
        return self._keep(super().detect_row_bits(cols, bits, cell_cols), fetch)

    def cellset_open(self, cols):
        cols = [int(x) for x in cols]
        if not 1 <= len(cols) <= self.c or len(set(cols)) != len(cols) or min(cols) < 0 or max(cols) >= self.c:
            raise ValueError("cellset_open: bad columns")
        CellsetTable.set_calls += 1
        self._set = (cols, new_set())

    def cellset_add(self):
        if self._set is None:
            raise Refused("cellset_add: no open cell set")
        rows, cols = self._cells
        if cols is None and len(rows):
            raise Refused("cellset_add: the last result is a row list")
        if len(rows):
            self._set = (self._set[0], add(self._set[1], self._set[0], self.n, self.c, rows, cols))

    def cellset_emit(self, fetch=True):
        if self._set is None:
            raise Refused("cellset_emit: no open cell set")
        rows, cols, codes, counts = emit(self._set[1], self.codes, self._set[0])
        self._cells = (rows, cols)
        return (rows, cols, codes, counts) if fetch else counts

    def cellset_close(self):
        self._set = None


class CellsetEngine(OracleEngine):
    """The oracle engine on `CellsetTable`s, with `lof_codes` (the numpy statement) and a count of its uploads."""
    table_cls = CellsetTable

    def __init__(self):
        self.uploads = 0

    def upload(self, codes, n_codes):
        self.uploads += 1
        return self.table_cls(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        self.uploads += 1
        return self.table_cls(t.codes, t.n_codes, t.values, t.kinds)

    def lof_codes(self, values, counts, k=20):
        from repair import lof_codes as L
        return L.lof_codes(values, counts, k)
