"""The dictionary encoding of a DataFrame's columns as the resident pipeline uploads it, and the edits `repair_frame` makes to it on the
host before the table is (re)built: NULL the known error cells, drop the classes only they held, write rule-repaired values back."""
import numpy as np


class FrameEncoding:
    """Columns `columns` of an n-row frame: `indices` [C][n] int32, the dictionary ENTRY of every cell in order of first appearance
    (-1 = NULL); `remaps[j][entry]`, the CODE of an entry; `dicts[j][code]`, the value behind a code; `pos`, column name -> j.

    The invariant, which every method keeps and `check()` states: `dicts[j]` holds distinct values in ascending order (strings by code
    point, numbers numerically: float64, NaN is NULL and never an entry), and the code of every entry that some row refers to is the
    rank of its value in `dicts[j]` -- the contract of `repair.encode`, so that codes mean the same on the value-space and on the
    resident path, and what `table_stats`, `depgraph`, `dc_codes` and `detect_codes` read off the dictionaries.  An entry no row refers
    to any more (pruned by `null_cells`) keeps a slot in `remaps[j]` whose content means nothing.  The table is built from (`indices`,
    `remaps`) on the device (`Table.from_dictionaries`); column j has max(remaps[j]) + 1 codes.

    What cells held before they were NULLed here is kept by (column, row) (`hold`; the first value recorded for a cell stays):
    `current_values` answers from it before it decodes."""

    def __init__(self, columns, indices, remaps, dicts):
        self.columns, self.indices, self.remaps, self.dicts = list(columns), indices, list(remaps), list(dicts)
        self.n = int(indices.shape[1])
        self.pos = {c: j for j, c in enumerate(self.columns)}
        self._held_keys, self._held_values = np.zeros(0, np.int64), np.zeros(0, object)

    @classmethod
    def of_frame(cls, df, columns):
        """The per-row work (value -> entry) is one hash pass per column (`pandas.factorize`: 42 ms per 10^6 string cells, against 67-105 ms
        for an Arrow `dictionary_encode` of the same column); the entry -> code gather runs on the device."""
        import pandas as pd
        idx, remaps, dicts = [], [], []
        for c in columns:
            s = df[c]
            numeric = pd.api.types.is_numeric_dtype(s) and not pd.api.types.is_bool_dtype(s)
            if numeric:
                codes, uniq = pd.factorize(s.to_numpy(dtype="float64", na_value=np.nan), use_na_sentinel=True)
            else:
                # one hash pass per column and run: inside RepairModel.run() the NULL detector / domain statistics have factorised the column
                # already (repair.utils.column_code_cache); categorical / Arrow-backed columns factorise through their own dictionary or buffer
                from repair.utils import column_factorize
                codes, uniq = column_factorize(df, c)
            vals = np.asarray(uniq, dtype=np.float64 if numeric else object)
            order = np.argsort(vals, kind="stable")
            remap = np.empty(len(vals), np.int32)
            remap[order] = np.arange(len(vals), dtype=np.int32)
            idx.append(codes.astype(np.int32, copy=False))
            remaps.append(remap)
            dicts.append(vals[order])
        return cls(columns, np.stack(idx) if idx else np.zeros((0, len(df)), np.int32), remaps, dicts)

    def decode(self, codes, cols):
        """The values behind (codes, column positions), None for -1."""
        codes, cols = np.asarray(codes), np.asarray(cols)
        out = np.empty(len(codes), object)
        for j in np.unique(cols):
            sel = cols == j
            c = codes[sel]
            v = np.empty(len(c), object)
            ok = c >= 0
            v[ok] = self.dicts[j][c[ok]]
            v[~ok] = None
            out[sel] = v
        return out

    def values(self, rows, j):
        """The raw values of the cells (rows, column j), None for NULL."""
        idx = self.indices[j, rows]
        v = np.empty(len(idx), object)
        v[idx >= 0] = self.dicts[j][self.remaps[j][idx[idx >= 0]]]
        v[idx < 0] = None
        return v

    def live_classes(self, j):
        """How many distinct values the rows of column j hold."""
        return len(np.unique(self.indices[j][self.indices[j] >= 0]))

    def null_cells(self, rows, cols, prune=()):
        """NULL the cells and drop the values that ONLY they held from the dictionaries of the columns `prune` -- the reference counts a
        target's classes over the frame with the error cells removed (model.py:1005, count(distinct y)), and num_class enters the softmax
        hessian factor K / (K - 1): a dead class would change every tree.  Returns what the cells held, which is kept (`hold`)."""
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int32)
        held = np.empty(len(rows), object)
        for j in np.unique(cols):
            held[cols == j] = self.values(rows[cols == j], j)
        self.indices[cols, rows] = -1
        for j in sorted(prune):
            remap = self.remaps[j]
            live = np.bincount(self.indices[j][self.indices[j] >= 0], minlength=len(remap)) > 0
            if not live.all():
                live_codes = np.sort(remap[live])                         # surviving old codes, ascending
                new = np.zeros(len(remap), np.int32)
                new[live] = np.searchsorted(live_codes, remap[live]).astype(np.int32)
                self.dicts[j], self.remaps[j] = self.dicts[j][live_codes], new
        self.hold(rows, cols, held)
        return held

    def write(self, j, rows, values):
        """Write `values` into the cells (rows, column j).  A value the column does not hold becomes a dictionary entry at its rank: the
        codes at and above it move up by one, so they stay the ascending ranks."""
        rows, values = np.asarray(rows, np.int64), np.asarray(values, object)
        for v in dict.fromkeys(values):
            k = int(np.searchsorted(self.dicts[j], v))
            if k < len(self.dicts[j]) and self.dicts[j][k] == v:
                entry = int(np.flatnonzero(self.remaps[j] == k)[0])
            else:
                remap = self.remaps[j]
                self.remaps[j] = np.append(np.where(remap >= k, remap + 1, remap), np.int32(k)).astype(np.int32)
                entry = len(remap)
                self.dicts[j] = np.concatenate([self.dicts[j][:k], np.array([v], self.dicts[j].dtype), self.dicts[j][k:]])
            self.indices[j, rows[values == v]] = entry

    def hold(self, rows, cols, values):
        """Record what cells held; a cell recorded before keeps its first value."""
        key, first = np.unique(np.asarray(cols, np.int64) * self.n + np.asarray(rows, np.int64), return_index=True)
        fresh = ~np.isin(key, self._held_keys)
        keys = np.concatenate([self._held_keys, key[fresh]])
        order = np.argsort(keys, kind="stable")
        self._held_keys, self._held_values = keys[order], np.concatenate([self._held_values, np.asarray(values, object)[first[fresh]]])[order]

    def current_values(self, rows, cols, codes):
        """What the cells held: the recorded value where there is one (they were NULLed here, before the upload), else the code decoded."""
        out = self.decode(codes, cols)
        if len(self._held_keys) and len(out):
            key = np.asarray(cols, np.int64) * self.n + np.asarray(rows, np.int64)
            at = np.minimum(np.searchsorted(self._held_keys, key), len(self._held_keys) - 1)
            hit = self._held_keys[at] == key
            out[hit] = self._held_values[at[hit]]
        return out

    def check(self):
        """The invariant of the class docstring, asserted (tests call it; the production path does not)."""
        assert self.indices.shape == (len(self.columns), self.n) and len(self.remaps) == len(self.dicts) == len(self.columns)
        for j, (remap, d) in enumerate(zip(self.remaps, self.dicts)):
            idx = self.indices[j]
            used = np.unique(idx[idx >= 0])
            assert idx.min(initial=-1) >= -1 and (len(used) == 0 or used[-1] < len(remap)), "column %d: an index outside its entries" % j
            assert all(d[i] < d[i + 1] for i in range(len(d) - 1)), "column %d: the dictionary is not ascending and distinct" % j
            assert d.dtype == object or not np.isnan(d).any(), "column %d: NaN is an entry" % j
            codes = remap[used]
            assert len(np.unique(codes)) == len(codes) and (len(codes) == 0 or (codes.min() >= 0 and codes.max() < len(d))), \
                "column %d: the codes of its live entries are not distinct ranks" % j
            assert len(remap) == 0 or int(remap.max()) + 1 <= max(len(d), 1), "column %d: a code beyond the dictionary" % j
        assert (np.diff(self._held_keys) > 0).all() and len(self._held_keys) == len(self._held_values)
