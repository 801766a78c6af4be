"""Fit once, repair later tables: what a resident repair run keeps of its fit, and how a later frame's codes reach it.

`FittedRepairModels` is everything an apply run needs and nothing it can recompute: the column names in table order, per column the
dictionary the FINAL pass of the fit run uploaded and its kind, the chain and, per chain target, its model blob, feature columns,
continuous / integral flags and y_values.  The reference left the apply run a TODO (python/repair/model.py:1094, "Runs the `repair` UDF
based on checkpoint files"); a picklable model handle is the checkpoint, this is what goes around it.

A later table has dictionaries of its own: its codes are ranks among ITS values.  `fitted_luts` gives, per column, the look-up table from
those codes to the fitted ones; `rgbm_table_recode` (csrc/rgbm_recode.hip; the statement is repair/recode_codes.py) applies them to the
dirty rows where they lie, in HBM.
"""
from typing import Any, Dict, List, Optional

import numpy as np

from repair.utils import setup_logger

_logger = setup_logger()

FORMAT = 1                  # of the file `save` writes; `load` refuses any other

_TAGS = {str: 0, bool: 1, int: 2, float: 3}     # the value types a dictionary may hold, as the file names them


def _library_version() -> int:
    from repair import _native
    return int(_native.lib().rgbm_version())


class FittedRepairModels:
    """columns [C]: the attribute names in table order;  dicts [C]: per column the ascending distinct values behind the fitted codes
    (float64 for a numeric column, an object array otherwise);  categorical [C]: the kind as `pipeline._upload` decides it (an object
    dictionary is categorical, a numeric one carries column values);  chain: the targets in prediction order;  targets {name: dict(blob:
    bytes, features: [names, in the fit's order], continuous, integral: bool, y_values: float64 array or None)};  rgbm_version: the
    library's numerics version at the fit;  version_mismatch: set by `load` when the running library's differs."""

    def __init__(self, columns: List[str], dicts: List[np.ndarray], categorical: List[bool], chain: List[str], targets: Dict[str, Dict[str, Any]],
                 rgbm_version: Optional[int] = None) -> None:
        self.columns = [str(c) for c in columns]
        self.dicts = [np.asarray(d) for d in dicts]
        self.categorical = [bool(k) for k in categorical]
        self.chain = [str(t) for t in chain]
        self.targets = {str(t): dict(d) for t, d in targets.items()}
        self.rgbm_version = _library_version() if rgbm_version is None else int(rgbm_version)
        self.format = FORMAT
        self.version_mismatch: Optional[str] = None
        if len(self.dicts) != len(self.columns) or len(self.categorical) != len(self.columns):
            raise ValueError("one dictionary and one kind per column expected")
        for t in self.chain:
            if t not in self.targets or t not in self.columns:
                raise ValueError("chain target `%s` has no kept model or is not a column" % t)
            unknown = [f for f in self.targets[t]["features"] if f not in self.columns]
            if unknown:
                raise ValueError("feature `%s` of target `%s` is not a column" % (unknown[0], t))

    @classmethod
    def from_pieces(cls, fit: Dict[str, Any]) -> "FittedRepairModels":
        """From the `fit` entry of `pipeline.repair_frame(keep_fit=True)`'s details."""
        return cls(fit["columns"], fit["dicts"], fit["categorical"], fit["chain"], fit["targets"])

    # ------------------------------------------------------------------ one file, no pickle
    def save(self, path: str) -> None:
        """One numpy archive, written (and read back) with allow_pickle=False: blobs as uint8 arrays, numeric dictionaries with their
        dtype, the others as unicode arrays with one type tag per entry.  ValueError, naming the column, for a dictionary that holds
        anything other than str, int, float or bool."""
        arrays: Dict[str, np.ndarray] = dict(format=np.array([FORMAT], np.int64), rgbm_version=np.array([self.rgbm_version], np.int64),
                                             columns=_unicode(self.columns), categorical=np.array(self.categorical, np.uint8),
                                             chain=_unicode(self.chain))
        for j, d in enumerate(self.dicts):
            if d.dtype != object:
                if d.dtype.kind not in "biuf":
                    raise ValueError("the dictionary of column `%s` holds %s values: only str, int, float and bool can be saved" % (self.columns[j], d.dtype))
                arrays["dict_%d" % j] = np.ascontiguousarray(d)
                continue
            tags = np.zeros(len(d), np.uint8)
            text = []
            for i, v in enumerate(d):
                v = v.item() if isinstance(v, np.generic) else v
                if type(v) not in _TAGS or (type(v) is str and v.endswith("\x00")):      # (a unicode array drops trailing NULs)
                    raise ValueError("the dictionary of column `%s` holds %r (%s): only str, int, float and bool can be saved"
                                     % (self.columns[j], v, type(v).__name__))
                tags[i] = _TAGS[type(v)]
                text.append(v if type(v) is str else repr(v))
            arrays["dict_%d" % j] = _unicode(text)
            arrays["tags_%d" % j] = tags
        for i, t in enumerate(self.chain):
            d = self.targets[t]
            arrays["blob_%d" % i] = np.frombuffer(bytes(d["blob"]), np.uint8)
            arrays["features_%d" % i] = _unicode(d["features"])
            arrays["flags_%d" % i] = np.array([bool(d["continuous"]), bool(d["integral"]), d.get("y_values") is not None], np.uint8)
            arrays["y_values_%d" % i] = np.asarray(d["y_values"] if d.get("y_values") is not None else [], np.float64)
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path: str) -> "FittedRepairModels":
        """Reads what `save` wrote.  ValueError for another format number; a different `rgbm_version()` is logged as a warning and
        recorded as `version_mismatch` (the models are bytes of that version's trainer; the predictor reads them as it reads any blob)."""
        with np.load(path, allow_pickle=False) as z:
            fmt = int(z["format"][0])
            if fmt != FORMAT:
                raise ValueError("%s holds a kept fit of format %d; this code reads format %d" % (path, fmt, FORMAT))
            columns = [str(c) for c in z["columns"]]
            categorical = [bool(k) for k in z["categorical"]]
            chain = [str(t) for t in z["chain"]]
            dicts = []
            for j in range(len(columns)):
                d = z["dict_%d" % j]
                if "tags_%d" % j in z.files:
                    tags = z["tags_%d" % j]
                    vals = np.empty(len(d), object)
                    vals[:] = [_untag(str(s), int(k)) for s, k in zip(d, tags)]
                    d = vals
                dicts.append(d)
            targets = {}
            for i, t in enumerate(chain):
                flags = z["flags_%d" % i]
                targets[t] = dict(blob=z["blob_%d" % i].tobytes(), features=[str(f) for f in z["features_%d" % i]], continuous=bool(flags[0]),
                                  integral=bool(flags[1]), y_values=np.asarray(z["y_values_%d" % i], np.float64) if flags[2] else None)
            version = int(z["rgbm_version"][0])
        out = cls(columns, dicts, categorical, chain, targets, rgbm_version=version)
        now = _library_version()
        if now != version:
            out.version_mismatch = "fitted with rgbm_version %d, applied with %d" % (version, now)
            _logger.warning("[Repairing Phase] %s: %s" % (path, out.version_mismatch))
        return out


def _unicode(strings: Any) -> np.ndarray:
    strings = [str(s) for s in strings]
    return np.array(strings, dtype=np.str_) if strings else np.zeros(0, dtype="<U1")


def _untag(s: str, tag: int) -> Any:
    if tag == 0:
        return s
    if tag == 1:
        return s == "True"
    return int(s) if tag == 2 else float(s)


def fitted_luts(fitted: FittedRepairModels, enc: Any) -> List[Optional[np.ndarray]]:
    """Per column of a later frame's `FrameEncoding`, the LUT from ITS codes to the fitted codes: int32 [max(len(enc.dicts[j]), 1)] (the
    codes of the table `enc` uploads), or None for a column the fit does not know (it is ignored: the codes stay).

      - a value found in the fitted dictionary gets its fitted code;
      - a CATEGORICAL value the fit never saw gets -1: the model treats it as missing, as it treats a category its training rows did not show;
      - a NUMERIC value the fit never saw gets the code of the nearest fitted value -- ties to the lower value, below the minimum the first
        code, above the maximum the last: `engine.nearest_code`, the rule of this code base for a number it has not seen, which agrees with
        LightGBM's midpoint bounds wherever both neighbours were training values;
      - every entry of an empty fitted dictionary is -1.
    ValueError, naming the column: a column numeric in one and object in the other; a fitted column absent from the frame."""
    from repair.engine import nearest_code
    at = {c: j for j, c in enumerate(fitted.columns)}
    for c in fitted.columns:
        if c not in enc.pos:
            raise ValueError("the fitted column `%s` is not in the frame" % c)
    luts: List[Optional[np.ndarray]] = []
    for j, c in enumerate(enc.columns):
        if c not in at:
            luts.append(None)
            continue
        new, old = enc.dicts[j], fitted.dicts[at[c]]
        lut = np.full(max(len(new), 1), -1, np.int32)
        if len(old) and len(new):
            if (new.dtype == object) != bool(fitted.categorical[at[c]]):
                raise ValueError("column `%s` is %s in the frame and %s in the fit" % (c, "categorical" if new.dtype == object else "numeric",
                                                                                    "categorical" if fitted.categorical[at[c]] else "numeric"))
            if new.dtype == object:
                code_of = {v: k for k, v in enumerate(old)}
                lut[:len(new)] = [code_of.get(v, -1) for v in new]
            else:
                lut[:len(new)] = nearest_code(np.asarray(old, np.float64), np.asarray(new, np.float64))
        luts.append(lut)
    return luts
