"""A code table translated into another code space: the numpy statement of `rgbm_table_recode` (csrc/rgbm_recode.hip) and what an
engine without a device runs when a kept fit is applied to a later table (repair/fitted.py).

A code outside [0, n_codes[col]) reads as NULL, as everywhere in the library.  Every figure is an integer, so `recode` DEFINES the
result and the device entry returns the same numbers, with no tolerance anywhere.
"""
from typing import Any, Optional, Sequence, Tuple

import numpy as np


def check_luts(n_codes: Sequence[int], luts: Sequence[Optional[Any]], n_codes_out: Sequence[int]) -> None:
    """The argument refusals of `rgbm_table_recode`, as ValueError."""
    if len(luts) != len(n_codes) or len(n_codes_out) != len(n_codes):
        raise ValueError("one LUT (or None) and one output dictionary size per column expected")
    for j, lut in enumerate(luts):
        if int(n_codes_out[j]) < 1:
            raise ValueError("column %d has an output dictionary of %d codes (at least 1)" % (j, int(n_codes_out[j])))
        if lut is None:
            if int(n_codes_out[j]) != int(n_codes[j]):
                raise ValueError("identity column %d changes its dictionary size (%d -> %d)" % (j, int(n_codes[j]), int(n_codes_out[j])))
            continue
        lut = np.asarray(lut)
        if len(lut) != max(int(n_codes[j]), 0):
            raise ValueError("the LUT of column %d has %d entries, its dictionary %d" % (j, len(lut), int(n_codes[j])))
        bad = np.flatnonzero((lut < -1) | (lut >= int(n_codes_out[j])))
        if len(bad):
            raise ValueError("column %d, LUT entry %d = %d is outside [-1, %d)" % (j, int(bad[0]), int(lut[bad[0]]), int(n_codes_out[j])))


def recode(codes: Any, n_codes: Sequence[int], luts: Sequence[Optional[Any]], n_codes_out: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    """codes [C][n] int32 with the dictionary sizes `n_codes` -> (codes_out [C][n] int32, unmapped [C] int64).

    A cell whose code is outside [0, n_codes[j]) is NULL (-1) in the result.  Under `luts[j] is None` every other code stays (and
    `n_codes_out[j]` must equal `n_codes[j]`); otherwise the cell holds `luts[j][code]`, an entry of [-1, n_codes_out[j]).
    unmapped[j] = cells of column j that were not NULL and are NULL in the result."""
    codes = np.asarray(codes, np.int32)
    check_luts(n_codes, luts, n_codes_out)
    out = np.full(codes.shape, -1, np.int32)
    unmapped = np.zeros(codes.shape[0], np.int64)
    for j, lut in enumerate(luts):
        v = codes[j]
        ok = (v >= 0) & (v < int(n_codes[j]))
        if lut is None:
            out[j][ok] = v[ok]
        else:
            out[j][ok] = np.asarray(lut, np.int32)[v[ok]]
            unmapped[j] = int((out[j][ok] < 0).sum())
    return out, unmapped
