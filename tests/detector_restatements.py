"""numpy restatement of rgbm_table_detect_cells (include/rgbm.h), shared by the CPU and the GPU tests of the value detectors."""
import numpy as np


def detect_cells(codes, cols, null_is_error, keep_lo, keep_hi, flag_bits):
    """codes [C][N] int32 (-1 = NULL) -> (rows int64, cols int32), ordered by position in `cols`, then ascending row.
    Cell (row, cols[j]) with code v is an error iff  v < 0 and null_is_error[j];  or v >= 0, keep_lo[j] <= keep_hi[j] and
    (v < keep_lo[j] or v > keep_hi[j]);  or v >= 0, flag_bits[j] is not None and bit v of it is set."""
    codes = np.asarray(codes, np.int32)
    cols = [int(c) for c in cols]
    if len(set(cols)) != len(cols) or any(c < 0 or c >= codes.shape[0] for c in cols):
        raise ValueError("columns must be distinct and in range")
    flag_bits = list(flag_bits) if flag_bits is not None else [None] * len(cols)
    out_r, out_c = [], []
    for j, c in enumerate(cols):
        v = codes[c].astype(np.int64)
        ok = v >= 0
        bad = (v < 0) & bool(null_is_error[j])
        lo, hi = int(keep_lo[j]), int(keep_hi[j])
        if lo <= hi:
            bad |= ok & ((v < lo) | (v > hi))
        if flag_bits[j] is not None:
            w = np.asarray(flag_bits[j], np.uint64)
            inside = ok & ((v >> 6) < len(w))
            vv = np.where(inside, v, 0)
            bit = (w[vv >> 6] >> (vv & 63).astype(np.uint64)) & np.uint64(1) if len(w) else np.zeros(len(v), np.uint64)
            bad |= inside & (bit != 0)
        r = np.flatnonzero(bad).astype(np.int64)
        out_r.append(r)
        out_c.append(np.full(len(r), c, np.int32))
    if not out_r:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    return np.concatenate(out_r), np.concatenate(out_c)
