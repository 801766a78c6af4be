"""numpy restatements of rgbm_table_detect_dc and rgbm_table_detect_row_bits (include/rgbm.h), written from their semantics: blocked
O(n^2) over codes and rank arrays.  Shared by the CPU and the GPU tests of the resident denial constraints; no code of the product."""
import numpy as np


class Refused(Exception):
    """The restated RGBM_ERR_PARAM: the groups of the EQ attributes hold more pairs than `max_pairs`."""
    code = -2


def _cells(rows, cell_cols):
    cc = np.asarray(cell_cols, np.int32).reshape(-1)
    if len(cc) == 0:
        return rows
    return np.tile(rows, len(cc)), np.repeat(cc, len(rows)).astype(np.int32)


def _operand(codes, n_codes, col, rank):
    v = codes[col].astype(np.int64)
    v = np.where((v < 0) | (v >= int(n_codes[col])), -1, v)
    if rank is not None:
        r = np.asarray(rank, np.int64)
        assert len(r) == int(n_codes[col])
        v = np.where(v >= 0, r[np.maximum(v, 0)], -1)
        v = np.where(v < 0, -1, v)
    return v


def group_pairs(codes, n_codes, preds):
    """Sum of |g|^2 over the groups of the EQ attributes (one group without any)."""
    eq = [p[1] for p in preds if p[0] == "EQ"]
    n = codes.shape[1]
    if not eq:
        return n * n
    key = np.stack([_operand(codes, n_codes, c, None) for c in eq], axis=1)
    _, cnt = np.unique(key, axis=0, return_counts=True)
    return int((cnt.astype(np.int64) ** 2).sum())


def detect_dc(codes, n_codes, preds, cell_cols=(), max_pairs=0, block=256):
    """preds: [(op, left_col, right_col, left_rank, right_rank)], op in 'EQ' / 'IQ' / 'LT' / 'GT'.  Row i violates iff some row j
    (j == i included) makes every predicate true."""
    codes = np.asarray(codes, np.int32)
    n = codes.shape[1]
    if any(p[0] not in ("EQ",) for p in preds) and max_pairs > 0 and group_pairs(codes, n_codes, preds) > max_pairs:
        raise Refused("more pairs than max_pairs")
    sides = [(op, _operand(codes, n_codes, lc, lr), _operand(codes, n_codes, rc, rr)) for op, lc, rc, lr, rr in preds]
    viol = np.zeros(n, bool)
    for i0 in range(0, n, block):
        m = np.ones((min(block, n - i0), n), bool)
        for op, L, R in sides:
            l, r = L[i0:i0 + block, None], R[None, :]
            if op == "EQ":
                m &= l == r
            elif op == "IQ":
                m &= l != r
            elif op == "LT":
                m &= (l >= 0) & (r >= 0) & (l < r)
            else:
                m &= (l >= 0) & (r >= 0) & (l > r)
        viol[i0:i0 + block] = m.any(axis=1)
    return _cells(np.flatnonzero(viol).astype(np.int64), cell_cols)


def detect_row_bits(codes, n_codes, cols, bits, cell_cols=()):
    """bits[k]: uint64 words holding n_codes[cols[k]] + 1 bits, the last one for NULL.  A row violates iff its bit is set in every column."""
    codes = np.asarray(codes, np.int32)
    ok = np.ones(codes.shape[1], bool)
    for c, w in zip(cols, bits):
        nc = int(n_codes[c])
        flags = np.unpackbits(np.ascontiguousarray(w, "<u8").view(np.uint8), bitorder="little")[:nc + 1].astype(bool)
        v = codes[c].astype(np.int64)
        ok &= flags[np.where((v < 0) | (v >= nc), nc, v)]
    return _cells(np.flatnonzero(ok).astype(np.int64), cell_cols)
