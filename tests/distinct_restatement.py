"""numpy restatement of rgbm_table_distinct_rows (include/rgbm.h): the definition of its result, written without a hash.

Rows are equal when all their codes are; NULL (-1) is a value of its own.  Groups come in order of FIRST OCCURRENCE, a group of cnt rows is
kept as ceil(cnt / 255) consecutive copies with the multiplicities 255, .., 255, cnt - 255 * (copies - 1) (the split rule of
repair.pipeline.distinct_rows, whose groups come in key order instead), inverse[i] = position of the first copy of row i's group."""
import numpy as np

MAX_MULT = 255


def distinct_rows(codes, max_mult=MAX_MULT):
    """codes [C][N] int32 -> (distinct [C][M] int32, mult [M] uint8, inverse [N] int64)."""
    codes = np.ascontiguousarray(codes, np.int32)
    C, N = codes.shape
    # groups of equal rows: a stable lexicographic sort of the rows, group borders where any column changes
    order = np.lexsort(codes[::-1])                              # stable: within a group the positions stay ascending
    s = codes[:, order]
    border = np.ones(N, bool)
    border[1:] = (s[:, 1:] != s[:, :-1]).any(axis=0)
    gid_sorted = np.cumsum(border) - 1                           # group number in key order
    first_sorted = order[border]                                 # first (smallest) position of each group
    counts_sorted = np.diff(np.append(np.flatnonzero(border), N))
    by_first = np.argsort(first_sorted, kind="stable")           # groups in order of first occurrence
    rank = np.empty(len(by_first), np.int64)
    rank[by_first] = np.arange(len(by_first))
    first, counts = first_sorted[by_first], counts_sorted[by_first]
    group_of_row = np.empty(N, np.int64)
    group_of_row[order] = rank[gid_sorted]
    copies = (counts + max_mult - 1) // max_mult
    start = np.concatenate([[0], np.cumsum(copies)[:-1]]).astype(np.int64)
    rows = np.repeat(first, copies)
    mult = np.full(len(rows), max_mult, np.int64)
    mult[start + copies - 1] = counts - (copies - 1) * max_mult
    return np.ascontiguousarray(codes[:, rows]), mult.astype(np.uint8), start[group_of_row]


def expand(distinct, inverse):
    """The table a distinct table stands for."""
    return np.ascontiguousarray(np.asarray(distinct)[:, np.asarray(inverse, np.int64)])
