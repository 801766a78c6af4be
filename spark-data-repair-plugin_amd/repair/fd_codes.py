"""The measures of a functional dependency X -> Y in code space: the numpy statement of `rgbm_table_fd_measures` (csrc/rgbm_fd.hip) and the
host path of `RepairMisc.discoverFunctionalDeps` when no device is present.

A code outside [0, n_codes[col]) reads as NULL, as `rgbm_table_detect_dc` reads it, and NULL is a value of its own on both sides (`<=>`),
as in `rgbm_table_detect_constraint`.  Every figure is an integer, so `fd_measures` DEFINES the result and the device entry returns the
same numbers, with no tolerance anywhere.
"""
from typing import Any, Dict, Sequence

import numpy as np

MAX_LHS = 11          # left-hand-side columns of one call (with the right-hand side, the 12 columns of a device key)


def _digits(codes: np.ndarray, n_codes: Sequence[int], col: int) -> np.ndarray:
    """code + 1, NULL (any code outside the dictionary) -> 0: the digit of the device's mixed-radix key."""
    v = codes[col].astype(np.int64)
    return np.where((v >= 0) & (v < int(n_codes[col])), v + 1, 0)


def check_lists(n_columns: int, lhs: Sequence[int], rhs_cols: Sequence[int]) -> None:
    """The argument refusals of `rgbm_table_fd_measures`, as ValueError."""
    lhs, rhs = [int(c) for c in lhs], [int(c) for c in rhs_cols]
    if len(lhs) > MAX_LHS:
        raise ValueError("at most %d left-hand-side columns" % MAX_LHS)
    if len(rhs) < 1:
        raise ValueError("at least one right-hand side")
    if any(c < 0 or c >= n_columns for c in lhs + rhs):
        raise ValueError("column index out of range")
    if len(set(lhs)) != len(lhs) or len(set(rhs)) != len(rhs):
        raise ValueError("a column is listed twice")
    if set(lhs) & set(rhs):
        raise ValueError("a right-hand side is also on the left-hand side")


def fd_measures(codes: Any, n_codes: Sequence[int], lhs: Sequence[int], rhs_cols: Sequence[int]) -> Dict[str, Any]:
    """One left-hand side X = `lhs` (0 .. 11 distinct columns; none: all rows form one group) of an int32 code table [C][n] against the
    right-hand sides `rhs_cols` (at least one, distinct, none in X).  All int64:

      groups          the number of distinct X-keys
      kept[r]         the sum, over the X-groups, of the largest number of rows of the group that share one value of Y = rhs_cols[r]
                      (n - kept = the fewest rows to remove for X -> Y to hold exactly: the g3 measure)
      violating[r]    the rows that lie in an X-group holding two or more distinct Y values
      xy_groups[r]    the number of distinct (X, Y) keys"""
    codes = np.asarray(codes, np.int32)
    check_lists(codes.shape[0], lhs, rhs_cols)
    n = codes.shape[1]
    gid = np.zeros(n, np.int64)                      # the dense id of every row's X-key; relabelled per column, so nothing can wrap
    groups = 1 if n else 0
    for c in lhs:
        uniq, gid = np.unique(gid * (max(int(n_codes[c]), 0) + 1) + _digits(codes, n_codes, int(c)), return_inverse=True)
        gid = gid.reshape(-1).astype(np.int64)
        groups = len(uniq)
    size = np.bincount(gid, minlength=groups).astype(np.int64)
    kept, violating, xy_groups = (np.zeros(len(rhs_cols), np.int64) for _ in range(3))
    for r, y in enumerate(rhs_cols):
        ny1 = max(int(n_codes[y]), 0) + 1
        uniq, count = np.unique(gid * ny1 + _digits(codes, n_codes, int(y)), return_counts=True)
        g = uniq // ny1
        best = np.zeros(groups, np.int64)
        np.maximum.at(best, g, count.astype(np.int64))
        distinct = np.bincount(g, minlength=groups)
        kept[r], violating[r], xy_groups[r] = best.sum(), size[distinct >= 2].sum(), len(uniq)
    return dict(groups=np.int64(groups), kept=kept, violating=violating, xy_groups=xy_groups)
