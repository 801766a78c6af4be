"""numpy restatements of the three library entries of the rule-based repairs (include/rgbm.h: rgbm_table_fd_map, rgbm_table_rule_fill,
rgbm_nearest_values), shared by the CPU engine of tests/test_rule_resident_cpu.py and the device comparisons of tests/test_gpu_rules.py,
and the synthetic frames both use."""
import numpy as np
import pandas as pd

from repair.costs import edit_distance


def fd_map(codes, n_codes, x, y):
    """`RepairModel._build_rule_model` on codes: per x code the single y code it occurs with over the rows where both are non-NULL."""
    xv, yv = np.asarray(codes[x], np.int64), np.asarray(codes[y], np.int64)
    ok = (xv >= 0) & (yv >= 0)
    lo = np.full(int(n_codes[x]), np.iinfo(np.int32).max, np.int64)
    hi = np.full(int(n_codes[x]), -1, np.int64)
    np.minimum.at(lo, xv[ok], yv[ok])
    np.maximum.at(hi, xv[ok], yv[ok])
    return np.where(lo == hi, lo, -1).astype(np.int32)


def rule_fill(codes, y, x, lut, row_begin, n_rows):
    """One rule step in place on rows [row_begin, row_begin + n_rows): returns pred per row."""
    lut = np.asarray(lut, np.int32)
    sl = slice(row_begin, row_begin + n_rows)
    if x < 0:
        pred = np.full(n_rows, lut[0], np.int32)
    else:
        xv = codes[x, sl]
        pred = np.where((xv >= 0) & (xv < len(lut)), lut[np.clip(xv, 0, len(lut) - 1)], -1).astype(np.int32)
    col = codes[y, sl]
    codes[y, sl] = np.where((col < 0) & (pred >= 0), pred, col)
    return pred


def nearest(cost, threshold):
    """Per row of a cost matrix (NaN = no cost) the position of its minimum when it is unique and <= threshold, else -1."""
    cost = np.asarray(cost, np.float64)
    out = np.full(cost.shape[0], -1, np.int32)
    for i, row in enumerate(cost):
        ok = ~np.isnan(row)
        if not ok.any():
            continue
        m = row[ok].min()
        at = np.flatnonzero(ok & (row == m))
        if len(at) == 1 and m <= threshold:
            out[i] = at[0]
    return out


def nearest_strings(a, b, threshold):
    if len(b) == 0:
        return np.full(len(a), -1, np.int32)
    return nearest(np.array([[edit_distance(x, y) for y in b] for x in a], np.float64).reshape(len(a), len(b)), threshold)


FD_CONSTRAINTS = "t1&t2&EQ(t1.c0,t2.c0)&IQ(t1.c1,t2.c1);t1&t2&EQ(t1.c1,t2.c1)&IQ(t1.c2,t2.c2)"


def fd_frame(n=2000, seed=3):
    """(frame, error cells): six string columns with c0 -> c1 -> c2 (a chain; c0 is itself a statistical-model target).  Among the error
    cells of c1 there are cells whose c0 value maps to one c1 value, cells whose c0 value (a05) is left with two c1 values in rows that are
    NOT error cells (a conflict), and cells whose c0 value (a19) occurs in no row with a c1 value left.  The error cells are GIVEN: cells
    found by the constraint detector would take every conflicting group out of the table, so no conflict could survive the NULL-out."""
    rng = np.random.default_rng(seed)
    k0 = rng.integers(0, 19, n)
    k0[rng.choice(n, 30, replace=False)] = 19
    k1 = k0 % 10
    k2 = k1 % 4
    c3 = (k0 + rng.integers(0, 3, n)) % 7
    c4 = rng.integers(0, 5, n)
    c5 = (k2 + rng.integers(0, 2, n)) % 3
    odd = np.flatnonzero(k0 == 5)[:6]
    k1[odd] = 9                                            # a05 occurs with b05 and b09: no single value
    df = pd.DataFrame({"tid": np.arange(n), "c0": ["a%02d" % v for v in k0], "c1": ["b%02d" % v for v in k1], "c2": ["c%d" % v for v in k2],
                       "c3": ["d%d" % v for v in c3], "c4": ["e%d" % v for v in c4], "c5": ["f%d" % v for v in c5]})
    cells = []
    pick = rng.choice(n, 260, replace=False)
    for i, r in enumerate(pick):
        cells.append((int(r), "c%d" % (i % 3)))
        if i % 5 == 0:
            cells.append((int(r), "c%d" % ((i + 1) % 3)))
    cells += [(int(r), "c1") for r in np.flatnonzero(k0 == 19)]          # a19: every c1 cell next to it is an error cell
    cells += [(int(r), "c1") for r in np.flatnonzero(k0 == 5)[6:10]]     # cells whose source is in conflict
    cells += [(int(r), "c4") for r in rng.choice(n, 40, replace=False)]
    cells = pd.DataFrame(sorted(set(cells)), columns=["tid", "attribute"])
    for j, (r, a) in enumerate(zip(cells["tid"], cells["attribute"])):
        if j % 2 == 0:
            df.loc[r, a] = None                              # half of the error cells are NULL, the others hold a (wrong) value
    return df, cells


def fd_detect_frame(n=2000, seed=4):
    """The frame for DETECTED cells (NULL + constraint detectors over FD_CONSTRAINTS): c0 has 60 values, so a violating group is small.
    NULLs in c0 and c4; two rows of group a05 hold another c1 value and one row of group a07 a NULL c1 (both groups are flagged whole,
    in c0 and c1); one row of group b03 holds another c2 value (the group is flagged in c1 and c2)."""
    rng = np.random.default_rng(seed)
    k0 = rng.integers(0, 60, n)
    k1 = k0 % 10
    k2 = k1 % 4
    c3 = (k0 + rng.integers(0, 3, n)) % 7
    c4 = rng.integers(0, 5, n)
    c5 = (k2 + rng.integers(0, 2, n)) % 3
    df = pd.DataFrame({"tid": np.arange(n), "c0": ["a%02d" % v for v in k0], "c1": ["b%02d" % v for v in k1], "c2": ["c%d" % v for v in k2],
                       "c3": ["d%d" % v for v in c3], "c4": ["e%d" % v for v in c4], "c5": ["f%d" % v for v in c5]})
    df.loc[np.flatnonzero(k0 == 5)[:2], "c1"] = "b09"
    df.loc[np.flatnonzero(k0 == 7)[0], "c1"] = None
    df.loc[np.flatnonzero(k1 == 3)[0], "c2"] = "c0"
    other = np.flatnonzero((k0 != 5) & (k0 != 7))
    df.loc[rng.choice(other, 40, replace=False), "c0"] = None
    df.loc[rng.choice(n, 40, replace=False), "c4"] = None
    return df
