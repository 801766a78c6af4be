"""A plain restatement of the cell-domain analysis (include/rgbm.h rgbm_table_pair_counts, rgbm_table_cell_domains), written without
`repair.domain`: what tests/test_gpu_domain_edges.py holds the kernels of csrc/rgbm_domain.hip to, and tests/test_domain_restatement_cpu.py
the product's numpy.  Counts are integers; every probability is a chain of IEEE double operations with one rounding each -- a subtraction,
a maximum, a division, an addition -- in the order the header gives, so both sides are compared byte for byte.  `plan` restates the rule by
which the library packs pairs into LDS groups and sizes its grid (the report of rgbm_table_pair_counts_report)."""
import numpy as np


def bins(codes, n_codes, luts, n_bins):
    """[c][n] int64 bins of a code matrix: a code that is NULL, below -1 or >= n_codes[col] goes to the NULL slot n_bins[col]; every other
    code goes through the column's LUT, if it has one; a result outside [0, n_bins[col]) goes to the NULL slot."""
    codes = np.asarray(codes)
    luts = luts or {}
    out = np.zeros(codes.shape, np.int64)
    for col in range(codes.shape[0]):
        d = int(n_bins[col])
        v = codes[col].astype(np.int64)
        b = np.full(len(v), d, np.int64)
        ok = (v >= 0) & (v < int(n_codes[col]))
        w = v[ok] if luts.get(col) is None else np.asarray(luts[col], np.int64)[v[ok]]
        b[ok] = np.where((w < 0) | (w >= d), d, w)
        out[col] = b
    return out


def pair_counts(codes, n_codes, pairs, luts, n_bins):
    """The dense (n_bins[x] + 1) x (n_bins[y] + 1) int64 table of every pair (x, y), NULL in the last slot of each side."""
    b = bins(codes, n_codes, luts, n_bins)
    out = []
    for x, y in pairs:
        t = np.zeros((int(n_bins[x]) + 1, int(n_bins[y]) + 1), np.int64)
        np.add.at(t, (b[x], b[y]), 1)
        out.append(t)
    return out


def cell_domains(codes, target, rows, joints, orientation, min_cnt, single_ok, beta, row_count, n_codes, luts=None, n_bins=None, info=None):
    """One Python loop per cell, in Python floats.

    joints[j]       the dense table of the pair that holds the target and correlated attribute j, as `pair_counts` returns it
    orientation[j]  (correlated column, True where the target is the x side of that pair)
    Returns (weak [m] uint8, top [m] int32, top_prob [m] float64, probs [m][d_a] float64).  `info`, a dict, receives what the generators
    assert on: wiped = cells whose fold an attribute wiped, tenth = cells with an element of count 1 (the 0.1 branch), tied = cells whose
    largest probability two or more values share."""
    codes = np.asarray(codes)
    n = codes.shape[1]
    n_bins = {c: int(n_codes[c]) for c in range(codes.shape[0])} if n_bins is None else n_bins
    b = bins(codes, n_codes, luts, n_bins)
    d_a, k, R = int(n_bins[target]), len(joints), float(row_count)
    assert len(single_ok) == d_a and len(orientation) == k and len(min_cnt) == k
    m = len(rows)
    weak, top, top_prob, probs = np.zeros(m, np.uint8), np.full(m, -1, np.int32), np.zeros(m, np.float64), np.zeros((m, d_a), np.float64)
    wiped = tenth = tied = 0
    for i in range(m):
        r = int(rows[i])
        if r < 0 or r >= n:
            continue                                            # a row outside the table: the empty domain
        cnts, j0 = [], 0
        for j in range(k):
            col, target_is_x = orientation[j]
            v, d_c = int(b[col, r]), int(n_bins[col])
            if v < d_c:
                line = joints[j][:d_a, v] if target_is_x else joints[j][v, :d_a]
                cnts.append([int(c) for c in line])
            else:
                cnts.append(None)                               # the correlated value is NULL
            mc = max(int(min_cnt[j]), 0)
            if cnts[j] is None or not any(c > mc for c in cnts[j]):
                j0 = j + 1                                      # no element: the fold before it is wiped
        wiped += int(j0 > 0)
        score, one = [], False
        for c in range(d_a):
            s = 0.0
            if single_ok[c]:
                for j in range(j0, k):
                    cnt = cnts[j][c]
                    if cnt > max(int(min_cnt[j]), 0):
                        one = one or cnt == 1
                        s = s + max(float(cnt) - 1.0, 0.1) / R
            score.append(s)
        tenth += int(one)
        den = 0.0
        if j0 < k:
            for c in range(d_a):
                den = den + score[c]
        best, bt, nbest = 0.0, -1, 0
        for c in range(d_a):
            p = score[c] / den if (j0 < k and den > 0.0) else 0.0
            probs[i, c] = p
            if p > best:
                best, bt, nbest = p, c, 1
            elif p == best and bt >= 0:
                nbest += 1
        tied += int(nbest > 1)
        valid = bt >= 0 and best > beta
        cur = int(codes[target, r])
        if cur < 0 or cur >= d_a:
            cur = -1
        weak[i] = 1 if (valid and cur >= 0 and cur == bt) else 0
        top[i] = bt if valid else -1
        top_prob[i] = best if valid else 0.0
    if info is not None:
        info.update(wiped=wiped, tenth=tenth, tied=tied)
    return weak, top, top_prob, probs


def plan(pairs, n_bins, n, lds_cells, max_cols, block=512):
    """The grouping rule and the grid of rgbm_table_pair_counts, in the shape of `Table.pair_counts_report()`: pairs in the given order; a
    pair above `lds_cells` on its own takes the HBM kernel (group -1); a group is closed before a pair whose cells or whose new columns
    would not fit.  Workgroups: about 16 blocks of rows each, at most 2048 // groups per group, rows per workgroup a multiple of the block."""
    out, cols, cells, group, largest, any_group = [], [], 0, 0, 0, False
    for x, y in pairs:
        c = (int(n_bins[x]) + 1) * (int(n_bins[y]) + 1)
        if c > lds_cells:
            out.append(dict(group=-1, slot_x=-1, slot_y=-1))
            continue
        need = (x not in cols) + (y not in cols)
        if cols and (cells + c > lds_cells or len(cols) + need > max_cols):
            group, cols, cells = group + 1, [], 0
        for col in (x, y):
            if col not in cols:
                cols.append(col)
        out.append(dict(group=group, slot_x=cols.index(x), slot_y=cols.index(y)))
        cells, any_group = cells + c, True
        largest = max(largest, cells)
    groups = group + 1 if any_group else 0
    grid_x = rows_per_wg = 0
    if groups:
        chunks = max(min(-(-n // (16 * block)), max(1, 2048 // groups)), 1)
        per_chunk = -(-n // chunks)
        rows_per_wg = -(-per_chunk // block) * block
        grid_x = -(-n // rows_per_wg)
    return dict(pairs=out, groups=groups, max_group_cells=largest, grid_x=grid_x, rows_per_wg=rows_per_wg, lds_cells=lds_cells, max_cols=max_cols)
