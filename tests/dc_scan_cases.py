"""Tables, predicate sets and a vectorised numpy statement for the order constraints that rgbm_table_detect_dc_scan (include/rgbm.h)
answers by sort and scan.  Shared by the CPU and the GPU tests of that entry; no code of the product.  The O(n^2) restatement
tests/dc_restatement.py::detect_dc is the yardstick of both: `scan_statement` is held to it on the CPU, and stands in for it where
n^2 is out of reach."""
import numpy as np

G, A, B, G2 = 0, 1, 2, 3                 # group column, two ranked value columns, a second (small) group column
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
SHAPES = ("singletons", "one", "mixed")


def group_sizes(n, tile):
    """`mixed`: groups of exactly tile + 1, tile, tile - 1, 65, 64, 63, 2 and 1 rows, largest first, each taken while it leaves at least
    as many rows again for the others; the rest in groups of 1 to 5 rows (drawn by the caller)."""
    sizes, left = [], n
    for s in (tile + 1, tile, tile - 1, 65, 64, 63, 2, 1):
        if 2 * s <= left + 1:
            sizes.append(s)
            left -= s
    return sizes, left


def three_sizes(n):
    """`three`: three groups of about 40 %, 35 % and 25 % of the rows.  However the device lays them out, two of them straddle an inner
    boundary of the positions -- for the caller to check with `straddles` at the boundary it is after."""
    a, b = n * 2 // 5, n * 7 // 20
    return [a, b, n - a - b]


def straddles(sizes, every):
    """Whether in EVERY order of groups of these sizes some group lies on both sides of each multiple of `every` inside the table."""
    from itertools import permutations
    n = sum(sizes)
    inner = set(range(every, n, every))
    return all(not (inner & set(np.cumsum(p)[:-1].tolist())) for p in permutations(sizes)) and bool(inner)


def make_table(n, shape, tile, seed=0, values=None):
    """codes [4][n] int32 and n_codes [4].  A and B: about 10 % NULLs, a NULL at row 0, at row n - 1 and on either side of every
    multiple of `tile`, and one code beyond the dictionary each; `mixed` has NULL and beyond-dictionary codes in G as well (one group)."""
    rng = np.random.default_rng(seed * 7919 + n)
    k = int(values or max(2, min(n, 40)))
    if shape == "singletons":
        g = rng.permutation(n)
        ng = n
    elif shape == "one":
        g = np.zeros(n, np.int64)
        ng = 1
    elif shape == "three":
        g = rng.permutation(np.repeat(np.arange(3), three_sizes(n)))
        ng = 3
    else:
        sizes, left = group_sizes(n, tile)
        while left > 0:
            s = int(min(rng.integers(1, 6), left))
            sizes.append(s)
            left -= s
        g = np.repeat(np.arange(len(sizes)), sizes)
        ng = len(sizes)
        small = np.flatnonzero(g >= min(8, ng - 1))
        if len(small) >= 4:                      # a NULL group: NULL and a code beyond the dictionary fall together
            g[small[-1]] = -1
            g[small[-2]] = ng + 3
            g[small[-3]] = -1
        g = g[rng.permutation(n)]
    cols = [g]
    for c in (A, B):
        v = rng.integers(0, k, n)
        v[rng.random(n) < 0.1] = -1
        edges = [0, n - 1] + [e + d for e in range(tile, n + 1, tile) for d in (-1, 0)]
        v[[e for e in edges if 0 <= e < n]] = -1
        if n >= 3:
            v[int(rng.integers(1, n - 1))] = k + c          # beyond the dictionary: NULL to every predicate
        cols.append(v)
    cols.append(rng.integers(-1, 3, n))
    return np.stack(cols).astype(np.int32), np.asarray([max(ng, 1), k, k, 3], np.int32)


def rank_arrays(n_codes, seed=0):
    """rank arrays with ties and "no number" entries: (A's own, B's own, A's and B's in one merged order)."""
    rng = np.random.default_rng(seed + 101)
    ka, kb = int(n_codes[A]), int(n_codes[B])

    def ranks(k, top):
        r = rng.integers(0, max(top, 1), k)
        r[rng.random(k) < 0.1] = -1
        return r.astype(np.int32)
    return ranks(ka, ka // 2 + 1), ranks(kb, kb // 2 + 1), ranks(ka, ka + kb), ranks(kb, ka + kb)


def pred_sets(n_codes, seed=0):
    """{name: [(op, left column, right column, left rank, right rank)]}"""
    ra, rb, ma, mb = rank_arrays(n_codes, seed)
    eq = ("EQ", G, G, None, None)
    return {
        "eq_gt_lt": [eq, ("GT", A, A, None, None), ("LT", B, B, None, None)],
        "eq_gt_lt_ranked": [eq, ("GT", A, A, ra, ra), ("LT", B, B, rb, rb)],
        "eq_lt_across": [eq, ("LT", A, B, ma, mb)],
        "gt_across_alone": [("GT", A, B, None, None)],
        "two_lt_no_eq": [("LT", A, A, None, None), ("LT", B, B, rb, rb)],
        "lt_gt_same_nobody": [eq, ("LT", A, A, None, None), ("GT", A, A, None, None)],
        "lt_ab_gt_ba": [("LT", A, B, ma, mb), ("GT", B, A, mb, ma)],
        "two_eq_gt": [eq, ("EQ", G2, G2, None, None), ("GT", A, A, ra, ra)],
    }


NOBODY = ("lt_gt_same_nobody",)
TWO_ORDER = "eq_gt_lt"                   # the set of the case that cannot pass without the entry


def _operand(codes, n_codes, col, rank):
    v = codes[col].astype(np.int64)
    ok = (v >= 0) & (v < int(n_codes[col]))
    if rank is not None:
        v = np.asarray(rank, np.int64)[np.where(ok, v, 0)]
        ok &= v >= 0
    return np.where(ok, v, -1)


def scan_statement(codes, n_codes, preds, cell_cols=()):
    """What rgbm_table_detect_dc_scan returns, in O(n log n): group by the EQ attributes; every order predicate as  L' < R'  (LT: a
    missing left operand never is below; GT: both sides negated); one predicate: L' below the group's maximum of R'; two: the rows
    sorted by (group, R1'), the suffix maximum of R2' inside the group, and per row the first sorted R1' above its L1'."""
    codes = np.asarray(codes, np.int32)
    n = codes.shape[1]
    eq = list(dict.fromkeys(p[1] for p in preds if p[0] == "EQ"))
    order = [p for p in preds if p[0] in ("LT", "GT")]
    assert all(p[0] in ("EQ", "LT", "GT") for p in preds) and 1 <= len(order) <= 2
    if eq and n:
        _, gid = np.unique(np.stack([_operand(codes, n_codes, c, None) for c in eq], axis=1), axis=0, return_inverse=True)
        gid = gid.reshape(-1).astype(np.int64)
    else:
        gid = np.zeros(n, np.int64)
    L, R = [], []
    for op, lc, rc, lr, rr in order:
        l, r = _operand(codes, n_codes, lc, lr), _operand(codes, n_codes, rc, rr)
        if op == "LT":
            L.append(np.where(l < 0, INT_MAX, l))
            R.append(r)
        else:
            L.append(np.where(l < 0, INT_MAX, -l))
            R.append(np.where(r < 0, INT_MIN, -r))
    if n == 0:
        viol = np.zeros(0, bool)
    elif len(order) == 1:
        gmax = np.full(int(gid.max()) + 1, INT_MIN, np.int64)
        np.maximum.at(gmax, gid, R[0])
        viol = L[0] < gmax[gid]
    else:
        ng = int(gid.max()) + 1
        assert ng < 2 ** 29
        by = np.lexsort((R[0], gid))
        sg, s1, s2 = gid[by], R[0][by], R[1][by]
        # suffix maximum per group: in reversed order the groups descend, so a running maximum of (ng - group, value) restarts by itself
        acc = np.maximum.accumulate(((ng - sg[::-1]) << 33) + (s2[::-1] + 2 ** 31))[::-1]
        suf = (acc & (2 ** 33 - 1)) - 2 ** 31
        pos = np.searchsorted((sg << 33) + (s1 + 2 ** 31), (gid << 33) + (L[0] + 2 ** 31), side="right")
        gend = np.searchsorted(sg, gid, side="right")
        viol = (pos < gend) & (suf[np.minimum(pos, n - 1)] > L[1])
    rows = np.flatnonzero(viol).astype(np.int64)
    cc = np.asarray(cell_cols, np.int32).reshape(-1)
    if len(cc) == 0:
        return rows
    return np.tile(rows, len(cc)), np.repeat(cc, len(rows)).astype(np.int32)


def small_frame(n=300, seed=11):
    """The tax frame of the whole-run tests: EQ(State)&GT(Salary)&LT(Tax) with NULLs, every attribute discrete."""
    import pandas as pd
    rng = np.random.default_rng(seed)
    state = rng.choice(np.array(["CA", "NY", "TX", "WA", None], object), n, p=[.3, .3, .2, .15, .05])
    salary = rng.integers(20, 60, n).astype(np.float64) * 1000
    tax = np.round(salary * 0.001 * rng.choice([0.9, 1.0, 1.0, 1.0, 1.1], n))        # mostly monotone in the salary: some violations
    salary[rng.random(n) < 0.08] = np.nan
    tax[rng.random(n) < 0.08] = np.nan
    kind = rng.choice(np.array(["a", "b", "c"], object), n)
    return pd.DataFrame({"tid": np.arange(n), "State": state, "Salary": salary, "Tax": tax, "Kind": kind})


FRAME_CONSTRAINT = "t1&t2&EQ(t1.State,t2.State)&GT(t1.Salary,t2.Salary)&LT(t1.Tax,t2.Tax)"
FRAME_TARGETS = ["State", "Salary", "Tax"]
