"""The four measures of `repair.fd_codes.fd_measures` once more in plain Python: dicts and Counters over the rows, no numpy grouping.  The
yardstick for the numpy statement and for `Table.fd_measures` alike; also the tables both test files share."""
from collections import Counter, defaultdict

import numpy as np

NULL = None


def _value(code, n_codes):
    """A code outside [0, n_codes) is NULL; NULL is a value of its own."""
    code = int(code)
    return code if 0 <= code < int(n_codes) else NULL


def fd_measures(codes, n_codes, lhs, rhs_cols):
    codes = np.asarray(codes)
    n = codes.shape[1]
    keys = [tuple(_value(codes[c][i], n_codes[c]) for c in lhs) for i in range(n)]
    size = Counter(keys)
    out = dict(groups=len(size), kept=[], violating=[], xy_groups=[])
    for y in rhs_cols:
        per_group = defaultdict(Counter)
        for i in range(n):
            per_group[keys[i]][_value(codes[y][i], n_codes[y])] += 1
        out["kept"].append(sum(max(c.values()) for c in per_group.values()))
        out["violating"].append(sum(size[k] for k, c in per_group.items() if len(c) >= 2))
        out["xy_groups"].append(sum(len(c) for c in per_group.values()))
    return out


def assert_same(got, want, what=""):
    """`got` (the statement or the device: int64 throughout) against `want` (this restatement or the statement)."""
    assert np.asarray(got["groups"]).dtype == np.int64 and int(got["groups"]) == int(want["groups"]), (what, "groups", got["groups"], want["groups"])
    for f in ("kept", "violating", "xy_groups"):
        g = np.asarray(got[f])
        assert g.dtype == np.int64 and g.shape == (len(want[f]),) and [int(v) for v in g] == [int(v) for v in want[f]], (what, f, g, want[f])


# the worked example of DESIGN.md 5o: rows (a, b), -1 = NULL; X = [a], Y = b
EXAMPLE = dict(codes=np.asarray([[0, 0, 0, 1, -1, -1], [0, 0, 1, 2, 3, 3]], np.int32), n_codes=[2, 4],
               want=dict(groups=3, kept=[5], violating=[3], xy_groups=[4]))

ROW_EDGES = (1, 2, 63, 64, 65, 257)


def mixed_table(n, c=12, seed=0, card=3, shape="skewed"):
    """[c][n] int32 with NULLs (-1), codes at n_codes, above it and below -1 (all NULL by the rule), and ties for a group's maximum.
    shape: "one" (every X column constant: one group), "singletons" (column 0 numbers the rows), "skewed" (a few heavy values)."""
    rng = np.random.default_rng(seed)
    n_codes = [card + (j % 3) for j in range(c)]
    if shape == "skewed":
        codes = np.stack([np.minimum(rng.geometric(0.45, n) - 1, n_codes[j] - 1) for j in range(c)]).astype(np.int32)
    elif shape == "one":
        codes = np.zeros((c, n), np.int32)
        codes[c - 1] = rng.integers(0, n_codes[c - 1], n)
        codes[c - 2] = np.arange(n) % 2               # two Y values, as even as n allows: a tie for the maximum when n is even
    else:
        codes = np.stack([rng.integers(0, n_codes[j], n) for j in range(c)]).astype(np.int32)
        codes[0] = np.arange(n)
        n_codes[0] = max(n, 1)
    if shape != "singletons":
        for j in (range(c) if shape == "skewed" else (c - 1,)):       # NULLs and the three kinds of out-of-range codes, in X and in Y
            hit = rng.random(n) < 0.12
            codes[j][hit] = rng.choice([-1, n_codes[j], n_codes[j] + 5, -7], int(hit.sum()))
    return codes.astype(np.int32), n_codes
