"""Case generators for the cell-domain analysis (tests/test_domain_restatement_cpu.py, tests/test_gpu_domain_edges.py): code tables, pair
lists and cell lists built for one edge of csrc/rgbm_domain.hip each.  A case carries the property it is built for -- `route(plan)` asserts
it on a plan in the shape of `Table.pair_counts_report()` (the library's report on the device, `domain_restatement.plan` without one),
`holds(...)` on the restatement's result -- and fails where the property is absent; no case drops a pair or a cell.  The limits come from
the library (`pair_counts_limits()`, `csrc_constant`), never from a copy."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-data-repair-plugin_amd"))

from tests import domain_restatement as R          # noqa: E402
from tests.helpers import csrc_constant            # noqa: E402

INT32_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def _limits():
    from repair import _native as N
    return dict(N.pair_counts_limits(), block=csrc_constant("PC_B"), max_k=csrc_constant("DOM_MAXK"))


def limits():
    """dict(lds_cells, max_cols, block, max_k): counters and distinct columns of a group, rows of a tile, attributes of a cell-domain call."""
    return dict(_limits())


def restated_plan(case):
    L = limits()
    return R.plan(case["pairs"], case["n_bins"], case["codes"].shape[1], L["lds_cells"], L["max_cols"], L["block"])


def _table(seed, n, cards, null=0.05):
    """codes [c][n]: uniform codes, about `null` of the cells NULL and -- from two rows on -- at least one NULL in every column."""
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, int(v), n) for v in cards]).astype(np.int32)
    codes[rng.random(codes.shape) < null] = -1
    if n >= 2:
        for j in range(len(cards)):
            codes[j, (7 * j + 1) % n] = -1
            codes[j, (7 * j + 2) % n] = (j % int(cards[j]))       # ... and never NULLs alone
    return codes


def _case(name, codes, n_codes, pairs, route, luts=None, n_bins=None, **more):
    nb = {c: int(n_codes[c]) for c in range(len(n_codes))}
    nb.update(n_bins or {})
    case = dict(name=name, codes=codes, n_codes=np.asarray(n_codes, np.int32), pairs=[(int(x), int(y)) for x, y in pairs], luts=dict(luts or {}),
                n_bins=nb, route=route, upload=codes, writes=None, host_defined=True)
    case.update(more)
    if codes.shape[1] >= 2:
        assert all((codes[j] < 0).any() for j in range(codes.shape[0])), name + ": a column without NULLs"
    return case


def _groups(plan):
    return [p["group"] for p in plan["pairs"]]


# ------------------------------------------------------------------------------------------------------------------ pair-count cases
def column_limit():
    """Nine pairs over 18 columns of 2-4 bins: the ninth opens a second group because of its columns alone."""
    L = limits()
    half = L["max_cols"] // 2
    cards = [2 + j % 3 for j in range(2 * half + 2)]
    pairs = [(2 * i, 2 * i + 1) for i in range(half + 1)]

    def route(plan):
        assert _groups(plan) == [0] * half + [1] and plan["groups"] == 2
        assert (plan["pairs"][half - 1]["slot_x"], plan["pairs"][half - 1]["slot_y"]) == (L["max_cols"] - 2, L["max_cols"] - 1)
        assert (plan["pairs"][half]["slot_x"], plan["pairs"][half]["slot_y"]) == (0, 1)
        assert sum((cards[x] + 1) * (cards[y] + 1) for x, y in pairs) <= plan["lds_cells"]          # the counters never closed a group
    return _case("column_limit", _table(1, 700, cards), cards, pairs, route)


def column_limit_room_for_one():
    """15 columns, then a pair with one new column (it fits, slot 15), then a pair with a new column (it closes the group)."""
    L = limits()
    mc = L["max_cols"]
    cards = [2 + j % 3 for j in range(mc + 2)]
    pairs = [(2 * i, 2 * i + 1) for i in range((mc - 2) // 2)] + [(mc - 2, 0), (mc - 1, 1), (mc, 2), (3, mc + 1)]
    k = len(pairs)

    def route(plan):
        assert _groups(plan) == [0] * (k - 2) + [1, 1] and plan["groups"] == 2
        assert plan["pairs"][k - 4] == dict(group=0, slot_x=mc - 2, slot_y=0)
        assert plan["pairs"][k - 3] == dict(group=0, slot_x=mc - 1, slot_y=1)                        # the sixteenth column
        assert plan["pairs"][k - 2] == dict(group=1, slot_x=0, slot_y=1)
        assert plan["pairs"][k - 1] == dict(group=1, slot_x=2, slot_y=3)                             # column 3 again, in another slot
    return _case("column_limit_room_for_one", _table(2, 900, cards), cards, pairs, route)


def column_staged_twice():
    """A group closed by its counters; the next group stages two of its columns again."""
    L = limits()
    d = int((L["lds_cells"] / 3.5) ** 0.5) - 1                   # three tables fit a group, four do not
    cards = [d, d, d, 5]
    pairs = [(0, 1), (0, 2), (1, 2), (3, 0), (2, 0), (1, 3)]

    def route(plan):
        assert 3 * (d + 1) ** 2 + 6 * (d + 1) <= plan["lds_cells"] < 4 * (d + 1) ** 2
        assert _groups(plan) == [0, 0, 0, 0, 1, 1]
        assert plan["pairs"][4] == dict(group=1, slot_x=0, slot_y=1) and plan["pairs"][5] == dict(group=1, slot_x=2, slot_y=3)
        assert plan["pairs"][3] == dict(group=0, slot_x=3, slot_y=0)
    return _case("column_staged_twice", _table(3, 5000, cards), cards, pairs, route)


def exact_fill_one_pair():
    """One pair of exactly the limit: (lds_cells / 2 - 1) x 1 bins -- also the widest bin index the uint16 tile carries."""
    L = limits()
    assert L["lds_cells"] % 2 == 0
    dx = L["lds_cells"] // 2 - 1
    assert dx < 65536
    n = 20000
    rng = np.random.default_rng(4)
    codes = np.stack([rng.integers(0, dx, n), np.zeros(n, np.int64)]).astype(np.int32)
    codes[0, :4], codes[1, :4] = [dx - 1, -1, -1, dx - 1], [0, -1, 0, -1]                     # the last bin and the NULL slot, with and without the other side's
    codes[:, 4:][rng.random((2, n - 4)) < 0.05] = -1

    def route(plan):
        assert plan["groups"] == 1 and _groups(plan) == [0] and plan["max_group_cells"] == plan["lds_cells"] == 2 * (dx + 1)
    return _case("exact_fill_one_pair", codes, [dx, 1], [(0, 1)], route, corner=(dx, 1))


def exact_fill_several_pairs():
    """Three pairs whose cells sum to the limit exactly; a fourth, of nine cells, has to open a group."""
    L = limits()
    rest = L["lds_cells"] - 100 * 100 - 2 * 8000
    assert rest > 0 and rest % 2 == 0
    cards = [99, 99, 7999, 1, rest // 2 - 1, 1, 2, 2]
    pairs = [(0, 1), (2, 3), (5, 4), (6, 7)]

    def route(plan):
        assert _groups(plan) == [0, 0, 0, 1] and plan["max_group_cells"] == plan["lds_cells"]
    return _case("exact_fill_several_pairs", _table(5, 6000, cards), cards, pairs, route)


def _pair_above(cells):
    """(a, b) bins of the smallest table above `cells`, as square as its factors allow: (a + 1) * (b + 1) > cells."""
    c = cells + 1
    while True:
        for f in range(int(c ** 0.5), 1, -1):
            if c % f == 0:
                return f - 1, c // f - 1
        c += 1


def one_above_the_limit():
    """The smallest dense table above the limit, and 142 x 254 bins: both take the HBM kernel; a small pair keeps a group beside them."""
    L = limits()
    a, b = _pair_above(L["lds_cells"])
    assert 143 * 255 > L["lds_cells"]
    cards = [a, b, 142, 254, 3]
    pairs = [(0, 1), (4, 0), (2, 3), (1, 0)]

    def route(plan):
        assert (a + 1) * (b + 1) - plan["lds_cells"] in (1, 2)
        assert _groups(plan) == [-1, 0, -1, -1] and plan["groups"] == 1
        assert plan["pairs"][0] == dict(group=-1, slot_x=-1, slot_y=-1)
    return _case("one_above_the_limit", _table(6, 20000, cards), cards, pairs, route)


def hbm_kernel_through_a_lut():
    """A 2000-code column binned to 300 bins through a LUT with NULL entries, against a 300-bin column, in both orientations."""
    rng = np.random.default_rng(7)
    cards = [2000, 300, 4]
    lut = (np.arange(2000) * 300 // 2000).astype(np.int32)
    lut[rng.choice(2000, 60, replace=False)] = -1
    lut[[0, 1999]] = [-1, 299]

    def route(plan):
        assert 301 * 301 > plan["lds_cells"] and _groups(plan) == [-1, -1, 0]
    return _case("hbm_kernel_through_a_lut", _table(7, 20000, cards), cards, [(0, 1), (1, 0), (2, 0)], route, luts={0: lut}, n_bins={0: 300})


def beyond_the_dictionary():
    """Codes at or above a column's dictionary (n_codes, n_codes + 5, 2^31 - 1) in the x column, the y column and the target of the pairs --
    one of them read through a LUT -- and -7 written after the upload: all of them count as NULL.  rgbm_table_write_cells refuses a code
    >= n_codes, so those are part of the uploaded matrix (rgbm_table_create takes what it is given); -7 goes through `write_cells`.
    For pair_counts and cell_domains only: no model is trained on this table."""
    cards = [6, 9, 5, 40]
    n = 3000
    up = _table(8, n, cards)
    lut = (np.arange(40) // 5).astype(np.int32)
    lut[[3, 17]] = -1
    for j in range(4):
        up[j, 100 + 10 * j:100 + 10 * j + 3] = [cards[j], cards[j] + 5, INT32_MAX]
    up[2, 50:53] = [cards[2], cards[2] + 5, INT32_MAX]           # rows whose other cells are ordinary
    rows = np.asarray([200, 201, 202, 203, 100], np.int64)
    cols = np.asarray([0, 1, 2, 3, 2], np.int32)
    vals = np.full(5, -7, np.int32)
    codes = up.copy()
    codes[cols, rows] = vals

    def route(plan):
        assert _groups(plan) == [0, 0, 0]
    return _case("beyond_the_dictionary", codes, cards, [(0, 1), (2, 0), (3, 2)], route, luts={3: lut}, n_bins={3: 8}, upload=up,
                 writes=(rows, cols, vals), host_defined=False)


@functools.lru_cache(maxsize=None)
def single_row_tail_n():
    """The smallest n above one workgroup's rows whose last workgroup sees exactly one row, by the restated geometry.  (With workgroups of
    about 16 blocks and rows per workgroup a multiple of the block, none exists below 15 * 16 * block + 1.)"""
    L = limits()
    for n in range(16 * L["block"] + 1, 64 * 16 * L["block"]):
        p = R.plan([(0, 1)], {0: 2, 1: 2}, n, L["lds_cells"], L["max_cols"], L["block"])
        if p["grid_x"] > 1 and (p["grid_x"] - 1) * p["rows_per_wg"] + 1 == n:
            return n
    raise AssertionError("no n with a last workgroup of one row")


def row_count_ns():
    b = limits()["block"]
    return [1, b, 16 * b - 1, 16 * b, 16 * b + 1, 32 * b + 1, single_row_tail_n()]


def row_counts(n, several_groups):
    """n on either side of the workgroup splits, with a pair list of one group or of several."""
    L = limits()
    d = int((L["lds_cells"] / 2.5) ** 0.5) - 1                   # two tables fit a group, three do not
    cards = [d, d, d, 3]
    pairs = [(0, 1), (0, 2), (1, 2), (2, 0), (1, 0), (3, 1)] if several_groups else [(0, 1), (1, 3)]
    b, tail = L["block"], single_row_tail_n()

    def route(plan):
        assert plan["groups"] == (3 if several_groups else 1) and -1 not in _groups(plan)
        assert plan["rows_per_wg"] % b == 0 and (plan["grid_x"] - 1) * plan["rows_per_wg"] < n <= plan["grid_x"] * plan["rows_per_wg"]
        assert plan["grid_x"] == (1 if n <= 16 * b else 2 if n <= 32 * b else 3 if n < tail else 16)
        if n == tail:
            assert n - (plan["grid_x"] - 1) * plan["rows_per_wg"] == 1
    return _case("row_counts_%d_%s" % (n, "groups" if several_groups else "group"), _table(100 + n % 97, n, cards), cards, pairs, route)


def largest_accepted_pair():
    """4095 x 4095 bins: exactly 2^24 cells, the largest table a call takes."""
    cards = [4095, 4095]

    def route(plan):
        assert 4096 * 4096 == 1 << 24 and _groups(plan) == [-1]
    return _case("largest_accepted_pair", _table(9, 2000, cards), cards, [(0, 1)], route)


def n_bins_below_n_codes():
    """No LUT and fewer bins than codes: the codes from n_bins on count as NULL."""
    cards = [50, 30, 4]

    def route(plan):
        assert _groups(plan) == [0, 0, 0]
    return _case("n_bins_below_n_codes", _table(10, 2500, cards), cards, [(0, 1), (1, 2), (2, 0)], route, n_bins={0: 20, 1: 29})


def pair_cases():
    """{name: generator}; a generator builds its case when called."""
    out = {f.__name__: f for f in (column_limit, column_limit_room_for_one, column_staged_twice, exact_fill_one_pair, exact_fill_several_pairs,
                                   one_above_the_limit, hbm_kernel_through_a_lut, beyond_the_dictionary, largest_accepted_pair,
                                   n_bins_below_n_codes)}
    for n in row_count_ns():
        for several in (False, True):
            out["row_counts_%d_%s" % (n, "groups" if several else "group")] = (lambda n=n, several=several: row_counts(n, several))
    return out


# ------------------------------------------------------------------------------------------------------------------ cell-domain cases
def _correlated(seed, n, d_a, corr_cards, keep=0.7, null=0.04):
    """codes [1 + len(corr_cards)][n]: the target in column 0; correlated attribute j follows the target with probability `keep`."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, d_a, n)
    cols = [t]
    for j, v in enumerate(corr_cards):
        cols.append(np.where(rng.random(n) < keep, (t * (j + 3) + j) % v, rng.integers(0, v, n)))
    codes = np.stack(cols).astype(np.int32)
    codes[rng.random(codes.shape) < null] = -1
    for j in range(codes.shape[0]):
        codes[j, (5 * j + 1) % n] = -1
    return codes


def _call(rows, corr, min_cnt, single_ok, beta, row_count):
    return dict(rows=np.asarray(rows, np.int64), corr=list(corr), min_cnt=[int(v) for v in min_cnt], single_ok=np.asarray(single_ok, bool),
                beta=float(beta), row_count=int(row_count))


def _cd_case(name, codes, n_codes, pairs, target, calls, holds, **more):
    case = _case(name, codes, n_codes, pairs, lambda plan: None, **more)
    case.update(target=target, calls=calls, holds=holds)
    for c in calls:
        assert all(target in case["pairs"][p] for p in c["corr"])
    return case


def restate_call(case, call, tables=None, info=None):
    """The restatement of one cell-domain call of a case; `tables`: the dense tables of the case's pairs (default: the restatement's)."""
    tables = R.pair_counts(case["codes"], case["n_codes"], case["pairs"], case["luts"], case["n_bins"]) if tables is None else tables
    t = case["target"]
    orient = [(case["pairs"][p][1], True) if case["pairs"][p][0] == t else (case["pairs"][p][0], False) for p in call["corr"]]
    return R.cell_domains(case["codes"], t, call["rows"], [tables[p] for p in call["corr"]], orient, call["min_cnt"], call["single_ok"],
                          call["beta"], call["row_count"], case["n_codes"], case["luts"], case["n_bins"], info=info)


def _outcomes(case, call, res):
    """(weak, valid with another current value, valid on a NULL cell, empty) cells of a restated call."""
    weak, top, _, _ = res
    rows, n, d_a = call["rows"], case["codes"].shape[1], case["n_bins"][case["target"]]
    inside = (rows >= 0) & (rows < n)
    cur = np.where(inside, case["codes"][case["target"], np.clip(rows, 0, n - 1)], -1)
    cur = np.where((cur < 0) | (cur >= d_a), -1, cur)
    return int(weak.sum()), int(((top >= 0) & (cur >= 0) & (cur != top)).sum()), int(((top >= 0) & (cur < 0)).sum()), int((top < 0).sum())


def widths_and_k(d_a):
    """Target widths 2, 12, 64 and 300 with k = 0, 1 and DOM_MAXK attributes: the target on the x side of some pairs and on the y side of
    others, one attribute binned through a LUT with NULL entries, a different min_cnt for every attribute, and an attribute whose min_cnt
    wipes every cell's fold -- first, in the middle, last.  Cells: every current value (NULL, the top, another), every outcome."""
    K = limits()["max_k"]
    n = {2: 300, 12: 4000, 64: 8000, 300: 20000}[d_a]
    m = {2: 300, 12: 600, 64: 257, 300: 120}[d_a]
    cards = [d_a] + [max(3, min(d_a, 40) + j) for j in range(K - 1)] + [200]
    codes = _correlated(20 + d_a, n, d_a, cards[1:], keep=0.8)
    lut = (np.arange(200) * 13 // 200).astype(np.int32)
    lut[[0, 7, 150]] = -1
    pairs = [(0, j) if j % 2 else (j, 0) for j in range(1, K + 1)]
    rng = np.random.default_rng(d_a)
    rows = np.sort(rng.choice(n, m, replace=False))
    ok = np.ones(d_a, bool)
    mins = [j % 4 for j in range(K)]
    wipe = lambda at: [n + 1 if j == at else mins[j] for j in range(K)]     # noqa: E731
    beta = {2: 0.55, 12: 0.3, 64: 0.1, 300: 0.05}[d_a]
    calls = [_call(rows, [], [], ok, beta, n), _call(rows, [K - 1], [1], ok, beta, n), _call(rows, [1], [0], ok, beta, n),
             _call(rows, range(K), mins, ok, beta, n), _call(rows, range(K), wipe(0), ok, beta, n),
             _call(rows, range(K), wipe(K // 2), ok, beta, n), _call(rows, range(K), wipe(K - 1), ok, beta, n)]

    def holds(results, infos):
        assert (results[0][1] < 0).all() and not results[0][3].any()                                 # k = 0: no domain anywhere
        assert infos[4]["wiped"] == infos[5]["wiped"] == infos[6]["wiped"] == m and (results[6][1] < 0).all()
        assert 0 < infos[3]["wiped"] < m                                                            # NULL values wipe some folds, not all
        assert results[4][3].tobytes() != results[3][3].tobytes() and results[5][3].tobytes() != results[4][3].tobytes()
        weak, other, on_null, empty = _outcomes(case, calls[3], results[3])
        assert weak > 0 and other > 0 and on_null > 0 and empty > 0, (weak, other, on_null, empty)
    case = _cd_case("widths_and_k_%d" % d_a, codes, cards, pairs, 0, calls, holds, luts={K: lut}, n_bins={K: 13})
    return case


def cell_list_edges():
    """m = 1, 255, 256, 257 cells; rows -1, n and n + 7 in the list; repeated rows."""
    n, d_a = 1000, 12
    cards = [d_a, 9, 14]
    codes = _correlated(31, n, d_a, cards[1:])
    rng = np.random.default_rng(31)
    ok = np.ones(d_a, bool)
    lists = [[5], rng.integers(0, n, 255), rng.integers(0, n, 256), rng.integers(0, n, 257),
             np.concatenate([[-1, n, n + 7, 3, 3, 3, n - 1, 0], rng.integers(0, n, 249), [-1]])]
    calls = [_call(r, [0, 1], [0, 1], ok, 0.2, n) for r in lists]

    def holds(results, infos):
        assert [len(r[0]) for r in results] == [1, 255, 256, 257, 258]
        top, rows = results[4][1], calls[4]["rows"]
        outside = (rows < 0) | (rows >= n)
        assert outside.sum() == 4 and (top[outside] == -1).all() and not results[4][3][outside].any() and (top[~outside] >= 0).any()
        assert top[3] == top[4] == top[5]
    return _cd_case("cell_list_edges", codes, cards, [(0, 1), (2, 0)], 0, calls, holds)


def ties():
    """A few hundred rows in which most joint counts repeat: at least a quarter of the cells have two or more values of the same largest
    probability, and 'first maximum' decides the top."""
    n, d_a = 360, 4
    i = np.arange(n)
    rng = np.random.default_rng(32)
    t = np.where(i < 240, i % d_a, rng.integers(0, d_a, n))
    a = np.where(i < 240, (i // d_a) % 6, rng.integers(6, 9, n))             # the random rows keep to values of their own
    b = np.where(i < 240, (i // 24) % 5, rng.integers(5, 8, n))
    codes = np.stack([t, a, b]).astype(np.int32)
    codes[0, [3, 250]], codes[1, [9, 300]], codes[2, [11, 301]] = -1, -1, -1
    rows = np.arange(n)
    ok = np.ones(d_a, bool)
    calls = [_call(rows, [0], [0], ok, 0.1, n), _call(rows, [0, 1], [0, 0], ok, 0.1, n), _call(rows, [1], [2], ok, 0.2, n)]

    def holds(results, infos):
        for info in infos:
            assert info["tied"] >= n // 4, infos
        assert sum(int(r[0].sum()) for r in results) > 0 and sum(int(((r[1] >= 0) & (r[0] == 0)).sum()) for r in results) > 0
    return _cd_case("ties", codes, [d_a, 9, 8], [(1, 0), (0, 2)], 0, calls, holds)


def beta_on_a_probability():
    """Cells whose domain is two values of equal score: p = 0.5 exactly.  beta = 0.5 leaves the domain empty (the comparison is strict); the
    largest double below 0.5 makes it valid."""
    n, d_a = 300, 3
    i = np.arange(n)
    t = np.where(i < 200, i % 2, 2)                    # attribute value 0: five rows of target 0, five of target 1, none of target 2 ...
    a = np.where(i < 200, i // 10, 20 + i % 3)
    codes = np.stack([t, a]).astype(np.int32)
    codes[0, 210], codes[1, 220] = -1, -1
    rows = np.arange(n)
    ok = np.ones(d_a, bool)
    below = float(np.nextafter(0.5, 0.0))
    calls = [_call(rows, [0], [0], ok, 0.5, n), _call(rows, [0], [0], ok, below, n)]

    def holds(results, infos):
        half = (results[0][3].max(axis=1) == 0.5)
        assert half.sum() >= 200 and (results[0][1][half] == -1).all() and (results[0][2][half] == 0.0).all()
        assert (results[1][1][half] == 0).all() and (results[1][2][half] == 0.5).all() and results[1][0][half].sum() == 100
        assert (results[0][1][~half] >= 0).any()                                                    # ... and domains above beta beside them
    return _cd_case("beta_on_a_probability", codes, [d_a, 23], [(0, 1)], 0, calls, holds)


def single_ok_edges():
    """single_ok all false (no score anywhere), and false on exactly the value that wins most often."""
    n, d_a = 2000, 12
    cards = [d_a, 10, 15]
    codes = _correlated(34, n, d_a, cards[1:])
    rows = np.arange(0, n, 4)
    everything = _call(rows, [0, 1], [0, 0], np.ones(d_a, bool), 0.2, n)
    case = _cd_case("single_ok_edges", codes, cards, [(0, 1), (2, 0)], 0, [everything], None)
    base = restate_call(case, everything)
    winner = int(np.bincount(base[1][base[1] >= 0], minlength=d_a).argmax())
    without = np.ones(d_a, bool)
    without[winner] = False
    case["calls"] = calls = [everything, _call(rows, [0, 1], [0, 0], np.zeros(d_a, bool), 0.2, n), _call(rows, [0, 1], [0, 0], without, 0.2, n)]

    def holds(results, infos):
        assert (results[1][1] < 0).all() and not results[1][3].any() and not results[1][0].any()
        won = results[0][1] == winner
        assert won.sum() > 10 and (results[2][1][won] != winner).all() and not results[2][3][:, winner].any()
        assert (results[2][1][won] >= 0).any()                                                      # another value takes the top
    case["holds"] = holds
    return case


def counts_of_one():
    """min_cnt = 0 on a sparse joint table: elements of count 1 carry 0.1, the other branch of the maximum."""
    n, d_a = 300, 12
    cards = [d_a, 40]
    codes = _correlated(35, n, d_a, cards[1:], keep=0.3)
    rows = np.arange(n)
    calls = [_call(rows, [0], [0], np.ones(d_a, bool), 0.3, n)]

    def holds(results, infos):
        assert infos[0]["tenth"] >= n // 4, infos
    return _cd_case("counts_of_one", codes, cards, [(1, 0)], 0, calls, holds)


def current_values():
    """The current value NULL, the top, another value, and at or above the target's bins (n_bins below n_codes without a LUT, and the
    codes beyond the dictionary of `beyond_the_dictionary`, whose table this is)."""
    case = beyond_the_dictionary()
    n, d_a = case["codes"].shape[1], int(case["n_bins"][2])
    rows = np.concatenate([np.arange(0, 400), [50, 51, 52, 100, 120, 121, 122, 202]])
    calls = [_call(rows, [1, 2], [0, 1], np.ones(d_a, bool), 0.2, n), _call(rows, [2], [0], np.ones(d_a, bool), 0.2, n)]

    def holds(results, infos):
        cur = case["codes"][2, rows]
        assert (cur >= d_a).sum() >= 6 and (cur == -7).sum() >= 1 and (cur == -1).sum() > 0
        assert not results[0][0][(cur >= d_a) | (cur < 0)].any() and (results[0][1][cur >= d_a] >= 0).any()
        weak, other, on_null, empty = _outcomes(case, calls[0], results[0])
        assert weak > 0 and other > 0 and on_null > 0 and empty > 0, (weak, other, on_null, empty)
    case.update(name="current_values", target=2, calls=calls, holds=holds)
    return case


def narrow_target_bins():
    """A target of 9 codes counted with 6 bins and no LUT: the codes 6 .. 8 are NULL as current values and have no table line."""
    n = 1500
    cards = [9, 8]
    codes = _correlated(36, n, 9, cards[1:])
    rows = np.arange(0, n, 3)
    calls = [_call(rows, [0], [1], np.ones(6, bool), 0.2, n)]

    def holds(results, infos):
        cur = codes[0, rows]
        assert (cur >= 6).sum() > 50 and not results[0][0][cur >= 6].any() and results[0][0].any() and results[0][3].shape[1] == 6
    return _cd_case("narrow_target_bins", codes, cards, [(1, 0)], 0, calls, holds, n_bins={0: 6})


def domain_cases():
    out = {"widths_and_k_%d" % d: (lambda d=d: widths_and_k(d)) for d in (2, 12, 64, 300)}
    out.update({f.__name__: f for f in (cell_list_edges, ties, beta_on_a_probability, single_ok_edges, counts_of_one, current_values,
                                        narrow_target_bins)})
    return out


def restate_case(case):
    """(results, infos) of every call of a cell-domain case on the restatement's own tables, with the case's properties asserted."""
    tables = R.pair_counts(case["codes"], case["n_codes"], case["pairs"], case["luts"], case["n_bins"])
    results, infos = [], []
    for call in case["calls"]:
        infos.append({})
        results.append(restate_call(case, call, tables, infos[-1]))
    case["holds"](results, infos)
    return tables, results
