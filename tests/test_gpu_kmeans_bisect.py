"""-m gpu: the device pass of the bisecting k-means (csrc/rgbm_kmeans.hip: rgbm_table_kmeans_bisect) against the numpy pass of
repair/qgram_bisect.py -- labels, counts, sizes and n_changed are integers that follow from float64 additions in one fixed order, so
equality, no tolerance -- and `RepairMisc.splitInputTable` with clustering_alg="bisecting" through the HIP engine against the numpy loop.

Labels other than node 0 get onto the device the way the loop puts them there (passes on passes), or in one call through
`Table.kmeans_assign`, which writes the same resident label array (tests/test_gpu_kmeans.py holds that call to its numpy step)."""

import numpy as np
import pytest

from tests import kmeans_restatement as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu


def _const(name):
    """A constant of the source, not a copy of it."""
    return csrc_constant(name)


WG_ROWS = _const("KM_B") * _const("KM_UNROLL")       # rows of one workgroup on a table of up to 512 workgroups
P_DOUBLES = _const("KB_LDS_P_DOUBLES")
COUNTERS = _const("KB_LDS_COUNTERS")
BALLOT_M = _const("KB_BALLOT_M")
MAX_M = _const("KB_MAX_M")
MAX_NODES = _const("KB_MAX_NODES")


def _table(n, n_codes, seed, cols=None, null=0.05):
    """A random code table [c][n] (NULLs included), the columns to cluster on and their offsets."""
    rng = np.random.default_rng(seed)
    n_codes = np.asarray(n_codes, np.int32)
    codes = np.stack([rng.integers(0, max(int(d), 1), n).astype(np.int32) if d > 0 else np.full(n, -1, np.int32) for d in n_codes])
    codes[rng.random(codes.shape) < null] = -1
    cols = np.arange(len(n_codes), dtype=np.int32) if cols is None else np.asarray(cols, np.int32)
    off = np.concatenate([[0], np.cumsum(n_codes[cols][:-1], dtype=np.int64)]).astype(np.int64)
    return codes, n_codes, cols, off, int(n_codes[cols].sum())


def _scores(d_tot, m, seed):
    rng = np.random.default_rng(1000 + seed)
    return rng.normal(size=(d_tot, 2 * m)) * 3.0, rng.random(2 * m) * 2.0


def _numpy_pass(codes, n_codes, cols, off, p, h, slot_of, child, prev):
    from repair import qgram_bisect as QB
    return QB.bisect_step(np.ascontiguousarray(codes[cols]), n_codes[cols], off, p, h, np.asarray(slot_of, np.int32), np.asarray(child, np.int32), prev)


def _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, prev):
    """One device pass against the numpy pass (prev None: first = 1); returns the labels."""
    counts, sizes, n_changed = table.kmeans_bisect(cols, off, slot_of, child, p, h, prev is None)
    a_r, c_r, s_r, n_r = _numpy_pass(codes, n_codes, cols, off, p, h, slot_of, child, prev)
    got = table.kmeans_read()
    assert got.dtype == np.int32 and counts.dtype == np.int64 and sizes.dtype == np.int64
    np.testing.assert_array_equal(got, a_r)
    np.testing.assert_array_equal(counts, c_r)
    np.testing.assert_array_equal(sizes, s_r)
    assert n_changed == n_r
    return got


def _first_pass(codes, n_codes, cols, off, d_tot, seed):
    """A fresh table and the root's pass: first = 1, node 0 into nodes 1 and 2."""
    from repair import _native as N
    table = N.Table(codes, n_codes)
    p, h = _scores(d_tot, 1, seed)
    labels = _check_pass(table, codes, n_codes, cols, off, p, h, [0, 0, 0], [1, 2], None)
    assert set(labels.tolist()) <= {1, 2}
    return table, labels


def _seeded(codes, n_codes, cols, off, d_tot, k, seed):
    """A fresh table whose resident labels are 0 .. k-1, set in one call of the k-means step; (table, labels)."""
    from repair import _native as N
    from repair import qgram_kmeans as Q
    table = N.Table(codes, n_codes)
    rng = np.random.default_rng(2000 + seed)
    p, h = rng.normal(size=(d_tot, k)), rng.random(k)
    table.kmeans_assign(cols, off, p, h, True)
    labels = table.kmeans_read()
    np.testing.assert_array_equal(labels, Q.assign_step(np.ascontiguousarray(codes[cols]), n_codes[cols], off, p, h, None)[0])
    assert len(set(labels.tolist())) > k // 2
    return table, labels


def _slots(k, m, n_nodes=None):
    """m of the nodes 0 .. k-1 are split (every other one while they last, so that nodes left alone lie between them), their children are
    the next 2m ids; slot_of names the slot for the parent and both children."""
    parents = (list(range(0, k, 2)) + list(range(1, k, 2)))[:m]
    parents.sort()
    n_nodes = k + 2 * m if n_nodes is None else n_nodes
    slot_of = np.full(n_nodes, -1, np.int32)
    child = np.arange(k, k + 2 * m, dtype=np.int32)
    for s, node in enumerate(parents):
        slot_of[[node, child[2 * s], child[2 * s + 1]]] = s
    return slot_of, child


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, 2 * WG_ROWS + 1])
def test_row_counts(n):
    codes, n_codes, cols, off, d_tot = _table(n, [5, 3], seed=n)
    table, labels = _first_pass(codes, n_codes, cols, off, d_tot, seed=n)
    p, h = _scores(d_tot, 2, n)                                  # and the level below: nodes 1 and 2 into 3 .. 6
    _check_pass(table, codes, n_codes, cols, off, p, h, [-1, 0, 1, 0, 0, 1, 1], [3, 4, 5, 6], labels)


def test_slots_doubling_to_the_largest_m():
    """The loop's own shape on a few thousand rows: level l splits all 2^l nodes of the level above, m = 1, 2, 4, .. 512, node ids up to
    2046; every pass against the numpy pass, the labels carried on the device from pass to pass."""
    from repair import _native as N
    n = 3 * WG_ROWS + 17
    codes, n_codes, cols, off, d_tot = _table(n, [7, 4, 11, 5, 9, 6, 3], seed=77)
    table, labels = N.Table(codes, n_codes), None
    m = 1
    while m <= MAX_M:
        parents = np.arange(m - 1, 2 * m - 1)                    # a complete binary tree in level order
        child = np.arange(2 * m - 1, 4 * m - 1, dtype=np.int32)
        slot_of = np.full(4 * m - 1, -1, np.int32)
        slot_of[parents] = np.arange(m)
        slot_of[child] = np.repeat(np.arange(m), 2)
        p, h = _scores(d_tot, m, m)
        labels = _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, labels)
        for again in range(2 if m in (1, 4, MAX_M) else 0):      # the level's later passes: the children are scored again, other centres
            p, h = _scores(d_tot, m, 10 * m + again)
            labels = _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, labels)
        m *= 2
    assert m == 2 * MAX_M and len(slot_of) == MAX_NODES - 1 and len(set(labels.tolist())) > MAX_M


@pytest.mark.parametrize("m", [1, 2, 3, BALLOT_M, BALLOT_M + 1, 32])
def test_slots_between_nodes_left_alone(m):
    """m of 64 nodes are split, nodes with slot_of = -1 lie between them, and the labels 60 .. 63 are beyond n_nodes (the children take the
    ids 40 .., so n_nodes = 60 is enough for them): those rows are untouched and counted nowhere."""
    codes, n_codes, cols, off, d_tot = _table(2 * WG_ROWS + 31, [7, 4, 11, 9, 5], seed=300 + m)
    table, labels = _seeded(codes, n_codes, cols, off, d_tot, 64, seed=m)
    if m <= 10:
        parents = list(range(0, 2 * m, 2))                       # 0, 2, 4, ..: the odd nodes between them are left alone
        slot_of = np.full(60, -1, np.int32)
        child = np.arange(40, 40 + 2 * m, dtype=np.int32)
        for s, node in enumerate(parents):
            slot_of[[node, child[2 * s], child[2 * s + 1]]] = s
        alone = ~np.isin(labels, parents + child.tolist())
        assert (labels >= 60).any() and alone.sum() > len(labels) // 2
    else:
        slot_of, child = _slots(64, m)
        alone = slot_of[labels] < 0
    p, h = _scores(d_tot, m, m)
    got = _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, labels)
    np.testing.assert_array_equal(got[alone], labels[alone])
    assert np.isin(got[~alone], child).all()                     # a scored row carries a child's id
    got2 = _check_pass(table, codes, n_codes, cols, off, *_scores(d_tot, m, m + 50), slot_of, child, got)
    np.testing.assert_array_equal(got2[alone], labels[alone])


SWEEPS = _const("KB_MAX_SWEEPS")


def _bound_cases():
    """where -> (m, d_tot, children named in slot_of).  P and h stay in LDS while (d_tot + 1) * (2m | 1) <= KB_LDS_P_DOUBLES, the counters while
    2m * d_tot <= KB_LDS_COUNTERS: the largest m at each bound for a d_tot that meets it exactly, one slot more, one dictionary entry more.
    Above the counter bound the pass is swept in windows of floor(KB_LDS_COUNTERS / 2 d_tot) slots, up to KB_MAX_SWEEPS of them; beyond that,
    with a d_tot whose single slot does not fit, or with children that slot_of does not name, the counters are global."""
    m_p, d_p = 5, P_DOUBLES // 11 - 1
    assert (d_p + 1) * (2 * m_p | 1) == P_DOUBLES and 2 * m_p * (d_p + 1) <= COUNTERS
    m_c, d_c = 24, COUNTERS // 48
    assert 2 * m_c * d_c == COUNTERS and (d_c + 1) * (2 * m_c | 1) > P_DOUBLES
    d_one = COUNTERS // 2                                        # a window of one slot
    assert COUNTERS // (2 * d_one) == 1 and COUNTERS // (2 * (d_one + 1)) == 0 and SWEEPS + 1 <= 64
    return {"p_at_bound": (m_p, d_p, True), "p_above_bound_m": (m_p + 1, d_p, True), "p_above_bound_d": (m_p, d_p + 1, True),
            "counters_at_bound": (m_c, d_c, True), "two_sweeps_m": (m_c + 1, d_c, True), "two_sweeps_d": (m_c, d_c + 1, True),
            "three_sweeps": (2 * m_c + 1, d_c, True), "children_not_named": (m_c + 1, d_c, False),
            "sweeps_at_cap": (SWEEPS, d_one, True), "sweeps_above_cap": (SWEEPS + 1, d_one, True),
            "one_slot_too_large": (2, d_one + 1, True)}


@pytest.mark.parametrize("where", sorted(_bound_cases()))
def test_lds_bounds(where):
    m, d_tot, named = _bound_cases()[where]
    first = d_tot // 2
    codes, n_codes, cols, off, d = _table(2 * WG_ROWS + 3, [first, d_tot - first], seed=d_tot + m, null=0.02)
    assert d == d_tot
    table, labels = _seeded(codes, n_codes, cols, off, d_tot, 64, seed=m)
    slot_of, child = _slots(64, m)
    if not named:
        slot_of[child] = -1                                      # a level's first pass may say so: no row carries a child's id yet
        assert not np.isin(labels, child).any()
    p, h = _scores(d_tot, m, m)
    got = _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, labels)
    if named:                                                    # and the level's next pass, the rows carrying their children's ids
        _check_pass(table, codes, n_codes, cols, off, *_scores(d_tot, m, m + 7), slot_of, child, got)


@pytest.mark.parametrize("n_cols", [1, 2, 17])
def test_column_counts(n_cols):
    codes, n_codes, cols, off, d_tot = _table(2 * WG_ROWS + 5, [3 + (j % 5) for j in range(n_cols)], seed=200 + n_cols)
    table, labels = _first_pass(codes, n_codes, cols, off, d_tot, seed=n_cols)
    p, h = _scores(d_tot, 2, n_cols)
    _check_pass(table, codes, n_codes, cols, off, p, h, [-1, 0, 1, 0, 0, 1, 1], [3, 4, 5, 6], labels)


def test_columns_out_of_table_order_and_a_subset():
    codes, n_codes, cols, off, d_tot = _table(WG_ROWS + 9, [4, 9, 6, 2], seed=3, cols=[2, 0, 3])
    table, labels = _first_pass(codes, n_codes, cols, off, d_tot, seed=3)
    p, h = _scores(d_tot, 1, 4)
    _check_pass(table, codes, n_codes, cols, off, p, h, [-1, -1, 0, 0, 0], [3, 4], labels)


def test_nulls_and_codes_outside_the_dictionary():
    """An all-NULL column, all-NULL rows (their scores are h alone) and a code >= n_codes, which is NULL."""
    codes, n_codes, cols, off, d_tot = _table(WG_ROWS + 100, [6, 0, 8], seed=9)
    codes[2, ::7] = 9                          # beyond the 8 codes the table declares for the column
    codes[2, 5::11] = 8
    codes[:, :300] = -1
    from repair import _native as N
    table = N.Table(codes, n_codes)
    p, _ = _scores(d_tot, 1, 9)
    got = _check_pass(table, codes, n_codes, cols, off, p, np.asarray([0.75, 0.25]), [0, 0, 0], [1, 2], None)
    assert (got[:300] == 2).all()
    got = _check_pass(table, codes, n_codes, cols, off, p, np.asarray([0.25, 0.25]), [0, 0, 0], [1, 2], got)
    assert (got[:300] == 1).all()              # a tie goes left


def test_identical_child_centres_every_row_goes_left():
    codes, n_codes, cols, off, d_tot = _table(WG_ROWS + 100, [6, 5], seed=10)
    table, labels = _seeded(codes, n_codes, cols, off, d_tot, 8, seed=10)
    slot_of, child = _slots(8, 3)
    p, h = _scores(d_tot, 3, 10)
    p[:, 1::2] = p[:, 0::2]
    h[1::2] = h[0::2]
    got = _check_pass(table, codes, n_codes, cols, off, p, h, slot_of, child, labels)
    assert not np.isin(got, child[1::2]).any() and all((got == c).any() for c in child[0::2])


@pytest.mark.parametrize("h_first", [False, True])
def test_addition_order_is_left_to_right(h_first):
    """((h + a) + b) + c with a, b, c = 1e16, 1, -(1e16 + 2) is -2; a + (b + c) is 0 and (a + c) + b is -1 (and the negated terms give
    2 against 0 and 1).  The right child scores -1.5 on the rows of code 0 and 1.5 on the rows of code 1, so the label tells the order."""
    from repair import _native as N
    big = 1e16
    assert (big + 1.0) + -(big + 2) == -2.0 and big + (1.0 + -(big + 2)) == 0.0 and (big + -(big + 2)) + 1.0 == -1.0
    n = 2 * WG_ROWS + 1
    n_codes = np.asarray([2, 2, 2, 1], np.int32)
    codes = np.zeros((4, n), np.int32)
    codes[:3, 1::2] = 1
    if h_first:                                # h carries the first term: only the rows of code 0 are pinned
        codes[:3] = 0
        h = np.asarray([big, 0.0])
        p = np.asarray([[1.0, -1.5], [0.0, 1.5], [-(big + 2), 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]])
    else:
        h = np.zeros(2)
        p = np.asarray([[big, -1.5], [-big, 1.5], [1.0, 0.0], [-1.0, 0.0], [-(big + 2), 0.0], [big + 2, 0.0], [0.0, 0.0]])
    cols, off = np.arange(4, dtype=np.int32), np.asarray([0, 2, 4, 6], np.int64)
    got = _check_pass(N.Table(codes, n_codes), codes, n_codes, cols, off, p, h, [0, 0, 0], [1, 2], None)
    want = np.ones(n, np.int32)                # left: -2 is below -1.5
    if not h_first:
        want[1::2] = 2                         # right: 1.5 is below 2
    np.testing.assert_array_equal(got, want)


def test_second_pass_counts_the_rows_that_moved():
    from repair import _native as N
    codes, n_codes, cols, off, d_tot = _table(3 * WG_ROWS + 5, [5, 7], seed=12, null=0.0)
    table, first = _first_pass(codes, n_codes, cols, off, d_tot, seed=12)
    p, h = _scores(d_tot, 1, 12)               # (the scores of _first_pass)
    counts, sizes, n_changed = table.kmeans_bisect(cols, off, [0, 0, 0], [1, 2], p, h, False)
    assert n_changed == 0 and np.array_equal(table.kmeans_read(), first) and int(sizes.sum()) == codes.shape[1]
    p2 = p.copy()
    p2[2, 1] = -1e6                            # every row of code 2 in column 0 goes right, every other row keeps its label
    counts, sizes, n_changed = table.kmeans_bisect(cols, off, [0, 0, 0], [1, 2], p2, h, False)
    moved = (codes[0] == 2) & (first != 2)
    assert n_changed == int(moved.sum()) > 0
    a_r, c_r, s_r, n_r = _numpy_pass(codes, n_codes, cols, off, p2, h, [0, 0, 0], [1, 2], first)
    assert n_r == n_changed
    np.testing.assert_array_equal(table.kmeans_read(), a_r)
    np.testing.assert_array_equal(counts, c_r)
    np.testing.assert_array_equal(sizes, s_r)
    fresh = N.Table(codes, n_codes)            # another table: the labels belong to the table
    with pytest.raises(N.RepairGbmError) as ei:
        fresh.kmeans_bisect(cols, off, [0, 0, 0], [1, 2], p, h, False)
    assert ei.value.code == -2


def test_refusals_leave_the_previous_labels():
    from repair import _native as N
    codes, n_codes, cols, off, d_tot = _table(WG_ROWS + 5, [5, 7], seed=13)
    table, first = _first_pass(codes, n_codes, cols, off, d_tot, seed=13)
    p, h = _scores(d_tot, 1, 13)
    so, ch = [0, 0, 0], [1, 2]

    def refused(cols_, off_, so_, ch_, p_, h_, first_=True):
        with pytest.raises(N.RepairGbmError) as ei:
            table.kmeans_bisect(cols_, off_, so_, ch_, p_, h_, first_)
        assert ei.value.code == -2, ei.value
        np.testing.assert_array_equal(table.kmeans_read(), first)

    refused(cols, off, so, np.zeros(0, np.int32), np.zeros((d_tot, 0)), np.zeros(0))                       # m < 1
    big_m = MAX_M + 1
    refused(cols, off, np.zeros(MAX_NODES, np.int32), np.zeros(2 * big_m, np.int32), np.zeros((d_tot, 2 * big_m)), np.zeros(2 * big_m))   # m > 512
    refused(cols, off, np.zeros(0, np.int32), ch, p, h)                                                     # no node
    refused(cols, off, np.zeros(MAX_NODES + 1, np.int32), ch, p, h)                                         # n_nodes > 2048
    refused(np.zeros(0, np.int32), np.zeros(0, np.int64), so, ch, p, h)                                     # no column
    refused(np.zeros(1025, np.int32), np.zeros(1025, np.int64), so, ch, p, h)                               # n_cols > 1024
    refused([0, 2], off, so, ch, p, h)                                                                      # a column outside the table
    refused([0, -1], off, so, ch, p, h)
    refused(cols, [0, 6], so, ch, p, h)                                                                     # 6 + 7 codes > d_tot = 12
    refused(cols, [-1, 5], so, ch, p, h)
    refused(cols, off, so, ch, p[:d_tot - 1], h)                                                            # d_tot too small for the dictionaries
    refused(cols, off, [0, 1, 0], ch, p, h)                                                                 # slot_of >= m
    refused(cols, off, [0, -2, 0], ch, p, h)                                                                # slot_of < -1
    refused(cols, off, so, [1, 3], p, h)                                                                    # child >= n_nodes
    refused(cols, off, so, [-1, 2], p, h)                                                                   # child < 0
    big = (1 << 27) // 64 + 1                                                                              # d_tot * 2m > 2^27: refused before P is read
    z, zi = np.zeros(64), np.zeros(64, np.int32)
    rc = N.lib().rgbm_table_kmeans_bisect(table.h, N._p(np.asarray(cols, np.int32), N.C.c_int32), N.C.c_int32(2), N._p(off, N.C.c_int64),
                                          N.C.c_int64(big), N._p(zi, N.C.c_int32), N.C.c_int32(64), N.C.c_int32(32), N._p(zi, N.C.c_int32),
                                          N._p(z, N.C.c_double), N._p(z, N.C.c_double), N.C.c_int32(1),
                                          N._p(np.zeros(1, np.int64), N.C.c_int64), N._p(np.zeros(64, np.int64), N.C.c_int64),
                                          N.C.byref(N.C.c_int64(0)))
    assert rc == -2
    np.testing.assert_array_equal(table.kmeans_read(), first)
    fresh = N.Table(codes, n_codes)
    with pytest.raises(N.RepairGbmError) as ei:                                                             # first == 0 without labels
        fresh.kmeans_bisect(cols, off, so, ch, p, h, False)
    assert ei.value.code == -2
    with pytest.raises(N.RepairGbmError):
        fresh.kmeans_read()
    counts, sizes, n_changed = table.kmeans_bisect(cols, off, so, ch, p, h, False)                          # and the table still steps
    assert n_changed == 0


def _frames():
    from tests.helpers import frame, load_golden
    return {"adult": frame(load_golden("adult")["input"]), "random": R.random_frame(5000)}


@pytest.mark.parametrize("k", ["4", "100"])
@pytest.mark.parametrize("name", ["adult", "random"])
def test_split_input_table_through_the_hip_engine(name, k, monkeypatch):
    from repair.api import Delphi
    from repair.engine import HipEngine
    from repair.misc import RepairMisc
    df = _frames()[name]
    Delphi.register_table("kb_" + name, df)
    opts = {"table_name": "kb_" + name, "row_id": "tid", "k": k, "clustering_alg": "bisecting"}

    class Counting(HipEngine):
        passes, reads = 0, 0

        def kmeans_bisect(self, *a, **kw):
            Counting.passes += 1
            return HipEngine.kmeans_bisect(self, *a, **kw)

        def kmeans_read(self, *a, **kw):
            Counting.reads += 1
            return HipEngine.kmeans_read(self, *a, **kw)

    misc = RepairMisc().options(opts)
    misc._engine_override = Counting(0)
    got = misc.splitInputTable()
    assert Counting.passes >= 2 and Counting.reads == 1
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    want = RepairMisc().options(opts).splitInputTable()
    assert got["tid"].tolist() == want["tid"].tolist() and got["k"].tolist() == want["k"].tolist()
    groups = sorted(set(got["k"]))
    assert groups == list(range(len(groups))) and 2 <= len(groups) <= int(k)
    if name == "random":
        assert len(groups) == int(k)
