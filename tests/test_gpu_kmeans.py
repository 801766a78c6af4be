"""-m gpu: the device step of the q-gram k-means (csrc/rgbm_kmeans.hip: rgbm_table_kmeans_assign / rgbm_table_kmeans_read) against the
numpy step of repair/qgram_kmeans.py -- labels, counts, sizes and n_changed are integers that follow from float64 additions in one fixed
order, so equality, no tolerance -- and `RepairMisc.splitInputTable` through the HIP engine against the numpy path."""

import numpy as np
import pytest

from tests import kmeans_restatement as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu


def _const(name):
    """A constant of the source, not a copy of it."""
    return csrc_constant(name)


WG_ROWS = _const("KM_B") * _const("KM_UNROLL")       # rows of one workgroup on a table of up to 512 workgroups
KC = _const("KM_KC")
P_DOUBLES = _const("KM_LDS_P_DOUBLES")
COUNTERS = _const("KM_LDS_COUNTERS")


def _case(n, n_codes, k, seed, cols=None, null=0.05):
    """A random code table [c][n] (NULLs included), the columns to cluster on, their offsets, P and h."""
    rng = np.random.default_rng(seed)
    n_codes = np.asarray(n_codes, np.int32)
    codes = np.stack([rng.integers(0, max(int(d), 1), n).astype(np.int32) if d > 0 else np.full(n, -1, np.int32) for d in n_codes])
    codes[rng.random(codes.shape) < null] = -1
    cols = np.arange(len(n_codes), dtype=np.int32) if cols is None else np.asarray(cols, np.int32)
    off = np.concatenate([[0], np.cumsum(n_codes[cols][:-1], dtype=np.int64)]).astype(np.int64)
    d_tot = int(n_codes[cols].sum())
    p = rng.normal(size=(d_tot, k)) * 3.0
    h = rng.random(k) * 2.0
    return codes, n_codes, cols, off, p, h


def _numpy_step(codes, n_codes, cols, off, p, h, prev=None):
    from repair import qgram_kmeans as Q
    return Q.assign_step(np.ascontiguousarray(codes[cols]), n_codes[cols], off, p, h, prev)


def _check_step(codes, n_codes, cols, off, p, h, table=None):
    """first = 1 on the device against the numpy step; returns (table, labels)."""
    from repair import _native as N
    table = table if table is not None else N.Table(codes, n_codes)
    counts, sizes, n_changed = table.kmeans_assign(cols, off, p, h, True)
    a_r, c_r, s_r, n_r = _numpy_step(codes, n_codes, cols, off, p, h)
    got = table.kmeans_read()
    assert got.dtype == np.int32 and counts.dtype == np.int64 and sizes.dtype == np.int64
    np.testing.assert_array_equal(got, a_r)
    np.testing.assert_array_equal(counts, c_r)
    np.testing.assert_array_equal(sizes, s_r)
    assert n_changed == n_r == codes.shape[1]
    return table, got


@pytest.mark.parametrize("n", [1, 63, 64, 65, WG_ROWS - 1, WG_ROWS, WG_ROWS + 1, 2 * WG_ROWS + 1])
def test_row_counts(n):
    _check_step(*_case(n, [5, 3], 3, seed=n))


@pytest.mark.parametrize("k", [2, 3, KC, KC + 1, 64])
def test_cluster_counts(k):
    _check_step(*_case(3 * WG_ROWS + 17, [7, 4, 11], k, seed=100 + k))


@pytest.mark.parametrize("n_cols", [1, 2, 17])
def test_column_counts(n_cols):
    _check_step(*_case(2 * WG_ROWS + 5, [3 + (j % 5) for j in range(n_cols)], 3, seed=200 + n_cols))


def test_columns_out_of_table_order_and_a_subset():
    _check_step(*_case(WG_ROWS + 9, [4, 9, 6, 2], 5, seed=3, cols=[2, 0, 3]))


@pytest.mark.parametrize("where", ["p_at_bound", "p_above_bound", "counters_at_bound", "counters_above_bound"])
def test_lds_bounds(where):
    """k = 2: P and h stay in LDS while (d_tot + 1) * (k | 1) <= KM_LDS_P_DOUBLES, the counters while k * d_tot <= KM_LDS_COUNTERS."""
    k = 2
    d_p = P_DOUBLES // (k | 1) - 1
    assert (d_p + 1) * (k | 1) == P_DOUBLES and COUNTERS % k == 0 and k * (d_p + 1) <= COUNTERS
    d_tot = {"p_at_bound": d_p, "p_above_bound": d_p + 1, "counters_at_bound": COUNTERS // k, "counters_above_bound": COUNTERS // k + 1}[where]
    first = d_tot // 2
    _check_step(*_case(2 * WG_ROWS + 3, [first, d_tot - first], k, seed=d_tot, null=0.02))


def test_nulls_and_codes_outside_the_dictionary():
    """An all-NULL column, all-NULL rows (label = arg-min of h, lowest id) and a code >= n_codes, which is NULL."""
    codes, n_codes, cols, off, p, h = _case(WG_ROWS + 100, [6, 0, 8], 4, seed=9)
    codes[2, ::7] = 9                          # beyond the 8 codes the table declares for the column
    codes[2, 5::11] = 8
    codes[:, :300] = -1
    h = np.asarray([0.75, 0.25, 0.25, 1.0])
    _, got = _check_step(codes, n_codes, cols, off, p, h)
    assert (got[:300] == 1).all()


def test_identical_centres_lower_id_wins():
    codes, n_codes, cols, off, p, h = _case(WG_ROWS + 100, [6, 5], KC + 2, seed=10)
    h[1] = -5.0                                # (a centre that wins rows)
    p[:, KC] = p[:, 1]
    h[KC] = h[1]                               # cluster KC (the second register chunk) repeats cluster 1
    p[:, 3] = p[:, 2]
    h[3] = h[2]                                # and 3 repeats 2 inside one chunk
    _, got = _check_step(codes, n_codes, cols, off, p, h)
    assert not np.isin(got, [3, KC]).any() and (got == 1).any()


@pytest.mark.parametrize("h_first", [False, True])
def test_addition_order_is_left_to_right(h_first):
    """((h + a) + b) + c with a, b, c = 1e16, 1, -(1e16 + 2) is -2; a + (b + c) is 0 and (a + c) + b is -1 (and the negated terms give
    2 against 0 and 1).  Cluster 1 scores -1.5 on the rows of code 0 and 1.5 on the rows of code 1, so the label tells the order."""
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
    _, got = _check_step(codes, n_codes, cols, off, p, h)
    want = np.zeros(n, np.int32)
    if not h_first:
        want[1::2] = 1
    np.testing.assert_array_equal(got, want)


def test_second_step_counts_the_rows_that_moved():
    from repair import _native as N
    codes, n_codes, cols, off, p, h = _case(3 * WG_ROWS + 5, [5, 7], 3, seed=12, null=0.0)
    table, first = _check_step(codes, n_codes, cols, off, p, h)
    counts, sizes, n_changed = table.kmeans_assign(cols, off, p, h, False)
    assert n_changed == 0 and np.array_equal(table.kmeans_read(), first)
    p2 = p.copy()
    p2[2, 2] = -1e6                            # every row of code 2 in column 0 goes to cluster 2, every other row keeps its label
    counts, sizes, n_changed = table.kmeans_assign(cols, off, p2, h, False)
    moved = (codes[0] == 2) & (first != 2)
    assert n_changed == int(moved.sum()) > 0
    a_r, c_r, s_r, n_r = _numpy_step(codes, n_codes, cols, off, p2, h, prev=first)
    assert n_r == n_changed
    np.testing.assert_array_equal(table.kmeans_read(), a_r)
    np.testing.assert_array_equal(counts, c_r)
    np.testing.assert_array_equal(sizes, s_r)
    fresh = N.Table(codes, n_codes)            # another table: the labels belong to the table
    with pytest.raises(N.RepairGbmError) as ei:
        fresh.kmeans_assign(cols, off, p, h, False)
    assert ei.value.code == -2
    with pytest.raises(N.RepairGbmError) as ei:
        fresh.kmeans_read()
    assert ei.value.code == -2


def test_refusals_leave_the_previous_labels():
    from repair import _native as N
    codes, n_codes, cols, off, p, h = _case(WG_ROWS + 5, [5, 7], 3, seed=13)
    table, first = _check_step(codes, n_codes, cols, off, p, h)
    d_tot = p.shape[0]

    def refused(cols_, off_, p_, h_, first_=True):
        with pytest.raises(N.RepairGbmError) as ei:
            table.kmeans_assign(cols_, off_, p_, h_, first_)
        assert ei.value.code == -2, ei.value
        np.testing.assert_array_equal(table.kmeans_read(), first)

    refused(cols, off, np.zeros((d_tot, 1)), np.zeros(1))                              # k < 2
    refused(cols, off, np.zeros((d_tot, 65)), np.zeros(65))                            # k > 64
    refused(np.zeros(0, np.int32), np.zeros(0, np.int64), p, h)                        # no column
    refused([0, 2], off, p, h)                                                         # a column outside the table
    refused([0, -1], off, p, h)
    refused(cols, [0, 6], p, h)                                                        # 6 + 7 codes > d_tot = 12
    refused(cols, [-1, 5], p, h)
    refused(cols, off, p[:d_tot - 1], h)                                               # d_tot too small for the dictionaries
    big = (1 << 27) // 64 + 1                                                          # d_tot * k > 2^27: refused before P is read
    z = np.zeros(64)
    rc = N.lib().rgbm_table_kmeans_assign(table.h, N._p(np.asarray(cols, np.int32), N.C.c_int32), N.C.c_int32(2), N._p(off, N.C.c_int64),
                                          N.C.c_int32(64), N._p(z, N.C.c_double), N.C.c_int64(big), N._p(z, N.C.c_double), N.C.c_int32(1),
                                          N._p(np.zeros(1, np.int64), N.C.c_int64), N._p(np.zeros(64, np.int64), N.C.c_int64),
                                          N.C.byref(N.C.c_int64(0)))
    assert rc == -2
    np.testing.assert_array_equal(table.kmeans_read(), first)
    counts, sizes, n_changed = table.kmeans_assign(cols, off, p, h, False)             # and the table still steps
    assert n_changed == 0


def _frames():
    from tests.helpers import frame, load_golden
    return {"adult": (frame(load_golden("adult")["input"]), "3"), "random": (R.random_frame(5000), "4")}


@pytest.mark.parametrize("name", ["adult", "random"])
def test_split_input_table_through_the_hip_engine(name, monkeypatch):
    from repair.api import Delphi
    from repair.engine import HipEngine
    from repair.misc import RepairMisc
    df, k = _frames()[name]
    Delphi.register_table("km_" + name, df)
    opts = {"table_name": "km_" + name, "row_id": "tid", "k": k}

    class Counting(HipEngine):
        steps = 0

        def kmeans_assign(self, *a, **kw):
            Counting.steps += 1
            return HipEngine.kmeans_assign(self, *a, **kw)

    misc = RepairMisc().options(opts)
    misc._engine_override = Counting(0)
    got = misc.splitInputTable()
    assert Counting.steps >= 1
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    want = RepairMisc().options(opts).splitInputTable()
    assert got["tid"].tolist() == want["tid"].tolist() and got["k"].tolist() == want["k"].tolist()
    assert sorted(set(got["k"])) == list(range(int(k)))
