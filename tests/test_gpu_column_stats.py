"""-m gpu: `rgbm_table_column_stats` (csrc/rgbm_colstats.hip: k_colstat_count, k_colstat_reduce) against its numpy statement
`repair.table_stats.column_stats` -- integers throughout, so equality, no tolerance -- and `RepairMisc.describe` / `generateDepGraph`
through the HIP engine against their numpy paths."""

import numpy as np
import pytest

from tests import misc_restatement as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu


def _const(name):
    """A constant of the source, not a copy of it."""
    return csrc_constant(name)


CC_LDS = _const("CC_LDS")                      # codes up to which the count pass keeps 32-bit counters in LDS
CHUNK = 256 * _const("CS_ITEMS")               # codes per block scan of the reduce pass


def _check(codes, n_codes, cols, luts=None, n_bins=0, table=None):
    from repair import _native as N
    from repair import table_stats as T
    table = table if table is not None else N.Table(codes, n_codes)
    got = table.column_stats(cols, len_luts=luts, n_bins=n_bins)
    want = T.column_stats(codes, n_codes, cols, len_luts=luts, n_bins=n_bins)
    for f in T.FIELDS:
        assert got[f].dtype == np.int64
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    if n_bins:
        assert got["edges"].dtype == np.int32 and got["edges"].shape == (len(cols), n_bins + 1)
        np.testing.assert_array_equal(got["edges"], want["edges"])
    else:
        assert got["edges"] is None
    return table, got


def _table(n, n_codes, seed, null=0.05):
    rng = np.random.default_rng(seed)
    n_codes = np.asarray(n_codes, np.int32)
    codes = np.stack([R.random_codes(rng, n, int(d), null=null) for d in n_codes])
    luts = [rng.integers(0, 40, int(d)).astype(np.int32) for d in n_codes]
    return codes, n_codes, luts


def test_constants_are_what_the_cases_below_assume():
    assert CC_LDS == 8192 and 100003 > 40 * CHUNK and CHUNK > 1


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025, 70001])
def test_row_counts(n):
    codes, n_codes, luts = _table(n, [5, 300], seed=n)
    _check(codes, n_codes, [0, 1], luts, n_bins=8)


@pytest.mark.parametrize("d", [1, 2, CC_LDS - 1, CC_LDS, CC_LDS + 1, 100003])
def test_code_counts_either_side_of_the_lds_histogram_and_over_many_scan_chunks(d):
    codes, n_codes, luts = _table(30011, [d, 3], seed=d, null=0.1)
    _check(codes, n_codes, [0, 1], luts, n_bins=8)
    _check(codes, n_codes, [0], None, n_bins=0)


@pytest.mark.parametrize("n_cols", [1, 2, 17])
def test_listed_column_counts(n_cols):
    codes, n_codes, luts = _table(5003, [2 + 37 * j for j in range(n_cols)], seed=300 + n_cols)
    _check(codes, n_codes, list(range(n_cols)), luts, n_bins=4)


def test_columns_out_of_table_order_one_listed_twice_and_luts_for_some():
    codes, n_codes, luts = _table(4099, [7, CC_LDS + 5, 3, 90], seed=11)
    cols = [3, 1, 3, 0]
    _check(codes, n_codes, cols, [luts[3], None, None, luts[0]], n_bins=8)
    _check(codes, n_codes, cols, None, n_bins=2)


def test_all_null_column_codes_outside_the_dictionary_and_first_or_last_code_only():
    n = 3001
    rng = np.random.default_rng(5)
    n_codes = np.asarray([4, 9, CC_LDS + 100, CC_LDS + 100, 6], np.int32)
    codes = np.stack([np.full(n, -1, np.int32),
                      rng.integers(-3, 14, n).astype(np.int32),                   # -3..-1 and 9..13 are NULL
                      np.where(rng.random(n) < 0.2, -1, 0).astype(np.int32),      # only the first code
                      np.full(n, CC_LDS + 99, np.int32),                          # only the last one
                      np.full(n, 5, np.int32)])
    luts = [rng.integers(1, 9, int(d)).astype(np.int32) for d in n_codes]
    _, got = _check(codes, n_codes, [0, 1, 2, 3, 4], luts, n_bins=8)
    assert got["nulls"][0] == n and got["distinct"][0] == 0 and (got["edges"][0] == -1).all()
    assert got["distinct"][2] == 1 and (got["edges"][2] == 0).all() and (got["edges"][3] == CC_LDS + 99).all()


@pytest.mark.parametrize("n_bins", [0, 1, 2, 8, 254])
def test_bin_counts_and_more_bins_than_distinct_values(n_bins):
    codes, n_codes, luts = _table(2503, [3, 1000, CC_LDS + 1], seed=40 + n_bins)
    _check(codes, n_codes, [0, 1, 2], luts, n_bins=n_bins)


def test_ranks_on_and_above_a_cumulative_count():
    codes = np.asarray([[0, 0, 1, 1, 3, 3, 4, 4]], np.int32)            # cumulative 2 4 4 6 8
    _, got = _check(codes, [5], [0], None, n_bins=4)                    # ranks 2 4 6 8: each lands on a cumulative count
    assert got["edges"].tolist() == [[0, 0, 1, 3, 4]]
    _, got = _check(codes[:, :7], [5], [0], None, n_bins=4)             # ranks 2 4 6 7
    assert got["edges"].tolist() == [[0, 0, 1, 3, 4]]
    _, got = _check(codes[:, 1:], [5], [0], None, n_bins=2)             # cumulative 1 3 3 5 7, ranks 4 (one above 3) and 7
    assert got["edges"].tolist() == [[0, 3, 4]]
    # the same on counts that cross the chunks of the reduce pass: 3 rows per code, ranks on every 3rd code boundary
    d = 2 * CHUNK + 77
    wide = np.repeat(np.arange(d, dtype=np.int32), 3)[None, :]
    _check(wide, [d], [0], None, n_bins=d // 100)
    _check(wide[:, :-1], [d], [0], None, n_bins=254)


def test_len_sum_beyond_32_bits_and_no_lut_for_some_columns():
    big = 2 ** 31 - 1
    codes = np.asarray([[0, 0, 0, 1, -1], [1, 1, 0, 0, 0]], np.int32)
    luts = [np.asarray([big, 7], np.int32), None]
    _, got = _check(codes, [2, 2], [0, 1, 0], [luts[0], None, luts[0]], n_bins=0)
    assert got["len_sum"].tolist() == [3 * big + 7, 0, 3 * big + 7] and 3 * big + 7 > 2 ** 32 and got["len_max"].tolist() == [big, 0, big]


def test_every_refusal_leaves_the_table_working():
    from repair import _native as N
    codes, n_codes, luts = _table(1000, [5, 7], seed=2)
    table, first = _check(codes, n_codes, [0, 1], luts, n_bins=8)

    def refused(cols, n_bins=0, codes_ok=(-1, -2)):
        with pytest.raises(N.RepairGbmError) as ei:
            table.column_stats(cols, n_bins=n_bins)
        assert ei.value.code in codes_ok, ei.value

    refused([])                                   # n_cols < 1
    refused([2])                                  # a column outside the table
    refused([0, -1])
    refused([0], n_bins=255)
    refused([0], n_bins=-1)
    cc, stats = np.asarray([0], np.int32), np.zeros(6, np.int64)
    rc = N.lib().rgbm_table_column_stats(table.h, N._p(cc, N.C.c_int32), N.C.c_int32(1), None, N.C.c_int32(8), N._p(stats, N.C.c_int64), None)
    assert rc in (-1, -2) and not stats.any()     # edges_out == NULL with n_bins > 0
    for a, b in ((None, stats), (cc, None)):
        rc = N.lib().rgbm_table_column_stats(table.h, N._p(a, N.C.c_int32), N.C.c_int32(1), None, N.C.c_int32(0), N._p(b, N.C.c_int64), None)
        assert rc == -1
    _, again = _check(codes, n_codes, [0, 1], luts, n_bins=8, table=table)
    np.testing.assert_array_equal(again["edges"], first["edges"])
    np.testing.assert_array_equal(table.read_column(1), codes[1])                # untouched


def test_other_entries_of_the_table_still_agree_after_column_stats():
    """The entry shares the table's scratch with every other relational step: count_codes and pair_counts after it, and it after them."""
    from repair import depgraph
    codes, n_codes, luts = _table(9001, [11, CC_LDS + 3, 4], seed=8)
    table, _ = _check(codes, n_codes, [1, 0, 2], None, n_bins=8)
    cnt, nn = table.count_codes(1)
    ok = codes[1] >= 0
    np.testing.assert_array_equal(cnt, np.bincount(codes[1][ok], minlength=int(n_codes[1])))
    assert nn == int((~ok).sum())
    np.testing.assert_array_equal(table.pair_counts([(0, 2)])[0], depgraph.dense_pair_counts(codes, n_codes, [(0, 2)])[0])
    _check(codes, n_codes, [2, 1], [luts[2], luts[1]], n_bins=2, table=table)


def _frames():
    from tests.helpers import frame, load_golden
    return {"adult": frame(load_golden("adult")["input"]), "random": R.misc_frame(5000)}


@pytest.mark.parametrize("name", ["adult", "random"])
def test_describe_and_dep_graph_through_the_hip_engine(name, monkeypatch, tmp_path):
    from repair.api import Delphi
    from repair.engine import HipEngine
    from repair.misc import RepairMisc
    df = _frames()[name]
    Delphi.register_table("cs_" + name, df)

    class Counting(HipEngine):
        stats, uploads = 0, 0

        def column_stats(self, *a, **kw):
            Counting.stats += 1
            return HipEngine.column_stats(self, *a, **kw)

        def upload_dictionaries(self, *a, **kw):
            Counting.uploads += 1
            return HipEngine.upload_dictionaries(self, *a, **kw)

    def opts(d):
        return {"table_name": "cs_" + name, "num_bins": "8", "path": str(tmp_path / d), "max_domain_size": "20", "max_attr_value_num": "6",
                "pairwise_attr_stat_threshold": "2.5", "edge_label": "1"}

    misc = RepairMisc().options(opts("gpu"))
    misc._engine_override = Counting(0)
    got = misc.describe()
    assert Counting.stats == 1 and Counting.uploads == 1
    misc.generateDepGraph()
    assert Counting.uploads == 2
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    host = RepairMisc().options(opts("host"))
    want = host.describe()
    host.generateDepGraph()
    assert list(got.columns) == list(want.columns) and got.to_dict("list") == want.to_dict("list")
    text = open(str(tmp_path / "gpu" / "depgraph.dot"), encoding="utf-8").read()
    assert text == open(str(tmp_path / "host" / "depgraph.dot"), encoding="utf-8").read()
    assert len(R.parse_dot(text)["edges"]) > 0
