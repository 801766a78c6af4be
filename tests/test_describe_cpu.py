"""CPU: `RepairMisc.describe` and its statement in code space, `repair.table_stats.column_stats`.

The two mirrors of the reference's `test_describe` (its expected rows are tests/golden/misc_describe_depgraph.json), and `column_stats`
against a restatement in VALUE space (tests/misc_restatement.py: pandas `nunique`, `isna().sum()` and ranks among the sorted values).
Everything is an integer or follows from integers by one division: equality throughout."""
import numpy as np
import pandas as pd
import pytest

from tests import misc_restatement as R

COLUMNS = ["attrName", "distinctCnt", "min", "max", "nullCnt", "avgLen", "maxLen", "hist"]


def _describe(df, name, **opts):
    from repair.api import Delphi
    from repair.misc import RepairMisc
    Delphi.register_table(name, df)
    return RepairMisc().options(dict({"table_name": name}, **opts)).describe()


def _rows(out, skip=()):
    assert list(out.columns) == COLUMNS
    rows = [[None if (not isinstance(v, list) and pd.isna(v)) else v for v in r] for r in out.itertuples(index=False, name=None) if r[0] not in skip]
    return sorted(rows, key=lambda r: r[0])


def test_describe_adult_gives_the_rows_of_the_reference():
    from tests.helpers import frame, load_golden
    out = _describe(frame(load_golden("adult")["input"]), "describe_adult")
    assert list(out["attrName"])[0] == "tid" and len(out) == 8           # frame order, one row per column
    assert _rows(out, skip=("tid",)) == R.golden()["describe"]["adult_without_tid"]


def test_describe_range_table_gives_the_rows_and_both_histograms_of_the_reference():
    g = R.golden()["describe"]["range"]
    i = np.arange(g["rows"])
    df = pd.DataFrame({"id": [str(v) for v in i], "v1": (i % 9).astype(np.int64), "v2": (i % 17).astype(np.float64)})
    assert _rows(_describe(df, "describe_range")) == g["expected"]


def test_describe_needs_a_table_name_and_a_sane_bin_count():
    from repair.misc import RepairMisc
    with pytest.raises(ValueError, match="Required options not found: table_name"):
        RepairMisc().describe()
    df = pd.DataFrame({"a": [1, 2, 3]})
    for bad in ("0", "255", "x"):
        with pytest.raises(ValueError, match="num_bins"):
            _describe(df, "describe_bins", num_bins=bad)
    assert len(_describe(df, "describe_bins", num_bins="254")["hist"][0]) == 254


def test_describe_edge_columns():
    """No value at all (numeric and string), one distinct number (max = min: no histogram), item sizes, integers printed as integers."""
    df = pd.DataFrame({"i32": np.asarray([5, 7, 7, 9], np.int32), "f": [1.5, np.nan, 1.5, 1.5], "nonum": [np.nan] * 4,
                       "nostr": np.asarray([None] * 4, dtype=object), "s": ["ab", None, "abcd", "ab"], "nullable": pd.array([1, None, 3, 3], dtype="Int64")})
    rows = {r[0]: r[1:] for r in _rows(_describe(df, "describe_edges", num_bins="2"))}
    assert rows["i32"] == [3, "5", "9", 0, 4, 4, [0.5, 0.5]]              # ranks 2, 4 of (5, 7, 7, 9): edges 5, 7, 9
    assert rows["f"] == [1, "1.5", "1.5", 1, 8, 8, None]
    assert rows["nonum"] == [0, None, None, 4, 8, 8, None]
    assert rows["nostr"] == [0, None, None, 4, 20, 20, None]
    assert rows["s"] == [2, None, None, 1, 3, 4, None]                    # ceil((2 + 4 + 2) / 3) = 3
    assert rows["nullable"] == [2, "1", "3", 1, 8, 8, [1.0, 0.0]]         # ranks 2, 3 of (1, 3, 3): edges 1, 3, 3
    assert len(_describe(df.iloc[:0], "describe_empty")) == 6


def test_describe_random_frame_against_pandas():
    df = R.misc_frame(700)
    out = _describe(df, "describe_random", num_bins="8").set_index("attrName")
    for c in df.columns:
        assert out.loc[c, "distinctCnt"] == df[c].nunique() and out.loc[c, "nullCnt"] == int(df[c].isna().sum())
    assert out.loc["level", "min"] == "0" and out.loc["level", "max"] == "3" and out.loc["const", "hist"] is None
    have = np.sort(df["score"].dropna().to_numpy())
    edges = [have[0]] + [have[-(-(i * len(have)) // 8) - 1] for i in range(1, 9)]
    assert out.loc["score", "hist"] == [float((edges[i + 1] - edges[i]) / (edges[8] - edges[0])) for i in range(8)]
    lens = df["text"].dropna().map(len)
    assert out.loc["text", "avgLen"] == -(-int(lens.sum()) // len(lens)) and out.loc["text", "maxLen"] == int(lens.max())
    assert (out.loc["none", "avgLen"], out.loc["none", "maxLen"]) == (20, 20)


def _check_against_values(codes, dicts, n_bins, cols=None):
    from repair import table_stats as T
    cols = list(range(len(dicts))) if cols is None else cols
    luts = [np.asarray([len(v) for v in dicts[c]] or [0], np.int32) for c in cols]
    got = T.column_stats(codes, [max(len(d), 1) for d in dicts], cols, len_luts=luts, n_bins=n_bins)
    assert all(got[f].dtype == np.int64 for f in T.FIELDS) and (n_bins == 0) == (got["edges"] is None)
    for j, c in enumerate(cols):
        values = [dicts[c][v] if 0 <= v < len(dicts[c]) else None for v in codes[c]]
        want = R.value_space_stats(values, dicts[c], n_bins)
        for f in T.FIELDS:
            assert int(got[f][j]) == want[f], (c, f)
        if n_bins:
            assert got["edges"].dtype == np.int32 and got["edges"][j].tolist() == want["edges"], c
    return got


@pytest.mark.parametrize("n_bins", [0, 1, 2, 8, 254])
@pytest.mark.parametrize("n", [1, 9, 500])
def test_column_stats_equals_the_value_space_restatement(n, n_bins):
    """NULLs, dictionary entries no row holds, an all-NULL column (a one-code domain without a row), codes outside the dictionary, a one-row frame."""
    rng = np.random.default_rng(1000 * n + n_bins)
    dicts = [R.random_dictionary(rng, d) for d in (1, 2, 7, 40, 300)] + [[]]
    codes = np.stack([R.random_codes(rng, n, len(d)) for d in dicts[:-1]] + [np.full(n, -1, np.int32)])
    codes[3, rng.random(n) < 0.1] = 40                  # beyond the dictionary: NULL
    got = _check_against_values(codes, dicts, n_bins)
    assert got["nulls"][5] == n and got["distinct"][5] == 0 and got["min_code"][5] == got["max_code"][5] == -1
    _check_against_values(codes, dicts, n_bins, cols=[4, 0, 4])       # out of table order, one listed twice


def test_ranks_on_and_above_a_cumulative_count():
    from repair import table_stats as T
    dicts = [["a", "b", "c", "d", "e"]]
    codes = np.asarray([[0, 0, 1, 1, 3, 3, 4, 4]], np.int32)            # counts 2 2 0 2 2: cumulative 2 4 4 6 8, code 2 never occurs
    got = _check_against_values(codes, dicts, 4)                        # ranks 2 4 6 8 land on the cumulative counts
    assert got["edges"].tolist() == [[0, 0, 1, 3, 4]]
    got = _check_against_values(codes[:, :7], dicts, 4)                 # m = 7: ranks 2 4 6 7 -- the last one above 6
    assert got["edges"].tolist() == [[0, 0, 1, 3, 4]]
    got = _check_against_values(codes[:, 1:], dicts, 2)                 # counts 1 2 0 2 2: ranks 4 (one above 3) and 7
    assert got["edges"].tolist() == [[0, 3, 4]]
    got = _check_against_values(codes, dicts, 254)                      # more bins than values
    assert sorted(set(got["edges"][0].tolist())) == [0, 1, 3, 4]
    no_lut = T.column_stats(codes, [5], [0], n_bins=0)
    assert no_lut["len_sum"][0] == 0 and no_lut["len_max"][0] == 0 and no_lut["edges"] is None


def test_column_stats_refuses_what_the_device_entry_refuses():
    from repair import table_stats as T
    codes = np.zeros((2, 4), np.int32)
    for kw in (dict(cols=[]), dict(cols=[2]), dict(cols=[-1]), dict(cols=[0], n_bins=255), dict(cols=[0], n_bins=-1), dict(cols=[0], len_luts=[None, None])):
        with pytest.raises(ValueError):
            T.column_stats(codes, [1, 1], **kw)
