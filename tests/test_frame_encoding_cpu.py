"""CPU: `repair.frame_encoding.FrameEncoding` -- the edits `repair_frame` makes to the dictionary encoding on the host -- against a plain
restatement: the same edits applied to a copy of the DataFrame, which `encode_frame` then encodes from scratch.  Required of every case:
the decoded table is equal, the codes `remaps[j][indices[j]]` and the dictionaries `dicts[j]` of the target (pruned) columns are equal,
and `check()` holds."""
import numpy as np
import pandas as pd
import pytest

from repair.frame_encoding import FrameEncoding
from repair.pipeline import encode_frame

COLS = ["s", "t", "x"]


def _frame():
    return pd.DataFrame({"s": ["m", "d", "m", "h", None, "d", "t", "m", "h", "d"],
                         "t": ["b", "a", "b", "c", "a", "b", "only", "a", None, "c"],
                         "x": [2.5, 1.0, np.nan, 2.5, 7.0, 1.0, 1.0, -3.0, 2.5, 7.0]})


def _decoded(enc):
    return [list(enc.values(np.arange(enc.n), j)) for j in range(len(enc.columns))]


def _codes(indices, remaps, j):
    return np.where(indices[j] >= 0, remaps[j][np.maximum(indices[j], 0)] if len(remaps[j]) else -1, -1)


def _same_as_restated(enc, edited, targets):
    """`enc` after its edits against `encode_frame` of the frame `edited` the same way."""
    enc.check()
    idx, remaps, dicts = encode_frame(edited, COLS)
    want = FrameEncoding(COLS, idx, remaps, dicts)
    assert _decoded(enc) == _decoded(want)
    for t in targets:
        j = COLS.index(t)
        assert np.array_equal(_codes(enc.indices, enc.remaps, j), _codes(idx, remaps, j)), t
        assert enc.dicts[j].dtype == dicts[j].dtype and list(enc.dicts[j]) == list(dicts[j]), t
        assert int(max(enc.remaps[j].max(initial=-1) + 1, 1)) == max(len(dicts[j]), 1)          # the code count the upload derives


def _null(df, cells):
    for r, c in cells:
        df.loc[r, c] = None
    return df


def test_encode_frame_is_the_encoding_and_check_holds():
    df = _frame()
    enc = FrameEncoding.of_frame(df, COLS)
    enc.check()
    idx, remaps, dicts = encode_frame(df, COLS)
    assert np.array_equal(idx, enc.indices) and all(np.array_equal(a, b) for a, b in zip(remaps, enc.remaps))
    assert enc.n == 10 and enc.pos == {"s": 0, "t": 1, "x": 2} and enc.columns == COLS
    assert list(enc.dicts[0]) == ["d", "h", "m", "t"] and enc.dicts[2].dtype == np.float64 and list(enc.dicts[2]) == [-3.0, 1.0, 2.5, 7.0]
    assert _decoded(enc)[2][2] is None and _decoded(enc)[0][4] is None                       # NaN and None are NULL
    assert [enc.live_classes(j) for j in range(3)] == [4, 4, 4]


# ---- write: insertion edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, values", [
    ([0], ["a"]),                       # before the first entry
    ([0, 2], ["e", "e"]),               # between two entries
    ([1], ["z"]),                       # after the last entry
    ([0, 4], ["h", "h"]),               # a value the column holds already (one of the cells is NULL)
    ([0, 4, 7], ["n", "a", "n"]),       # two different new values in one call
], ids=["before first", "between", "after last", "existing", "two new"])
def test_write_keeps_the_codes_the_ascending_ranks(rows, values):
    df = _frame()
    enc = FrameEncoding.of_frame(df, COLS)
    cells = [(r, "s") for r in rows]
    held = enc.null_cells(rows, [0] * len(rows), prune=[0, 1])        # as `repair_frame` does: the cells are NULLed, then written
    assert list(held) == [df.loc[r, "s"] for r in rows]
    enc.write(0, rows, values)
    edited = _null(_frame(), cells)
    for r, v in zip(rows, values):
        edited.loc[r, "s"] = v
    _same_as_restated(enc, edited, ["s", "t"])


# ---- null_cells: NULL-and-prune edges -------------------------------------------------------------------------------------------
def test_nulling_the_only_holder_prunes_a_target_column_and_leaves_another():
    enc = FrameEncoding.of_frame(_frame(), COLS)
    held = enc.null_cells([6, 6], [1, 0], prune=[1])                  # `only` in t (a target), `t` in s (not one)
    assert list(held) == ["only", "t"]
    assert list(enc.dicts[1]) == ["a", "b", "c"] and enc.live_classes(1) == 3
    assert list(enc.dicts[0]) == ["d", "h", "m", "t"] and enc.live_classes(0) == 3          # the entry stays, no row holds it
    _same_as_restated(enc, _null(_frame(), [(6, "t"), (6, "s")]), ["t"])


def test_nulling_every_cell_of_a_column():
    enc = FrameEncoding.of_frame(_frame(), COLS)
    held = enc.null_cells(np.arange(10), np.full(10, 1), prune=[1])
    assert list(held) == list(_frame()["t"])
    assert len(enc.dicts[1]) == 0 and enc.live_classes(1) == 0 and (enc.indices[1] == -1).all()
    _same_as_restated(enc, _null(_frame(), [(r, "t") for r in range(10)]), ["t"])


def test_numeric_column_values_are_float64_and_nan_is_null():
    enc = FrameEncoding.of_frame(_frame(), COLS)
    held = enc.null_cells([7, 2, 4], [2, 2, 2], prune=[2])            # -3.0 has one holder; row 2 is NaN already; 7.0 keeps a holder
    assert list(held) == [-3.0, None, 7.0]
    assert enc.dicts[2].dtype == np.float64 and list(enc.dicts[2]) == [1.0, 2.5, 7.0]
    edited = _frame()
    edited.loc[[7, 2, 4], "x"] = np.nan
    _same_as_restated(enc, edited, ["x"])


def test_the_empty_cell_list_changes_nothing():
    enc = FrameEncoding.of_frame(_frame(), COLS)
    held = enc.null_cells(np.zeros(0, np.int64), np.zeros(0, np.int32), prune=[0, 1, 2])
    assert len(held) == 0
    enc.write(0, np.zeros(0, np.int64), np.zeros(0, object))
    _same_as_restated(enc, _frame(), COLS)
    assert list(enc.current_values(np.array([6]), np.array([1]), np.array([3]))) == ["only"]


# ---- held values ----------------------------------------------------------------------------------------------------------------
def test_the_first_value_recorded_for_a_cell_wins_and_other_cells_decode():
    enc = FrameEncoding.of_frame(_frame(), COLS)
    enc.null_cells([0, 6], [0, 1], prune=[0, 1])                      # first pass: `m` of (0, s) and `only` of (6, t) are recorded
    held = enc.null_cells([0, 3, 6], [0, 0, 1], prune=[0, 1])         # second pass: (0, s) and (6, t) are NULL by now
    assert list(held) == [None, "h", None]
    enc.check()
    rows, cols = np.array([0, 3, 6, 1, 4]), np.array([0, 0, 1, 0, 0], np.int32)
    codes = np.array([-1, -1, -1, 0, -1], np.int32)                   # (1, s) was never recorded: its code decodes; (4, s) is a NULL
    assert list(enc.current_values(rows, cols, codes)) == ["m", "h", "only", "d", None]
    enc.hold([1], [0], ["first"])
    enc.hold([1, 1], [0, 0], ["second", "third"])
    assert list(enc.current_values(np.array([1]), np.array([0]), np.array([0]))) == ["first"]
    assert list(enc.decode(np.array([2, -1, 1]), np.array([1, 1, 2]))) == ["c", None, 1.0]
