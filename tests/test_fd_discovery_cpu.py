"""CPU: functional-dependency discovery.  The numpy statement `repair.fd_codes.fd_measures` against the plain-Python
restatement (tests/fd_restatement.py), the rules of the level-wise search (`repair.fd_discovery.discover`) on frames built by hand, the round
trip of every reported dependency through the value-space `ConstraintErrorDetector`, and the options of `RepairMisc.discoverFunctionalDeps`.
Everything is an integer: equality throughout."""
import itertools

import numpy as np
import pandas as pd
import pytest

from tests import fd_restatement as R

COLUMNS = ["lhs", "rhs", "groups", "removed_rows", "violating_rows", "error", "constraint"]


# ---------------------------------------------------------------------------------------------
# the statement against the restatement
# ---------------------------------------------------------------------------------------------
def _statement(codes, n_codes, lhs, rhs):
    from repair.fd_codes import fd_measures
    return fd_measures(codes, n_codes, lhs, rhs)


def test_worked_example_by_value():
    e = R.EXAMPLE
    got = _statement(e["codes"], e["n_codes"], [0], [1])
    R.assert_same(got, e["want"])
    R.assert_same(got, R.fd_measures(e["codes"], e["n_codes"], [0], [1]))
    assert e["codes"].shape[1] - int(got["kept"][0]) == 1                 # removed


@pytest.mark.parametrize("shape", ["one", "singletons", "skewed"])
@pytest.mark.parametrize("n", R.ROW_EDGES)
def test_statement_equals_the_restatement(n, shape):
    codes, n_codes = R.mixed_table(n, seed=n, shape=shape)
    c = codes.shape[0]
    for n_lhs in (0, 1, 2, 3, 11):
        lhs = list(range(n_lhs))
        rhs = [j for j in range(c) if j not in lhs]
        for pick in (rhs[-1:], rhs[-2:], rhs):
            R.assert_same(_statement(codes, n_codes, lhs, pick), R.fd_measures(codes, n_codes, lhs, pick), (n, shape, n_lhs, pick))


def test_ties_nulls_and_codes_outside_the_dictionary():
    # one group (x = 0) with y values 0, 0, 1, 1 (a tie), one NULL group whose y is NULL written four ways: a single (NULL, NULL) key
    codes = np.asarray([[0, 0, 0, 0, -1, 3, 9, -5], [0, 0, 1, 1, -1, 2, 7, -2]], np.int32)
    got = _statement(codes, [3, 2], [0], [1])
    R.assert_same(got, dict(groups=2, kept=[2 + 4], violating=[4], xy_groups=[3]))
    R.assert_same(got, R.fd_measures(codes, [3, 2], [0], [1]))
    got = _statement(codes, [3, 2], [], [0, 1])                           # no left-hand side: one group
    R.assert_same(got, dict(groups=1, kept=[4, 4], violating=[8, 8], xy_groups=[2, 3]))


def test_statement_refuses_what_the_entry_refuses():
    codes, n_codes = R.mixed_table(10, c=13)
    for lhs, rhs in (([0], []), ([0, 0], [1]), ([0], [1, 1]), ([0], [0]), ([13], [1]), ([0], [-1]), (list(range(12)), [12])):
        with pytest.raises(ValueError):
            _statement(codes, n_codes, lhs, rhs)


# ---------------------------------------------------------------------------------------------
# the search rules, on frames built by hand
# ---------------------------------------------------------------------------------------------
def _discover(df, name, **opts):
    from repair.api import Delphi
    from repair.misc import RepairMisc
    Delphi.register_table(name, df)
    m = RepairMisc().options(dict({"table_name": name}, **opts))
    m._engine_override = None
    import os
    old = os.environ.get("REPAIR_RESIDENT")
    os.environ["REPAIR_RESIDENT"] = "0"                                   # the numpy statement, whatever the machine holds
    try:
        return m.discoverFunctionalDeps()
    finally:
        if old is None:
            del os.environ["REPAIR_RESIDENT"]
        else:
            os.environ["REPAIR_RESIDENT"] = old


def _deps(out):
    return [(l, r) for l, r in zip(out["lhs"], out["rhs"])]


def xor_frame(n=64):
    i = np.arange(n)
    a, b = i % 2, (i // 2) % 2
    return pd.DataFrame({"tid": i, "a": a.astype(str), "b": b.astype(str), "c": (a ^ b).astype(str)})


def exact_frame(n=60):
    """a -> c exactly; b is free; d is constant; tid numbers the rows."""
    i = np.arange(n)
    return pd.DataFrame({"tid": i, "a": (i % 5).astype(str), "b": (i % 4).astype(str), "c": ((i % 5) // 2).astype(str), "d": ["k"] * n})


def dirty_frame(n, k):
    """a -> c with exactly k dirty rows: ten a values, c = a % 3, and k rows of different groups' tails set to another value."""
    i = np.arange(n)
    a = i % 10
    c = a % 3
    c[np.arange(k) * 10 + 3] = 7                                          # k rows of the group a = 3, whose other rows hold c = 0
    assert k < n // 10 // 2
    return pd.DataFrame({"tid": i, "a": a.astype(str), "c": c.astype(str)})


def test_xor_is_found_at_size_two_and_not_at_size_one():
    df = xor_frame()
    two = _discover(df, "fd_xor", row_id="tid", max_lhs_size="2")
    assert ("a,b", "c") in _deps(two) and ("a", "c") not in _deps(two) and ("b", "c") not in _deps(two)
    assert set(_deps(two)) == {("a,b", "c"), ("a,c", "b"), ("b,c", "a")}
    one = _discover(df, "fd_xor", row_id="tid", max_lhs_size="1")
    assert _deps(one) == []


def test_exact_dependency_keeps_its_supersets_out():
    out = _discover(exact_frame(), "fd_exact", row_id="tid", max_lhs_size="3")
    assert ("a", "c") in _deps(out)
    assert not any(r == "c" and l != "a" and "a" in l.split(",") for l, r in _deps(out))
    row = out[(out["lhs"] == "a") & (out["rhs"] == "c")].iloc[0]
    assert (row["groups"], row["removed_rows"], row["violating_rows"], row["error"]) == (5, 0, 0, 0.0)
    assert row["constraint"] == "t1&t2&EQ(t1.a,t2.a)&IQ(t1.c,t2.c)"


def test_row_id_like_column_is_on_no_left_hand_side_and_nowhere_when_named():
    df = exact_frame()
    named = _discover(df, "fd_rid", row_id="tid", max_lhs_size="2")
    assert not any("tid" in l.split(",") or r == "tid" for l, r in _deps(named))
    free = _discover(df, "fd_rid", max_lhs_size="2")                      # tid is a key: its results are discarded, its supersets skipped
    assert not any("tid" in l.split(",") for l, r in _deps(free))
    assert _deps(free) == _deps(named)                                    # and nothing but a key determines tid


def test_constant_column_is_in_no_record(caplog):
    import logging
    with caplog.at_level(logging.INFO, logger="repair.misc"):
        out = _discover(exact_frame(), "fd_const", row_id="tid", max_lhs_size="2")
    assert not any("d" in l.split(",") or r == "d" for l, r in _deps(out))
    assert any("constant" in rec.getMessage() and "d" in rec.getMessage() for rec in caplog.records)


@pytest.mark.parametrize("n,k,below,at", [(1000, 7, "0.006", "0.007"), (100, 29, "0.28", "0.29")])
def test_threshold_is_exact_in_the_decimal_text(n, k, below, at):
    if (n, k) == (100, 29):
        # 29 dirty rows of 100 need a group that still holds more clean ones: a = 0 in 60 rows, 1 and 2 in 20 each, c = a, and 29 rows
        # of a = 0 set to another value (31 stay); neither column is constant within 29 rows
        i = np.arange(n)
        a = np.where(i < 60, 0, np.where(i < 80, 1, 2))
        c = a.copy()
        c[:k] = 5
        df = pd.DataFrame({"tid": i, "a": a.astype(str), "c": c.astype(str)})
        assert int(0.29 * 100) == 28                                      # the case floating point gets wrong
    else:
        df = dirty_frame(n, k)
    assert ("a", "c") not in _deps(_discover(df, "fd_dirty", row_id="tid", targets="c", max_lhs_size="1", max_error=below))
    out = _discover(df, "fd_dirty", row_id="tid", targets="c", max_lhs_size="1", max_error=at)
    assert _deps(out) == [("a", "c")]
    assert int(out["removed_rows"][0]) == k and out["error"][0] == k / n


def test_targets_restrict_right_hand_sides_only():
    df = xor_frame()
    out = _discover(df, "fd_targets", row_id="tid", targets="c", max_lhs_size="2")
    assert _deps(out) == [("a,b", "c")]                                   # a and b still serve on the left


def _codes_of(df, cols):
    from repair.frame_encoding import FrameEncoding
    enc = FrameEncoding.of_frame(df, cols)
    codes = np.stack([np.where(i >= 0, r[np.maximum(i, 0)] if len(r) else -1, -1).astype(np.int32) for i, r in zip(enc.indices, enc.remaps)])
    return codes, [max(len(d), 1) for d in enc.dicts]


def test_equal_partition_pruning_drops_nothing_and_saves_calls():
    from repair import fd_codes, fd_discovery
    for df in (exact_frame(), xor_frame(), _hand_frame()):
        cols = [c for c in df.columns if c != "tid"]
        codes, n_codes = _codes_of(df, cols)
        measure = lambda lhs, rhs: fd_codes.fd_measures(codes, n_codes, lhs, rhs)  # noqa: E731
        with_, without = {}, {}
        a = fd_discovery.discover(measure, len(df), cols, cols, 3, "0.0", "1.0", stats=with_)
        b = fd_discovery.discover(measure, len(df), cols, cols, 3, "0.0", "1.0", stats=without, prune_equal_partitions=False)
        assert a == b and with_["calls"] <= without["calls"]
    assert with_["calls"] < without["calls"]                              # the hand frame holds exact dependencies to prune by


def test_records_are_ordered_by_size_positions_and_right_hand_side():
    out = _discover(_hand_frame(), "fd_order", row_id="tid", max_lhs_size="3", max_error="0.02")
    cols = [c for c in _hand_frame().columns if c != "tid"]
    key = [(len(l.split(",")), [cols.index(a) for a in l.split(",")], cols.index(r)) for l, r in _deps(out)]
    assert key == sorted(key) and len(key) == len(set(map(str, key))) and len(key) > 3


def test_minimality_by_brute_force():
    """Every reported dependency holds, none of its proper subsets does, and every minimal one over non-key left-hand sides is reported."""
    from repair import fd_discovery
    df = _hand_frame()
    cols = [c for c in df.columns if c != "tid"]
    codes, n_codes = _codes_of(df, cols)
    n, limit = len(df), fd_discovery.max_removed_rows("0.02", len(df))
    out = _discover(df, "fd_brute", row_id="tid", max_lhs_size="2", max_error="0.02")
    removed = lambda X, y: n - R.fd_measures(codes, n_codes, list(X), [y])["kept"][0]  # noqa: E731
    groups = lambda X: R.fd_measures(codes, n_codes, list(X), [[j for j in range(len(cols)) if j not in X][0]])["groups"]  # noqa: E731
    live = [j for j in range(len(cols)) if removed((), j) > limit]
    want = []
    for k in (1, 2):
        for X in itertools.combinations(live, k):
            if any(groups(S) == n for r in range(1, k + 1) for S in itertools.combinations(X, r)):
                continue
            for y in live:
                if y in X or removed(X, y) > limit:
                    continue
                if any(removed(S, y) <= limit for r in range(1, k) for S in itertools.combinations(X, r)):
                    continue
                want.append((",".join(cols[j] for j in X), cols[y]))
    assert _deps(out) == want and len(want) >= 4


# ---------------------------------------------------------------------------------------------
# round trip through the value-space detector
# ---------------------------------------------------------------------------------------------
def _hand_frame(n=240):
    """city -> state exactly; (city, street) -> zip with three dirty rows; phone determines nothing; NULLs on both sides."""
    rng = np.random.default_rng(7)
    i = np.arange(n)
    city = i % 8
    street = (i // 8) % 5
    zipc = city * 5 + street
    zipc[[11, 95, 170]] = 99
    state = city // 3
    phone = rng.integers(0, 30, n)
    df = pd.DataFrame({"tid": i, "city": ["c%d" % v for v in city], "street": ["s%d" % v for v in street], "zip": ["z%02d" % v for v in zipc],
                       "state": ["st%d" % v for v in state], "phone": phone.astype(np.int64)})
    df.loc[[5, 13, 21], "city"] = None                                    # city 5 NULL in three rows: NULL is a group of its own
    df.loc[[40, 41], "state"] = None
    return df


def _flagged_rows(df, constraint):
    from repair.errors import ConstraintErrorDetector
    det = ConstraintErrorDetector(constraints=constraint).setUp("tid", df, [], [c for c in df.columns if c != "tid"])
    return int(det.detect()["tid"].nunique())


def _hospital():
    from tests.helpers import frame, load_golden
    df = frame(load_golden("hospital")["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    return df


@pytest.mark.parametrize("which", ["hand", "xor", "exact", "hospital"])
def test_constraint_text_flags_exactly_the_violating_rows(which):
    df = dict(hand=_hand_frame, xor=xor_frame, exact=exact_frame, hospital=_hospital)[which]()
    out = _discover(df, "fd_roundtrip_" + which, row_id="tid", max_lhs_size="2", max_error="0.01")
    assert len(out) > 0
    for rec in out.head(200).itertuples(index=False):
        flagged = _flagged_rows(df, rec.constraint)
        assert flagged == rec.violating_rows, (rec.lhs, rec.rhs, flagged, rec.violating_rows)
        if rec.removed_rows == 0:
            assert flagged == 0
        assert rec.removed_rows <= rec.violating_rows and rec.error == rec.removed_rows / len(df)


def test_a_column_name_that_breaks_the_predicate_pattern_is_left_out(caplog):
    import logging
    df = exact_frame().rename(columns={"c": "c&x"})
    with caplog.at_level(logging.WARNING, logger="repair.misc"):
        out = _discover(df, "fd_badname", row_id="tid", max_lhs_size="1")
    assert not any("c&x" in l or "c&x" in r for l, r in _deps(out))
    assert any("c&x" in rec.getMessage() and "left out" in rec.getMessage() for rec in caplog.records)


# ---------------------------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------------------------
def test_option_errors():
    from repair.misc import RepairMisc
    with pytest.raises(ValueError, match="Required options not found: table_name"):
        RepairMisc().discoverFunctionalDeps()
    df = exact_frame()
    for opt, bad in (("max_lhs_size", "0"), ("max_lhs_size", "5"), ("max_lhs_size", "x"), ("max_lhs_size", "-1"), ("max_error", "x"),
                     ("max_error", "-0.1"), ("max_error", "1.0"), ("max_lhs_group_ratio", "-1"), ("max_lhs_group_ratio", "y")):
        with pytest.raises(ValueError, match=opt):
            _discover(df, "fd_opts", **{opt: bad})
    with pytest.raises(ValueError, match="do not exist"):
        _discover(df, "fd_opts", row_id="nope")
    with pytest.raises(ValueError, match="do not exist"):
        _discover(df, "fd_opts", targets="a,nope")
    with pytest.raises(ValueError, match="row id"):
        _discover(df, "fd_opts", row_id="tid", targets="tid")


def test_frame_columns_and_dtypes():
    out = _discover(exact_frame(), "fd_dtypes", row_id="tid")
    assert list(out.columns) == COLUMNS and len(out) > 0
    assert [str(out[c].dtype) for c in COLUMNS] == ["object", "object", "int64", "int64", "int64", "float64", "object"]
    empty = _discover(exact_frame().iloc[:0], "fd_dtypes_empty", row_id="tid")
    assert list(empty.columns) == COLUMNS and len(empty) == 0
    assert [str(empty[c].dtype) for c in COLUMNS] == ["object", "object", "int64", "int64", "int64", "float64", "object"]


def test_report_gives_its_limits_without_a_table():
    """rgbm_table_fd_measures_report needs no device for the two limits; right-hand sides without a table are a bad argument."""
    import ctypes
    from repair import _native
    from repair.fd_codes import MAX_LHS
    from tests.helpers import csrc_constant
    assert _native.fd_measures_limits() == dict(lds_cells=csrc_constant("FD_LDS"), max_lhs=csrc_constant("FD_MAX_LHS"))
    assert MAX_LHS == csrc_constant("FD_MAX_LHS") and csrc_constant("FD_LDS") * 4 <= 64 * 1024
    out = np.zeros(4, np.int32)
    rc = _native.lib().rgbm_table_fd_measures_report(None, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_int32(1))
    assert rc == -1 and b"rgbm_table_fd_measures_report" in _native.lib().rgbm_last_error()


def test_every_guarded_node_id_of_the_gpu_file_is_collected():
    """tests/test_fd_gpu_guarded.py counts the passed tests against this list: a renamed test or parameter must not quietly shrink it."""
    import os
    import subprocess
    import sys
    from tests.test_fd_gpu import GUARDED
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])     # the child sees the packages this process sees
    out = subprocess.run([*python, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", *GUARDED], cwd=root,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode("utf-8", "replace")
    got = [line.strip() for line in out.splitlines() if line.startswith("tests/") and "::" in line]
    assert sorted(got) == sorted(GUARDED) and len(set(GUARDED)) == len(GUARDED) >= 20, out[-2000:]


def test_group_ratio_prunes_supersets_of_wide_left_hand_sides():
    from repair import fd_codes, fd_discovery
    df = _hand_frame()
    cols = [c for c in df.columns if c != "tid"]
    codes, n_codes = _codes_of(df, cols)
    measure = lambda lhs, rhs: fd_codes.fd_measures(codes, n_codes, lhs, rhs)  # noqa: E731
    wide, narrow = {}, {}
    a = fd_discovery.discover(measure, len(df), cols, cols, 2, "0.0", "1.0", stats=wide)
    b = fd_discovery.discover(measure, len(df), cols, cols, 2, "0.0", "0.1", stats=narrow)       # phone (30 groups of 240 rows) is above 0.1 * n
    assert narrow["calls"] < wide["calls"]
    assert all(r in a for r in b) and not any("phone" in r["lhs"] and len(r["lhs"]) > 1 for r in b)
