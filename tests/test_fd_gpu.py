"""-m gpu: `rgbm_table_fd_measures` (csrc/rgbm_fd.hip) against its numpy statement `repair.fd_codes.fd_measures` -- integers throughout, so
equality, no tolerance -- on both of its routes, and `RepairMisc.discoverFunctionalDeps` through the HIP engine against its numpy path.
Every case first asserts, through `Table.fd_measures_report()`, that each right-hand side took the route the case is built for.  A table's
`n_codes` are only numbers: a small table with large declared dictionaries carries a large span, which is how the hash route is reached
with few rows.  tests/test_fd_gpu_guarded.py runs the smallest of these cases once more under guard zones and poison (GUARDED below).

(The file is not named test_gpu_*.py: tests/guarded_runs.py lists every file of that pattern in its families, and it stays as it is.)"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from tests import fd_restatement as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

FD_LDS = csrc_constant("FD_LDS")               # 32-bit counters of a dense joint table on the LDS route
MAX_LHS = csrc_constant("FD_MAX_LHS")
LDS, HASH = 0, 1
ROWS = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097)
SENTINEL = 77


def _routes(n_codes, lhs, rhs):
    span = 1
    for c in lhs:
        span *= max(int(n_codes[c]), 0) + 1
    return [LDS if span * (max(int(n_codes[y]), 0) + 1) <= FD_LDS else HASH for y in rhs]


def _check(codes, n_codes, lhs, rhs, routes=None, table=None):
    """The device against the statement; `routes`: LDS or HASH for all right-hand sides, or a list."""
    from repair import _native as N
    from repair.fd_codes import fd_measures
    table = table if table is not None else N.Table(codes, n_codes)
    got = table.fd_measures(lhs, rhs)
    rep = table.fd_measures_report()
    assert rep["routes"] == _routes(n_codes, lhs, rhs) and rep["lds_cells"] == FD_LDS and rep["max_lhs"] == MAX_LHS
    if routes is not None:
        assert rep["routes"] == (list(routes) if isinstance(routes, (list, tuple)) else [routes] * len(rhs)), rep
    R.assert_same(got, fd_measures(codes, n_codes, lhs, rhs), (lhs, rhs))
    return table, got


def _on_route(n, route, seed=0, shape="skewed", c=12):
    """tests/fd_restatement.mixed_table, with the dictionary of column 0 declared FD_LDS codes wide for the hash route (any left-hand side
    that holds column 0 then spans more than the LDS route takes)."""
    codes, n_codes = R.mixed_table(n, c=c, seed=seed, shape=shape)
    if route == HASH:
        n_codes[0] = max(n_codes[0], FD_LDS)
    return codes, n_codes


def test_constants_are_what_the_cases_below_assume():
    from repair import _native as N
    assert N.fd_measures_limits() == dict(lds_cells=FD_LDS, max_lhs=MAX_LHS) and MAX_LHS == 11 and FD_LDS >= 64


ROW_CASES = [(r, n) for r in (LDS, HASH) for n in ROWS]
ROW_IDS = ["%s-%d" % ("lds" if r == LDS else "hash", n) for r, n in ROW_CASES]


@pytest.mark.parametrize("route,n", ROW_CASES, ids=ROW_IDS)
def test_row_counts(route, n):
    codes, n_codes = _on_route(n, route, seed=n)
    table, _ = _check(codes, n_codes, [0, 1], [2, 3, 11], route)
    _check(codes, n_codes, [0], [5], route, table=table)


def _factors(v):
    """v = a * b with a the largest divisor up to sqrt(v); (1, v) for a prime: an empty left-hand side then spans 1."""
    a = max(d for d in range(1, int(v ** 0.5) + 1) if v % d == 0)
    return a, v // a


def _limit_table(a, b, n=3001, seed=0):
    """x with a - 1 codes (a = 1: no column on the left), y with b - 1 codes and a wider y2; row 0 holds the highest codes of both (the last
    counter of the joint table), row 1 NULLs."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-1, max(a - 1, 1), n)
    y = rng.integers(-1, b - 1, n) if b > 1 else np.full(n, -1)
    x[0], y[0], x[1], y[1] = a - 2, b - 2, -1, -1
    y2 = np.minimum(rng.geometric(0.3, n) - 1, 5)
    return np.stack([x, y, y2]).astype(np.int32), [max(a - 1, 1), b - 1, 6]


LIMIT_IDS = ["below", "at", "above"]


@pytest.mark.parametrize("delta", [-1, 0, 1], ids=LIMIT_IDS)
def test_lds_limit(delta):
    a, b = _factors(FD_LDS + delta)
    codes, n_codes = _limit_table(a, b, seed=delta + 1)
    lhs = [0] if a > 1 else []
    span = a if a > 1 else 1
    assert span * b == FD_LDS + delta
    _check(codes, n_codes, lhs, [1], LDS if delta <= 0 else HASH)


def test_lds_limit_with_two_columns_on_the_left_and_a_call_that_straddles_it():
    a, b = _factors(FD_LDS)
    a1, a2 = _factors(a)
    assert a1 > 1 and a1 * a2 * b == FD_LDS
    rng = np.random.default_rng(3)
    n = 2999
    codes = np.stack([rng.integers(-1, a1 - 1, n), rng.integers(-1, a2 - 1, n), rng.integers(-1, b - 1, n), rng.integers(-1, b, n),
                      rng.integers(-1, 2, n)]).astype(np.int32)
    codes[:3, 0] = (a1 - 2, a2 - 2, b - 2)
    n_codes = [a1 - 1, a2 - 1, b - 1, b, 2]
    _check(codes, n_codes, [0, 1], [2], LDS)
    _check(codes, n_codes, [0, 1], [3], HASH)                             # one more code on the right: one row of counters too many
    _check(codes, n_codes, [0, 1], [3, 2, 4], [HASH, LDS, LDS])           # both routes in one call


@pytest.mark.parametrize("shape", ["one", "singletons"])
def test_hash_route_one_group_and_all_singletons(shape):
    codes, n_codes = _on_route(3000, HASH, seed=5, shape=shape)
    _, got = _check(codes, n_codes, [0, 1], [10, 11, 5], HASH)
    assert int(got["groups"]) == (1 if shape == "one" else 3000)


@pytest.mark.parametrize("n", [2048, 2049])
def test_hash_route_either_side_of_a_capacity_step(n):
    codes, n_codes = _on_route(n, HASH, seed=n, shape="singletons")       # n keys: the table of 2 n slots doubles between the two
    _check(codes, n_codes, [0], [1, 2], HASH)
    _check(codes, n_codes, [0, 3], [1], HASH)


def test_hash_route_key_span_just_below_two_to_the_63():
    rng = np.random.default_rng(9)
    n = 1500
    top = (1 << 21) - 1
    codes = np.stack([rng.choice([0, 1, top - 1, top - 2, -1], n), rng.choice([0, top - 1, -1], n), rng.choice([0, 1, top - 2], n),
                      rng.integers(-1, 4, n)]).astype(np.int32)
    n_codes = [top, top, top - 1, 4]                                      # radices 2^21, 2^21, 2^21 - 1
    assert (top + 1) ** 2 * top < 1 << 63 <= (top + 1) ** 3
    _check(codes, n_codes, [0, 1, 2], [3], HASH)


@pytest.mark.parametrize("route", [LDS, HASH], ids=["lds", "hash"])
@pytest.mark.parametrize("n_lhs", [0, 1, 2, 3, 11])
def test_left_and_right_hand_side_counts(n_lhs, route):
    codes, n_codes = R.mixed_table(1237, c=13, seed=n_lhs, card=2 if route == LDS else 3)
    if route == HASH and n_lhs > 0:
        n_codes[0] = FD_LDS
    if route == HASH and n_lhs == 0:
        n_codes[11] = n_codes[12] = FD_LDS + 7                            # no left-hand side: the right-hand side alone is too wide
    if route == LDS and n_lhs == 11:                                      # eleven columns of one code and NULL: 2^11 keys
        n_codes[:11] = [1] * 11
        n_codes[11] = n_codes[12] = min(3, FD_LDS // 2048 - 1)
    lhs = list(range(n_lhs))
    rest = [j for j in range(13) if j not in lhs]
    table = None
    for rhs in ([12], [12, 11], rest):
        want = None if (route == HASH and n_lhs == 0 and rhs is rest) else route
        table, _ = _check(codes, n_codes, lhs, rhs, want, table=table)


@pytest.mark.parametrize("route", [LDS, HASH], ids=["lds", "hash"])
def test_ties_nulls_and_codes_outside_the_dictionary(route):
    codes = np.asarray([[0, 0, 0, 0, -1, 3, 9, -5], [0, 0, 1, 1, -1, 2, 7, -2]], np.int32)
    n_codes = [3, 2]
    if route == HASH:                                                     # the same codes, wider dictionaries: 3 and 2 are values now
        codes = np.where(codes == 3, FD_LDS, np.where(codes == 9, FD_LDS + 6, codes)).astype(np.int32)
        n_codes = [FD_LDS, 2]
    _, got = _check(codes, n_codes, [0], [1], route)
    R.assert_same(got, dict(groups=2, kept=[6], violating=[4], xy_groups=[3]))
    e = R.EXAMPLE
    _, got = _check(e["codes"], e["n_codes"], [0], [1], LDS)
    R.assert_same(got, e["want"])


@pytest.fixture(scope="module")
def larger():
    rng = np.random.default_rng(200003)
    n = 200003
    n_codes = [7, 40, 3000, 11, 5, 200]
    codes = np.stack([np.minimum(rng.geometric(8.0 / (d + 8), n) - 1, d - 1) for d in n_codes]).astype(np.int32)
    codes[3] = (codes[1] * 3 + codes[0]) % 11                             # (0, 1) -> 3, with dirt
    dirt = rng.random(n) < 0.003
    codes[3][dirt] = rng.integers(0, 11, int(dirt.sum()))
    for j in range(6):
        codes[j][rng.random(n) < 0.01] = -1
    from repair import _native as N
    return codes, n_codes, N.Table(codes, n_codes)


@pytest.mark.parametrize("lhs,rhs,route", [([0, 1], [3, 4], LDS), ([0], [1, 5, 4], LDS), ([2], [0, 1, 3, 4, 5], HASH), ([1, 5, 0], [2, 3, 4], HASH),
                                           ([1, 0], [3, 5, 2], [LDS, HASH, HASH])],
                         ids=["lds-2", "lds-1", "hash-1", "hash-3", "both"])
def test_larger_table(larger, lhs, rhs, route):
    codes, n_codes, table = larger
    _check(codes, n_codes, lhs, rhs, route, table=table)


def test_results_do_not_depend_on_the_run(larger):
    codes, n_codes, table = larger
    a = table.fd_measures([2, 0], [1, 3])
    b = table.fd_measures([2, 0], [1, 3])
    R.assert_same(a, b)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def test_refusals_leave_everything_as_it_was():
    from repair import _native as N
    ARG, PARAM = -1, -2
    top = (1 << 21) - 1
    codes, n_codes = R.mixed_table(300, c=13, seed=1)
    n_codes[10] = n_codes[11] = n_codes[12] = top                         # three columns that span 2^63 together
    table = N.Table(codes, n_codes)
    cells = table.detect_nulls([0, 4])
    assert len(cells[0]) > 0
    first = table.fd_measures([0], [1, 2])
    report = table.fd_measures_report()
    lib = N.lib()
    i32 = lambda v: np.asarray(v, np.int32)  # noqa: E731
    outs = [np.full(1, SENTINEL, np.int64)] + [np.full(4, SENTINEL, np.int64) for _ in range(3)]

    def call(lhs, n_lhs, rhs, n_rhs, t=table.h, o=outs):
        return lib.rgbm_table_fd_measures(t, _p(lhs, C.c_int32), C.c_int32(n_lhs), _p(rhs, C.c_int32), C.c_int32(n_rhs),
                                          *[_p(a, C.c_int64) for a in o])

    l1, r2 = i32([0]), i32([1, 2])
    refusals = [
        ("no table", lambda: call(l1, 1, r2, 2, t=None), ARG),
        ("no left-hand side array", lambda: call(None, 1, r2, 2), ARG),
        ("no right-hand side array", lambda: call(l1, 1, None, 2), ARG),
        *[("no output array %d" % k, (lambda k=k: call(l1, 1, r2, 2, o=[None if j == k else a for j, a in enumerate(outs)])), ARG) for k in range(4)],
        ("n_lhs < 0", lambda: call(l1, -1, r2, 2), ARG),
        ("n_lhs = 12", lambda: call(i32(range(12)), 12, i32([12]), 1), ARG),
        ("n_rhs = 0", lambda: call(l1, 1, r2, 0), ARG),
        ("n_rhs < 0", lambda: call(l1, 1, r2, -1), ARG),
        ("left column out of range", lambda: call(i32([13]), 1, r2, 2), ARG),
        ("left column negative", lambda: call(i32([-1]), 1, r2, 2), ARG),
        ("right column out of range", lambda: call(l1, 1, i32([1, 13]), 2), ARG),
        ("left column twice", lambda: call(i32([0, 3, 0]), 3, r2, 2), ARG),
        ("right column twice", lambda: call(l1, 1, i32([2, 2]), 2), ARG),
        ("right-hand side in X", lambda: call(i32([0, 2]), 2, r2, 2), ARG),
        ("span of 2^63", lambda: call(i32([10, 11, 12]), 3, r2, 2), PARAM),
    ]
    assert (top + 1) ** 3 == 1 << 63
    for what, fn, code in refusals:
        assert fn() == code, what
        assert b"rgbm_table_fd_measures" in lib.rgbm_last_error(), what
        assert all((a == SENTINEL).all() for a in outs), what
        assert table.fd_measures_report() == report, what
        again = table._fetch_cells(len(cells[0]), True)
        assert np.array_equal(again[0], cells[0]) and np.array_equal(again[1], cells[1]), what
    # the report refuses a count that is not the last call's, and needs a table for any
    out = np.zeros(8, np.int32)
    assert lib.rgbm_table_fd_measures_report(table.h, _p(out, C.c_int32), C.c_int32(3)) == ARG
    assert lib.rgbm_table_fd_measures_report(None, _p(out, C.c_int32), C.c_int32(1)) == ARG
    assert lib.rgbm_table_fd_measures_report(table.h, None, C.c_int32(2)) == ARG
    # after a successful call the cell list is intact too, and the call gives what it gave before
    R.assert_same(table.fd_measures([0], [1, 2]), first)
    _check(codes, n_codes, [0, 11], [1, 2, 3], HASH, table=table)
    again = table._fetch_cells(len(cells[0]), True)
    assert np.array_equal(again[0], cells[0]) and np.array_equal(again[1], cells[1])
    fresh = N.Table(codes, n_codes)
    assert fresh.fd_measures_report()["routes"] == []                     # before any call


def _discover(df, name, engine, **opts):
    import os
    from repair.api import Delphi
    from repair.misc import RepairMisc
    Delphi.register_table(name, df)
    m = RepairMisc().options(dict({"table_name": name}, **opts))
    m._engine_override = engine
    old = os.environ.get("REPAIR_RESIDENT")
    if engine is None:
        os.environ["REPAIR_RESIDENT"] = "0"
    try:
        return m.discoverFunctionalDeps()
    finally:
        if engine is None:
            if old is None:
                del os.environ["REPAIR_RESIDENT"]
            else:
                os.environ["REPAIR_RESIDENT"] = old


class _Counting:
    """The HIP engine, counting the calls that reach the device entry."""

    def __init__(self):
        from repair.engine import HipEngine
        self.engine, self.calls = HipEngine(0), 0

    def upload_dictionaries(self, indices, remaps):
        return self.engine.upload_dictionaries(indices, remaps)

    def fd_measures(self, table, lhs, rhs):
        self.calls += 1
        return self.engine.fd_measures(table, lhs, rhs)


@pytest.mark.parametrize("which", ["hospital", "hand"])
def test_discover_through_the_hip_engine_gives_the_frame_of_the_numpy_path(which):
    from tests import test_fd_discovery_cpu as T
    df = T._hospital() if which == "hospital" else T._hand_frame()
    opts = dict(row_id="tid", max_lhs_size="2", max_error="0.01")
    engine = _Counting()
    got = _discover(df, "fd_gpu_" + which, engine, **opts)
    want = _discover(df, "fd_gpu_" + which, None, **opts)
    assert engine.calls > 1 and len(want) > 0
    pd.testing.assert_frame_equal(got, want, check_exact=True)


# what tests/test_fd_gpu_guarded.py runs once more under guard zones and poison: the row edges up to 257 on both routes, the limit edges, the refusals
GUARDED = (["tests/test_fd_gpu.py::test_row_counts[%s]" % i for i, (_, n) in zip(ROW_IDS, ROW_CASES) if n <= 257]
           + ["tests/test_fd_gpu.py::test_lds_limit[%s]" % i for i in LIMIT_IDS]
           + ["tests/test_fd_gpu.py::test_lds_limit_with_two_columns_on_the_left_and_a_call_that_straddles_it",
              "tests/test_fd_gpu.py::test_refusals_leave_everything_as_it_was"])
