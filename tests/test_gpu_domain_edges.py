"""-m gpu: the kernels of csrc/rgbm_domain.hip (rgbm_table_pair_counts, rgbm_table_cell_domains) at their edges, against the plain restatement
of tests/domain_restatement.py on the cases of tests/domain_cases.py -- counts exactly, flags and top values exactly, probabilities byte for
byte; no comparison has a tolerance.  Every case first asserts, through `Table.pair_counts_report()`, that the library planned what the
restated grouping rule plans and took the route the case is built for; then it compares.  Also here: a second count call on one table
followed by the domains, every refusal with its error code and a valid call after it, and the length check of `single_ok`.
tests/test_domain_restatement_cpu.py holds the product's numpy and the generators to the same restatement without a device.

Not covered by any test: the 2^30 rows a workgroup sees at most, which keep a 32-bit LDS counter from wrapping -- no small table reaches it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import domain_cases as DC
from tests import domain_restatement as R

pytestmark = pytest.mark.gpu

PAIR_CASES = DC.pair_cases()
DOMAIN_CASES = DC.domain_cases()
ERR_ARG, ERR_PARAM = -1, -2                                  # include/rgbm.h


@functools.lru_cache(maxsize=None)
def _restated(name):
    """(case, dense tables, results of the cell-domain calls or None): computed once per case, shared, never written."""
    if name in PAIR_CASES:
        case = PAIR_CASES[name]()
        return case, R.pair_counts(case["codes"], case["n_codes"], case["pairs"], case["luts"], case["n_bins"]), None
    case = DOMAIN_CASES[name]()
    tables, results = DC.restate_case(case)
    return case, tables, results


def _upload(case):
    from repair import _native as N
    tab = N.Table(case["upload"], case["n_codes"])
    if case["writes"] is not None:
        tab.write_cells(*case["writes"])
        for c in range(case["codes"].shape[0]):
            assert np.array_equal(tab.read_column(c), case["codes"][c])
    return tab


def _count_and_check(tab, case, tables):
    """The count call, the route through the report, then the tables."""
    n = case["codes"].shape[1]
    got = tab.pair_counts(case["pairs"], luts=case["luts"] or None, n_bins=case["n_bins"])
    report = tab.pair_counts_report()
    assert report == DC.restated_plan(case), (report, DC.restated_plan(case))
    case["route"](report)
    assert len(got) == len(tables)
    for p, g, w in zip(case["pairs"], got, tables):
        assert g.shape == w.shape and np.array_equal(g, w), p
        assert int(g.sum()) == n, p
    return got


def _with(n_bins, col, bins):
    out = dict(n_bins)
    out[col] = bins
    return out


def _same(got, want, with_probs):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].dtype == np.uint8 and got[1].dtype == np.int32
    assert got[2].tobytes() == want[2].tobytes()
    if with_probs:
        assert got[3].shape == want[3].shape and got[3].tobytes() == want[3].tobytes()
    else:
        assert got[3] is None


def _domains(tab, case, call, want_probs):
    return tab.cell_domains(case["target"], call["rows"], call["corr"], call["min_cnt"], call["single_ok"], call["beta"], call["row_count"],
                            want_probs=want_probs)


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pair_counts_edge(name):
    case, tables, _ = _restated(name)
    _count_and_check(_upload(case), case, tables)


@pytest.mark.parametrize("name", sorted(DOMAIN_CASES))
def test_cell_domains_edge(name):
    case, tables, results = _restated(name)
    tab = _upload(case)
    _count_and_check(tab, case, tables)
    for call, want in zip(case["calls"], results):
        _same(_domains(tab, case, call, True), want, True)
        _same(_domains(tab, case, call, False), want, False)


def test_domains_follow_the_second_count_call():
    """Two count calls on one table -- other pairs, other order, other orientations, other bins of one column -- then the domains with
    indices into the second list: offsets, orientations and bins are the second call's."""
    case, tables, _ = _restated("widths_and_k_12")
    K = DC.limits()["max_k"]
    tab = _upload(case)
    first = dict(case, pairs=case["pairs"][:3] + [(1, 2)], luts={}, n_bins=_with(case["n_bins"], K, int(case["n_codes"][K])))
    _count_and_check(tab, first, R.pair_counts(first["codes"], first["n_codes"], first["pairs"], first["luts"], first["n_bins"]))
    second = dict(case, pairs=[(y, x) for x, y in reversed(case["pairs"])])
    t2 = [np.ascontiguousarray(t.T) for t in reversed(tables)]
    _count_and_check(tab, second, t2)
    n, d_a = case["codes"].shape[1], case["n_bins"][0]
    rows = np.arange(0, n, 7)
    for corr, mins in ((list(range(K)), [j % 3 for j in range(K)]), ([0], [0]), ([K - 1, 2, 5], [2, 0, 1])):
        call = dict(rows=rows, corr=corr, min_cnt=mins, single_ok=np.ones(d_a, bool), beta=0.3, row_count=n)
        want = DC.restate_call(second, call, t2)
        assert (want[1] >= 0).any() and (want[1] < 0).any()
        _same(_domains(tab, second, call, True), want, True)
    # the same indices on the first order read other attributes: the comparison above could not pass on the first call's state
    assert DC.restate_call(case, dict(call, corr=[0], min_cnt=[0]), tables)[3].tobytes() != DC.restate_call(second, dict(call, corr=[0], min_cnt=[0]), t2)[3].tobytes()


def _refused(code, f, *a, **kw):
    from repair import _native as N
    with pytest.raises(N.RepairGbmError) as e:
        f(*a, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_leave_the_table_as_it_was():
    from repair import _native as N
    case, tables, results = _restated("cell_list_edges")
    n, d_a = case["codes"].shape[1], case["n_bins"][0]
    call, want = case["calls"][4], results[4]
    ok = np.ones(d_a, bool)
    tab = _upload(case)
    assert tab.pair_counts_report()["pairs"] == [] and tab.pair_counts_report()["groups"] == 0
    _refused(ERR_PARAM, tab.cell_domains, 0, call["rows"], [0], [0], ok, 0.2, n)                      # before any count call
    pairs = case["pairs"] + [(1, 2)]
    lut = np.arange(int(case["n_codes"][2]), dtype=np.int32) // 2
    counted = dict(case, pairs=pairs, luts={2: lut}, n_bins=_with(case["n_bins"], 2, 7))
    t3 = R.pair_counts(counted["codes"], counted["n_codes"], pairs, counted["luts"], counted["n_bins"])
    want = DC.restate_call(counted, call, t3)
    assert (want[1] >= 0).any()

    def still_right():
        assert tab.pair_counts_report() == DC.restated_plan(counted)
        _same(_domains(tab, counted, call, True), want, True)

    _count_and_check(tab, counted, t3)
    still_right()
    K = DC.limits()["max_k"]
    for bad in (lambda: tab.cell_domains(0, call["rows"], [0] * (K + 1), [0] * (K + 1), ok, 0.2, n),    # k = 9
                lambda: tab.cell_domains(0, call["rows"], [0, 3], [0, 0], ok, 0.2, n),                  # a pair index out of range
                lambda: tab.cell_domains(0, call["rows"], [-1], [0], ok, 0.2, n),
                lambda: tab.cell_domains(0, call["rows"], [0, 2], [0, 0], ok, 0.2, n),                  # a pair that does not hold the target
                lambda: tab.cell_domains(2, call["rows"], [1], [0], np.ones(7, bool), 0.2, n),          # a target counted through a LUT
                lambda: tab.pair_counts([(0, 1), (1, 1)]),                                              # a pair (x, x)
                lambda: tab.pair_counts([(0, 1)], n_bins={1: 0}),                                       # n_bins of 0
                lambda: tab.pair_counts([(0, 1)], n_bins={0: 4096, 1: 4095}),                           # one pair above 2^24 cells
                lambda: tab.pair_counts([(0, 1), (1, 2), (2, 0)], n_bins={0: 4095, 1: 4095, 2: 4095}),  # 3 * 2^24 cells in the call
                lambda: tab.write_cells([0], [1], [int(case["n_codes"][1])])):                          # (codes beyond a dictionary are not written)
        _refused(ERR_PARAM, bad)
        still_right()
    _refused(ERR_ARG, tab.cell_domains, 0, call["rows"], [0], [0], ok, 0.2, 0)                         # row_count 0
    _refused(ERR_ARG, tab.cell_domains, 3, call["rows"], [0], [0], ok, 0.2, n)                         # the target outside the table
    still_right()
    # a column index outside the table: the wrapper sizes its result by the columns, so the entry itself is called
    nb, out = np.asarray(case["n_codes"], np.int32), np.zeros(64, np.int64)
    for cols in ([0, 3], [-1, 0]):
        pc = np.asarray(cols, np.int32)
        rc = N.lib().rgbm_table_pair_counts(tab.h, pc.ctypes.data_as(C.POINTER(C.c_int32)), C.c_int32(1), None, nb.ctypes.data_as(C.POINTER(C.c_int32)),
                                            out.ctypes.data_as(C.POINTER(C.c_int64)))
        assert rc == ERR_PARAM and not out.any()
    still_right()
    # the report of another call's pair count is refused; a valid count call afterwards is right
    head = np.zeros(6, np.int64)
    assert N.lib().rgbm_table_pair_counts_report(tab.h, head.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 C.c_int32(len(pairs) + 1)) == ERR_ARG
    _count_and_check(tab, case, tables)
    _same(_domains(tab, case, call, True), results[4], True)


def test_single_ok_must_hold_one_entry_per_bin_of_the_target():
    """The entry uploads n_bins[target] bytes of `single_ok` whatever its length: the wrapper refuses any other length."""
    case, tables, results = _restated("narrow_target_bins")             # 9 codes, 6 bins
    tab = _upload(case)
    _count_and_check(tab, case, tables)
    call = case["calls"][0]
    for bad in (1, 5, 7, 9):
        with pytest.raises(ValueError, match="single_ok"):
            tab.cell_domains(0, call["rows"], call["corr"], call["min_cnt"], np.ones(bad, bool), call["beta"], call["row_count"])
    _same(_domains(tab, case, call, True), results[0], True)
