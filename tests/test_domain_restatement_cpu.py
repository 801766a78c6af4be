"""CPU: the product's numpy statement of the cell-domain analysis (repair.domain.HostBackend) against the plain restatement of
tests/domain_restatement.py on the generators of tests/domain_cases.py -- counts exactly, probabilities byte for byte -- and the generators
held to their purpose without a device: every case's route asserted on the restated grouping rule, every cell-domain property on the
restatement.  What `repair.domain` does not define (rows outside the table, codes beyond a dictionary) is checked on the restatement alone.
tests/test_gpu_domain_edges.py runs the same cases on the device."""
import numpy as np
import pytest

from tests import domain_cases as DC
from tests import domain_restatement as R

PAIR_CASES = DC.pair_cases()
DOMAIN_CASES = DC.domain_cases()


def _host(case):
    from repair import domain as D
    luts = {c: np.asarray(l, np.int32) for c, l in case["luts"].items()}
    return D.HostBackend(case["codes"], D.View(sorted(case["n_bins"]), case["n_bins"], luts, sorted(luts)))


def test_limits_come_from_the_library():
    L = DC.limits()
    assert L["lds_cells"] > 0 and L["lds_cells"] % 2 == 0 and 2 <= L["max_cols"] and L["block"] % 64 == 0 and L["max_k"] >= 1
    # the widest bin index of an LDS pair fits the uint16 tile
    assert L["lds_cells"] // 2 - 1 < 1 << 16


def test_restated_bins_send_everything_outside_to_the_null_slot():
    codes = np.asarray([[0, 4, 5, 10, -1, -7, 2 ** 31 - 1, 3], [0, 1, 2, 3, 3, 2, 1, 0]], np.int32)
    lut = np.asarray([0, 1, -1, 2, 9], np.int32)
    b = R.bins(codes, [5, 4], {0: lut}, {0: 3, 1: 2})
    assert b[0].tolist() == [0, 3, 3, 3, 3, 3, 3, 2] and b[1].tolist() == [0, 1, 2, 2, 2, 2, 1, 0]
    t, = R.pair_counts(codes, [5, 4], [(0, 1)], {0: lut}, {0: 3, 1: 2})
    assert t.shape == (4, 3) and t.sum() == 8 and t[3].tolist() == [0, 2, 4]


def test_restated_plan_on_a_hand_made_list():
    """Limits of 100 counters and 4 columns: closed by the counters, closed by the columns, a pair of its own above the limit."""
    nb = {0: 4, 1: 4, 2: 4, 3: 9, 4: 1, 5: 1, 6: 1, 7: 10}
    p = R.plan([(0, 1), (1, 2), (0, 2), (2, 0), (3, 7), (4, 5), (0, 1), (5, 6), (6, 4), (1, 2)], nb, 10000, 100, 4, 512)
    assert [q["group"] for q in p["pairs"]] == [0, 0, 0, 0, -1, 1, 1, 2, 2, 3]
    assert [(q["slot_x"], q["slot_y"]) for q in p["pairs"]] == [(0, 1), (1, 2), (0, 2), (2, 0), (-1, -1), (0, 1), (2, 3), (0, 1), (1, 2), (0, 1)]
    assert p["groups"] == 4 and p["max_group_cells"] == 100 and p["rows_per_wg"] == 5120 and p["grid_x"] == 2
    assert R.plan([(3, 7)], nb, 700, 100, 4, 512)["groups"] == 0


@pytest.mark.parametrize("name", sorted(PAIR_CASES))
def test_pair_case_holds_to_its_purpose_and_the_host_counts_equal_the_restatement(name):
    case = PAIR_CASES[name]()
    n = case["codes"].shape[1]
    case["route"](DC.restated_plan(case))
    want = R.pair_counts(case["codes"], case["n_codes"], case["pairs"], case["luts"], case["n_bins"])
    for (x, y), w in zip(case["pairs"], want):
        assert w.shape == (case["n_bins"][x] + 1, case["n_bins"][y] + 1) and int(w.sum()) == n
    if "corner" in case:                                     # the exact-fill pair reaches its last counter and its widest bin
        assert want[0][-1, -1] > 0 and want[0][case["corner"][0] - 1, 0] > 0
    if case["writes"] is not None:
        assert not np.array_equal(case["upload"], case["codes"]) and (case["codes"] >= case["n_codes"][:, None]).any() and (case["codes"] < -1).any()
    # a code >= n_codes without a LUT is a bin to repair.domain where n_bins allows it; the library counts it as NULL: not defined there
    if case["host_defined"]:
        got = [j.dense() for j in _host(case).pair_counts(case["pairs"])]
        for p, g, w in zip(case["pairs"], got, want):
            assert g.shape == w.shape and np.array_equal(g, w), p


@pytest.mark.parametrize("name", sorted(DOMAIN_CASES))
def test_domain_case_holds_to_its_purpose_and_the_host_domains_equal_the_restatement(name):
    from repair import domain as D
    case = DOMAIN_CASES[name]()
    tables, results = DC.restate_case(case)                  # asserts the case's properties
    n = case["codes"].shape[1]
    ptab = D.PairTable(case["pairs"], [D.Joint.from_dense(t) for t in tables])
    host = _host(case)
    compared = 0
    for call, want in zip(case["calls"], results):
        assert want[3].shape == (len(call["rows"]), case["n_bins"][case["target"]])
        if not case["host_defined"] or ((call["rows"] < 0) | (call["rows"] >= n)).any():
            continue
        corr = [case["pairs"][p][1] if case["pairs"][p][0] == case["target"] else case["pairs"][p][0] for p in call["corr"]]
        for want_probs in (True, False):
            hw, ht, hp, hprobs = host.cell_domains(case["target"], call["rows"], corr, ptab, call["min_cnt"], call["single_ok"], call["beta"],
                                                   call["row_count"], want_probs=want_probs)
            assert np.array_equal(hw, want[0]) and np.array_equal(ht, want[1]) and hp.tobytes() == want[2].tobytes()
            assert (hprobs is None) if not want_probs else (hprobs.tobytes() == want[3].tobytes())
        compared += 1
    assert compared > 0 or not case["host_defined"]


def test_the_single_row_tail_needs_more_rows_than_the_other_cases():
    """Why one row count exceeds the 20 000 rows of every other case: under the restated geometry no smaller table beyond one workgroup ends
    in a workgroup of a single row."""
    L = DC.limits()
    n = DC.single_row_tail_n()
    assert n == 15 * 16 * L["block"] + 1
    p = R.plan([(0, 1)], {0: 2, 1: 2}, n, L["lds_cells"], L["max_cols"], L["block"])
    assert p["grid_x"] == 16 and p["rows_per_wg"] == 16 * L["block"]
