"""CPU: the probability modes at their edges, on the oracle -- the generator of tests/prob_edges.py (K = 63 ... 303 classes) gives
ties inside one 64-class lane, exact zeros, all-zero cells and moved top-1s, so a device test on it cannot pass vacuously; the
renormalising sum is the reference's left-to-right sum on every interpreter; the renormalised probabilities sum to 1 within the
rounding of that arithmetic; the string packing at its edges and a numpy DP as a second opinion on repair.costs.edit_distance; the
hospital targets with more than 64 classes on both paths."""
import math

import numpy as np
import pandas as pd
import pytest

from repair.costs import Levenshtein, edit_distance
from repair.model import RepairModel
from tests import prob_edges as E
from tests.test_prob_modes_cpu import CostOracleEngine, _both_paths, _hospital_model, _select, _seq_sum, _sorted, _weighted_pmf, _weighted_probs

# a probability vector whose left-to-right sum is 1 - 2^-52 and whose exactly rounded sum (math.fsum; `sum()` from Python 3.12 on
# compensates too) is 1.0
SEQ_VECTOR = [float.fromhex(h) for h in (
    "0x1.0c26ac072df8fp-9", "0x1.6621a1ca266dap-2", "0x1.d2816f6d65e7ep-9", "0x1.2430106c6d5d7p-4", "0x1.e07da694b4503p-4",
    "0x1.5554c0ed8bb45p-6", "0x1.16993f88996b6p-5", "0x1.93ce8455be7f3p-4", "0x1.a990b111e51d9p-4", "0x1.3d0d4274a038fp-7",
    "0x1.369d93dbb78cap-4", "0x1.cf963f690129cp-4")]
SEQ_NORM = float.fromhex("0x1.ffffffffffffep-1")


@pytest.fixture(scope="module")
def oracle_cases():
    out = {}
    for K in E.KS:
        codes, cards = E.make_edge_table(K)
        out[K] = E.null_cell_probabilities(E.train_oracle(codes, cards, K), codes)
    return out


@pytest.mark.parametrize("K", E.KS)
def test_generator_conditions_hold_on_the_oracle(oracle_cases, K):
    null_rows, proba = oracle_cases[K]
    assert len(null_rows) >= 300 and proba.shape == (len(null_rows), K)
    assert len(E.absent_classes(K)) >= 3
    E.check_probabilities(K, proba)
    cur = E.cur_codes(K, len(null_rows))
    assert {0, K - 1, -1, K, K + 5} <= set(cur.tolist()) and (K <= 64 or {63, 64} <= set(cur.tolist()))
    plain_top1 = _select(proba, 1, -1.0, None, None, None)[0][:, 0]
    for name, (cost, special) in E.cost_matrices(K).items():
        crow = E.cost_rows(len(null_rows), len(cost) - 1)
        assert set(crow.tolist()) == set(range(-1, len(cost) - 1)) and set(special) == set(E.SPECIAL_ROWS)
        for w in E.WEIGHTS:                                     # the header excludes a denominator of exactly 0
            den = 1.0 + w * cost[:-1]
            assert not (den == 0.0).any()
        for renorm in (False, True):
            for w in E.WEIGHTS:
                p = _weighted_probs(proba, crow, cost, w, renorm)
                assert np.isfinite(p).all()                     # nothing Python could not order, no overflow
                E.check_weighted(K, p, crow, special, plain_top1)
                if w == 0.7:
                    assert (p[crow == special["negative"]] < 0.0).any()
    # a stable top-k: with -1.0 the tied zero-probability classes are selected, in class order
    if K >= 128:
        cls, pr, _, _ = _select(proba, K, -1.0, None, None, None)
        i = int(np.argmax((proba == 0.0).sum(axis=1)))
        z = cls[i][pr[i] == 0.0]
        assert len(z) >= 2 and (np.diff(z) > 0).all()


def test_renormalised_probabilities_sum_to_one_within_the_rounding_of_the_contract(oracle_cases):
    """norm is a left-to-right sum (K - 1 roundings, each at most 2^-53 relative to a partial sum <= norm) and every p_c / norm rounds
    once more: |sum(p) - 1| <= K 2^-53 to first order, 2 K 2^-53 with room for the higher orders.  Cells with norm > 0 and no
    negative probability (those cancel), on the K = 303 reference cells, plain and with either cost matrix."""
    K = 303
    _, proba = oracle_cases[K]
    bound = 2 * K * 2.0 ** -53
    checked = 0
    settings = [(None, None, 0.0)] + [(E.cost_rows(len(proba), len(c) - 1), c, w) for c, _ in E.cost_matrices(K).values() for w in E.WEIGHTS]
    for crow, cost, w in settings:
        raw = _weighted_probs(proba, crow, cost, w, False)
        p = _weighted_probs(proba, crow, cost, w, True)
        for i in range(len(p)):
            if (raw[i] >= 0.0).all() and _seq_sum(raw[i].tolist()) > 0.0:
                assert abs(math.fsum(p[i].tolist()) - 1.0) <= bound, (i, w)
                checked += 1
    assert checked >= 3 * len(proba)


def test_the_renormalising_sum_is_the_left_to_right_sum():
    """The reference sums with Spark's `aggregate(probs, 0.0, (acc, x) -> acc + x)`.  On SEQ_VECTOR that sum and the exactly rounded
    one differ in the last bit, and so do the quotients: a compensated sum (math.fsum, Python 3.12's `sum`) fails here on any interpreter."""
    assert math.fsum(SEQ_VECTOR) == 1.0 and _seq_sum(SEQ_VECTOR) == SEQ_NORM != 1.0
    want = [x / SEQ_NORM for x in SEQ_VECTOR]
    assert sum(a != b for a, b in zip(want, SEQ_VECTOR)) >= 6            # dividing by fsum's 1.0 would leave the vector as it is
    # the tests' restatement
    p = _weighted_probs(np.array([SEQ_VECTOR]), None, None, 0.0, True)
    assert p[0].tolist() == want
    cls, pr, cp, _ = _weighted_pmf(np.array([SEQ_VECTOR]), 12, 0.0, np.array([1]), None, None, 0.0, True)
    assert cp[0] == want[1] and pr[0].tolist() == sorted(want, reverse=True)
    # the value-space path: RepairModel._compute_repair_pmf renormalises once a cost function is set
    classes = ["v%02d" % k for k in range(12)]
    m = RepairModel().setRowId("tid").setUpdateCostFunction(Levenshtein())
    cells = pd.DataFrame({"tid": [0], "attribute": ["a"], "current_value": [None]})
    rows = pd.DataFrame({"tid": [0], "a": [None]})
    out = m._compute_repair_pmf({"a": (classes, [np.array(SEQ_VECTOR)], None)}, rows, rows, cells, [])
    got = {d["class"]: d["prob"] for d in out["pmf"].iloc[0]}
    assert got == dict(zip(classes, want))
    # with a current value the costs weigh first; the sum of the weighted values is again the sequential one
    cells = pd.DataFrame({"tid": [0], "attribute": ["a"], "current_value": ["v03"]})
    out = m._compute_repair_pmf({"a": (classes, [np.array(SEQ_VECTOR)], None)}, rows, rows, cells, [])
    weight = float(m._get_option_value(*m._opt_cost_weight))
    w = [x * (1.0 / (1.0 + weight * edit_distance("v03", c))) for x, c in zip(SEQ_VECTOR, classes)]
    norm = _seq_sum(w)
    got = {d["class"]: d["prob"] for d in out["pmf"].iloc[0]}
    assert got == {c: x / norm for c, x in zip(classes, w)} and out["current_value"].iloc[0]["prob"] == w[3] / norm


def test_pack_code_points_at_the_edges():
    """Offsets of pools whose first or last string is empty; code points 0, 0x10FFFF and lone surrogates survive the packing."""
    from repair._native import pack_code_points
    for strs in (["", "ab", ""], ["", ""], [""], ["", "\x00", "\U0010FFFF\ud800", "\udfff", ""], ["x" * 65, ""], ["", "x" * 65]):
        cp, off = pack_code_points(strs)
        assert cp.dtype == np.int32 and off.dtype == np.int64 and off[0] == 0 and len(off) == len(strs) + 1 and off[-1] == len(cp)
        assert (np.diff(off) == [len(s) for s in strs]).all()
        for i, s in enumerate(strs):
            assert cp[off[i]:off[i + 1]].tolist() == [ord(ch) for ch in s]
    cp, _ = pack_code_points(["\x00\U0010FFFF" + chr(0xD800) + chr(0xDFFF)])
    assert cp.tolist() == [0, 0x10FFFF, 0xD800, 0xDFFF]


def test_the_numpy_dp_agrees_with_the_product_distance():
    """The second opinion of the device tests is itself held to repair.costs.edit_distance and to distances known by construction."""
    rng = np.random.default_rng(17)
    for _ in range(200):
        a = "".join(rng.choice(list("abc\x00\ud800"), size=int(rng.integers(0, 40))))
        b = "".join(rng.choice(list("abc\x00\ud800"), size=int(rng.integers(0, 40))))
        assert E.levenshtein_dp(a, b) == edit_distance(a, b) == edit_distance(b, a)
    s = "".join(rng.choice(list("ab"), size=300))
    assert E.levenshtein_dp(s, s) == 0 and E.levenshtein_dp(s[:100], s) == 200 and E.levenshtein_dp("", s) == 300 and E.levenshtein_dp(s, "") == 300
    assert E.levenshtein_dp("kitten", "sitting") == 3


def test_hospital_wide_targets_equal_the_value_space_path(oracle_backend):
    """`Sample` (303 classes) and `Score` (55): the hospital targets beyond one 64-class chunk, which the six targets of
    test_hospital_frames_equal_the_value_space_path (44 classes at most) do not reach."""
    eng = CostOracleEngine()
    make = lambda: _hospital_model(Levenshtein(), delta=60).setTargets(["Score", "Sample"]).option("model.lgb.n_estimators", "12")  # noqa: E731
    a, b, fast = _both_paths(make, eng, compute_repair_score=True)
    info = fast._last_resident_info
    assert info is not None, "the run did not take the resident path"
    wide = [info["columns"][t] for t, blob in info["models"].items() if eng.load_model(blob).info()["num_class"] > 64]
    assert wide and int(b["attribute"].isin(wide).sum()) >= 20
    pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)
