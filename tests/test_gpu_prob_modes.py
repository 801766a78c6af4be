"""-m gpu: the probability modes on the device -- rgbm_edit_distance against repair.costs.edit_distance, rgbm_table_repair_pmf_weighted
against a per-cell restatement of `_compute_repair_pmf`'s loop on the same model's probabilities (bit for bit), and `run()` with
`repair.pmf.resident` against the value-space path on the HIP estimators (exact frames)."""
import os
import time

import numpy as np
import pandas as pd
import pytest

from repair.costs import Levenshtein, UserDefinedUpdateCostFunction, edit_distance
from tests.test_prob_modes_cpu import MODES, _error_cells, _hospital_model, _model, _sorted, _synthetic_frame, _weighted_pmf

pytestmark = pytest.mark.gpu


def _rand_strings(rng, n, lengths, alphabet):
    return ["".join(rng.choice(alphabet, size=int(rng.choice(lengths)))) for _ in range(n)]


def test_edit_distance_equals_the_python_distance():
    from repair import _native as N
    rng = np.random.default_rng(7)
    ascii_ = list("abcde")
    wide = list("日本語中文한국😀😃🎉é") + ["\U0001F600", "é"]
    lengths = [0, 1, 2, 5, 63, 64, 65, 130, 300]
    for alphabet in (ascii_, wide, ascii_ + wide):
        a = _rand_strings(rng, 40, lengths, alphabet) + ["", "a", "😀"]
        b = _rand_strings(rng, 30, lengths, alphabet) + ["", "ab"]
        got = N.edit_distance(a, b)
        want = np.array([[edit_distance(x, y) for y in b] for x in a], np.int32)
        assert got.shape == (len(a), len(b)) and np.array_equal(got, want)
    # near-identical long strings (small distances across the 64-code-point boundary) and empty pools
    base = "".join(rng.choice(ascii_, size=200))
    a = [base[:k] for k in (63, 64, 65, 199, 200)] + [base[:100] + "x" + base[101:]]
    got = N.edit_distance(a, a)
    assert np.array_equal(got, np.array([[edit_distance(x, y) for y in a] for x in a], np.int32))
    assert N.edit_distance([], ["a"]).shape == (0, 1) and N.edit_distance(["a"], []).shape == (1, 0)


def _table_and_model(seed=3, n=6000):
    from repair import _native as N
    from repair.engine import balanced_class_weight
    from tests.synth import make_table
    dirty, _, cards = make_table(n, 6, seed=seed, null_ratio=0.05)
    tab = N.Table(dirty, cards, device_id=0)
    t = int(np.argmax(cards))
    feats = [c for c in range(6) if c != t]
    Kt = int(cards[t])
    m = tab.train(t, feats, class_weight=balanced_class_weight(np.bincount(dirty[t][dirty[t] >= 0], minlength=Kt)),
                  objective=0 if Kt == 2 else 1, num_class=max(Kt, 2), n_estimators=10, learning_rate=0.2)
    return tab, m, t, feats, Kt


def test_weighted_pmf_equals_the_python_loop():
    tab, m, t, feats, K = _table_and_model()
    # the model's probabilities of every NULL cell: the plain pmf with every class kept
    rows, cls, pr = tab.repair_pmf(m, t, feats, top_k=K, threshold=-1.0)
    proba = np.zeros((len(rows), K))
    for i in range(len(rows)):
        proba[i, cls[i]] = pr[i]
    n = len(rows)
    rng = np.random.default_rng(11)
    R = 9
    cost = rng.integers(0, 12, (R + 1, K)).astype(np.float64)
    cost[rng.random((R + 1, K)) < 0.2] = np.nan                     # None costs
    cost[R] = np.where(rng.random(K) < 0.5, 0.0, np.nan)           # the self row
    cost_rows = rng.integers(-1, R, n).astype(np.int32)           # -1: leave the cell alone
    cur = rng.integers(-1, K, n).astype(np.int32)                 # -1: the current value is not a class
    for top_k, thres in ((3, 0.0), (K, 0.0), (K + 4, 0.05), (5, 0.2)):
        for renorm in (False, True):
            for weight in (0.1, 0.7):
                _, gc, gp, gcp, gtc = tab.repair_pmf_weighted(m, t, feats, top_k=top_k, threshold=thres, cur_codes=cur, cost_rows=cost_rows,
                                                              cost=cost, weight=weight, renormalise=renorm)
                wc, wp, wcp, wtc = _weighted_pmf(proba, top_k, thres, cur, cost_rows, cost, weight, renorm)
                assert np.array_equal(gc, wc) and gp.tobytes() == wp.tobytes() and gcp.tobytes() == wcp.tobytes()
                assert np.array_equal(np.isnan(gtc), np.isnan(wtc)) and np.array_equal(gtc[~np.isnan(gtc)], wtc[~np.isnan(wtc)])
    # no costs, no renormalisation: rgbm_table_repair_pmf bit for bit
    for top_k, thres in ((3, 0.0), (K + 2, 0.1)):
        r0, c0, p0, cp0 = tab.repair_pmf(m, t, feats, top_k=top_k, threshold=thres, cur_codes=cur)
        r1, c1, p1, cp1, tc1 = tab.repair_pmf_weighted(m, t, feats, top_k=top_k, threshold=thres, cur_codes=cur)
        assert np.array_equal(r0, r1) and np.array_equal(c0, c1) and p0.tobytes() == p1.tobytes() and cp0.tobytes() == cp1.tobytes()
        assert np.isnan(tc1).all()


def _both_paths_hip(make, **flags):
    slow = make()
    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        a = slow.run(**flags)
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    fast = make().option("repair.pmf.resident", "true")
    b = fast.run(**flags)
    assert fast._last_resident_info is not None, "the run did not take the resident path"
    return a, b


def _equal(a, b, repair_data=False):
    assert list(a.columns) == list(b.columns) and len(a) == len(b) > 0
    if repair_data:
        pd.testing.assert_frame_equal(a.sort_values("tid").reset_index(drop=True), b.sort_values("tid").reset_index(drop=True), check_exact=True)
    else:
        pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)


COSTS = {"none": lambda: None, "lev": Levenshtein, "lev_one": lambda: Levenshtein(targets=["c2"]),
         "user": lambda: UserDefinedUpdateCostFunction(lambda x, y: float(abs(len(x) - len(y)) + (x[-1] != y[-1])))}


@pytest.mark.parametrize("cf", list(COSTS))
def test_run_synthetic_frames_equal_the_value_space_path(cf):
    df = _synthetic_frame(20000, 6, seed=11)
    ec = _error_cells(df, seed=12, ratio=0.01)
    for flags in MODES:
        ml = "compute_repair_score" in flags or "maximal_likelihood_repair" in flags
        if ml and cf not in ("lev", "user"):
            continue
        # the Null detector's cells (no current value), and given cells with current values for the Levenshtein score
        for cells in ((None, ec) if cf == "lev" and "compute_repair_score" in flags else (None,)):
            a, b = _both_paths_hip(lambda: _model(df, cf=COSTS[cf](), delta=200, cells=cells), **flags)
            _equal(a, b, flags.get("repair_data", False))


@pytest.mark.parametrize("flags", [dict(compute_repair_score=True), dict(maximal_likelihood_repair=True),
                                   dict(maximal_likelihood_repair=True, repair_data=True)])
def test_run_hospital_equals_the_value_space_path(flags):
    a, b = _both_paths_hip(lambda: _hospital_model(Levenshtein(), delta=60), **flags)
    _equal(a, b, flags.get("repair_data", False))


@pytest.mark.parametrize("flags", MODES[:2])
def test_run_boston_continuous_targets_equal_the_value_space_path(flags):
    import tests.test_quality as Q
    df = Q._boston_frame()[0]
    a, b = _both_paths_hip(lambda: _model(df, cf=Levenshtein(), **{"model.lgb.n_estimators": "20"}), **flags)
    _equal(a, b)


def test_run_score_on_a_million_rows():
    """compute_repair_score on 1M rows through the resident path (device and host-shaping times printed); the value-space path
    only on a 50k-row slice, for the frame."""
    n = 1_000_000
    df = _synthetic_frame(n, 8, seed=13, null_ratio=0.01)
    ec = _error_cells(df, seed=14, ratio=0.005)
    m = _model(df, cf=Levenshtein(), delta=1000, cells=ec, **{"model.max_training_row_num": "100000", "model.lgb.n_estimators": "6"})
    m = m.option("repair.pmf.resident", "true")
    t0 = time.perf_counter()
    out = m.run(compute_repair_score=True)
    wall = time.perf_counter() - t0
    info = m._last_resident_info
    assert info is not None and 0 < len(out) <= len(ec)
    tm = info["times"]
    print("1M rows, %d error cells, run(compute_repair_score=True): %.2fs wall, resident pipeline %.2fs (train %.2fs, infer %.2fs), "
          "host shaping %.2fs" % (len(ec), wall, tm.get("pipeline_wall", 0.0), tm.get("train", 0.0), tm.get("infer", 0.0), tm.get("host_shape", 0.0)))
    small = df.iloc[:50000].reset_index(drop=True)
    sec = ec[ec["tid"] < 50000].reset_index(drop=True)
    t0 = time.perf_counter()
    a, b = _both_paths_hip(lambda: _model(small, cf=Levenshtein(), delta=100, cells=sec), compute_repair_score=True)
    print("50k-row slice, both paths: %.2fs" % (time.perf_counter() - t0))
    _equal(a, b)
