"""CPU: the probability modes of `RepairModel.run()` (compute_repair_candidate_prob / compute_repair_prob / compute_repair_score /
maximal_likelihood_repair) on the resident pipeline behind the option `repair.pmf.resident`.

The job logic runs on a CPU engine (the oracle engine of tests/helpers plus a numpy restatement of the two new library entries,
rgbm_table_repair_pmf_weighted and rgbm_edit_distance) and the value-space path on the oracle estimator backend: both sides share
the oracle's arithmetic, so the frames must be equal cell for cell."""
import math
import os

import numpy as np
import pandas as pd
import pytest

from repair.costs import Levenshtein, UserDefinedUpdateCostFunction, edit_distance
from repair.errors import NullErrorDetector
from repair.model import RepairModel
from tests.helpers import OracleEngine, frame, load_golden
from tests.synth import make_table


def _seq_sum(xs):
    """The reference's `aggregate(probs, 0.0, (acc, x) -> acc + x)`: a plain left-to-right double sum.  Not `sum()`, which is a
    compensated sum from Python 3.12 on."""
    acc = 0.0
    for x in xs:
        acc = acc + x
    return acc


def _weighted_probs(proba, cost_rows, cost, weight, renormalise):
    """Per cell, the re-weighting and renormalisation of RepairModel._compute_repair_pmf on class indices: [m][K] float64."""
    out = np.empty(np.shape(proba), np.float64)
    for i in range(len(out)):
        p = [float(x) for x in proba[i]]
        row = int(cost_rows[i]) if cost is not None and cost_rows is not None else -1
        if row >= 0:
            p = [x * (1.0 / (1.0 + weight * c)) if not math.isnan(c) else x for x, c in zip(p, cost[row])]
        if renormalise:
            norm = _seq_sum(p)
            p = [x / norm for x in p] if norm > 0 else p
        out[i] = p
    return out


def _select(p, top_k, threshold, cur_codes, cost_rows, cost):
    """The stable top-k, the current value's probability and the top-1's cost of final probabilities `p` [m][K]."""
    m, K = p.shape
    cls = np.full((m, top_k), -1, np.int32)
    pr = np.zeros((m, top_k), np.float64)
    cp = np.zeros(m, np.float64)
    tc = np.full(m, np.nan, np.float64)
    for i in range(m):
        q = p[i].tolist()
        row = int(cost_rows[i]) if cost is not None and cost_rows is not None else -1
        cc = int(cur_codes[i]) if cur_codes is not None else -1
        cp[i] = q[cc] if 0 <= cc < K else 0.0
        order = [j for j in sorted(range(K), key=lambda j: -q[j]) if q[j] > threshold][:top_k]
        for k, j in enumerate(order):
            cls[i, k], pr[i, k] = j, q[j]
        if cost is not None and order:
            tc[i] = cost[row if row >= 0 else len(cost) - 1][order[0]]
    return cls, pr, cp, tc


def _weighted_pmf(proba, top_k, threshold, cur_codes, cost_rows, cost, weight, renormalise):
    """Per cell, the loop of RepairModel._compute_repair_pmf / _compute_score on class indices (the contract of
    rgbm_table_repair_pmf_weighted, include/rgbm.h)."""
    return _select(_weighted_probs(np.asarray(proba, np.float64), cost_rows, cost, weight, renormalise), top_k, threshold, cur_codes,
                   cost_rows, cost)


class CostOracleEngine(OracleEngine):
    """OracleEngine with the two entries of the probability modes restated in numpy / Python."""

    class _Table(OracleEngine._Table):
        def gather_rows(self, rows):
            return CostOracleEngine._Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)

        def repair_pmf_weighted(self, model, target_col, feat_cols, top_k=32, threshold=0.0, cur_codes=None, cost_rows=None, cost=None,
                                weight=0.0, renormalise=False):
            rows = np.flatnonzero(self.codes[target_col] < 0).astype(np.int64)
            K = model.info()["num_class"]
            proba = model.predict(np.ascontiguousarray(self.codes[list(feat_cols)][:, rows])) if len(rows) else np.zeros((0, K))
            cls, pr, cp, tc = _weighted_pmf(np.asarray(proba, np.float64), top_k, threshold, cur_codes, cost_rows,
                                            None if cost is None else np.asarray(cost, np.float64), weight, renormalise)
            return rows, cls, pr, cp, tc

    def upload(self, codes, n_codes):
        return CostOracleEngine._Table(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return CostOracleEngine._Table(t.codes, t.n_codes)

    def edit_distance(self, a, b):
        return np.array([[edit_distance(x, y) for y in b] for x in a], np.int32).reshape(len(a), len(b))


def _synthetic_frame(n, cols, seed, null_ratio=0.03):
    dirty, _, cards = make_table(n, cols, seed=seed, null_ratio=null_ratio)
    df = pd.DataFrame({"tid": np.arange(n)})
    for c in range(cols):
        # values of different lengths, so the edit distances differ between classes
        v = np.array(["v%d" % c + "x" * (k % 4) + "%02d" % k for k in range(int(cards[c]))], object)[np.maximum(dirty[c], 0)]
        v[dirty[c] < 0] = None
        df["c%d" % c] = v
    return df


def _error_cells(df, seed, ratio=0.02):
    """The NULL cells plus a random share of non-NULL cells: error cells with a current value, so the costs weigh."""
    rng = np.random.default_rng(seed)
    out = []
    for c in [c for c in df.columns if c != "tid"]:
        pick = df[c].isna().to_numpy() | (rng.random(len(df)) < ratio)
        out.append(pd.DataFrame({"tid": df["tid"].to_numpy()[pick], "attribute": c}))
    return pd.concat(out, ignore_index=True)


def _model(df, cf=None, delta=None, cells=None, **opts):
    m = RepairModel().setInput(df).setRowId("tid")
    m = m.setErrorCells(cells) if cells is not None else m.setErrorDetectors([NullErrorDetector()])
    if cf is not None:
        m = m.setUpdateCostFunction(cf)
    if delta is not None:
        m = m.setRepairDelta(delta)
    for k, v in dict({"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2"}, **opts).items():
        m = m.option(k, str(v))
    return m


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


def _both_paths(make, engine, **flags):
    """(value-space frame, resident frame, resident model) of the same run."""
    slow = make()
    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        a = slow.run(**flags)
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    fast = make().option("repair.pmf.resident", "true")
    fast._engine_override = engine
    b = fast.run(**flags)
    return a, b, fast


MODES = [dict(compute_repair_candidate_prob=True), dict(compute_repair_prob=True), dict(compute_repair_score=True),
         dict(maximal_likelihood_repair=True), dict(maximal_likelihood_repair=True, repair_data=True)]


def test_option_is_registered_and_parsed():
    assert "repair.pmf.resident" in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_pmf_resident) is False
    for raw, want in (("true", True), ("1", True), ("false", False), ("0", False)):
        assert m.option("repair.pmf.resident", raw)._get_option_value(*RepairModel._opt_pmf_resident) is want
    with pytest.raises(ValueError, match="Non-existent key"):
        m.option("repair.pmf.residents", "true")


def test_without_the_option_the_probability_modes_keep_the_value_space_path(oracle_backend):
    df = _synthetic_frame(600, 5, seed=9)
    for cf, flags in ((None, dict(compute_repair_candidate_prob=True)), (Levenshtein(), dict(compute_repair_prob=True))):
        m = _model(df, cf=cf)
        m._engine_override = CostOracleEngine()
        m.run(**flags)
        assert getattr(m, "_last_resident_info", None) is None
    m = _model(df, cf=Levenshtein(), delta=20).option("repair.pmf.resident", "false")
    m._engine_override = CostOracleEngine()
    m.run(maximal_likelihood_repair=True)
    assert getattr(m, "_last_resident_info", None) is None


# maximal likelihood (and the score) needs a cost function without targets: run() rejects the other combinations
CASES = [(cf, f) for cf in (None, "lev", "lev_one", "user") for f in MODES
         if cf in ("lev", "user") or not ("compute_repair_score" in f or "maximal_likelihood_repair" in f)]
# the training-row sample and the hyper-parameter search reach the probability modes through the same runner as the plain run: both
# option sets with Levenshtein(), for the top-1 frame and for maximal likelihood + repair_data (appended, so the ids above keep)
OPTION_SETS = {"lev_sampled": {"model.max_training_row_num": "700"},
               "lev_search": {"model.hp.max_evals": "3", "model.hp.no_progress_loss": "2"}}
CASES += [(cf, f) for cf in OPTION_SETS for f in (MODES[1], MODES[4])]


@pytest.mark.parametrize("cells", [False, True])
@pytest.mark.parametrize("cf,flags", CASES)
def test_synthetic_frames_equal_the_value_space_path(oracle_backend, cf, flags, cells):
    df = _synthetic_frame(1500, 5, seed=21)
    make_cf = {None: lambda: None, "lev": Levenshtein, "lev_sampled": Levenshtein, "lev_search": Levenshtein,
               "lev_one": lambda: Levenshtein(targets=["c2"]),
               "user": lambda: UserDefinedUpdateCostFunction(lambda x, y: float(abs(len(x) - len(y)) + (x[-1] != y[-1])))}[cf]
    ec = _error_cells(df, seed=22) if cells else None
    a, b, fast = _both_paths(lambda: _model(df, cf=make_cf(), delta=40, cells=ec, **OPTION_SETS.get(cf, {})), CostOracleEngine(), **flags)
    assert fast._last_resident_info is not None, "the run did not take the resident path"
    assert len(a) > 0 and list(a.columns) == list(b.columns)
    if flags.get("repair_data"):
        pd.testing.assert_frame_equal(a.sort_values("tid").reset_index(drop=True), b.sort_values("tid").reset_index(drop=True), check_exact=True)
    else:
        pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)


@pytest.mark.parametrize("flags", MODES[:2])
def test_adult_frames_equal_the_value_space_path(oracle_backend, flags):
    df = frame(load_golden("adult")["input"])
    a, b, fast = _both_paths(lambda: _model(df, cf=Levenshtein()), CostOracleEngine(), **flags)
    assert fast._last_resident_info is not None, "the run did not take the resident path"
    pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)


def test_user_cost_dividing_by_zero_falls_back(oracle_backend):
    """1 + weight * cost == 0 raises ZeroDivisionError in the Python loop: the run leaves the resident path and behaves as before."""
    df = _synthetic_frame(600, 4, seed=4)
    m = _model(df, cf=UserDefinedUpdateCostFunction(lambda x, y: -10.0), cells=_error_cells(df, seed=5)).option("repair.pmf.resident", "true")
    m._engine_override = CostOracleEngine()
    with pytest.raises(ZeroDivisionError):
        m.run(compute_repair_candidate_prob=True)
    assert getattr(m, "_last_resident_info", None) is None


def test_pack_code_points():
    from repair._native import pack_code_points
    strs = ["", "a", "héllo", "日本語", "a😀b", "x" * 70]
    cp, off = pack_code_points(strs)
    assert cp.dtype == np.int32 and off.dtype == np.int64 and len(off) == len(strs) + 1 and off[0] == 0
    for i, s in enumerate(strs):
        assert off[i + 1] - off[i] == len(s)
        assert cp[off[i]:off[i + 1]].tolist() == [ord(ch) for ch in s]
    cp, off = pack_code_points([])
    assert len(cp) == 0 and off.tolist() == [0]


def test_weighted_pmf_restatement_without_costs_is_the_plain_top_k():
    """The restatement used above reduces to oracle/prep.top_k_pmf when no cost and no renormalisation apply."""
    from oracle import prep as P
    rng = np.random.default_rng(3)
    proba = rng.dirichlet(np.ones(7), size=50)
    proba[5, 2] = proba[5, 3]                      # a tie
    cls, pr, cp, tc = _weighted_pmf(proba, 4, 0.05, None, None, None, 0.1, False)
    want_cls, want_pr = P.top_k_pmf(proba, 4, 0.05)
    assert np.array_equal(cls, want_cls) and np.array_equal(pr, want_pr) and np.isnan(tc).all()


def _hospital_model(cf, delta=None):
    import tests.test_quality as Q
    df, _, cells = Q._hospital()
    m = RepairModel().setInput(df).setRowId("tid").setErrorCells(cells).setDiscreteThreshold(400).setTargets(Q.HOSPITAL_TARGETS) \
        .option("model.hp.max_evals", "1").setUpdateCostFunction(cf)
    return m.setRepairDelta(delta) if delta is not None else m


@pytest.mark.parametrize("flags", [dict(compute_repair_prob=True), dict(compute_repair_score=True), dict(maximal_likelihood_repair=True),
                                   dict(maximal_likelihood_repair=True, repair_data=True)])
def test_hospital_frames_equal_the_value_space_path(oracle_backend, flags):
    """Given error cells with their current values (typos): the costs re-weigh the distributions and enter the score."""
    a, b, fast = _both_paths(lambda: _hospital_model(Levenshtein(), delta=60), CostOracleEngine(), **flags)
    assert fast._last_resident_info is not None, "the run did not take the resident path"
    assert len(a) > 50
    if flags.get("repair_data"):
        pd.testing.assert_frame_equal(a.sort_values("tid").reset_index(drop=True), b.sort_values("tid").reset_index(drop=True), check_exact=True)
    else:
        pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)


@pytest.mark.parametrize("flags", MODES[:2])
def test_boston_continuous_targets_equal_the_value_space_path(oracle_backend, flags):
    """Continuous targets: the prediction with prob 1.0, made on the un-repaired pmf chain (continuous cells filled in target
    order, discrete ones left NULL) -- and the discrete targets after them are scored on that chain."""
    import tests.test_quality as Q
    df = Q._boston_frame()[0]
    make = lambda: _model(df, cf=Levenshtein(), **{"model.lgb.n_estimators": "20"})  # noqa: E731
    a, b, fast = _both_paths(make, CostOracleEngine(), **flags)
    assert fast._last_resident_info is not None, "the run did not take the resident path"
    pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)
