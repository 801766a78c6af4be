"""CPU: LOFOutlierErrorDetector in code space (repair/lof_codes.py) and `RepairModel.run()` with it on the resident pipeline behind
`error.lof.resident`.

The code-space scores are held to scikit-learn's `LocalOutlierFactor(novelty=False)` on tie-free columns -- within 2^-44 relative (1/16
of the 2^-40 guard band the lowering keeps around the threshold), flags identical -- the medians to `np.median` bit for bit, and whole
runs on a CPU engine (the oracle engine of tests/helpers, the numpy restatement of rgbm_table_detect_cells and the numpy statement
standing in for rgbm_lof_1d) to the value-space path on the oracle estimator backend."""
import warnings

import numpy as np
import pandas as pd
import pytest

from repair import detect_codes as DC
from repair import lof_codes as L
from repair.errors import LOFOutlierErrorDetector, NullErrorDetector, ScikitLearnBackedErrorDetector
from repair.model import RepairModel
from repair.pipeline import NotResidentEligible
from tests import detector_restatements as R
from tests.helpers import OracleEngine

BOUND = 2.0 ** -44


# ---------------------------------------------------------------------------------------------- the statement against scikit-learn
def _columns():
    """{name: column as the detector's estimator sees it (NULLs filled)}: seeded, tie-free."""
    rng = np.random.default_rng(20)
    out = {}
    for n in (2, 3, 20, 21, 22, 500, 3000):
        out["normal_%d" % n] = rng.normal(size=n)
        out["lognormal_%d" % n] = rng.lognormal(size=n)
    for name, x in (("normal", rng.normal(size=3000)), ("lognormal", rng.lognormal(size=3000))):
        x[rng.integers(0, 3000, 600)] = x[:600][rng.integers(0, 600, 600)]             # exact duplicates, a few copies each
        out[name + "_duplicates"] = x
    for name, x in (("normal", rng.normal(size=3000)), ("lognormal", rng.lognormal(size=3001))):
        nul = rng.random(len(x)) < 0.1
        x[nul] = np.median(x[~nul])                                                     # 10 % median fill (odd and even n of the rest)
        out[name + "_median_fill"] = x
    for m in (19, 20, 21, 40):
        x = rng.normal(size=500)
        x[:m] = x[m]                                                                    # one value with m + 1 copies ...
        out["normal_copies_%d" % (m + 1)] = x
        x = rng.lognormal(size=500)
        x[:m - 1] = x[m]                                                                # ... and with m copies
        out["lognormal_copies_%d" % m] = x
    x = rng.normal(size=500)
    x[[7, 250, 499]] = [50.0, -70.0, 90.5]
    out["far_outliers"] = x
    return out


@pytest.fixture(scope="module")
def against_sklearn():
    """{name: (relative deviation of the scores, flags equal, n_ties, n_near, flagged rows)} of every column of `_columns`."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    res = {}
    for name, x in _columns().items():
        v, c = np.unique(x, return_counts=True)
        lof, bad, n_ties, n_near = L.lof_codes(v, c, 20)
        est = neighbors.LocalOutlierFactor(novelty=False)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                             # "n_neighbors is greater than ...", "Duplicate values ..."
            pred = est.fit_predict(x.reshape(-1, 1))
        ref = -est.negative_outlier_factor_
        at = np.searchsorted(v, x)
        res[name] = (float(np.max(np.abs(lof[at] - ref) / np.abs(ref))), bool(np.array_equal(pred < 0, bad[at])), n_ties, n_near,
                     int((pred < 0).sum()))
    return res


@pytest.mark.parametrize("name", sorted(_columns()))
def test_scores_and_flags_equal_scikit_learn(against_sklearn, name):
    rel, same, n_ties, n_near, flagged = against_sklearn[name]
    assert n_ties == 0 and n_near == 0
    assert same, "the flagged rows differ"
    assert rel < BOUND, "relative deviation %.3g" % rel
    if name == "far_outliers":
        assert flagged >= 3


def test_measured_deviation_stays_inside_a_sixteenth_of_the_guard_band(against_sklearn):
    assert len(against_sklearn) == len(_columns()) == 27           # 14 sizes, 2 with duplicates, 2 filled, 8 with copies, 1 with outliers
    worst = max(r[0] for r in against_sklearn.values())
    assert worst < BOUND, "largest relative deviation from scikit-learn %.3g (bound 2^-44 = %.3g, guard band 2^-40 = %.3g)" % (
        worst, BOUND, L.NEAR_BAND)
    assert L.NEAR_BAND == 16 * BOUND and L.THRESHOLD == 1.5


# ---------------------------------------------------------------------------------------------- medians and the fill
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 100, 101])
def test_median_from_counts_is_numpy_median(n):
    rng = np.random.default_rng(n)
    for trial in range(20):
        x = rng.normal(size=n) if trial % 2 else np.round(rng.normal(size=n), 1)
        v, c = np.unique(x, return_counts=True)
        assert L.median_from_counts(v, c) == float(np.median(x))
    # between two dictionary values: their mean, as numpy rounds it
    assert L.median_from_counts([0.1, 0.7], [3, 3]) == float(np.median([0.1] * 3 + [0.7] * 3)) == (0.1 + 0.7) / 2.0
    with pytest.raises(ValueError):
        L.median_from_counts([], [])


@pytest.mark.parametrize("case", ["median_is_a_value", "median_between_values", "no_null", "all_null", "a_code_without_rows"])
def test_filled_multiset_is_unique_of_fillna(case):
    x = dict(median_is_a_value=[1.0, 2.0, 2.0, 5.0, 9.0, np.nan, np.nan], median_between_values=[1.0, 2.0, 5.0, 9.0, np.nan, np.nan, np.nan],
             no_null=[3.0, 1.0, 1.0, 8.0], all_null=[np.nan] * 4, a_code_without_rows=[1.0, 2.0, 5.0, 9.0, np.nan])[case]
    s = pd.Series(x, dtype=np.float64)
    values = np.unique(s.dropna().to_numpy())
    counts = np.array([(s == v).sum() for v in values], np.int64)
    if case == "a_code_without_rows":                                                   # a dictionary entry whose rows are gone
        values, counts = np.insert(values, 2, 3.5), np.insert(counts, 2, 0)
    med = float(np.median(s.dropna())) if s.notna().any() else 0.0
    want_v, want_c = np.unique(s.fillna(med).to_numpy(), return_counts=True)
    v, c, med_at, code_at = L.filled_multiset(values, counts, int(s.isna().sum()))
    assert np.array_equal(v, want_v) and np.array_equal(c, want_c)
    live = counts > 0
    assert np.array_equal(v[code_at[live]], values[live]) and (code_at[~live] == -1).all()
    if s.isna().any():
        assert v[med_at] == med
    elif med_at >= 0:
        assert v[med_at] == med
    if case == "median_between_values":
        assert med not in values and c[med_at] == 3
    if case == "all_null":
        assert v.tolist() == [0.0] and c.tolist() == [4]


# ---------------------------------------------------------------------------------------------- ties, the band, refusals
def test_a_symmetric_boundary_tie_is_counted_and_resolved_to_the_left():
    lof, bad, n_ties, n_near = L.lof_codes([0.0, 1.0, 2.0], [1, 1, 1], k=1)
    assert n_ties == 1                                          # the middle value: either neighbour at distance 1, one fits
    k_, m, self_taken, l, r, side, part, kdist, tie = L.lof_windows([0.0, 1.0, 2.0], [1, 1, 1], k=1)
    assert tie.tolist() == [False, True, False] and (l[1], r[1], side[1]) == (0, 1, 1)
    # both candidates fit: no tie
    assert L.lof_codes([0.0, 1.0, 2.0], [1, 1, 1], k=2)[2] == 0
    # an integer-valued column
    x = np.random.default_rng(5).integers(0, 50, 500).astype(np.float64)
    v, c = np.unique(x, return_counts=True)
    assert L.lof_codes(v, c, 20)[2] > 0


def _lower(values, k=20, null=0):
    """`build_descriptors` for one LOF detector on one column named `x` holding `values` and `null` NULL cells."""
    values = np.asarray(values, np.float64)
    v, c = np.unique(values, return_counts=True)
    return DC.build_descriptors([dict(kind="lof", attrs=["x"], k=k)], ["x"], [v], {"x": np.dtype(np.float64)}, lambda j: c, ["x"],
                                n_rows=len(values) + null)


def test_the_lowering_refuses_ties_and_single_rows_and_names_the_attribute():
    x = np.random.default_rng(5).integers(0, 50, 500)
    with pytest.raises(NotResidentEligible, match="`x`.*tied"):
        _lower(x)
    with pytest.raises(NotResidentEligible, match="`x`: 1 row"):
        _lower([4.0])
    with pytest.raises(ValueError, match="row count"):
        DC.build_descriptors([dict(kind="lof", attrs=["x"], k=20)], ["x"], [np.array([1.0, 2.0])], {"x": np.dtype(np.float64)},
                             lambda j: np.array([1, 1]), ["x"])


@pytest.mark.parametrize("n,refused", [(30, True), (41, True), (42, False), (43, False)])
def test_the_lowering_refuses_a_column_scikit_learn_searches_by_brute_force(n, refused):
    """`algorithm='auto'` is brute force when n_neighbors >= n // 2: its x^2 + y^2 - 2xy distances lose the differences of values that are
    large next to their spread (epoch seconds, ids, years), and neither the tie count nor the band would notice."""
    sk = pytest.importorskip("sklearn.neighbors")
    x = 1e8 + np.random.default_rng(n).normal(size=n)
    est = sk.LocalOutlierFactor(novelty=False).fit(x.reshape(-1, 1))
    assert est._fit_method == ("brute" if refused else "kd_tree")
    if refused:
        with pytest.raises(NotResidentEligible, match="`x`.*brute force"):
            _lower(x)
        assert len(_lower(x, k=n // 2 - 1)) == 1                              # fewer neighbours: a tree search again
    else:
        d, = _lower(x)
        v = np.unique(x)
        bad = DC.unpack_bits(d["flag_bits"], len(v)) if d["flag_bits"] is not None else np.zeros(len(v), bool)
        assert np.array_equal(bad[np.searchsorted(v, x)], est.fit_predict(x.reshape(-1, 1)) < 0)
        ref = -est.negative_outlier_factor_
        lof = L.lof_codes(v, np.ones(len(v), np.int64), 20)[0][np.searchsorted(v, x)]
        assert np.max(np.abs(lof - ref) / np.abs(ref)) < BOUND
    # the NULL cells count: 38 values and 4 NULLs are 42 rows
    if n == 42:
        assert len(_lower(x[:38], null=4)) == 1
        with pytest.raises(NotResidentEligible, match="brute force"):
            _lower(x[:38], null=3)


def test_the_lowering_refuses_a_span_whose_squares_overflow():
    x = 1e160 * np.random.default_rng(1).normal(size=100)
    with pytest.raises(NotResidentEligible, match="span"):
        _lower(x)
    assert len(_lower(x * 1e-12)) == 1
    assert len(_lower(x * 1e-15)) == 1                                        # 1e145: still large, the span inside the bound


def test_a_score_inside_the_band_is_counted_and_refused():
    # k = 1: lof of the last value is (t + 1e-10) / (1 + 1e-10) with t its distance to the pair (0, 1): 1.5 at t = 1.5 + 0.5e-10
    t = 1.5 + 0.5e-10
    lof, bad, n_ties, n_near = L.lof_codes([0.0, 1.0, 1.0 + t], [1, 1, 1], k=1)
    assert abs(lof[2] - 1.5) <= 1.5 * 2.0 ** -40 and n_near == 1 and n_ties == 0
    assert L.lof_codes([0.0, 1.0, 1.0 + t + 1e-9], [1, 1, 1], k=1)[3] == 0
    # in the lowering: the same three values behind a far pair, so that the column is one scikit-learn searches with a tree (n // 2 > k)
    with pytest.raises(NotResidentEligible, match="within rounding"):
        _lower([-1000.0, -999.0, 0.0, 1.0, 1.0 + t], k=1)


def test_refusals():
    for values, counts, k in (([1.0], [1], 20), ([1.0, np.nan], [1, 1], 20), ([1.0, np.inf], [1, 1], 20), ([-np.inf, 1.0], [1, 1], 20),
                              ([1.0, 2.0], [1, 1], 0), ([1.0, 2.0], [1, 1], 65), ([2.0, 1.0], [1, 1], 20), ([1.0, 1.0], [1, 1], 20),
                              ([1.0, 2.0], [1, 0], 20), ([], [], 20)):
        with pytest.raises(ValueError):
            L.lof_codes(values, counts, k)
    assert L.lof_codes([1.0], [2], 20)[0].tolist() == [1.0]                 # one value, two rows: n = 2
    assert L.lof_codes([1.0, 2.0], [1, 1], 64)[1].tolist() == [False, False]


def test_the_lowering_maps_flags_back_to_codes_and_flags_nulls_with_the_median():
    rng = np.random.default_rng(3)
    x = rng.normal(size=300)
    x[[5, 6]] = [40.0, -35.0]
    d, = _lower(x, null=7)
    v = np.unique(x)
    flagged = DC.unpack_bits(d["flag_bits"], len(v))
    assert d["kinds"] == ["lof"] and d["null_is_error"] is False and (d["keep_lo"], d["keep_hi"]) == DC.NO_RANGE
    assert flagged[[0, len(v) - 1]].all() and d["codes_flagged"] == int(flagged.sum())
    # a column whose median is the outlier: most cells NULL, the rest spread out -> the NULL cells are the flagged ones' kin
    y = np.r_[np.full(40, 100.0), rng.normal(size=41)]
    sk = pytest.importorskip("sklearn.neighbors")
    col = pd.Series(np.r_[y, [np.nan] * 9])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        pred = sk.LocalOutlierFactor(novelty=False).fit_predict(col.fillna(float(np.median(y))).to_frame())
    d, = _lower(y, null=9)
    assert d["null_is_error"] == bool(pred[-1] < 0)


# ---------------------------------------------------------------------------------------------- whole runs
OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "6", "model.lgb.learning_rate": "0.2"}
ON = "error.lof.resident"


class LofTable(OracleEngine._Table):
    def detect_cells(self, cols, null_is_error, keep_lo, keep_hi, flag_bits=None):
        return R.detect_cells(self.codes, cols, null_is_error, keep_lo, keep_hi, flag_bits)


class LofEngine(OracleEngine):
    """The oracle engine with `detect_cells` and `lof_codes` (the numpy statement, as rgbm_lof_1d computes it), and a call record."""

    def __init__(self):
        self.lof_calls = []

    def upload(self, codes, n_codes):
        return LofTable(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return LofTable(t.codes, t.n_codes, t.values, t.kinds)

    def lof_codes(self, values, counts, k=20):
        self.lof_calls.append((len(values), int(np.sum(counts)), k))
        return L.lof_codes(values, counts, k)


def _run_frame(n=240, seed=7, tied=False):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 6, n)
    a = np.array(["a%d" % v for v in g], object)
    b = np.array(["b%d" % (v % 3) for v in g], object)
    x = g * 1.5 + rng.normal(0, 0.3, n)                    # doubles: no two differences alike
    b[[40, 41]] = None
    x[[8, 120]] = [99.0, -50.0]
    x[[9, 200, 201]] = np.nan
    df = pd.DataFrame({"tid": np.arange(n), "a": a, "b": b, "x": x})
    if tied:
        df["k"] = (g * 10 + rng.integers(0, 3, n)).astype(np.int64)
        df.loc[[8, 30], "k"] = [900, -400]
    return df


def _model(df, engine=None, on=False, targets=("b", "x"), detectors=None):
    dets = detectors if detectors is not None else [NullErrorDetector(), LOFOutlierErrorDetector()]
    m = RepairModel().setInput(df).setRowId("tid").setTargets(list(targets)).setDiscreteThreshold(50).setErrorDetectors(dets)
    for key, val in OPTS.items():
        m = m.option(key, str(val))
    if on:
        m = m.option(ON, "true")
    m._engine_override = engine
    return m


def _sorted(df, repair_data):
    return df.sort_values(["tid"] if repair_data else ["tid", "attribute"]).reset_index(drop=True)


@pytest.fixture
def pandas_detector_calls(monkeypatch):
    calls = []
    impl = ScikitLearnBackedErrorDetector._detect_impl

    def counted(self):
        calls.append(type(self).__name__)
        return impl(self)
    monkeypatch.setattr(ScikitLearnBackedErrorDetector, "_detect_impl", counted)
    return calls


def test_option_is_registered_and_parsed():
    assert ON in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_lof_resident) is False
    assert m.option(ON, "true")._get_option_value(*RepairModel._opt_lof_resident) is True


@pytest.mark.parametrize("repair_data", [False, True])
def test_run_on_the_resident_table_equals_the_value_space_run(oracle_backend, monkeypatch, pandas_detector_calls, repair_data):
    pytest.importorskip("sklearn")
    df = _run_frame()
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df).run(repair_data=repair_data)
    monkeypatch.delenv("REPAIR_RESIDENT")
    assert len(pandas_detector_calls) == 1 and len(slow) > 0
    if not repair_data:
        cur = slow.loc[slow["attribute"] == "x", "current_value"]
        assert {99.0, -50.0} <= set(cur.dropna().astype(float)) and cur.isna().sum() == 3
    eng = LofEngine()
    fast = _model(df, eng, on=True)
    fast_frame = fast.run(repair_data=repair_data)
    assert fast._last_detection_on_device is True
    assert eng.lof_calls == [(df["x"].nunique(), len(df), 20)]             # 237 values, the three NULLs on a median of their own
    assert len(pandas_detector_calls) == 1                                  # no pandas detector since the value-space run
    info = {d["attribute"]: d for d in fast._last_resident_info["value_detectors"]}
    assert info["x"]["kinds"] == ["null", "lof"] and info["x"]["codes_flagged"] >= 2 and info["b"]["kinds"] == ["null"]
    pd.testing.assert_frame_equal(_sorted(slow, repair_data), _sorted(fast_frame, repair_data), check_exact=True)


def test_option_off_never_asks_the_engine(oracle_backend, monkeypatch, pandas_detector_calls):
    pytest.importorskip("sklearn")
    df = _run_frame()
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    eng = LofEngine()
    off = _model(df, eng, on=False)
    off_frame = off.run()
    assert off._last_detection_on_device is False and eng.lof_calls == [] and len(pandas_detector_calls) == 2
    assert off._device_detection_plan(df, ["x"], False, False) is None
    pd.testing.assert_frame_equal(_sorted(slow, False), _sorted(off_frame, False), check_exact=True)


def test_a_tied_integer_column_comes_back_through_the_fallback(oracle_backend, monkeypatch, pandas_detector_calls, caplog):
    pytest.importorskip("sklearn")
    import logging
    df = _run_frame(tied=True)
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df, targets=("b", "x", "k")).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    eng = LofEngine()
    fast = _model(df, eng, on=True, targets=("b", "x", "k"))
    with caplog.at_level(logging.INFO):
        fast_frame = fast.run()
    assert fast._last_detection_on_device is False
    assert len(eng.lof_calls) >= 1 and len(pandas_detector_calls) == 2      # the engine was asked, refused `k`, the pandas detector ran
    assert any("LOF detector on `k`" in r.getMessage() for r in caplog.records)
    assert (slow["attribute"] == "k").any()
    pd.testing.assert_frame_equal(_sorted(slow, False), _sorted(fast_frame, False), check_exact=True)


def test_a_small_offset_table_comes_back_through_the_fallback(oracle_backend, monkeypatch, pandas_detector_calls):
    """40 rows of epoch-like values: scikit-learn searches them by brute force and its distances are not the exact differences, so the
    plan leaves the detector in value space (and the frame is the value-space run's)."""
    sk = pytest.importorskip("sklearn.neighbors")
    df = _run_frame().iloc[:40].reset_index(drop=True)
    df["x"] = df["x"] + 1e8
    assert sk.LocalOutlierFactor(novelty=False).fit(df[["x"]].fillna(0.0))._fit_method == "brute"
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    eng = LofEngine()
    fast = _model(df, eng, on=True)
    fast_frame = fast.run()
    assert fast._last_detection_on_device is False and eng.lof_calls == [] and len(pandas_detector_calls) == 2
    assert len(slow) > 0
    pd.testing.assert_frame_equal(_sorted(slow, False), _sorted(fast_frame, False), check_exact=True)
    # the rule is scikit-learn's: n_neighbors >= rows // 2
    for n, taken in ((41, False), (42, True)):
        sub = _run_frame(n=240).iloc[:n]
        assert (_model(sub, LofEngine(), on=True)._device_detection_plan(sub, ["x"], False, False) is not None) == taken


class _MyLof(LOFOutlierErrorDetector):
    pass


def test_the_plan_takes_exactly_the_lof_detector():
    pytest.importorskip("sklearn")
    from sklearn.ensemble import IsolationForest
    from sklearn.neighbors import LocalOutlierFactor
    df = _run_frame()
    plan = _model(df, LofEngine(), on=True)._device_detection_plan(df, ["x"], False, False)
    assert plan["value_detectors"] == [dict(kind="lof", attrs=["x"], k=20)]
    for dets in ([NullErrorDetector(), _MyLof()],
                 [NullErrorDetector(), ScikitLearnBackedErrorDetector(lambda: IsolationForest(random_state=0))],
                 [NullErrorDetector(), ScikitLearnBackedErrorDetector(lambda: LocalOutlierFactor(novelty=False))]):
        assert _model(df, LofEngine(), on=True, detectors=dets)._device_detection_plan(df, ["x"], False, False) is None
    inf = df.assign(x=df["x"].where(df.index != 3, np.inf))
    assert _model(inf, LofEngine(), on=True)._device_detection_plan(inf, ["x"], False, False) is None
    wide = df.assign(x=df["x"] * 1e155)                              # scikit-learn's squared distances overflow: its error to report
    assert _model(wide, LofEngine(), on=True)._device_detection_plan(wide, ["x"], False, False) is None
    assert _model(wide, LofEngine(), on=True)._device_detection_plan(wide.assign(x=wide["x"] * 1e-10), ["x"], False, False) is not None
    text = df.assign(x=df["x"].astype(str))
    assert _model(text, LofEngine(), on=True)._device_detection_plan(text, ["x"], False, False) is None
