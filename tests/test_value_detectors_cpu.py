"""CPU: the value detectors (RegExErrorDetector, DomainValues, GaussianOutlierErrorDetector) as predicates on dictionary codes
(repair/detect_codes.py) and `RepairModel.run()` with them on the resident pipeline behind `error.value_detectors.resident`.

The descriptor builders are held to the value-space detectors of repair/errors.py cell for cell, the quartiles to `np.percentile` bit
for bit, and whole runs on a CPU engine (the oracle engine of tests/helpers plus the numpy restatement of rgbm_table_detect_cells in
tests/detector_restatements.py) to the value-space path on the oracle estimator backend."""
import numpy as np
import pandas as pd
import pytest

from repair import detect_codes as DC
from repair.errors import (ConstraintErrorDetector, DomainValues, GaussianOutlierErrorDetector, LOFOutlierErrorDetector, NullErrorDetector,
                           RegExErrorDetector)
from repair.model import RepairModel
from repair.pipeline import encode_frame
from tests import detector_restatements as R
from tests.helpers import OracleEngine, frame, load_golden


class DetectTable(OracleEngine._Table):
    """The oracle engine's table with `detect_cells` (and the two analysis entries, served by repair.domain on the host)."""
    calls = 0

    def detect_cells(self, cols, null_is_error, keep_lo, keep_hi, flag_bits=None):
        DetectTable.calls += 1
        return R.detect_cells(self.codes, cols, null_is_error, keep_lo, keep_hi, flag_bits)

    def pair_counts(self, pairs, luts=None, n_bins=None):
        from repair import domain as D
        self._view = D.View(sorted(n_bins), n_bins, luts or {}, [])
        self._pairs = [tuple(map(int, p)) for p in pairs]
        self._joints = D.HostBackend(self.codes, self._view).pair_counts(self._pairs)
        return [j.dense() for j in self._joints]

    def cell_domains(self, target_col, rows, pair_idx, min_cnt, single_ok, beta, row_count, want_probs=False):
        from repair import domain as D
        tab = D.PairTable(self._pairs, self._joints)
        corr = [[c for c in self._pairs[p] if c != target_col][0] for p in pair_idx]
        return D.HostBackend(self.codes, self._view).cell_domains(target_col, rows, corr, tab, min_cnt, single_ok, beta, row_count, want_probs)


class DetectEngine(OracleEngine):
    def upload(self, codes, n_codes):
        return DetectTable(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return DetectTable(t.codes, t.n_codes, t.values, t.kinds)


# ---------------------------------------------------------------------------------------------- the builders against the detectors
def _spec(d, continuous):
    if type(d) is RegExErrorDetector:
        return dict(kind="regex", attr=d.attr, regex=d.regex)
    if type(d) is DomainValues:
        return None if d.attr in continuous else dict(kind="domain", attr=d.attr, values=list(d.values), autofill=d.autofill,
                                                      min_count_thres=d.min_count_thres)
    if type(d) is GaussianOutlierErrorDetector:
        return dict(kind="outlier", attrs=list(continuous))
    raise AssertionError(d)


def _value_cells(df, detectors, targets, continuous):
    """Cells of the value-space detectors: sorted [(column position, row position)]."""
    cols = [c for c in df.columns if c != "tid"]
    out = set()
    for d in detectors:
        cells = d.setUp("tid", df, list(continuous), list(targets)).detect()
        rpos = pd.Series(np.arange(len(df)), index=df["tid"].to_numpy()).reindex(cells["tid"].to_numpy()).to_numpy()
        out |= {(cols.index(a), int(r)) for a, r in zip(cells["attribute"], rpos)}
    return sorted(out)


def _code_cells(df, detectors, targets, continuous, null_all=False):
    """The same through the dictionaries: descriptors -> restated device entry.  Returns (cells, descriptors)."""
    cols = [c for c in df.columns if c != "tid"]
    idx, remaps, dicts = encode_frame(df, cols)
    codes = np.stack([np.where(idx[j] >= 0, remaps[j][np.maximum(idx[j], 0)] if len(remaps[j]) else -1, -1) for j in range(len(cols))]).astype(np.int32)
    counts = lambda j: np.bincount(codes[j][codes[j] >= 0], minlength=len(dicts[j]))  # noqa: E731
    specs = [s for s in (_spec(d, continuous) for d in detectors if type(d) is not NullErrorDetector) if s is not None]
    descs = DC.build_descriptors(specs, cols, dicts, {c: df[c].dtype for c in cols}, counts, list(targets), null_all=null_all)
    assert [d["col"] for d in descs] == sorted(d["col"] for d in descs) and len({d["col"] for d in descs}) == len(descs)
    r, c = R.detect_cells(codes, [d["col"] for d in descs], [d["null_is_error"] for d in descs], [d["keep_lo"] for d in descs],
                          [d["keep_hi"] for d in descs], [d["flag_bits"] for d in descs])
    cells = list(zip(c.tolist(), r.tolist()))
    assert cells == sorted(set(cells)), "each cell once, ordered by (column, row)"
    for d in descs:                                       # the summary figure is the number of flagged dictionary entries
        sel = codes[d["col"]][r[c == d["col"]]]
        assert len(np.unique(sel[sel >= 0])) <= d["codes_flagged"] <= len(dicts[d["col"]])
    return cells, descs


def _small_frame():
    """int64, float with NaN, bool, nullable Int64, float32 and a string column whose values are full of regex metacharacters."""
    rng = np.random.default_rng(11)
    n = 120
    s = rng.choice(["a.b", "a+b", "(c)", "d|e", "x[1]", "a?b", "aXb"], n, p=[.3, .25, .2, .1, .05, .05, .05]).astype(object)
    s[[4, 50]] = None
    f = np.round(rng.normal(10, 2, n), 1)
    f[[0, 7, n - 1]] = np.nan
    f[[3, 60]] = [55.5, -40.0]
    f[9] = 2.0
    i = rng.integers(0, 30, n).astype(np.int64)
    i[[2, 30]] = [1000, -700]
    ni = pd.array(rng.integers(0, 12, n), dtype="Int64")
    ni[[5, 6]] = pd.NA
    counted = np.repeat(["v4", "v5", "v6"], [4, 5, 6]).tolist()             # counts exactly at, one above and two above a threshold of 4
    m = np.array((counted + ["v9"] * (n - len(counted)))[:n], object)
    return pd.DataFrame({"tid": np.arange(n) * 3 + 1, "s": s, "f": f, "i": i, "b": rng.random(n) < 0.4, "ni": ni,
                         "f32": rng.integers(0, 9, n).astype(np.float32) / 10, "m": m})


SMALL_CASES = [
    ("regex_none", [RegExErrorDetector("s", ".")], ()),
    ("regex_all", [RegExErrorDetector("s", "^$")], ()),
    ("regex_some", [RegExErrorDetector("s", r"^a.b$")], ()),
    ("regex_blank", [RegExErrorDetector("s", "  "), RegExErrorDetector("s", "")], ()),
    ("regex_unknown_attr", [RegExErrorDetector("nope", "x"), RegExErrorDetector("tid", "x")], ()),
    ("regex_int64", [RegExErrorDetector("i", r"^\d$"), RegExErrorDetector("i", r"\.")], ()),
    ("regex_float", [RegExErrorDetector("f", r"^\d+\.0$")], ()),
    ("regex_float_two", [RegExErrorDetector("f", r"^2$")], ()),
    ("regex_bool", [RegExErrorDetector("b", "^True$")], ()),
    ("regex_nullable_int", [RegExErrorDetector("ni", "^1")], ()),
    ("regex_float32", [RegExErrorDetector("f32", r"^0\.[1-3]$")], ()),
    ("domain_metachars", [DomainValues("s", values=["a.b", "(c)", "d|e", "a+b"])], ()),
    ("domain_empty", [DomainValues("s", values=[])], ()),
    ("domain_blank_value", [DomainValues("s", values=[""])], ()),
    ("domain_autofill_at_threshold", [DomainValues("m", autofill=True, min_count_thres=4)], ()),
    ("domain_autofill_one_above", [DomainValues("m", autofill=True, min_count_thres=5)], ()),
    ("domain_autofill_none_passes", [DomainValues("m", values=["v5"], autofill=True, min_count_thres=10 ** 6)], ()),
    ("domain_autofill_int", [DomainValues("i", autofill=True, min_count_thres=3)], ()),
    ("domain_autofill_float32", [DomainValues("f32", autofill=True, min_count_thres=12)], ()),
    ("domain_autofill_bool", [DomainValues("b", autofill=True, min_count_thres=60)], ()),
    ("domain_on_continuous", [DomainValues("f", values=["1"])], ("f", "i")),
    ("outlier", [GaussianOutlierErrorDetector()], ("f", "i", "f32")),
    ("outlier_and_regex_one_column", [GaussianOutlierErrorDetector(), RegExErrorDetector("f", r"^1\d\."), RegExErrorDetector("f", r"\.[0-4]$")], ("f",)),
    ("everything", [RegExErrorDetector("s", r"^a"), DomainValues("s", values=["b"]), DomainValues("m", autofill=True, min_count_thres=4),
                    GaussianOutlierErrorDetector(), RegExErrorDetector("i", "^[12]")], ("f", "i")),
]


@pytest.mark.parametrize("name,detectors,continuous", SMALL_CASES, ids=[c[0] for c in SMALL_CASES])
def test_descriptors_give_the_cells_of_the_value_space_detectors(name, detectors, continuous):
    df = _small_frame()
    targets = [c for c in df.columns if c != "tid"]
    want = _value_cells(df, detectors, targets, continuous)
    got, descs = _code_cells(df, detectors, targets, continuous)
    assert got == want
    if name == "regex_none":
        assert len(want) == 2                                  # the NULL cells only: `attr IS NULL` is part of the detector
    if name in ("regex_all", "domain_empty"):
        assert len(want) == len(df)
    if name in ("regex_blank", "regex_unknown_attr", "domain_on_continuous"):
        assert want == [] and descs == []
    if name == "regex_float_two":
        assert len(want) == len(df)                            # the float 2.0 prints as '2.0', never '2'
    if name == "domain_autofill_at_threshold":
        assert len(want) == 4                                  # 4 occurrences are not MORE than 4
    if name == "domain_autofill_one_above":
        assert len(want) == 4 + 5
    if name == "outlier":
        d = {x["attribute"]: x for x in descs}
        assert all(x["flag_bits"] is None and not x["null_is_error"] for x in descs)        # range only, NULLs are not outliers
        assert d["f"]["keep_lo"] > 0 and d["f"]["keep_hi"] < df["f"].nunique() - 1
    if name == "outlier_and_regex_one_column":
        assert len(descs) == 1 and descs[0]["kinds"] == ["outlier", "regex", "regex"] and descs[0]["null_is_error"]


def test_targets_restrict_the_detectors_and_null_rides_along():
    df = _small_frame()
    dets = [RegExErrorDetector("s", "^a"), RegExErrorDetector("i", "^1"), GaussianOutlierErrorDetector()]
    want = _value_cells(df, dets + [NullErrorDetector()], ["s", "f", "ni"], ("f", "i"))
    got, descs = _code_cells(df, dets, ["s", "f", "ni"], ("f", "i"), null_all=True)
    assert got == want
    assert [(d["attribute"], d["kinds"]) for d in descs] == [("s", ["null", "regex"]), ("f", ["null", "outlier"]), ("ni", ["null"])]


@pytest.fixture(scope="module")
def hospital():
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    df["ZipCode"] = pd.to_numeric(df["ZipCode"], errors="coerce")            # one continuous attribute (typos become NULL)
    return df


HOSPITAL_CASES = [
    ("regex_none", [RegExErrorDetector("State", "^[a-z]")]),
    ("regex_some", [RegExErrorDetector("State", "^al$"), RegExErrorDetector("MeasureCode", r"^[a-z]+-[a-z]*-?\d+[a-z]?$")]),
    ("regex_all", [RegExErrorDetector("City", "^$")]),
    ("regex_float_column", [RegExErrorDetector("ZipCode", r"^35\d+\.0$")]),
    ("autofill_every_target", None),
    ("outlier", [GaussianOutlierErrorDetector()]),
]


@pytest.mark.parametrize("name,detectors", HOSPITAL_CASES, ids=[c[0] for c in HOSPITAL_CASES])
def test_descriptors_on_the_hospital_frame(hospital, name, detectors):
    from tests.test_quality import HOSPITAL_TARGETS
    if detectors is None:
        detectors = [DomainValues(attr=c, autofill=True, min_count_thres=4) for c in HOSPITAL_TARGETS]       # the default detectors
    want = _value_cells(hospital, detectors, HOSPITAL_TARGETS, ("ZipCode",))
    got, _ = _code_cells(hospital, detectors, HOSPITAL_TARGETS, ("ZipCode",))
    assert got == want
    if name == "regex_none":
        assert len(want) == int(hospital["State"].isna().sum())              # `attr IS NULL` is all that is left
    else:
        assert len(want) > 0
    if name == "regex_all":
        assert len(want) == len(hospital)


# ---------------------------------------------------------------------------------------------- quartiles from counts
def _expanded_check(values, counts):
    values, counts = np.asarray(values, np.float64), np.asarray(counts, np.int64)
    expanded = np.repeat(values, counts)
    q = DC.percentiles_from_counts(values, counts, (25, 75))
    ref = np.percentile(expanded, [25, 75])
    assert q.dtype == np.float64 and q[0] == ref[0] and q[1] == ref[1], (values, counts, q, ref)
    lo, hi = DC.tukey_fences(values, counts)
    rlo, rhi = ref[0] - 1.5 * (ref[1] - ref[0]), ref[1] + 1.5 * (ref[1] - ref[0])
    assert lo == rlo and hi == rhi
    klo, khi = DC.kept_code_range(values, lo, hi)
    bad = (values < lo) | (values > hi)
    assert np.array_equal(bad, (np.arange(len(values)) < klo) | (np.arange(len(values)) > khi))
    return q


def test_quartiles_equal_numpy_percentile_bit_for_bit():
    rng = np.random.default_rng(5)
    for n in range(1, 41):                                   # every n, those with an integral 0.25 (n - 1) among them
        v = np.sort(rng.normal(0, 1e3, n))
        _expanded_check(v, np.ones(n, np.int64))
        _expanded_check(np.arange(n) * 0.1, np.ones(n, np.int64))
    for trial in range(400):
        D = int(rng.integers(1, 30))
        kind = trial % 4
        if kind == 0:
            v = np.unique(rng.normal(0, 1, D) * 10.0 ** rng.integers(-8, 8))
        elif kind == 1:
            v = np.unique(rng.integers(-50, 50, D)).astype(np.float64)
        elif kind == 2:
            v = np.unique(np.round(rng.random(D), 2))
        else:
            v = np.unique(rng.normal(1e15, 1.0, D))           # neighbours a few ulps apart
        c = rng.integers(0, 4, len(v)) if trial % 3 else rng.integers(1, 2000, len(v))       # zero counts and heavy duplicates
        if c.sum() == 0:
            c[0] = 1
        _expanded_check(v, c)
    _expanded_check([1.0, 2.0, 1e6], [1000, 1000, 1])
    _expanded_check([3.5], [1])
    _expanded_check([3.5], [17])
    assert np.array_equal(DC.order_statistics([2, 0, 3], [0, 1, 2, 3, 4]), [0, 0, 2, 2, 2])


def test_integer_columns_take_the_same_quartiles():
    """`np.percentile` on an int64 column subtracts in integers before it interpolates; the dictionaries are float64."""
    rng = np.random.default_rng(9)
    for _ in range(100):
        x = rng.integers(-10 ** 6, 10 ** 6, int(rng.integers(1, 60)))
        v, c = np.unique(x, return_counts=True)
        ref = np.percentile(x, [25, 75])
        q = DC.percentiles_from_counts(v.astype(np.float64), c)
        assert q[0] == ref[0] and q[1] == ref[1]


def test_outlier_edges_all_null_and_single_value():
    n = 40
    df = pd.DataFrame({"tid": np.arange(n), "allnull": np.full(n, np.nan), "one": np.full(n, 7.25), "x": np.r_[np.arange(n - 1) * 1.0, 500.0]})
    dets = [GaussianOutlierErrorDetector()]
    want = _value_cells(df, dets, ["allnull", "one", "x"], ("allnull", "one", "x"))
    got, descs = _code_cells(df, dets, ["allnull", "one", "x"], ("allnull", "one", "x"))
    assert got == want == [(2, n - 1)]
    assert [d["attribute"] for d in descs] == ["one", "x"]            # the all-NULL column is skipped, as the detector skips it
    one = descs[0]
    assert one["keep_lo"] > one["keep_hi"] and one["flag_bits"] is None and one["codes_flagged"] == 0


def test_bit_packing_round_trip():
    rng = np.random.default_rng(2)
    for n in (0, 1, 63, 64, 65, 129, 1000):
        f = rng.random(n) < 0.5
        w = DC.pack_bits(f)
        assert w.dtype == np.uint64 and len(w) == (n + 63) // 64
        assert np.array_equal(DC.unpack_bits(w, n), f)
        for c in np.flatnonzero(f)[:5].tolist():
            assert (int(w[c // 64]) >> (c % 64)) & 1


# ---------------------------------------------------------------------------------------------- whole runs
OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "6", "model.lgb.learning_rate": "0.2"}
ON = "error.value_detectors.resident"
TARGETS = ["b", "c", "x", "k"]
C_PATTERN = r"^(x[.+]y|\(z\)|w\|v)$"


def _run_frame(n=240, seed=7):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 6, n)
    a = np.array(["a%d" % v for v in g], object)
    b = np.array(["b%d" % (v % 3) for v in g], object)
    c = np.array([["x.y", "x+y", "(z)", "w|v"][v % 4] for v in g], object)
    k = (g * 10 + rng.integers(0, 3, n)).astype(np.int64)
    x = g * 1.5 + np.round(rng.normal(0, 0.3, n), 2)
    b[[5, 17]] = ["b9", "bq"]                 # typos that occur once: flagged by the value domain, and the only rows of their class
    b[[40, 41]] = None
    b[60] = "b%d" % ((g[60] + 1) % 3)         # breaks a -> b
    c[[3, 99]] = ["x.z", None]
    x[[8, 120]] = [99.0, -50.0]
    x[[9, 200]] = np.nan
    return pd.DataFrame({"tid": np.arange(n), "a": a, "b": b, "c": c, "k": k, "x": x, "name": np.array(["n%04d" % i for i in range(n)], object)})


def _model(df, detectors, engine=None, on=False, targets=TARGETS, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setTargets(targets).setDiscreteThreshold(50).setErrorDetectors(detectors)
    for key, val in dict(OPTS, **opts).items():
        m = m.option(key, str(val))
    if on:
        m = m.option(ON, "true")
    m._engine_override = engine
    return m


def _sorted(df, repair_data):
    return df.sort_values(["tid"] if repair_data else ["tid", "attribute"]).reset_index(drop=True)


def _three_ways(monkeypatch, df, make_detectors, repair_data=False, expect_device=True, **kw):
    """(value-space frame, option-on model) -- after checking that the option-on run, the option-off run on the same engine and the
    value-space run give one frame."""
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df, make_detectors(), **kw).run(repair_data=repair_data)
    monkeypatch.delenv("REPAIR_RESIDENT")
    off = _model(df, make_detectors(), DetectEngine(), on=False, **kw)
    off_frame = off.run(repair_data=repair_data)
    assert off._last_detection_on_device is False
    before = DetectTable.calls
    fast = _model(df, make_detectors(), DetectEngine(), on=True, **kw)
    fast_frame = fast.run(repair_data=repair_data)
    assert fast._last_detection_on_device is expect_device
    assert (DetectTable.calls > before) == expect_device
    pd.testing.assert_frame_equal(_sorted(slow, repair_data), _sorted(off_frame, repair_data), check_exact=True)
    pd.testing.assert_frame_equal(_sorted(slow, repair_data), _sorted(fast_frame, repair_data), check_exact=True)
    return slow, fast


@pytest.fixture(scope="module")
def run_df():
    return _run_frame()


def test_option_is_registered_and_parsed():
    assert ON in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_value_detectors_resident) is False
    assert m.option(ON, "true")._get_option_value(*RepairModel._opt_value_detectors_resident) is True


ALONE = {
    "regex": lambda: [RegExErrorDetector("c", C_PATTERN)],
    "domain": lambda: [DomainValues("b", autofill=True, min_count_thres=4)],
    "outlier": lambda: [GaussianOutlierErrorDetector()],
}


@pytest.mark.parametrize("which", sorted(ALONE))
def test_each_detector_alone(oracle_backend, monkeypatch, run_df, which):
    slow, fast = _three_ways(monkeypatch, run_df, ALONE[which])
    assert len(slow) > 0
    info = fast._last_resident_info["value_detectors"]
    attr = dict(regex="c", domain="b", outlier="x")[which]
    d = {x["attribute"]: x for x in info}[attr]
    assert which in d["kinds"] and d["cells"] > 0 and d["codes_flagged"] > 0
    # repair_data without a NULL detector keeps the value-space path (NULL target cells of dirty rows would stay NULL), as before
    _three_ways(monkeypatch, run_df, ALONE[which], repair_data=True, expect_device=False)


@pytest.mark.parametrize("which", sorted(ALONE))
@pytest.mark.parametrize("repair_data", [False, True])
def test_each_detector_with_the_null_detector(oracle_backend, monkeypatch, run_df, which, repair_data):
    _three_ways(monkeypatch, run_df, lambda: [NullErrorDetector()] + ALONE[which](), repair_data=repair_data)


def _all_detectors():
    return [NullErrorDetector(), ConstraintErrorDetector(constraints="a->b"), RegExErrorDetector("c", C_PATTERN), RegExErrorDetector("k", "^[0-4]"),
            DomainValues("b", autofill=True, min_count_thres=4), DomainValues("c", values=["x.y", "x+y", "(z)", "w|v", "x.z"]),
            GaussianOutlierErrorDetector()]


@pytest.mark.parametrize("repair_data", [False, True])
def test_all_detectors_with_null_and_a_constraint(oracle_backend, monkeypatch, run_df, repair_data):
    slow, fast = _three_ways(monkeypatch, run_df, _all_detectors, repair_data=repair_data)
    info = {x["attribute"]: x for x in fast._last_resident_info["value_detectors"]}
    assert info["c"]["kinds"] == ["null", "regex", "domain"] and info["k"]["kinds"] == ["null", "regex", "outlier"]
    assert info["x"]["kinds"] == ["null", "outlier"]
    assert info["b"]["cells"] >= 4                                                # two typos and two NULLs at least


@pytest.mark.parametrize("repair_data", [False, True])
def test_with_the_cell_domain_analysis(oracle_backend, monkeypatch, run_df, repair_data):
    slow, fast = _three_ways(monkeypatch, run_df, _all_detectors, repair_data=repair_data,
                             **{"error.domain_analysis.enabled": "true", "error.domain_threshold_beta": "0.5"})
    assert "noisy_cells" in fast._last_resident_info and "value_detectors" in fast._last_resident_info


def test_a_typo_that_occurs_once_takes_the_re_encode_path(oracle_backend, monkeypatch, run_df, caplog):
    """`b9` and `bq` occur once each and the value domain flags them: their classes are left without rows once the cells are NULLed, so
    the dictionaries are rebuilt without them (pipeline.DeadClasses) -- and the detector summary survives that second pass."""
    import logging
    with caplog.at_level(logging.INFO):
        slow, fast = _three_ways(monkeypatch, run_df, lambda: [NullErrorDetector(), DomainValues("b", autofill=True, min_count_thres=4)])
    assert any("re-encoding the target dictionaries" in r.getMessage() for r in caplog.records)
    cur = set(slow.loc[slow["attribute"] == "b", "current_value"].dropna())
    assert {"b9", "bq"} <= cur
    d = {x["attribute"]: x for x in fast._last_resident_info["value_detectors"]}["b"]
    assert d["kinds"] == ["null", "domain"] and d["codes_flagged"] == 2 and d["cells"] == 4


class _MyRegex(RegExErrorDetector):
    pass


class _MyOutlier(GaussianOutlierErrorDetector):
    pass


FALLBACKS = {
    "regex_subclass": (lambda: [NullErrorDetector(), _MyRegex("c", C_PATTERN)], TARGETS),
    "outlier_subclass": (lambda: [NullErrorDetector(), _MyOutlier()], TARGETS),
    "lof": (lambda: [NullErrorDetector(), LOFOutlierErrorDetector()], TARGETS),
    "regex_on_a_non_discretizable_attribute": (lambda: [NullErrorDetector(), RegExErrorDetector("name", "^n0"), RegExErrorDetector("c", C_PATTERN)],
                                               TARGETS + ["name"]),
}


@pytest.mark.parametrize("which", sorted(FALLBACKS))
def test_fall_backs_keep_the_value_space_detection(oracle_backend, monkeypatch, run_df, which):
    make, targets = FALLBACKS[which]
    slow, _ = _three_ways(monkeypatch, run_df, make, expect_device=False, targets=targets)
    assert len(slow) > 0


def test_a_non_numeric_continuous_column_keeps_the_value_space_detection(run_df):
    m = _model(run_df, [NullErrorDetector(), GaussianOutlierErrorDetector()], DetectEngine(), on=True)
    assert m._device_detection_plan(run_df, ["x", "k"], False, False) is not None
    assert m._device_detection_plan(run_df, ["x", "c"], False, False) is None
    nullable = run_df.assign(k=run_df["k"].astype("Int64"))          # the pandas detector's masked comparison is its own to report
    assert _model(nullable, [NullErrorDetector(), GaussianOutlierErrorDetector()], DetectEngine(), on=True)._device_detection_plan(
        nullable, ["x", "k"], False, False) is None
    big = run_df.assign(k=run_df["k"] + 2 ** 60)
    assert _model(big, [NullErrorDetector(), GaussianOutlierErrorDetector()], DetectEngine(), on=True)._device_detection_plan(big, ["x", "k"], False, False) is None


def test_pipeline_detect_error_cells_merges_with_constraints():
    """`detect_error_cells` with descriptors: NULL detection rides in the `detect_cells` call and constraint cells merge as before."""
    from repair.pipeline import detect_error_cells
    rng = np.random.default_rng(3)
    codes = rng.integers(-1, 5, (4, 300)).astype(np.int32)
    t = DetectTable(codes, [5, 5, 5, 5])
    descs = [dict(col=2, null_is_error=False, keep_lo=1, keep_hi=3, flag_bits=None), dict(col=0, null_is_error=True, keep_lo=0, keep_hi=-1,
                                                                                         flag_bits=DC.pack_bits([0, 1, 0, 0, 1]))]
    r, c = detect_error_cells(t, [0, 2, 3], constraints=[([1], 2)], detect_nulls=True, value_detectors=descs)
    want = set()
    want |= {(0, i) for i in np.flatnonzero((codes[0] < 0) | (codes[0] == 1) | (codes[0] == 4))}
    want |= {(2, i) for i in np.flatnonzero((codes[2] < 0) | (codes[2] == 0) | (codes[2] == 4))}
    want |= {(3, i) for i in np.flatnonzero(codes[3] < 0)}
    vr, vc = t.detect_constraint([1], 2, cell_cols=[2])
    want |= set(zip(vc.tolist(), vr.tolist()))
    assert list(zip(c.tolist(), r.tolist())) == sorted(want)
    assert descs[0]["cells"] == int(((codes[2] < 0) | (codes[2] == 0) | (codes[2] == 4)).sum())
    # without NULL detection only the descriptors' own predicates count, and a target without any predicate is not read
    r, c = detect_error_cells(t, [0, 2, 3], detect_nulls=False, value_detectors=descs)
    assert set(c.tolist()) == {0, 2} and (codes[2][r[c == 2]] >= 0).all()
