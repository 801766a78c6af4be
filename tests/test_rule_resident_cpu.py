"""CPU: `RepairModel.setRepairByRules(True)` on the resident pipeline behind the option `model.rule.resident`: FD rule models, constant
models and nearest-value merges as steps of the resident run.

The job logic runs on a CPU engine (the oracle engine of tests/helpers plus the numpy restatements of rgbm_table_fd_map,
rgbm_table_rule_fill and rgbm_nearest_values in tests/rule_restatements.py), the value-space path on the oracle estimator backend:
both sides share the oracle's arithmetic, so the frames must be equal cell for cell."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from repair.costs import Levenshtein, UserDefinedUpdateCostFunction
from repair.errors import ConstraintErrorDetector, NullErrorDetector, RegExErrorDetector
from repair.model import RepairModel
from tests import rule_restatements as R
from tests.helpers import GOLDEN, OracleEngine


class RuleOracleEngine(OracleEngine):
    """OracleEngine with the three entries of the rule-based repairs restated in numpy."""

    class _Table(OracleEngine._Table):
        def gather_rows(self, rows):
            return RuleOracleEngine._Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)

        def fd_map(self, x, y):
            return R.fd_map(self.codes, self.n_codes, x, y)

        def rule_fill(self, y, x, lut, row_begin=0, n_rows=None, want_labels=True):
            return R.rule_fill(self.codes, y, x, lut, row_begin, self.n - row_begin if n_rows is None else n_rows)

    def upload(self, codes, n_codes):
        return RuleOracleEngine._Table(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return RuleOracleEngine._Table(t.codes, t.n_codes)

    def nearest_values(self, a, b, threshold, cost=None):
        return R.nearest(cost, threshold) if cost is not None else R.nearest_strings(a, b, threshold)


OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2"}


def _model(df, cells=None, detectors=None, cf=None, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setRepairByRules(True)
    if cells is not None:
        m = m.setErrorCells(cells)
    if detectors is not None:
        m = m.setErrorDetectors(detectors)
    if cf is not None:
        m = m.setUpdateCostFunction(cf).option("model.rule.repair_by_nearest_values.disabled", "")
    for k, v in dict(OPTS, **opts).items():
        m = m.option(k, str(v))
    return m


def _both_paths(make, **flags):
    """(value-space frame, resident frame, resident model) of the same run."""
    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        a = make().run(**flags)
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    fast = make().option("model.rule.resident", "true")
    fast._engine_override = RuleOracleEngine()
    b = fast.run(**flags)
    assert getattr(fast, "_last_resident_info", None) is not None, "the run did not take the resident path"
    return a, b, fast


def _sorted(df, repair_data=False):
    return df.sort_values(["tid"] if repair_data else ["tid", "attribute"]).reset_index(drop=True)


def _rows(df):
    return [[None if v is None or (isinstance(v, float) and np.isnan(v)) else v for v in r]
            for r in _sorted(df)[["tid", "attribute", "current_value", "repaired"]].to_numpy(dtype=object).tolist()]


def _fd_detectors():
    return [NullErrorDetector(), ConstraintErrorDetector(constraints=R.FD_CONSTRAINTS)]


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "rule_repairs.json"), encoding="utf-8") as f:
        return json.load(f)


def test_option_is_registered_and_parsed():
    assert "model.rule.resident" in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_rule_resident) is False
    assert m.option("model.rule.resident", "true")._get_option_value(*RepairModel._opt_rule_resident) is True


def test_reference_rows_of_repair_by_functional_deps(oracle_backend, golden, tmp_path):
    g = golden["functional_deps"]
    df = pd.DataFrame(g["rows"], columns=g["columns"])
    cells = pd.DataFrame(g["error_cells"], columns=["tid", "attribute"])
    path = tmp_path / "constraints.txt"
    path.write_text(g["constraint"])
    a, b, fast = _both_paths(lambda: _model(df, cells, [NullErrorDetector(), ConstraintErrorDetector(str(path))], **g["options"]))
    assert _rows(a) == g["expected"] and _rows(b) == g["expected"]
    last = _sorted(b).iloc[-1]
    assert last["tid"] == 6 and last["repaired"] is None
    assert [(s["target"], s["kind"], s["x"]) for s in fast._last_resident_info["rule_steps"]] == [("y", "fd", "x")]


def test_reference_rows_of_repair_by_nearest_values(oracle_backend, golden):
    g = golden["nearest_values"]
    df = pd.DataFrame(g["rows"], columns=g["columns"])
    cells = pd.DataFrame(g["error_cells"], columns=["tid", "attribute"])
    make = lambda: _model(df, cells, cf=Levenshtein(targets=g["cost_targets"]), **g["options"])  # noqa: E731
    a, b, fast = _both_paths(make)
    assert _rows(a) == g["expected"] and _rows(b) == g["expected"]
    assert fast._last_resident_info["nearest_values"] == {"v0": 3, "v1": 3}
    a, b, _ = _both_paths(lambda: make().setTargets(g["targets_run"]))
    assert _rows(a) == g["expected_targets_run"] and _rows(b) == g["expected_targets_run"]


@pytest.fixture(scope="module")
def fd_data():
    return R.fd_frame()


@pytest.mark.parametrize("repair_data", [False, True])
def test_fd_chain_equals_the_value_space_path(oracle_backend, fd_data, repair_data):
    """c0 -> c1 -> c2 with given error cells: c0 is repaired by its model first, then c1 from c0, then c2 from c1."""
    df, cells = fd_data
    a, b, fast = _both_paths(lambda: _model(df, cells, _fd_detectors()), repair_data=repair_data)
    pd.testing.assert_frame_equal(_sorted(a, repair_data), _sorted(b, repair_data), check_exact=True)
    steps = {s["target"]: s for s in fast._last_resident_info["rule_steps"]}
    assert [s["target"] for s in fast._last_resident_info["rule_steps"]] == ["c1", "c2"]          # the chain order
    assert steps["c1"]["kind"] == "fd" and steps["c1"]["x"] == "c0" and steps["c2"]["x"] == "c1"
    assert steps["c1"]["mapped"] > 0 and steps["c1"]["conflict"] > 0 and steps["c1"]["unseen"] > 0
    assert steps["c1"]["mapped"] + steps["c1"]["conflict"] + steps["c1"]["unseen"] + steps["c1"]["null_source"] == steps["c1"]["cells"]
    if not repair_data:
        c1 = b[b["attribute"] == "c1"]
        assert int(c1["repaired"].isna().sum()) == steps["c1"]["conflict"] + steps["c1"]["unseen"] + steps["c1"]["null_source"]


@pytest.mark.parametrize("repair_data", [False, True])
def test_fd_chain_with_device_detection_equals_the_value_space_path(oracle_backend, repair_data):
    """The same frame with the cells DETECTED (NULL + constraint detectors): the device-detection entry of the resident path."""
    df = R.fd_detect_frame()
    a, b, fast = _both_paths(lambda: _model(df, None, _fd_detectors()), repair_data=repair_data)
    assert fast._last_detection_on_device
    pd.testing.assert_frame_equal(_sorted(a, repair_data), _sorted(b, repair_data), check_exact=True)
    steps = {s["target"]: s for s in fast._last_resident_info["rule_steps"]}
    assert steps["c1"]["kind"] == "fd" and steps["c2"]["kind"] == "fd" and steps["c1"]["cells"] > 0


def _constant_frame():
    rng = np.random.default_rng(11)
    n = 400
    one = np.array(["x", "y", "z"], object)[rng.choice(3, n, p=[0.8, 0.1, 0.1])]
    df = pd.DataFrame({"tid": np.arange(n), "one": one, "none": np.array(["p", "q"], object)[rng.integers(0, 2, n)],
                       "f0": ["u%d" % v for v in rng.integers(0, 4, n)], "f1": ["w%d" % v for v in rng.integers(0, 3, n)],
                       "t": ["k%d" % v for v in rng.integers(0, 3, n)]})
    cells = [(int(r), "one") for r in np.flatnonzero(one != "x")] + [(int(r), "none") for r in range(n)] + \
            [(int(r), "t") for r in rng.choice(n, 30, replace=False)]
    return df, pd.DataFrame(cells, columns=["tid", "attribute"])


@pytest.mark.parametrize("repair_data", [False, True])
def test_constant_steps_equal_the_value_space_path(oracle_backend, repair_data):
    """`one`: its error cells hold every y and z, one class is left (PoorModel('x')); `none`: every cell is an error cell (PoorModel(None))."""
    df, cells = _constant_frame()
    a, b, fast = _both_paths(lambda: _model(df, cells), repair_data=repair_data)
    pd.testing.assert_frame_equal(_sorted(a, repair_data), _sorted(b, repair_data), check_exact=True)
    kinds = {s["target"]: (s["kind"], s["mapped"]) for s in fast._last_resident_info["rule_steps"]}
    assert kinds["one"][0] == "constant" and kinds["one"][1] > 0 and kinds["none"] == ("constant", 0)
    if not repair_data:
        assert set(b[b["attribute"] == "one"]["repaired"]) == {"x"} and b[b["attribute"] == "none"]["repaired"].isna().all()


def _nearest_frame():
    """`w`: live values abcd / abxx / zzzzzz.  Current values: 'abcz' and 'abcc' (1 from abcd, 2 from abxx: a unique minimum),
    'abxd' (1 from abcd and 1 from abxx: a tie), 'abxxyy' (2 from abxx = the threshold, 4 from abcd), 'zzz' (3 from zzzzzz: above it),
    '' and NULL (no merge).  `one`: a single live value 'solo' (a one-value domain).  `f*`: features."""
    rng = np.random.default_rng(5)
    n = 300
    w = np.array(["abcd", "abxx", "zzzzzz"], object)[rng.integers(0, 3, n)]
    one = np.array(["solo"] * n, object)
    typos = ["abcz", "abcc", "abxd", "abxxyy", "zzz", "", None, "abcz"]
    cells = []
    for i, v in enumerate(typos * 3):
        w[i] = v
        cells.append((i, "w"))
    for i, v in enumerate(["sol", "sxxo", "so", "solo!"]):
        one[40 + i] = v
        cells.append((40 + i, "one"))
    df = pd.DataFrame({"tid": np.arange(n), "w": w, "one": one, "f0": ["u%d" % v for v in rng.integers(0, 4, n)],
                       "f1": ["w%d" % v for v in rng.integers(0, 3, n)]})
    return df, pd.DataFrame(cells, columns=["tid", "attribute"])


def _user_cost(x, y):
    if x[0] != y[0] and len(y) > 1:
        raise ValueError("no cost between values of different initials")     # compute() turns it into None
    return float(abs(len(x) - len(y)) + sum(p != q for p, q in zip(x, y)))


@pytest.mark.parametrize("repair_data", [False, True])
@pytest.mark.parametrize("cf", ["lev", "lev_w", "user"])
def test_nearest_values_equal_the_value_space_path(oracle_backend, cf, repair_data):
    df, cells = _nearest_frame()
    make_cf = {"lev": Levenshtein, "lev_w": lambda: Levenshtein(targets=["w"]), "user": lambda: UserDefinedUpdateCostFunction(_user_cost)}[cf]
    a, b, fast = _both_paths(lambda: _model(df, cells, cf=make_cf(), **{"model.rule.merge_threshold": "2.0"}), repair_data=repair_data)
    pd.testing.assert_frame_equal(_sorted(a, repair_data), _sorted(b, repair_data), check_exact=True)
    info = fast._last_resident_info
    merged = info["merged_cells"]
    assert info["nearest_values"]["w"] == len(merged[merged["attribute"] == "w"]) > 0
    if cf == "lev":
        got = {(c, r) for c, r in zip(merged["current_value"], merged["repaired"])}
        assert got == {("abcz", "abcd"), ("abcc", "abcd"), ("abxxyy", "abxx"), ("sol", "solo"), ("sxxo", "solo"), ("so", "solo"), ("solo!", "solo")}
    if cf == "lev_w":
        assert "one" not in info["nearest_values"]
    if not repair_data:
        # a merged cell is not repaired by a model as well: it occurs once, with the merged value
        keys = list(zip(b["tid"], b["attribute"]))
        assert len(keys) == len(set(keys))
        got = b.merge(merged, on=["tid", "attribute"], suffixes=("", "_merged"))
        assert len(got) == len(merged) and (got["repaired"] == got["repaired_merged"]).all()


def test_without_the_option_nothing_changes(oracle_backend, fd_data):
    df, cells = fd_data
    m = _model(df, cells, _fd_detectors())
    m._engine_override = RuleOracleEngine()
    m.run()
    assert getattr(m, "_last_resident_info", None) is None
    m = _model(df, cells, _fd_detectors()).option("model.rule.resident", "false")
    m._engine_override = RuleOracleEngine()
    m.run()
    assert getattr(m, "_last_resident_info", None) is None


def test_excluded_cases_stay_on_the_value_space_path(oracle_backend, fd_data):
    df, cells = fd_data

    def ran_resident(m, **flags):
        m = m.option("model.rule.resident", "true")
        m._engine_override = RuleOracleEngine()
        m.run(**flags)
        return getattr(m, "_last_resident_info", None) is not None

    assert ran_resident(_model(df, cells, _fd_detectors()))
    # the probability modes combined with rules
    assert not ran_resident(_model(df, cells, _fd_detectors()).option("repair.pmf.resident", "true"), compute_repair_candidate_prob=True)
    # regex-structure repair
    assert not ran_resident(_model(df, cells, _fd_detectors() + [RegExErrorDetector("c5", "f[0-9]")], **{"model.rule.repair_by_regex.disabled": ""}))
    # an FD model for a continuous y
    num = df.assign(c1=df["c1"].map(lambda v: None if v is None else float(v[1:])))
    assert not ran_resident(_model(num, cells, _fd_detectors()))
    # a cycle among the FD sources: the value-space path keeps its assertion
    cyc = [NullErrorDetector(), ConstraintErrorDetector(constraints=R.FD_CONSTRAINTS + ";t1&t2&EQ(t1.c2,t2.c2)&IQ(t1.c0,t2.c0)")]
    m = _model(df, cells, cyc).option("model.rule.resident", "true")
    m._engine_override = RuleOracleEngine()
    with pytest.raises(AssertionError):
        m.run()
    assert getattr(m, "_last_resident_info", None) is None


def _hospital_model():
    from tests.helpers import frame, load_golden
    from tests.test_quality import HOSPITAL_TARGETS
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400).setTargets(HOSPITAL_TARGETS).setRepairByRules(True).setErrorDetectors(
        [NullErrorDetector(), ConstraintErrorDetector(constraints=";".join(ln for ln in g["constraints"].splitlines() if ln.strip()))])
    for k, v in dict(OPTS, **{"model.lgb.n_estimators": "10"}).items():
        m = m.option(k, v)
    return m


def test_hospital_with_its_constraints_equals_the_value_space_path(oracle_backend):
    """BASELINE.json configs[1] as the reference uses it: denial constraints detect the cells and give the FD rule models."""
    a, b, fast = _both_paths(_hospital_model)
    assert fast._last_detection_on_device and len(a) > 1000
    pd.testing.assert_frame_equal(_sorted(a), _sorted(b), check_exact=True)
    steps = fast._last_resident_info["rule_steps"]
    assert len(steps) >= 4 and all(s["kind"] == "fd" for s in steps) and sum(s["mapped"] for s in steps) > 0


def test_restatements_against_the_python_definitions():
    """The numpy restatements the CPU engine runs on equal the value-space definitions they stand for."""
    rng = np.random.default_rng(2)
    codes = rng.integers(-1, 6, (2, 500)).astype(np.int32)
    codes[1] = np.where(codes[0] % 2 == 0, codes[0] // 2, codes[1])
    df = pd.DataFrame({"x": codes[0], "y": codes[1]}).astype(object).where(lambda d: d >= 0, None)
    fm = RepairModel()._build_rule_model(df, "x", "y").fd_map
    want = np.array([fm.get(k, -1) for k in range(6)], np.int32)
    assert np.array_equal(R.fd_map(codes, [6, 6], 0, 1), want)
    before = codes.copy()
    pred = R.rule_fill(codes, 1, 0, want, 100, 300)
    assert np.array_equal(codes[1, :100], before[1, :100]) and np.array_equal(codes[1, 400:], before[1, 400:])
    x = before[0, 100:400]
    assert np.array_equal(pred, np.where(x >= 0, want[np.maximum(x, 0)], -1))
    assert np.array_equal(codes[1, 100:400], np.where((before[1, 100:400] < 0) & (pred >= 0), pred, before[1, 100:400]))
    cost = np.array([[1.0, 2.0, 3.0], [2.0, 2.0, 5.0], [np.nan, 2.0, 2.5], [np.nan, np.nan, np.nan], [3.0, np.nan, 2.5]])
    assert R.nearest(cost, 2.0).tolist() == [0, -1, 1, -1, -1]
    assert R.nearest_strings(["abc", "xyz"], ["abd", "abc", "xbz"], 1.0).tolist() == [1, 2]
    assert R.nearest_strings(["abc"], [], 1.0).tolist() == [-1]
