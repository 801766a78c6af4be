"""CPU: `RepairModel.run(detect_errors_only=True)` on the resident table (`error.detect_only.resident`, `pipeline.detect_frame`) against the
value-space frame, on a CPU engine whose tables hold the cell set as tests/cellset_restatement.py states it; the refusals with their
reasons; and `pipeline.detect_error_cells(on_device=True)` against its host merge on random tables."""
import logging

import numpy as np
import pandas as pd
import pytest

from repair.errors import (ConstraintErrorDetector, DomainValues, ErrorModel, GaussianOutlierErrorDetector, LOFOutlierErrorDetector,
                           NullErrorDetector, RegExErrorDetector, ScikitLearnBackedErrorDetector)
from repair.model import RepairModel
from tests.cellset_restatement import CellsetEngine, CellsetTable, Refused
from tests.helpers import frame, load_golden
from tests.test_quality import HOSPITAL_TARGETS

ON = "error.detect_only.resident"
ROUTES = {"error.value_detectors.resident": "true", "error.constraints.resident": "true", "error.lof.resident": "true"}


def _hospital():
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    df["ZipCode"] = pd.to_numeric(df["ZipCode"], errors="coerce")            # one continuous attribute (typos become NULL)
    return df


def _adult():
    return frame(load_golden("adult")["input"])


def _hospital_detectors():
    return [NullErrorDetector(),
            ConstraintErrorDetector(constraints="t1&t2&EQ(t1.HospitalName,t2.HospitalName)&IQ(t1.City,t2.City);"
                                                "t1&t2&EQ(t1.MeasureCode,t2.MeasureCode)&IQ(t1.Condition,t2.Condition)&IQ(t1.Stateavg,t2.Stateavg)"),
            RegExErrorDetector("State", "^al$"), DomainValues("MeasureCode", autofill=True, min_count_thres=4), GaussianOutlierErrorDetector()]


def _adult_detectors():
    return [NullErrorDetector(), ConstraintErrorDetector(constraints=load_golden("adult")["constraints"].replace("\n", ";") + ";Sex->Relationship"),
            RegExErrorDetector("Age", r"^(\d|>)"), DomainValues("Country", values=["United-States"])]


FRAMES = {"hospital": (_hospital, _hospital_detectors, None, 80), "hospital_targets": (_hospital, _hospital_detectors, HOSPITAL_TARGETS + ["Sample"], 80),
          "adult": (_adult, _adult_detectors, None, 80)}


def _model(df, detectors, targets, thres, engine=None, on=False, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(thres).setErrorDetectors(detectors)
    if targets:
        m = m.setTargets(targets)
    for key, val in dict(ROUTES, **opts).items():
        m = m.option(key, str(val))
    if on:
        m = m.option(ON, "true")
    m._engine_override = engine
    return m


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


def _both(df, make, targets, thres, **opts):
    """(value-space frame, the model of the resident run, its frame, its engine)"""
    slow = _model(df, make(), targets, thres, **opts).run(detect_errors_only=True)
    eng = CellsetEngine()
    m = _model(df, make(), targets, thres, eng, on=True, **opts)
    fast = m.run(detect_errors_only=True)
    return slow, m, fast, eng


def _same(slow, fast):
    assert list(fast.columns) == list(slow.columns) == ["tid", "attribute", "current_value"]
    pd.testing.assert_frame_equal(_sorted(slow), _sorted(fast), check_exact=True)        # dtypes and None included


def test_option_is_registered_and_off_by_default():
    assert ON in RepairModel.option_keys
    assert RepairModel()._get_option_value(*RepairModel._opt_detect_only_resident) is False


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_detect_only_on_the_resident_table_equals_the_value_space_frame(name):
    make_df, make, targets, thres = FRAMES[name]
    df = make_df()
    sets = CellsetTable.set_calls
    slow, m, fast, eng = _both(df, make, targets, thres)
    assert m._last_detection_on_device is True and eng.uploads == 1 and CellsetTable.set_calls == sets + 1
    assert len(slow) > 0 and slow["current_value"].isna().any() and slow["current_value"].notna().any()
    _same(slow, fast)
    # the frame's own order: attribute in frame column order, then row position
    cols = [c for c in df.columns if c != "tid"]
    pos = pd.Series(np.arange(len(df)), index=df["tid"].to_numpy())
    key = [(cols.index(a), int(pos[t])) for t, a in zip(fast["tid"], fast["attribute"])]
    assert key == sorted(key)
    info = m._last_resident_info
    assert {"encode", "upload", "detect", "pipeline_wall"} <= set(info["times"])
    if name.startswith("hospital"):
        assert info["constraint_routes"] == ["fd", "dc"]
        kinds = {d["attribute"]: d["kinds"] for d in info["value_detectors"]}
        assert kinds["State"] == ["null", "regex"] and kinds["MeasureCode"] == ["null", "domain"] and kinds["ZipCode"] == ["null", "outlier"]
        by_attr = fast.groupby("attribute").size()
        assert {d["attribute"]: d["cells"] for d in info["value_detectors"] if d["attribute"] == "State"}["State"] <= by_attr["State"]
    else:
        assert info["constraint_routes"] == ["row_bits", "row_bits", "fd"]


def test_cells_of_non_discretizable_targets_stay():
    """`Sample` holds 333 distinct values (threshold 80): no model could repair it, and detect-only returns its cells all the same."""
    df = _hospital()
    slow, m, fast, _ = _both(df, _hospital_detectors, HOSPITAL_TARGETS + ["Sample"], 80)
    assert df["Sample"].nunique() > 80 and (fast["attribute"] == "Sample").sum() == df["Sample"].isna().sum() > 0
    assert m._last_detection_on_device is True
    # the repair run's plan detects in the candidates only and would have refused these NULL cells
    assert _model(df, _hospital_detectors(), HOSPITAL_TARGETS + ["Sample"], 80, CellsetEngine())._device_detection_plan(df, ["ZipCode"], False, False) is None


@pytest.mark.parametrize("name", ["hospital_targets", "adult"])
def test_with_the_cell_domain_analysis(name):
    make_df, make, targets, thres = FRAMES[name]
    df = make_df()
    opts = {"error.domain_analysis.enabled": "true", "error.domain_threshold_beta": "0.5"}
    slow_all = _model(df, make(), targets, thres).run(detect_errors_only=True)
    slow, m, fast, _ = _both(df, make, targets, thres, **opts)
    assert m._last_detection_on_device is True
    _same(slow, fast)
    info = m._last_resident_info
    assert info["noisy_cells"] == len(slow_all) and info["weak_cells"] == len(slow_all) - len(slow)      # weak cells leave
    assert info["weak_cells"] > 0 or name == "adult"                             # (none of adult's 46 cells is a weak label)
    vm = _model(df, make(), targets, thres, **opts)
    input_df, continuous = vm._check_input_table()
    _, _, pairwise, _ = ErrorModel("tid", vm.targets, thres, vm.error_detectors, None, vm.opts).detect(input_df, continuous)
    assert pairwise and info["pairwise_attr_stats"] == pairwise


def test_no_detectors_means_the_defaults():
    df = _hospital()
    slow, m, fast, eng = _both(df, list, HOSPITAL_TARGETS, 80)
    assert m._last_detection_on_device is True and eng.uploads == 1 and len(slow) > 0
    _same(slow, fast)
    assert {d["attribute"]: d["kinds"] for d in m._last_resident_info["value_detectors"]}["City"] == ["null", "domain"]
    # the defaults hold DomainValues: without the value detectors' option they stay with pandas
    off = _model(df, [], HOSPITAL_TARGETS, 80, CellsetEngine(), on=True, **{"error.value_detectors.resident": "false"})
    _same(slow, off.run(detect_errors_only=True))
    assert off._last_detection_on_device is False


def test_lof_on_the_resident_table():
    pytest.importorskip("sklearn")
    from tests.test_lof_codes_cpu import _run_frame
    df = _run_frame()
    make = lambda: [NullErrorDetector(), LOFOutlierErrorDetector()]  # noqa: E731
    slow, m, fast, _ = _both(df, make, ["b", "x"], 50)
    assert m._last_detection_on_device is True and {"99.0", "-50.0"} <= set(fast["current_value"].dropna())
    _same(slow, fast)


@pytest.mark.parametrize("opts", [{"model.lgb.boosting_type": "dart"}, {"model.max_training_column_num": "2"}], ids=["dart", "two_columns"])
def test_model_options_do_not_matter(opts):
    df = _adult()
    m = _model(df, _adult_detectors(), None, 80, CellsetEngine(), on=True, **opts)
    input_df, continuous = m._check_input_table()
    assert m._resident_plan(input_df, ["Sex"], continuous, {"Sex": 2}, False, False) is None        # the repair run would not qualify
    slow, m, fast, _ = _both(df, _adult_detectors, None, 80, **opts)
    assert m._last_detection_on_device is True
    _same(slow, fast)


class _NeverEngine(CellsetEngine):
    def upload(self, codes, n_codes):
        raise AssertionError("the engine was asked to upload")

    def upload_dictionaries(self, indices, remaps):
        raise AssertionError("the engine was asked to upload")


def test_option_off_never_touches_the_engine():
    df = _adult()
    slow = _model(df, _adult_detectors(), None, 80).run(detect_errors_only=True)
    m = _model(df, _adult_detectors(), None, 80, _NeverEngine(), on=False)
    _same(slow, m.run(detect_errors_only=True))
    assert m._last_detection_on_device is False


class _RefusingTable(CellsetTable):
    def detect_row_bits(self, cols, bits, cell_cols=(), fetch=True):
        raise Refused("rgbm_table_detect_row_bits: refused by this table")


class _RefusingEngine(CellsetEngine):
    table_cls = _RefusingTable


class _MyDetector(ScikitLearnBackedErrorDetector):
    pass


def _lof():
    from sklearn.neighbors import LocalOutlierFactor
    return LocalOutlierFactor(novelty=False)


def _given_cells(m):
    return m.setErrorCells(pd.DataFrame({"tid": [3, 5], "attribute": ["Sex", "Age"]}))


REFUSALS = {
    "given_error_cells": (lambda: _adult_detectors(), _given_cells, CellsetEngine, "error cells are given"),
    "a_detector_with_targets": (lambda: [NullErrorDetector(), ConstraintErrorDetector(constraints="Sex->Relationship", targets=["Sex"])], None, CellsetEngine,
                                "has targets of its own"),
    "a_scikit_learn_detector": (lambda: [NullErrorDetector(), _MyDetector(_lof)],
                                None, CellsetEngine, "is not a detector the resident table restates"),
    "a_constraint_that_does_not_lower": (lambda: [NullErrorDetector(), ConstraintErrorDetector(constraints="t1&t2&EQ(t1.Sex,t2.Relationship)&IQ(t1.Age,t2.Age)")],
                                         None, CellsetEngine, "does not lower"),
    "a_refusing_engine": (lambda: _adult_detectors(), None, _RefusingEngine, "refused by this table"),
    "no_engine": (lambda: _adult_detectors(), None, None, "no engine for the resident table"),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals_return_the_value_space_frame_and_say_why(which, caplog, monkeypatch):
    if which == "a_scikit_learn_detector":
        pytest.importorskip("sklearn")
    make, extra, engine_cls, reason = REFUSALS[which]
    df = _adult()
    slow_m = _model(df, make(), None, 80)
    slow = (extra(slow_m) if extra else slow_m).run(detect_errors_only=True)
    if engine_cls is None:
        monkeypatch.setenv("REPAIR_RESIDENT", "0")
    m = _model(df, make(), None, 80, engine_cls() if engine_cls else None, on=True)
    m = extra(m) if extra else m
    with caplog.at_level(logging.INFO):
        fast = m.run(detect_errors_only=True)
    assert m._last_detection_on_device is False
    assert any("not taken" in r.getMessage() and reason in r.getMessage() for r in caplog.records), [r.getMessage() for r in caplog.records]
    _same(slow, fast)


def test_the_empty_result():
    df = _adult().dropna().reset_index(drop=True)
    slow, m, fast, eng = _both(df, lambda: [NullErrorDetector()], None, 80)
    assert m._last_detection_on_device is True and eng.uploads == 1
    assert len(slow) == 0 and len(fast) == 0
    pd.testing.assert_frame_equal(slow, fast, check_exact=True)                  # columns and dtypes of the value-space path


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_detect_error_cells_on_device_equals_the_host_merge(seed):
    """Overlapping detectors, given cells, cells outside the targets."""
    from repair import detect_codes as DC
    from repair.pipeline import detect_error_cells
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    codes = rng.integers(-1, 5, (6, n)).astype(np.int32)
    n_codes = [5] * 6
    targets = [4, 0, 2, 3][:int(rng.integers(1, 5))]
    given = (rng.integers(-2, n + 2, 50), rng.integers(0, 6, 50).astype(np.int32))            # rows outside the table, columns outside the targets

    def descs():
        return [dict(col=2, null_is_error=False, keep_lo=1, keep_hi=3, flag_bits=None),
                dict(col=0, null_is_error=True, keep_lo=0, keep_hi=-1, flag_bits=DC.pack_bits([0, 1, 0, 0, 1])),
                dict(col=5, null_is_error=True, keep_lo=0, keep_hi=-1, flag_bits=None)]       # not a target
    cons = [([1], 2), ([5], 0), dict(kind="dc", preds=[("EQ", 1, 1, None, None), ("IQ", 2, 2, None, None), ("GT", 3, 3, None, None)], refs=[1, 2, 3, 5]),
            dict(kind="dc_scan", preds=[("EQ", 1, 1, None, None), ("LT", 4, 4, None, None)], refs=[1, 4])]
    for kw in (dict(detect_nulls=True), dict(detect_nulls=True, value_detectors=True), dict(detect_nulls=False, value_detectors=True, error_cells=given),
               dict(detect_nulls=True, constraints=cons, error_cells=given), dict(detect_nulls=False, constraints=cons, value_detectors=True),
               dict(detect_nulls=False)):
        host_d = descs() if kw.get("value_detectors") else None
        dev_d = descs() if kw.get("value_detectors") else None
        t = CellsetTable(codes, n_codes)
        r, c = detect_error_cells(CellsetTable(codes, n_codes), targets, **dict(kw, value_detectors=host_d))
        sets = CellsetTable.set_calls
        r2, c2, v2 = detect_error_cells(t, targets, on_device=True, **dict(kw, value_detectors=dev_d))
        assert CellsetTable.set_calls == sets + 1 and t._set is None                                                 # opened once, closed
        assert np.array_equal(r, r2) and np.array_equal(c, c2) and r2.dtype == np.int64 and c2.dtype == np.int32, kw
        assert np.array_equal(v2, codes[c.astype(np.int64), r]) and v2.dtype == np.int32
        if host_d:
            assert [d.get("cells") for d in host_d] == [d.get("cells") for d in dev_d]
    # a table without the methods: today's path, and the codes read from it
    from tests.test_dc_scan_cpu import ScanTable as Plain
    assert not hasattr(Plain, "cellset_open")
    r3, c3, v3 = detect_error_cells(Plain(codes, n_codes), targets, constraints=cons, detect_nulls=True, on_device=True)
    r, c = detect_error_cells(Plain(codes, n_codes), targets, constraints=cons, detect_nulls=True)
    assert np.array_equal(r, r3) and np.array_equal(c, c3) and np.array_equal(v3, codes[c.astype(np.int64), r])
