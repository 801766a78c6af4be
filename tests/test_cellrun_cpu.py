"""CPU: a resident REPAIR run whose error cells stay in the table's cell set from detection through the null-out (`error.cells.resident`,
`pipeline._cells_on_set`) against the same run on the host route -- the frame and the details exactly -- on a CPU engine whose tables hold
the set as tests/cellrun_restatement.py states it; the call record of such a run; the fall-backs with their reasons; and every case
generator of tests/test_cellrun_gpu.py held to its purpose on the restatement alone."""
import logging

import numpy as np
import pandas as pd
import pytest

from repair.costs import Levenshtein
from repair.errors import ConstraintErrorDetector, DomainValues, GaussianOutlierErrorDetector, NullErrorDetector, RegExErrorDetector
from repair.model import RepairModel
from tests import cellrun_cases as X
from tests import rule_restatements as R
from tests.cellrun_restatement import CellrunEngine, CellrunTable, OldEngine, RecordingTable, Refused
from tests.helpers import load_golden
from tests.test_detect_only_cpu import ROUTES, _adult, _hospital
from tests.test_quality import HOSPITAL_TARGETS
from tests.test_rule_resident_cpu import RuleOracleEngine, _nearest_frame
from tests.test_value_detectors_cpu import _run_frame

ON = "error.cells.resident"
OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2"}
ANALYSIS = {"error.domain_analysis.enabled": "true", "error.domain_threshold_beta": "0.5"}
SAME_DETAILS = ("pairwise_attr_stats", "noisy_cells", "weak_cells", "value_detectors")


class _RunTable(RecordingTable):
    """The recording table with the two rule entries, so that runs with rule-based repairs stay on the resident path."""

    def gather_rows(self, rows):
        return RuleOracleEngine._Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)

    def fd_map(self, x, y):
        return R.fd_map(self.codes, self.n_codes, x, y)

    def rule_fill(self, y, x, lut, row_begin=0, n_rows=None, want_labels=True):
        return R.rule_fill(self.codes, y, x, lut, row_begin, self.n - row_begin if n_rows is None else n_rows)


class _RunEngine(CellrunEngine):
    table_cls = _RunTable

    def nearest_values(self, a, b, threshold, cost=None):
        return R.nearest(cost, threshold) if cost is not None else R.nearest_strings(a, b, threshold)


def _hospital_detectors():
    """Two denial constraints, a pattern that keeps the two real states (`al`, `ak`) and flags the typos, a value domain filled from the
    frequent measure codes, and the outlier detector (for the continuous `ZipCode`)."""
    return [NullErrorDetector(),
            ConstraintErrorDetector(constraints="t1&t2&EQ(t1.HospitalName,t2.HospitalName)&IQ(t1.City,t2.City);"
                                                "t1&t2&EQ(t1.MeasureCode,t2.MeasureCode)&IQ(t1.Condition,t2.Condition)&IQ(t1.Stateavg,t2.Stateavg)"),
            RegExErrorDetector("State", "^a[lk]$"), DomainValues("MeasureCode", autofill=True, min_count_thres=4), GaussianOutlierErrorDetector()]


def _adult_detectors():
    """The golden file's two single-tuple statements, a pattern on `Age` and a value domain on `Sex`.  (The detect-only tests add
    `Sex->Relationship` and a one-value domain of `Country`: on these 20 rows they leave `Relationship` without a class and `Country` with
    one, and no model could be trained.)"""
    return [NullErrorDetector(), ConstraintErrorDetector(constraints=load_golden("adult")["constraints"].replace("\n", ";")),
            RegExErrorDetector("Age", r"^(\d|>)"), DomainValues("Sex", values=["Male", "Female"])]


def _model(df, detectors, targets, thres, engine, on, cells=None, rules=False, cf=None, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(thres)
    if detectors is not None:
        m = m.setErrorDetectors(detectors)
    if targets:
        m = m.setTargets(targets)
    if cells is not None:
        m = m.setErrorCells(cells)
    if rules:
        m = m.setRepairByRules(True).option("model.rule.resident", "true")
    if cf is not None:
        m = m.setUpdateCostFunction(cf).option("model.rule.repair_by_nearest_values.disabled", "")
    for key, val in dict(OPTS, **dict(ROUTES, **opts)).items():
        m = m.option(key, str(val))
    if on:
        m = m.option(ON, "true")
    m._engine_override = engine
    return m


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


def _on_and_off(make):
    """(the model of the option-off run, its frame, the option-on model, its frame, its engine): both on the resident path."""
    off = make(_RunEngine(), False)
    off_frame = off.run()
    assert off._last_resident_info is not None and "cells_route" not in off._last_resident_info
    eng = _RunEngine()
    on = make(eng, True)
    on_frame = on.run()
    assert on._last_resident_info is not None and on._last_detection_on_device is off._last_detection_on_device
    pd.testing.assert_frame_equal(_sorted(off_frame), _sorted(on_frame), check_exact=True)
    for key in SAME_DETAILS:
        assert on._last_resident_info.get(key) == off._last_resident_info.get(key), key
    return off, off_frame, on, on_frame, eng


def _set_route(on, eng, given=0, nearest=False):
    """The call record of a run on the set's route; `given`: the passes whose cells are given (by the user, or by the first pass)."""
    assert on._last_resident_info["cells_route"] == "set"
    calls = eng.calls
    assert not {"read_cells", "null_cells", "cell_domains"} & set(calls), calls
    assert ("rows_of_cells" in calls) == nearest and ("write_cells" in calls) == nearest
    assert eng.cell_uploads().count("cellset_add_cells") == given <= calls.count("cellset_open") == eng.uploads
    assert calls.count("cellset_null") == calls.count("cellset_open") == calls.count("cellset_close") >= 1
    assert calls.count("cellset_rows") == (0 if nearest else calls.count("cellset_open"))


def test_option_is_registered_and_off_by_default():
    assert ON in RepairModel.option_keys
    assert RepairModel()._get_option_value(*RepairModel._opt_cells_resident) is False
    assert RepairModel().option(ON, "true")._get_option_value(*RepairModel._opt_cells_resident) is True


FRAMES = {"hospital": (_hospital, _hospital_detectors, HOSPITAL_TARGETS, 80), "adult": (_adult, _adult_detectors, None, 80)}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_detected_cells_with_constraints_value_detectors_and_the_analysis(oracle_backend, name):
    make_df, make, targets, thres = FRAMES[name]
    df = make_df()
    off, frame, on, _, eng = _on_and_off(lambda e, flag: _model(df, make(), targets, thres, e, flag, **ANALYSIS))
    assert on._last_detection_on_device is True and len(frame) > 0 and eng.uploads >= 1
    info = on._last_resident_info
    assert info["noisy_cells"] >= len(frame) and "pairwise_attr_stats" in info and info["value_detectors"]
    assert info["weak_cells"] > 0 or name == "adult"
    second_pass = name == "hospital"                  # some measure codes occur in error cells only: the dictionaries are rebuilt
    assert eng.uploads == (2 if second_pass else 1)
    _set_route(on, eng, given=1 if second_pass else 0)
    # the pruning ran in the set: once per examined target, after ONE pair-count pass, between a count-only and a fetching emit
    first = eng.calls[:eng.calls.index("cellset_null")]
    host_calls = off._engine_override.calls
    assert first.count("pair_counts") == 1 and first.count("cellset_drop_weak") == host_calls.count("cell_domains")     # one per examined target
    assert first.count("cellset_drop_weak") >= 1 or name == "adult"                  # (no attribute of adult's 20 rows is correlated enough)
    assert all(first.index("pair_counts") < i < len(first) - 1 for i, c in enumerate(first) if c == "cellset_drop_weak") and first[-1] == "cellset_emit"
    assert {"read_cells", "null_cells", "rows_of_cells"} <= set(host_calls)          # what the host route sends up


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_given_error_cells(oracle_backend, name):
    make_df, make, targets, thres = FRAMES[name]
    df = make_df()
    cols = targets or [c for c in df.columns if c != "tid"]
    rng = np.random.default_rng(5)
    cells = pd.DataFrame({"tid": df["tid"].to_numpy()[rng.integers(0, len(df), 40)], "attribute": np.asarray(cols, object)[rng.integers(0, 3, 40)]})
    cells = cells.drop_duplicates().sample(frac=1.0, random_state=1).reset_index(drop=True)          # in no order
    off, frame, on, _, eng = _on_and_off(lambda e, flag: _model(df, make(), targets, thres, e, flag, cells=cells, **ANALYSIS))
    assert on._last_detection_on_device is False and 0 < len(frame) <= len(cells)
    _set_route(on, eng, given=1)
    assert eng.uploads == 1 and eng.cell_uploads() == ["cellset_add_cells"]          # the error cells went up once


def test_the_second_pass_of_dead_classes(oracle_backend, caplog):
    """`b9` and `bq` occur once and the value domain flags them: the dictionaries are rebuilt and the second pass gets its cells as given."""
    df = _run_frame()
    make = lambda: [NullErrorDetector(), DomainValues("b", autofill=True, min_count_thres=4)]  # noqa: E731
    with caplog.at_level(logging.INFO):
        off, frame, on, _, eng = _on_and_off(lambda e, flag: _model(df, make(), ["b", "c", "x", "k"], 50, e, flag))
    assert sum("re-encoding the target dictionaries" in r.getMessage() for r in caplog.records) == 2
    assert {"b9", "bq"} <= set(frame.loc[frame["attribute"] == "b", "current_value"].dropna())
    assert eng.uploads == 2 and eng.calls.count("cellset_open") == 2
    _set_route(on, eng, given=1)
    assert eng.cell_uploads() == ["cellset_add_cells"]                               # the second pass alone sends cells: the first detected its own


def test_nearest_value_merges(oracle_backend):
    df, cells = _nearest_frame()
    off, frame, on, _, eng = _on_and_off(lambda e, flag: _model(df, None, None, 80, e, flag, cells=cells, rules=True, cf=Levenshtein(),
                                                                **{"model.rule.merge_threshold": "2.0"}))
    merged, merged_off = on._last_resident_info["merged_cells"], off._last_resident_info["merged_cells"]
    assert len(merged) > 0
    pd.testing.assert_frame_equal(_sorted(merged), _sorted(merged_off), check_exact=True)
    assert on._last_resident_info["nearest_values"] == off._last_resident_info["nearest_values"]
    _set_route(on, eng, given=1, nearest=True)
    # the null-out came from the set; only the dirty rows of the cells that were not merged are looked up
    assert eng.calls.index("cellset_null") < eng.calls.index("write_cells") < eng.calls.index("rows_of_cells")


def test_an_engine_without_the_entries_takes_the_host_route(oracle_backend, caplog):
    df = _adult()
    with caplog.at_level(logging.INFO):
        m = _model(df, _adult_detectors(), None, 80, OldEngine(), True, **ANALYSIS)
        frame = m.run()
    want = _model(df, _adult_detectors(), None, 80, _RunEngine(), False, **ANALYSIS).run()
    pd.testing.assert_frame_equal(_sorted(want), _sorted(frame), check_exact=True)
    assert m._last_resident_info["cells_route"] == "host"
    said = [r.getMessage() for r in caplog.records if "route is not taken" in r.getMessage()]
    assert said and "cellset_add_cells" in said[0] and "cellset_rows" in said[0], said


def test_a_world_of_two_ranks_takes_the_host_route(monkeypatch, caplog):
    from repair import dist, pipeline
    codes, n_codes, _ = X.table(300, 2)
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    assert "2 ranks" in pipeline.set_route_refusal(CellrunTable(codes, n_codes), [1, 2])
    tab = RecordingTable(codes, n_codes)
    with caplog.at_level(logging.INFO):
        res = pipeline.repair_table(None, tab, [1, 2], {}, detect_nulls=False, error_cells=(np.zeros(0, np.int64), np.zeros(0, np.int32)),
                                    cells_resident=True)
    assert res["cells_route"] == "host" and len(res["rows"]) == 0 and "cellset_open" not in tab.calls
    assert any("route is not taken" in r.getMessage() and "2 ranks" in r.getMessage() for r in caplog.records)
    monkeypatch.setattr(dist, "world", lambda: (0, 1))
    assert pipeline.set_route_refusal(CellrunTable(codes, n_codes), [1, 2]) is None
    assert pipeline.set_route_refusal(CellrunTable(codes, n_codes), []) == "no target attribute"
    tab = RecordingTable(codes, n_codes)
    res = pipeline.repair_table(None, tab, [1, 2], {}, detect_nulls=False, error_cells=(np.zeros(0, np.int64), np.zeros(0, np.int32)), cells_resident=True)
    assert res["cells_route"] == "set" and len(res["rows"]) == 0 and len(res["dirty_rows"]) == 0 and tab._set is None
    assert tab.calls == ["cellset_open", "cellset_emit", "cellset_emit", "cellset_null", "cellset_rows", "cellset_close"]
    # and without the keyword the result says nothing about a route
    assert "cells_route" not in pipeline.repair_table(None, RecordingTable(codes, n_codes), [1, 2], {}, detect_nulls=False,
                                                      error_cells=(np.zeros(0, np.int64), np.zeros(0, np.int32)))


def test_phases_one_and_two_on_random_tables_equal_the_host_route():
    """`_cells_on_set` against `_detect_and_prune` + `_null_and_merge`: cells, currents, dirty rows and the table itself, with overlapping
    detectors, given cells in no order, `only_noisy_targets`, and a detector that raises (the set is closed)."""
    from repair import pipeline as P
    for seed in range(4):
        n = [1, 65, 300, 4097][seed]
        codes, n_codes, _ = X.table(n, seed)
        targets = [[1], [2, 1], [5, 1, 2, 9], [4, 2, 1]][seed]
        given = X.given_cells(n, targets, seed) if seed % 2 else None
        cons = [([0], 1), ([0], 2)] if seed >= 2 else []
        for noisy_only in (False, True):
            host, dev = RecordingTable(codes, n_codes), RecordingTable(codes, n_codes)
            a = P._detect_and_prune(host, targets, cons, True, given, noisy_only, None, None, None)
            b = P._null_and_merge(None, host, a[2], a[0], a[1], None)
            got = P._cells_on_set(None, dev, targets, cons, True, given, noisy_only, None, None, None, None)
            for x, y in zip(a[:2] + b[:3] + b[4:], got[:2] + got[6:9] + got[10:]):
                assert np.array_equal(x, y) and x.dtype == y.dtype
            assert a[2] == got[2] and got[9] is None and np.array_equal(host.codes, dev.codes) and dev._set is None
            assert not {"read_cells", "null_cells", "rows_of_cells"} & set(dev.calls)

    class Raising(RecordingTable):
        def detect_constraint(self, *a, **kw):
            raise Refused("refused by this table")
    tab = Raising(codes, n_codes)
    with pytest.raises(Refused):
        P._cells_on_set(None, tab, [1, 2], [([0], 1)], True, None, False, None, None, None, None)
    assert tab._set is None and tab.calls[-1] == "cellset_close"


# ---------------------------------------------------------------------------------------------- the generators of the GPU file
@pytest.mark.parametrize("which", list(X.SETS))
@pytest.mark.parametrize("n", X.SIZES)
def test_generic_cases_reach_every_entry(n, which):
    case = X.generic_case(n, which)
    cols = case["set_cols"]
    assert cols != sorted(cols) or len(cols) == 1
    rows, gcols = case["given"][0]
    inside = (rows >= 0) & (rows < n) & np.isin(gcols, cols)
    keys = gcols[inside].astype(np.int64) * n + rows[inside]
    assert len(np.unique(keys)) < len(keys)                                          # duplicates
    assert ((rows < 0) | (rows >= n)).any() and (~np.isin(gcols, cols)).any() and ((gcols < 0) | (gcols >= X.C)).any()
    assert {(0, cols[0]), (n - 1, cols[-1])} <= set(zip(rows.tolist(), gcols.tolist()))
    assert (np.diff(keys) < 0).any() or n == 1                                       # not sorted
    rec = dict(X.drive(CellrunTable(case["codes"], case["n_codes"]), case))
    assert rec["detected.counts"].sum() > 0 or not {5, 9} & set(cols)                # (row 0 holds a NULL in columns 5 and 9)
    assert rec["detected.counts"].sum() < rec["with the given cells.counts"].sum()
    assert np.array_equal(rec["cell list after the empty add"], rec["detected.rows"])
    assert rec["null.cells"] == len(rec["after null.rows"]) > 0 and (rec["after null.codes"] == -1).all()
    assert 0 < len(rec["rows"]) == rec["rows.count"] <= rec["null.cells"]
    changed = rec["null.table"] != case["codes"]
    assert changed.sum() == (case["codes"][rec["after null.cols"], rec["after null.rows"]] >= 0).sum()   # every other code untouched
    if n >= 64:
        assert rec["drop_weak 1.cells"] > 0 and rec["drop_weak 1.weak"] == rec["drop_weak 1.flags of cell_domains"].sum()


@pytest.mark.parametrize("kind", X.PRUNE_KINDS)
def test_pruning_cases_prune_what_they_are_for(kind):
    case = X.prune_case(kind)
    rec = X.drive(CellrunTable(case["codes"], case["n_codes"]), case)
    X.purpose(case, rec)
    d = dict(rec)
    if kind == "two_in_one_word":
        r = case["weak_rows"][1]
        assert len(r) == 2 and r[0] // 64 == r[1] // 64
    if kind == "first_and_last_word":
        assert case["weak_rows"][1].tolist() == [0, X.PRUNE_N - 1] and X.PRUNE_N // 64 > 1
    if kind == "several_targets":
        assert len(case["prune"]) == 2 and d["drop_weak 2.cells"] > 0
    # the pruned cells left the set, the others stayed
    last = case["prune"][-1]["target"]
    before, after = d["with the given cells.counts"].sum(), d["after drop_weak %d.counts" % last].sum()
    assert before - after == sum(d["drop_weak %d.weak" % p["target"]] for p in case["prune"])


def test_rows_and_many_blocks_cases():
    sizes = {}
    for kind in ("empty", "every_row", "block_edges"):
        case = X.rows_case(kind)
        sizes[kind] = dict(X.drive(CellrunTable(case["codes"], case["n_codes"]), case))["rows"]
    assert len(sizes["empty"]) == 0 and np.array_equal(sizes["every_row"], np.arange(X.PRUNE_N))
    assert sizes["block_edges"].tolist() == [0, 63, 64, X.PROWS - 1, X.PROWS, 2 * X.PROWS - 1, 2 * X.PROWS]
    case = X.many_blocks_case()
    rec = dict(X.drive(CellrunTable(case["codes"], case["n_codes"]), case))
    assert case["codes"].shape[1] == 200003 and min(rec["nulls"], rec["cells"], rec["constraint"]) > 0
    assert rec["detected.counts"].sum() < rec["nulls"] + rec["cells"] + rec["constraint"]            # they overlap
    for t in (1, 2):
        assert 0 < rec["drop_weak %d.weak" % t] < rec["drop_weak %d.cells" % t]
