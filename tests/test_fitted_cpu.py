"""Fit once, repair later tables, without a device: the numpy statement of `rgbm_table_recode` and `repair.fitted.fitted_luts`
against the plain loops of tests/fitted_restatement.py, and the kept fit through `RepairModel` / `pipeline.repair_frame` on the oracle
engine -- a run that applies its own fit to the SAME frame gives the fit run's frame cell for cell; a fit of the first half of the rows
applied to the second half gives the restatement's values; later frames with values the fit never saw; save / load; every refusal."""
import logging

import numpy as np
import pandas as pd
import pytest

from repair import recode_codes
from repair.errors import ConstraintErrorDetector, NullErrorDetector
from repair.fitted import FORMAT, FittedRepairModels, fitted_luts
from repair.frame_encoding import FrameEncoding
from repair.model import RepairModel
from repair.pipeline import repair_frame
from tests import fitted_cases as FC
from tests import fitted_restatement as FR
from tests.helpers import OracleEngine, load_golden
from tests.test_quality import HOSPITAL_TARGETS, _boston_frame, _hospital

OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2"}
PARAMS = dict(n_estimators=8, learning_rate=0.2, max_depth=7, num_leaves=31)


class FittedOracleEngine(OracleEngine):
    """The oracle engine with the two entries an apply run needs: `recode` is the numpy statement, `load_model` the oracle's loader."""

    def __init__(self):
        self.recodes = 0

    def recode(self, table, luts, n_codes_out):
        self.recodes += 1
        out, unmapped = recode_codes.recode(table.codes, table.n_codes, luts, n_codes_out)
        return OracleEngine._Table(out, n_codes_out), unmapped

    def load_model(self, blob):
        from oracle import oracle as O
        return O.OracleModel.load(blob)

    def train(self, *a, **kw):
        self.trained = getattr(self, "trained", 0) + 1
        return OracleEngine.train(self, *a, **kw)


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


# ---------------------------------------------------------------------------------------------- statements against plain loops
@pytest.mark.parametrize("cid", FC.case_ids())
def test_recode_statement_equals_the_plain_loops(cid):
    c = FC.case(cid)
    got, un = recode_codes.recode(c["codes"], c["n_codes"], c["luts"], c["n_codes_out"])
    want, wun = FR.recode_loops(c["codes"], c["n_codes"], c["luts"], c["n_codes_out"])
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(un, wun)
    assert all(int(got[j].max(initial=-1)) < int(c["n_codes_out"][j]) and int(got[j].min(initial=-1)) >= -1 for j in range(len(got)))


def test_recode_statement_refusals():
    codes, nc = np.zeros((2, 3), np.int32), [2, 3]
    for luts, out, why in (([None, None], [2, 0], "at least 1"), ([None, None], [2, 4], "identity column 1"),
                           ([[0, 2], None], [2, 3], "column 0, LUT entry 1 = 2"), ([[0, -2], None], [2, 3], "column 0, LUT entry 1 = -2"),
                           ([[0], None], [2, 3], "has 1 entries"), ([None], [2], "per column")):
        with pytest.raises(ValueError, match=why):
            recode_codes.recode(codes, nc, luts, out)


def _fit_of(columns, dicts, categorical):
    return FittedRepairModels(columns, dicts, categorical, [], {}, rgbm_version=0)


def _obj(values):
    a = np.empty(len(values), object)
    a[:] = values
    return a


def test_fitted_luts_equal_the_plain_loops():
    fit = _fit_of(["cat", "num", "empty", "ints"], [_obj(["a", "c", "d"]), np.array([1.0, 2.0, 4.0, 10.0]), np.zeros(0, np.float64),
                                                    np.array([1, 5, 9], np.int64)], [True, False, False, False])
    df = pd.DataFrame({"tid": np.arange(8),
                       "cat": ["a", "b", "c", "zz", None, "d", "a", "a"],                  # b, zz: categories the fit never saw
                       "num": [3.0, 0.5, 11.0, 2.0, 7.0, 1.5, np.nan, 4.0],                  # 3.0, 1.5 and 7.0: exact ties; below; above
                       "empty": [1.0, 2.0, np.nan, 1.0, 1.0, 1.0, 1.0, 1.0],
                       "ints": [3.0, 7.0, 9.0, 0.0, 5.5, 1.0, 100.0, 5.0],                   # a float dictionary against an int one
                       "extra": list("abcdefgh")})
    enc = FrameEncoding.of_frame(df, [c for c in df.columns if c != "tid"])
    luts = fitted_luts(fit, enc)
    assert luts[enc.pos["extra"]] is None
    for c in fit.columns:
        j, k = enc.pos[c], fit.columns.index(c)
        want = FR.lut_loops(list(fit.dicts[k]), fit.categorical[k], list(enc.dicts[j]), enc.dicts[j].dtype == object)
        assert luts[j].dtype == np.int32 and np.array_equal(luts[j], want), c
    assert list(luts[enc.pos["cat"]]) == [0, -1, 1, 2, -1]                                   # a b c d zz
    assert list(luts[enc.pos["num"]]) == [0, 0, 1, 1, 2, 2, 3]                               # 0.5 1.5 2 3 4 7 11: ties go to the lower value
    assert list(luts[enc.pos["empty"]]) == [-1, -1]
    assert list(luts[enc.pos["ints"]]) == [0, 0, 0, 1, 1, 1, 2, 2]                           # 0 1 3 5 5.5 7 9 100
    with pytest.raises(ValueError, match="`num`"):
        fitted_luts(_fit_of(["num"], [_obj(["1.0"])], [True]), enc)                           # numeric in the frame, categorical in the fit
    with pytest.raises(ValueError, match="`cat`"):
        fitted_luts(_fit_of(["cat"], [np.array([1.0])], [False]), enc)
    with pytest.raises(ValueError, match="`gone`"):
        fitted_luts(_fit_of(["cat", "gone"], [_obj(["a"]), _obj(["a"])], [True, True]), enc)


# ---------------------------------------------------------------------------------------------- runs on the oracle engine
def _hospital_model(df, cells=None, detectors=None, keep=False, fitted=None, engine=None, targets=HOSPITAL_TARGETS):
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400)
    if targets:
        m = m.setTargets(list(targets))
    m = m.setErrorCells(cells) if cells is not None else m.setErrorDetectors(detectors)
    for k, v in dict(OPTS, **({"model.fitted.keep": "true"} if keep else {})).items():
        m = m.option(k, v)
    if fitted is not None:
        m = m.setFittedModels(fitted)
    m._engine_override = engine if engine is not None else FittedOracleEngine()
    return m


@pytest.fixture(scope="module")
def hospital_fit():
    """The hospital fixture fitted once with its given cells (shared, never modified): (frame, cells, the two fit-run frames, the fit)."""
    from repair import gbm
    from tests.helpers import OracleBackend
    prev = gbm.set_backend(OracleBackend)
    try:
        df, _, cells = _hospital()
        cells = cells[["tid", "attribute"]]
        m = _hospital_model(df, cells=cells, keep=True)
        out = m.run()
        assert m._last_resident_info is not None and "fit" in m._last_resident_info
        fit = m.fittedModels()
        data = _hospital_model(df, cells=cells).run(repair_data=True)
    finally:
        gbm.set_backend(prev)
    return df, cells, out, data, fit


def test_same_frame_given_cells_equals_the_fit_run(oracle_backend, hospital_fit):
    df, cells, out, data, fit = hospital_fit
    assert sorted(fit.chain) == sorted(HOSPITAL_TARGETS) and fit.columns == [c for c in df.columns if c != "tid"] and len(out) > 100
    assert all(fit.categorical) and all(len(fit.targets[t]["blob"]) > 100 and not fit.targets[t]["continuous"] for t in fit.chain)
    eng = FittedOracleEngine()
    m = _hospital_model(df, cells=cells, fitted=fit, engine=eng)
    again = m.run()
    assert eng.recodes == 1 and not getattr(eng, "trained", 0)                               # one device recode, no fit
    pd.testing.assert_frame_equal(_sorted(out), _sorted(again))
    info = m._last_resident_info["fitted"]
    assert set(info) == {"unmapped", "unfitted_cells", "recode_seconds"} and not any(info["unmapped"].values())
    assert info["unfitted_cells"] == {}          # (`setTargets` names the fitted targets: the given cells of other attributes never reach the table)
    again_data = _hospital_model(df, cells=cells, fitted=fit).run(repair_data=True)
    pd.testing.assert_frame_equal(data.sort_values("tid").reset_index(drop=True), again_data.sort_values("tid").reset_index(drop=True))


def test_same_frame_with_detectors_equals_the_fit_run(oracle_backend):
    g = load_golden("hospital")
    df, _, _ = _hospital()
    dets = lambda: [NullErrorDetector(), ConstraintErrorDetector(constraints=";".join(ln for ln in g["constraints"].splitlines() if ln.strip()))]  # noqa: E731
    m = _hospital_model(df, detectors=dets(), keep=True)
    out = m.run()
    fit = m.fittedModels()
    assert len(out) > 20 and set(fit.chain) <= set(HOSPITAL_TARGETS)
    eng = FittedOracleEngine()
    m2 = _hospital_model(df, detectors=dets(), fitted=fit, engine=eng, targets=fit.chain)
    again = m2.run()
    assert eng.recodes == 1 and not getattr(eng, "trained", 0) and m2._last_detection_on_device == m._last_detection_on_device
    pd.testing.assert_frame_equal(_sorted(out), _sorted(again))
    data = _hospital_model(df, detectors=dets(), targets=fit.chain).run(repair_data=True)
    again_data = _hospital_model(df, detectors=dets(), fitted=fit, targets=fit.chain).run(repair_data=True)
    pd.testing.assert_frame_equal(data.sort_values("tid").reset_index(drop=True), again_data.sort_values("tid").reset_index(drop=True))


def _boston_model(df, keep=False, fitted=None):
    m = RepairModel().setInput(df).setRowId("tid").setErrorDetectors([NullErrorDetector()])
    for k, v in dict(OPTS, **({"model.fitted.keep": "true"} if keep else {})).items():
        m = m.option(k, v)
    if fitted is not None:
        m = m.setFittedModels(fitted)
    m._engine_override = FittedOracleEngine()
    return m


def test_same_frame_with_continuous_targets_boston(oracle_backend):
    df, _ = _boston_frame()
    m = _boston_model(df, keep=True)
    out = m.run()
    fit = m.fittedModels()
    kinds = {t: (fit.targets[t]["continuous"], fit.targets[t]["integral"]) for t in fit.chain}
    assert kinds["CRIM"] == (True, False) and kinds["TAX"] == (True, True) and kinds["RAD"] == (False, False)
    assert np.array_equal(fit.targets["CRIM"]["y_values"], fit.dicts[fit.columns.index("CRIM")])
    m2 = _boston_model(df, fitted=fit)
    pd.testing.assert_frame_equal(_sorted(out), _sorted(m2.run()))
    data, again = _boston_model(df).run(repair_data=True), _boston_model(df, fitted=fit).run(repair_data=True)
    pd.testing.assert_frame_equal(data.sort_values("tid").reset_index(drop=True), again.sort_values("tid").reset_index(drop=True))


def _apply_frame(fit, df, cells, engine=None, **kw):
    frame_, details = repair_frame(engine or FittedOracleEngine(), df, "tid", error_cells=cells, detect_nulls=False, want_details=True, fitted=fit, **kw)
    return frame_, details


def _load(blob):
    from oracle import oracle as O
    return O.OracleModel.load(blob)


def _as_dict(frame_):
    return {(r.tid, r.attribute): r.repaired for r in frame_.itertuples(index=False)}


@pytest.fixture(scope="module")
def half_fit():
    """Boston's first half fitted through `repair_frame(keep_fit=True)`, NULL cells as error cells: (first half, second half, the fit)."""
    df, _ = _boston_frame()
    a, b = df.iloc[:253].reset_index(drop=True), df.iloc[253:].reset_index(drop=True)
    targets = ["CRIM", "RAD", "TAX", "LSTAT"]
    _, details = repair_frame(FittedOracleEngine(), a, "tid", targets=targets, base_params=PARAMS, continuous_columns=["CRIM", "TAX", "LSTAT"],
                              want_details=True, keep_fit=True)
    return a, b, FittedRepairModels.from_pieces(details["fit"])


def _null_cells(df, attrs):
    return pd.DataFrame([(r, a) for a in attrs for r in df["tid"][df[a].isna().to_numpy()]], columns=["tid", "attribute"])


def test_first_half_fit_applied_to_the_second_half_equals_the_restatement(half_fit):
    a, b, fit = half_fit
    cells = _null_cells(b, fit.chain)
    got, details = _apply_frame(fit, b, cells)
    want = FR.apply_loops(fit, b, "tid", list(cells.itertuples(index=False, name=None)), _load)
    assert len(got) == len(cells) > 60 and _as_dict(got) == want
    # the second half holds numbers the first never showed: they went to the nearest fitted value, nothing numeric is unmapped
    new_values = sum(int((~np.isin(b[c].dropna().to_numpy(np.float64), fit.dicts[fit.columns.index(c)])).sum())
                     for c in fit.columns if not fit.categorical[fit.columns.index(c)])
    assert new_values > 100 and not any(details["fitted"]["unmapped"][c] for c in fit.columns if not fit.categorical[fit.columns.index(c)])


def test_later_frame_with_values_the_fit_never_saw(half_fit):
    a, b, fit = half_fit
    cells = _null_cells(b, fit.chain)
    before = _apply_frame(fit, b, cells)[1]["fitted"]["unmapped"]
    b = b.copy()
    dirty = sorted(set(cells["tid"]))
    b.loc[b["tid"] == dirty[0], "CHAS"] = "7"                      # a category the fit never saw, in a feature of a dirty row
    b.loc[b["tid"] == dirty[1], "NOX"] = 123.456                   # a number the fit never saw, in a feature
    free = [r for r in dirty if not pd.isna(b.loc[b["tid"] == r, "RAD"].iloc[0])][0]
    b.loc[b["tid"] == free, "RAD"] = "99"                          # a value the fit never saw in a NON-error target cell
    got, details = _apply_frame(fit, b, cells)
    want = FR.apply_loops(fit, b, "tid", list(cells.itertuples(index=False, name=None)), _load)
    assert _as_dict(got) == want and (free, "RAD") not in _as_dict(got)
    after = details["fitted"]["unmapped"]        # (the second half holds RAD categories of its own: counted before and after)
    assert after["CHAS"] == before["CHAS"] + 1 and after["RAD"] == before["RAD"] + 1 and after["NOX"] == before["NOX"] == 0
    assert {c: k for c, k in after.items() if c not in ("CHAS", "RAD")} == {c: k for c, k in before.items() if c not in ("CHAS", "RAD")}


def test_error_cells_in_an_attribute_without_a_kept_model(half_fit, caplog):
    a, b, fit = half_fit
    cells = pd.concat([_null_cells(b, fit.chain), pd.DataFrame({"tid": b["tid"].iloc[[2, 5, 9]].to_numpy(), "attribute": ["AGE", "AGE", "DIS"]})],
                      ignore_index=True)
    with caplog.at_level(logging.WARNING):
        got, details = _apply_frame(fit, b, cells)
    assert not set(got["attribute"]) & {"AGE", "DIS"} and details["fitted"]["unfitted_cells"] == {"AGE": 2, "DIS": 1}
    warned = [r.getMessage() for r in caplog.records if "without a kept model" in r.getMessage()]
    assert len(warned) == 1 and "`AGE`: 2" in warned[0] and "`DIS`: 1" in warned[0]
    assert _as_dict(got) == FR.apply_loops(fit, b, "tid", list(cells.itertuples(index=False, name=None)), _load)
    # ... and through RepairModel: the cells are left out of the result
    m = RepairModel().setInput(b).setRowId("tid").setErrorCells(cells).setFittedModels(fit)
    m._engine_override = FittedOracleEngine()
    out = m.run()
    assert len(out) and not set(out["attribute"]) & {"AGE", "DIS"} and m._last_resident_info["fitted"]["unfitted_cells"] == {"AGE": 2, "DIS": 1}


def test_save_and_load_give_the_same_apply_run(half_fit, tmp_path):
    a, b, fit = half_fit
    path = str(tmp_path / "fit.npz")
    fit.save(path)
    with np.load(path, allow_pickle=False) as z:                    # opens without pickle; blobs are bytes, dictionaries keep their dtype
        assert int(z["format"][0]) == FORMAT and z["blob_0"].dtype == np.uint8 and z["dict_%d" % fit.columns.index("CRIM")].dtype == np.float64
        assert z["dict_%d" % fit.columns.index("RAD")].dtype.kind == "U" and all(z[k].dtype != object for k in z.files)
    back = FittedRepairModels.load(path)
    assert back.columns == fit.columns and back.chain == fit.chain and back.categorical == fit.categorical and back.version_mismatch is None
    assert back.rgbm_version == fit.rgbm_version and all(back.targets[t]["blob"] == fit.targets[t]["blob"] for t in fit.chain)
    assert all(x.dtype == y.dtype and list(x) == list(y) for x, y in zip(back.dicts, fit.dicts))
    cells = _null_cells(b, fit.chain)
    pd.testing.assert_frame_equal(_apply_frame(fit, b, cells)[0], _apply_frame(back, b, cells)[0])
    m = RepairModel().setInput(b).setRowId("tid").setErrorCells(cells).setFittedModels(path)       # a path is loaded
    m._engine_override = FittedOracleEngine()
    assert len(m.run()) > 0


def test_save_and_load_refusals(half_fit, tmp_path, caplog):
    a, b, fit = half_fit
    bad = FittedRepairModels(["x", "y"], [_obj(["a", (1, 2)]), _obj(["a", True, 3, 2.5])], [True, True], [], {}, rgbm_version=fit.rgbm_version)
    with pytest.raises(ValueError, match="column `x`"):
        bad.save(str(tmp_path / "bad.npz"))
    ok = FittedRepairModels(["y"], [_obj(["a", True, 3, 2.5])], [True], [], {}, rgbm_version=fit.rgbm_version - 1)
    ok.save(str(tmp_path / "ok.npz"))
    with caplog.at_level(logging.WARNING):
        back = FittedRepairModels.load(str(tmp_path / "ok.npz"))
    assert [type(v) for v in back.dicts[0]] == [str, bool, int, float] and list(back.dicts[0]) == ["a", True, 3, 2.5]
    assert back.version_mismatch is not None and any("rgbm_version" in r.getMessage() for r in caplog.records)
    with np.load(str(tmp_path / "ok.npz"), allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["format"] = np.array([FORMAT + 1], np.int64)
    with open(str(tmp_path / "other.npz"), "wb") as f:
        np.savez(f, **arrays)
    with pytest.raises(ValueError, match="format %d" % (FORMAT + 1)):
        FittedRepairModels.load(str(tmp_path / "other.npz"))


def test_every_refusal_says_why(oracle_backend, half_fit, monkeypatch):
    a, b, fit = half_fit
    cells = _null_cells(b, fit.chain)

    def model(**kw):
        m = RepairModel().setInput(b).setRowId("tid").setErrorCells(cells).setFittedModels(fit)
        m._engine_override = kw.get("engine", FittedOracleEngine())
        return m
    for flags in (dict(compute_repair_candidate_prob=True), dict(compute_repair_prob=True)):
        with pytest.raises(ValueError, match="probability modes"):
            model().run(**flags)
    with pytest.raises(ValueError, match="setRepairByRules"):
        model().setRepairByRules(True).run()
    with pytest.raises(ValueError, match="fitted targets"):
        model().setTargets(["CRIM"]).run()
    m = model()
    m._engine_override = None
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    with pytest.raises(ValueError, match="no engine"):
        m.run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    from repair import dist
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    with pytest.raises(ValueError, match="2 ranks"):
        model().run()
    monkeypatch.undo()
    with pytest.raises(ValueError, match="`LSTAT` is not in the"):
        m = RepairModel().setInput(b.drop(columns=["LSTAT"])).setRowId("tid").setErrorCells(cells[cells["attribute"] != "LSTAT"]).setFittedModels(fit)
        m._engine_override = FittedOracleEngine()
        m.run()
    with pytest.raises(ValueError, match="rule steps"):
        repair_frame(FittedOracleEngine(), b, "tid", error_cells=cells, detect_nulls=False, fitted=fit, rules=dict(fd={}, nearest=None))
    with pytest.raises(ValueError, match="probability modes"):
        repair_frame(FittedOracleEngine(), b, "tid", error_cells=cells, detect_nulls=False, fitted=fit, want_pmf=True)


def test_fitted_models_raises_when_nothing_was_kept(oracle_backend):
    df, _ = _boston_frame()
    with pytest.raises(ValueError, match="model.fitted.keep"):
        RepairModel().fittedModels()
    m = _boston_model(df)                                           # the option is off: nothing new is kept, the details hold no dictionaries
    m.run()
    assert m._last_resident_info is not None and "fit" not in m._last_resident_info and "fitted" not in m._last_resident_info
    assert not any(isinstance(v, dict) and "dicts" in v for v in m._last_resident_info.values())
    with pytest.raises(ValueError, match="model.fitted.keep"):
        m.fittedModels()
    m = _boston_model(df, keep=True)                                # the value-space path keeps nothing
    m._engine_override = None
    import os
    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        m.run()
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    with pytest.raises(ValueError, match="value-space path"):
        m.fittedModels()
    # rule steps and a multi-rank job: the details name the reason instead of the pieces, and `fittedModels()` raises it
    from repair import dist, pipeline
    d = pd.DataFrame({"tid": np.arange(4), "k": list("abab"), "v": list("xyxy"), "w": list("pqrs")})
    enc = FrameEncoding.of_frame(d, ["k", "v", "w"])
    got = pipeline._fit_pieces(enc, dict(fit=dict(chain=[1], y_values={}, integral=[], rule_targets=[1]), models={}), {})
    assert "fit" not in got and "rule steps (`v`)" in got["fit_refusal"]
    prev = dist.world
    dist.world = lambda: (0, 2)
    try:
        got = pipeline._fit_pieces(enc, dict(fit=dict(chain=[1], y_values={}, integral=[], rule_targets=[]), models={1: b""}), {})
    finally:
        dist.world = prev
    assert "fit" not in got and "2 ranks" in got["fit_refusal"]
    m._kept_fit, m._kept_fit_why = None, got["fit_refusal"]
    with pytest.raises(ValueError, match="2 ranks"):
        m.fittedModels()
