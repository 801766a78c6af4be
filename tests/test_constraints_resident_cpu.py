"""CPU: every parsed denial constraint as a program on dictionary codes (repair/dc_codes.py) and `RepairModel.run()` with them on the
resident pipeline behind `error.constraints.resident`.

The lowering is held to `errors._violating_rows` row for row, and whole runs on a CPU engine (the oracle engine of tests/helpers plus
the numpy restatements of rgbm_table_detect_dc / rgbm_table_detect_row_bits in tests/dc_restatement.py) to the value-space path on the
oracle estimator backend."""
import logging

import numpy as np
import pandas as pd
import pytest

from repair import dc_codes as DC
from repair.errors import ConstraintErrorDetector, NullErrorDetector, _violating_rows, parse_constraint
from repair.model import RepairModel
from repair.pipeline import encode_frame
from tests import dc_restatement as R
from tests.helpers import OracleEngine, frame, load_golden


class DcTable(OracleEngine._Table):
    """The oracle engine's table with the two new entries, answered by the restatements."""
    calls = 0
    max_pairs_default = 0

    def detect_dc(self, preds, cell_cols=(), max_pairs=0):
        DcTable.calls += 1
        return R.detect_dc(self.codes, self.n_codes, preds, cell_cols, max_pairs=max_pairs or type(self).max_pairs_default)

    def detect_row_bits(self, cols, bits, cell_cols=()):
        DcTable.calls += 1
        return R.detect_row_bits(self.codes, self.n_codes, cols, bits, cell_cols)

    def gather_rows(self, rows):
        return type(self)(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)


class DcEngine(OracleEngine):
    table_cls = DcTable

    def upload(self, codes, n_codes):
        return self.table_cls(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return self.table_cls(t.codes, t.n_codes, t.values, t.kinds)


class RefusingTable(DcTable):
    max_pairs_default = 1            # every pair program is over the bound: the restated RGBM_ERR_PARAM


class RefusingEngine(DcEngine):
    table_cls = RefusingTable


# ---------------------------------------------------------------------------------------------- the lowering against the host detector
def _encode(df, cols):
    idx, remaps, dicts = encode_frame(df, cols)
    codes = np.stack([np.where(idx[j] >= 0, remaps[j][np.maximum(idx[j], 0)] if len(remaps[j]) else -1, -1) for j in range(len(cols))]).astype(np.int32)
    return codes, [max(len(d), 1) for d in dicts], dicts


def _device_rows(df, stmt, cols=None):
    """Violating rows of `stmt` through the dictionaries: lowering -> restated device entry.  Returns (rows, program)."""
    cols = cols or [c for c in df.columns if c != "tid"]
    codes, n_codes, dicts = _encode(df, cols)
    prog = DC.lower_constraint(parse_constraint(stmt), cols, dicts, {c: df[c].dtype for c in cols})
    if isinstance(prog, tuple):
        from oracle import prep as P
        return P.constraint_rows(codes, prog[0], prog[1]), prog
    if prog["kind"] == "dc":
        return R.detect_dc(codes, n_codes, prog["preds"]), prog
    return R.detect_row_bits(codes, n_codes, prog["cols"], prog["bits"]), prog


def _same_rows(df, stmt):
    got, prog = _device_rows(df, stmt)
    want = np.flatnonzero(_violating_rows(df, parse_constraint(stmt)))
    assert np.array_equal(got, want), stmt
    return want, prog


def test_both_adult_constraints_on_the_adult_fixture():
    g = load_golden("adult")
    df = frame(g["input"])
    stmts = [l for l in g["constraints"].splitlines() if l.strip()]
    assert len(stmts) == 2
    total = 0
    for s in stmts:
        want, prog = _same_rows(df, s)
        assert prog["kind"] == "row_bits" and [df.columns[1:][c] for c in prog["refs"]] == ["Sex", "Relationship"]
        total += len(want)
    assert total > 0


def _mixed_frame(n=240, seed=3):
    rng = np.random.default_rng(seed)
    s = rng.choice(np.array(["a", "b", "c", None], object), n, p=[.4, .3, .2, .1])
    i = rng.integers(0, 9, n).astype(np.int64)
    f = np.round(rng.normal(3, 2, n), 1)
    f[rng.random(n) < 0.1] = np.nan
    t = rng.choice(np.array(["1", "1.0", "x", "2", "02", None], object), n)          # "1" and "1.0", "2" and "02": tied numbers; "x": none
    ni = pd.array(rng.integers(0, 5, n), dtype="Int64")
    ni[rng.random(n) < 0.1] = pd.NA
    return pd.DataFrame({"tid": np.arange(n), "s": s, "i": i, "f": f, "t": t, "ni": ni, "nan": np.full(n, np.nan),
                         "none": np.array([None] * n, object), "g": rng.integers(0, 12, n).astype(np.int64)})


@pytest.fixture(scope="module")
def mixed():
    return _mixed_frame()


SINGLE = [
    't1&EQ(t1.s,"a")&EQ(t1.i,"3")',
    't1&IQ(t1.s,"a")&IQ(t1.i,"3")',                       # IQ is true for a NULL cell
    't1&IQ(t1.s,"zzz")&IQ(t1.none,"a")',
    't1&EQ(t1.s,"a")&IQ(t1.s,"a")',                       # two predicates on one column: ANDed, nobody
    't1&LT(t1.i,"4")&GT(t1.i,"1")',                       # integral column
    't1&LT(t1.f,"3.05")&GT(t1.f,"-1")',                   # float column
    't1&EQ(t1.f,"3.0")&IQ(t1.i,"3.0")',                   # astype(str) of a float column is "3.0", of an int column "3"
    't1&GT(t1.t,"0.5")&LT(t1.t,"1.5")',                   # strings "1", "1.0", "x"
    't1&EQ(t1.t,"1")&IQ(t1.t,"1.0")',
    't1&EQ(t1.ni,"3")&GT(t1.ni,"2")',                     # nullable integers
    't1&LT(t1.nan,"1")&IQ(t1.s,"a")',                     # NaN-only column
    't1&IQ(t1.nan,"1")&IQ(t1.none,"1")',
    "t1&EQ(t1.s,'a')&GT(t1.g,5)",                         # quotes of the other kind, none at all
]


@pytest.mark.parametrize("stmt", SINGLE)
def test_single_tuple_constraints(mixed, stmt):
    _, prog = _same_rows(mixed, stmt)
    assert prog["kind"] == "row_bits" and len(set(prog["cols"])) == len(prog["cols"])


TWO = [
    "t1&t2&IQ(t1.s,t2.s)&IQ(t1.i,t2.i)",                                    # two IQs, no EQ
    "t1&t2&EQ(t1.g,t2.g)&IQ(t1.s,t2.s)&IQ(t1.ni,t2.ni)",                    # NULL is a value of its own under IQ, equal to NULL under EQ
    "t1&t2&EQ(t1.s,t2.s)&IQ(t1.none,t2.none)&IQ(t1.i,t2.i)",                # nobody: the all-NULL column never differs
    "t1&t2&EQ(t1.g,t2.g)&GT(t1.i,t2.i)&LT(t1.f,t2.f)",                      # EQ + GT + LT
    "t1&t2&EQ(t1.g,t2.g)&EQ(t1.s,t2.s)&LT(t1.t,t2.t)",                      # tied ranks: "1" is not below "1.0"
    "t1&t2&EQ(t1.g,t2.g)&GT(t1.t,t2.t)&GT(t1.ni,t2.ni)",
    "t1&t2&LT(t1.i,t2.i)&GT(t1.f,t2.f)",                                    # no EQ at all
    "t1&t2&EQ(t1.g,t2.g)&LT(t1.i,t2.f)",                                    # across two attributes: one merged order
    "t1&t2&EQ(t1.s,t2.s)&LT(t1.t,t2.i)&GT(t1.f,t2.ni)",
    "t1&t2&EQ(t1.g,t2.g)&LT(t1.nan,t2.nan)",                                # NaN-only column: nobody
    "t1&t2&EQ(t1.g,t2.g)&GT(t1.i,t2.nan)",
    "t1&t2&EQ(t1.g,t2.g)&EQ(t1.s,t2.s)",                                    # EQ only: every row
    "t1&t2&EQ(t1.g,t2.g)&LT(t1.i,t2.i)&GT(t1.i,t2.i)",                      # nobody
]


NOBODY = {TWO[2], TWO[9], TWO[12]}


@pytest.mark.parametrize("stmt", TWO)
def test_two_tuple_constraints(mixed, stmt):
    want, prog = _same_rows(mixed, stmt)
    assert prog["kind"] == "dc"
    if stmt in NOBODY:
        assert len(want) == 0


def test_rank_arrays(mixed):
    cols = [c for c in mixed.columns if c != "tid"]
    _, _, dicts = _encode(mixed, cols)
    dt = {c: mixed[c].dtype for c in cols}
    p = DC.lower_constraint(parse_constraint("t1&t2&EQ(t1.g,t2.g)&LT(t1.i,t2.i)&GT(t1.t,t2.t)&LT(t1.i,t2.f)&GT(t1.nan,t2.nan)"), cols, dicts, dt)["preds"]
    assert p[1][3] is None and p[1][4] is None                     # an ascending numeric dictionary: the codes are the ranks
    t = dict(zip(dicts[cols.index("t")].tolist(), p[2][3].tolist()))
    assert t["1"] == t["1.0"] and t["2"] == t["02"] and t["x"] == -1 and t["1"] < t["2"] and p[2][3] is p[2][4]
    li, rf = p[3][3], p[3][4]                                      # one merged order: rank order = numeric order across both dictionaries
    vi, vf = np.asarray(dicts[cols.index("i")], float), np.asarray(dicts[cols.index("f")], float)
    assert np.array_equal(li[:, None] < rf[None, :], vi[:, None] < vf[None, :]) and np.array_equal(li[:, None] > rf[None, :], vi[:, None] > vf[None, :])
    assert p[4][3].tolist() == [-1]                                # a column without a value: one code, no number
    a, b = DC.dense_ranks([3.0, np.nan, 1.0, 3.0], [2.0, 1.0])
    assert a.tolist() == [2, -1, 0, 2] and b.tolist() == [1, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("stmt", ["t1&t2&EQ(t1.a,t2.a)&IQ(t1.b,t2.b)&IQ(t1.c,t2.c)", "t1&t2&EQ(t1.a,t2.a)&GT(t1.x,t2.x)&LT(t1.y,t2.y)",
                                  "t1&t2&GT(t1.x,t2.x)&LT(t1.y,t2.y)&IQ(t1.b,t2.b)", "t1&t2&EQ(t1.a,t2.a)&EQ(t1.b,t2.b)&EQ(t1.c,t2.c)"])
def test_random_frames(seed, stmt):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 401))

    def holes(a):
        a = a.astype(object)
        a[rng.random(n) < 0.15] = None
        return a

    df = pd.DataFrame({"tid": np.arange(n), "a": holes(rng.integers(0, 1 + n // 8, n)), "b": holes(rng.choice(["p", "q", "r"], n)),
                       "c": holes(rng.integers(0, 3, n)), "x": np.where(rng.random(n) < 0.1, np.nan, rng.integers(0, 20, n).astype(float)),
                       "y": np.where(rng.random(n) < 0.1, np.nan, np.round(rng.random(n) * 5, 1))})
    want, prog = _same_rows(df, stmt)
    assert prog["kind"] == "dc" and (len(want) == n if "GT" not in stmt and "IQ" not in stmt else True)


# ---------------------------------------------------------------------------------------------- what stays in value space
STAYS = [
    ("t1&t2&EQ(t1.s,t2.i)&IQ(t1.f,t2.f)", "compares two attributes"),
    ("t1&t2&EQ(t1.s,t2.s)&IQ(t1.i,t2.f)", "compares two attributes"),
    ("t1&t2&EQ(t1.i,t2.i)&LT(t1.i,t2.f)&IQ(t1.s,t2.s)", "under an EQ / IQ and under an LT / GT"),
    ("t1&t2&IQ(t1.f,t2.f)&GT(t1.f,t2.f)", "under an EQ / IQ and under an LT / GT"),
    ("t1&t2&" + "&".join(["IQ(t1.s,t2.s)", "IQ(t1.i,t2.i)"] * 8 + ["LT(t1.f,t2.f)"]), "17 predicates"),
    ('t1&EQ(t1.s,"a")&GT(t1.i,"abc")', "not a number"),
    ("t1&t2&EQ(t1.tid,t2.tid)&LT(t1.f,t2.f)", "not a column of the table"),
]


@pytest.mark.parametrize("stmt,why", STAYS)
def test_what_stays_in_value_space(mixed, caplog, stmt, why):
    cols = [c for c in mixed.columns if c != "tid"]
    _, _, dicts = _encode(mixed, cols)
    with pytest.raises(DC.NotLowerable, match=why):
        DC.lower_constraint(parse_constraint(stmt), cols, dicts, {c: mixed[c].dtype for c in cols})
    m = _model(mixed, stmt, DcEngine(), on=True, targets=["s", "i", "g"])
    with caplog.at_level(logging.INFO):
        assert m._device_detection_plan(mixed, [], False, False) is None
    assert any("stays with the value-space detector" in r.getMessage() and why in r.getMessage() for r in caplog.records)


def test_wide_keys_stay_in_value_space():
    n = 40
    wide = pd.DataFrame({"k%02d" % j: np.arange(n) % (j + 2) for j in range(13)})
    cols = list(wide.columns)
    _, _, dicts = _encode(wide, cols)
    dt = {c: wide[c].dtype for c in cols}
    stmt = "t1&t2&" + "&".join("EQ(t1.%s,t2.%s)" % (c, c) for c in cols) + "&LT(t1.k00,t2.k01)"
    with pytest.raises(DC.NotLowerable, match="13 EQ attributes"):
        DC.lower_constraint(parse_constraint(stmt.replace("LT(t1.k00,t2.k01)", "IQ(t1.k00,t2.k00)&IQ(t1.k01,t2.k01)")), cols, dicts, dt)
    # a key span of 2^63 or more: four attributes of 2^16 values each
    preds = parse_constraint("t1&t2&EQ(t1.a,t2.a)&EQ(t1.b,t2.b)&EQ(t1.c,t2.c)&EQ(t1.d,t2.d)&IQ(t1.e,t2.e)&IQ(t1.f,t2.f)")
    with pytest.raises(DC.NotLowerable, match="2\\^63"):
        DC.check_constraint(preds, list("abcdef"), dict(a=1 << 16, b=1 << 16, c=1 << 16, d=1 << 16, e=2, f=2))
    assert DC.check_constraint(preds, list("abcdef"), dict(a=1 << 16, b=1 << 16, c=1 << 16, d=1 << 14, e=2, f=2)) == "dc"


# ---------------------------------------------------------------------------------------------- whole runs
OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "6", "model.lgb.learning_rate": "0.2"}
ON = "error.constraints.resident"


def _model(df, constraints, engine=None, on=False, targets=(), thres=80, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(thres) \
        .setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints=constraints)])
    if targets:
        m = m.setTargets(list(targets))
    for key, val in dict(OPTS, **opts).items():
        m = m.option(key, str(val))
    if on:
        m = m.option(ON, "true")
    m._engine_override = engine
    return m


def _sorted(df):
    return df.sort_values(["tid", "attribute"]).reset_index(drop=True)


def _three_ways(monkeypatch, df, constraints, engine_cls=DcEngine, expect_device=True, **kw):
    """The option-on run, the option-off run on the same engine and the value-space run give one frame."""
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _model(df, constraints, **kw).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    off = _model(df, constraints, engine_cls(), on=False, **kw)
    off_frame = off.run()
    assert off._last_detection_on_device is False
    before = DcTable.calls
    fast = _model(df, constraints, engine_cls(), on=True, **kw)
    fast_frame = fast.run()
    assert fast._last_detection_on_device is expect_device
    assert DcTable.calls > before
    pd.testing.assert_frame_equal(_sorted(slow), _sorted(off_frame), check_exact=True)
    pd.testing.assert_frame_equal(_sorted(slow), _sorted(fast_frame), check_exact=True)
    return slow


def test_option_is_registered_and_parsed():
    assert ON in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_constraints_resident) is False
    assert m.option(ON, "true")._get_option_value(*RepairModel._opt_constraints_resident) is True


def _adult():
    g = load_golden("adult")
    return frame(g["input"]), ";".join(l for l in g["constraints"].splitlines() if l.strip())


def test_option_off_keeps_the_plan(mixed):
    df, cons = _adult()
    assert _model(df, cons, DcEngine(), on=False)._device_detection_plan(df, [], False, False) is None
    plan = _model(df, cons, DcEngine(), on=True)._device_detection_plan(df, [], False, False)
    assert plan is not None and len(plan["constraints"]) == 2
    # an `X -> Y` constraint is the old tuple with the option on or off
    for on in (False, True):
        plan = _model(mixed, "t1&t2&EQ(t1.g,t2.g)&IQ(t1.s,t2.s)", DcEngine(), on=on, targets=["s", "g"])._device_detection_plan(mixed, [], False, False)
        assert plan["constraints"] == [(["g"], "s")]
    # a program that references a target outside the discretizable candidates stays with the pandas detectors, like an `X -> Y` one
    assert _model(mixed, "t1&t2&EQ(t1.g,t2.g)&LT(t1.f,t2.f)", DcEngine(), on=True, targets=["s", "g", "f"],
                  thres=20)._device_detection_plan(mixed, [], False, False) is None


def test_run_adult_with_its_two_statements(oracle_backend, monkeypatch):
    df, cons = _adult()
    slow = _three_ways(monkeypatch, df, cons)
    assert len(slow) > 0


def _hospital():
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    return df


HOSPITAL_CONS = ("t1&t2&EQ(t1.HospitalName,t2.HospitalName)&IQ(t1.ZipCode,t2.ZipCode)&IQ(t1.City,t2.City);"
                 "t1&t2&EQ(t1.City,t2.City)&GT(t1.ZipCode,t2.ZipCode)")
HOSPITAL_TARGETS = ["City", "State", "ZipCode", "Condition", "MeasureCode", "HospitalOwner"]


def test_run_hospital_with_two_iqs_and_an_order_predicate(oracle_backend, monkeypatch):
    slow = _three_ways(monkeypatch, _hospital(), HOSPITAL_CONS, targets=HOSPITAL_TARGETS, thres=400)
    assert {"City", "ZipCode"} <= set(slow["attribute"])


def test_a_refusing_engine_falls_back(oracle_backend, monkeypatch, caplog):
    """`max_pairs`: the device refuses the pair program (RGBM_ERR_PARAM), the run continues in value space and gives the same frame."""
    with caplog.at_level(logging.INFO):
        _three_ways(monkeypatch, _hospital(), HOSPITAL_CONS, engine_cls=RefusingEngine, expect_device=False, targets=HOSPITAL_TARGETS, thres=400)
    assert any("more pairs than max_pairs" in r.getMessage() for r in caplog.records)


def test_pipeline_detect_error_cells_takes_programs_next_to_tuples():
    from repair.pipeline import NotResidentEligible, detect_error_cells
    rng = np.random.default_rng(4)
    codes = rng.integers(-1, 5, (4, 300)).astype(np.int32)
    t = DcTable(codes, [5, 5, 5, 5])
    dc = dict(kind="dc", preds=[("EQ", 0, 0, None, None), ("GT", 1, 1, None, None), ("LT", 3, 2, None, None)], refs=[0, 1, 3, 2])
    flags = [np.r_[rng.random(5) < 0.5, True], np.r_[rng.random(5) < 0.5, False]]
    from repair.detect_codes import pack_bits
    rb = dict(kind="row_bits", cols=[2, 0], bits=[pack_bits(f) for f in flags], refs=[2, 0])
    r, c = detect_error_cells(t, [0, 2, 3], constraints=[([1], 2), dc, rb], detect_nulls=False)
    want = set()
    vr, vc = t.detect_constraint([1], 2, cell_cols=[2])
    want |= set(zip(vc.tolist(), vr.tolist()))
    vr, vc = R.detect_dc(codes, [5] * 4, dc["preds"], cell_cols=[0, 3, 2])          # the references that are targets
    want |= set(zip(vc.tolist(), vr.tolist()))
    vr, vc = R.detect_row_bits(codes, [5] * 4, rb["cols"], rb["bits"], cell_cols=[2, 0])
    want |= set(zip(vc.tolist(), vr.tolist()))
    assert list(zip(c.tolist(), r.tolist())) == sorted(want) and len(want) > 0
    # a program none of whose references is a target is not evaluated
    before = DcTable.calls
    detect_error_cells(t, [1], constraints=[rb], detect_nulls=False)
    assert DcTable.calls == before
    with pytest.raises(NotResidentEligible, match="max_pairs"):
        detect_error_cells(RefusingTable(codes, [5, 5, 5, 5]), [0], constraints=[dc], detect_nulls=False)
