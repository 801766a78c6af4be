"""CPU: regex-structure repair in value space (repair/regex_structure.py) -- the lexer and grammar of RegexBase.g4, the refusals, the
statement against `re.search` on the derived pattern -- and `RepairModel.run()` with `model.rule.repair_by_regex.disabled=""`: on the
value-space path (oracle estimator backend), and on the resident pipeline behind `model.rule.regex.resident` through a CPU engine whose
`regex_structure` is the statement, where the frame must equal the value-space frame cell for cell."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from repair import regex_structure as RS
from repair.errors import NullErrorDetector, RegExErrorDetector
from repair.model import RepairModel
from repair.regex_structure import ANCHOR_END, ANCHOR_START, Capture, Constant, NotRepairable, Program, parse, repair_value, repair_values
from tests import detector_restatements as DR
from tests.helpers import GOLDEN
from tests.regex_cases import class_bits, pooled_cases, random_cases, re_repair
from tests.test_rule_resident_cpu import RuleOracleEngine

DIGITS = class_bits("0123456789")


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "regex_structure.json"), encoding="utf-8") as f:
        return json.load(f)


# ---------------------------------------------------------------------------------------------- lexer, grammar, refusals
def test_golden_rows(golden):
    for g in golden["token_lists"]:
        assert [list(t) for t in RS.flatten(g["pattern"])] == g["tokens"]
    assert len(golden["repairs"]) == 7
    for pattern, value, expected in golden["repairs"]:
        assert repair_value(parse(pattern), value) == expected
        assert re_repair(parse(pattern), value) == expected
    assert repair_value(parse("^[0-9]{1,3}%"), None) is None


def test_lexer_ties():
    assert RS.tokenize("a{2}") == [("RANGE", "a{2}")]                      # longest match: RANGE over SYMBOL / CONSTANT
    assert RS.tokenize(" patients") == [("CONSTANT", " patients")]          # one CONSTANT, the blank included (WS is tab, CR, LF)
    assert RS.tokenize("%") == [("CONSTANT", "%")]
    assert RS.tokenize("f[0-9]") == [("SYMBOL", "f"), ("PATTERN", "[0-9]")]   # equal lengths: the earlier rule (SYMBOL, PATTERN)
    assert RS.tokenize("fo[0-9]{2}") == [("CONSTANT", "fo"), ("RANGE", "[0-9]{2}")]
    assert RS.tokenize("7") == [("SYMBOL", "7")] and RS.tokenize("77") == [("CONSTANT", "77")]
    assert RS.tokenize("ab\t\r\ncd") == [("CONSTANT", "ab"), ("CONSTANT", "cd")]
    assert RS.tokenize("[a-c9]{1,}x{,3}") == [("RANGE", "[a-c9]{1,}"), ("RANGE", "x{,3}")]
    with pytest.raises(NotRepairable, match="SYMBOL"):
        parse("f[0-9]")


@pytest.mark.parametrize("pattern, reason", [
    ("ab#cd", "no rule"), ("abc{2}", "no rule"), ("(a|b)", "no rule"), ("[a-]{2}", "no rule"), ("a{,}", "no rule"),
    ("f[0-9]", "SYMBOL"), ("^a$", "SYMBOL"), ("a{2}^b{2}", "CARET"), ("a{2}$b{2}", "DOLLAR"), ("*a{2}", "STAR"), ("a{2}|", "ALTERNATION"),
    ("a{2}||b{2}", "ALTERNATION"), ("^$", "expression"), ("", "expression"), ("^", "expression"),
    ("[z-a]{2}", "backwards"), ("a{3,2}", "min > max"), ("a{,3}", "{,n}"), ("a{65536}", "above 65535"), ("a{1,65536}", "above 65535"),
    ("-".join(["[a]{1}"] * 17), "33 segments"), ("a{1}-a{1}", "no rule"),       # (`-a` is a CONSTANT, `{` is then alone)
    ("[0-9]", "no counted class"), ("^[a-z]+.*$", "no counted class"),
])
def test_refusals(pattern, reason):
    with pytest.raises(NotRepairable) as e:
        parse(pattern)
    assert reason in str(e.value)


def test_limits_that_are_accepted():
    assert parse("a{65535}").segs == (Capture(1 << 97, 65535, 65535),)
    assert len(parse("-".join(["[a]{1}"] * 16) + "-").segs) == 32
    assert parse("[A-z]{0,}").segs[0] == Capture(sum(1 << c for c in range(65, 123)), 0, -1)
    assert parse("[0-9a]{2}").segs[0].cls == DIGITS | 1 << 97


def test_vanishing_tokens():
    # PATTERN alone, ANY, STAR, PLUS, MAYBE, ALTERNATION leave nothing behind: the reference's naive approach
    p = parse("^[a-z]+.*[0-9]{2}?|x{1}id_$")
    assert p == Program(ANCHOR_START | ANCHOR_END, (Capture(DIGITS, 2, 2), Capture(1 << ord("x"), 1, 1), Constant("id_")))
    assert parse("[a-z]abc.") == Program(0, (Constant("abc"),))
    assert repair_value(p, "42x???") == "42xid_" and repair_value(p, "a42x???") is None


# ---------------------------------------------------------------------------------------------- the statement
def test_statement_equals_re_search_on_the_derived_pattern():
    for cases in (random_cases(20000), pooled_cases()):           # 20 000 programs with a string each; the 5 000 cases the GPU suite runs too
        matched = 0
        for program, s in cases:
            got = repair_value(program, s)
            assert got == re_repair(program, s), (program, s)
            matched += got is not None
        assert len(cases) // 5 <= matched <= 4 * len(cases) // 5, matched


def test_bounds_start_and_anchors():
    lower = class_bits("abcdefghijklmnopqrstuvwxyz")
    assert repair_value(parse("^[0-9]{2,}%$"), "123456!") == "123456%"             # {m,} is unbounded
    assert repair_value(parse("^[0-9]{2,}%$"), "1!") is None
    assert repair_value(parse("^[0-9]{0}%$"), "!") == "%"                           # m = 0 ...
    assert repair_value(parse("^[0-9]{0,2}[a-z]{0,}xy$"), "??") == "xy"             # ... captures nothing
    assert repair_value(Program(0, (Capture(DIGITS, 2, 3), Constant("#"))), "ab1c2345!!") == "234#"      # a leftmost start that is not 0
    assert repair_value(Program(0, (Capture(DIGITS, 0, 3),)), "ab12") == ""          # the empty match at 0 is the leftmost
    two = (Capture(DIGITS, 2, 2),)
    assert [repair_value(Program(a, two), "x12y") for a in range(4)] == ["12", None, None, None]
    assert [repair_value(Program(a, two), "12y") for a in range(4)] == ["12", "12", None, None]
    assert [repair_value(Program(a, two), "x12") for a in range(4)] == ["12", None, "12", None]
    assert [repair_value(Program(a, two), "12") for a in range(4)] == ["12"] * 4
    assert [repair_value(Program(a, two), "123") for a in range(4)] == ["12", "12", "23", None]
    # greedy, then back: the first capture gives one up
    assert repair_value(Program(ANCHOR_START | ANCHOR_END, (Capture(lower, 1, -1), Capture(lower, 2, 2))), "abcde") == "abcde"
    assert repair_value(Program(ANCHOR_START | ANCHOR_END, (Capture(lower, 1, -1), Constant("__"), Capture(lower, 1, 1))), "abcde") == "abc__e"
    assert repair_values(parse("^[0-9]{1,3}%$"), ["5x", None, "", "1234", "12345"]) == ["5%", None, None, "123%", None]


@pytest.mark.parametrize("cp", [0x0A, 0x0D, 0x85, 0x2028, 0x2029])
def test_line_terminators_are_left_alone_by_the_callers(cp):
    program = parse("^[0-9]{1,3} patients$")
    s = "12 patient" + chr(cp)
    assert repair_value(program, s) is None and re_repair(program, s) is None       # no wildcard takes it
    assert RS.has_line_terminator(s) and not RS.has_line_terminator("12 patients\x0b\x0c\x1c")
    calls = []

    def evaluate(p, pool):
        calls.append(list(pool))
        return repair_values(p, pool)

    values, skipped = RS.repair_cells(program, ["12 patixnts", s, None, "12 patixnts", "7 patients" + chr(cp)], evaluate)
    assert values == ["12 patients", None, None, "12 patients", None] and skipped == 2
    assert calls == [["12 patixnts"]]                                                # every DISTINCT string once, the terminators never


# ---------------------------------------------------------------------------------------------- RepairModel.run()
OPTS = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2"}
PATTERN = "^[0-9]{1,3} patients$"
ON = {"model.rule.repair_by_regex.disabled": ""}


def _frame(n=300, seed=11, dirty=((5, "32 patixxts"), (17, "619 paxienxs"), (40, "x2 patixxts"))):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, n)
    sample = np.array([["10 patients", "20 patients", "32 patients", "619 patients"][v] for v in g], object)
    size = np.array([["s", "m", "l", "xl"][v] for v in g], object)
    ward = np.array(["w%d" % ((v + rng.integers(0, 2)) % 3) for v in g], object)
    df = pd.DataFrame({"tid": np.arange(n), "size": size, "ward": ward, "sample": sample})
    for r, v in dirty:
        df.loc[r, "sample"] = v
    return df


def _model(df, cells=None, engine=None, detectors=None, **opts):
    m = RepairModel().setInput(df).setRowId("tid").setRepairByRules(True).setTargets(["sample", "ward"])
    m = m.setErrorDetectors(detectors if detectors is not None else [RegExErrorDetector("sample", PATTERN)])
    if cells is not None:
        m = m.setErrorCells(cells)
    for k, v in dict(OPTS, **opts).items():
        m = m.option(k, str(v))
    m._engine_override = engine
    return m


def _sorted(df, repair_data=False):
    return df.sort_values(["tid"] if repair_data else ["tid", "attribute"]).reset_index(drop=True)


def _by_cell(df):
    return {(int(r[0]), r[1]): (r[2], r[3]) for r in df[["tid", "attribute", "current_value", "repaired"]].to_numpy(dtype=object)}


def test_value_space_run_repairs_by_structure(oracle_backend, monkeypatch):
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    df = _frame()
    out = _by_cell(_model(df, **ON).run())
    assert out[(5, "sample")] == ("32 patixxts", "32 patients") and out[(17, "sample")] == ("619 paxienxs", "619 patients")
    cur, rep = out[(40, "sample")]                               # the third cell goes to the model
    assert cur == "x2 patixxts" and rep in {"10 patients", "20 patients", "32 patients", "619 patients"}
    assert len(out) == 3
    # the repaired table: the repaired values are in it, and rows 5 and 17 are clean rows (they precede the dirty ones)
    data = _model(df, **ON).run(repair_data=True)
    assert data["tid"].tolist()[-1] == 40 and set(data["tid"].tolist()[:-1]) == set(range(300)) - {40}
    by_tid = data.set_index("tid")["sample"]
    assert by_tid[5] == "32 patients" and by_tid[17] == "619 patients" and by_tid[40] == rep
    # a clean row with a repaired value is a training row: with every other `619 patients` row gone, the class survives through row 17 alone
    only = df[(df["sample"] != "619 patients")].reset_index(drop=True)
    m = _model(only, **ON)
    seen = []
    orig = RepairModel._build_repair_models

    def spy(self, base, *a, **kw):
        seen.append(base[base["tid"] == 17]["sample"].tolist())
        return orig(self, base, *a, **kw)

    monkeypatch.setattr(RepairModel, "_build_repair_models", spy)
    m.run()
    assert seen == [["619 patients"]]
    monkeypatch.undo()
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    # disabled (the default): the frame of today -- all three cells are the model's
    off = _by_cell(_model(df).run())
    assert set(off) == set(out) and off[(5, "sample")][0] == "32 patixxts" and off[(5, "sample")][1] != "32 patixxts"
    assert all(rep in {"10 patients", "20 patients", "32 patients", "619 patients"} for _, rep in off.values())


def test_unparsable_pattern_and_two_detectors(oracle_backend, monkeypatch):
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    df = _frame()
    cells = pd.DataFrame([(5, "sample"), (17, "sample"), (40, "sample")], columns=["tid", "attribute"])
    # a pattern without a structure repairs nothing: the run is the disabled one
    bad = _by_cell(_model(df, cells, detectors=[RegExErrorDetector("sample", "^([0-9]+) patients$")], **ON).run())
    off = _by_cell(_model(df, cells).run())
    assert bad == off
    # two detectors on one attribute: the first that repairs a cell wins, the second takes what is left
    two = [RegExErrorDetector("sample", "^[0-9]{3} patients$"), RegExErrorDetector("sample", "[0-9]{1,2} people")]
    out = _by_cell(_model(df, cells, detectors=two, **ON).run())
    assert out[(17, "sample")][1] == "619 patients" and out[(5, "sample")][1] == "32 people" and out[(40, "sample")][1] == "2 people"


class RegexOracleEngine(RuleOracleEngine):
    """RuleOracleEngine with the value detectors' `detect_cells` restated in numpy and `regex_structure` = the statement."""
    regex_calls = 0

    class _Table(RuleOracleEngine._Table):
        def gather_rows(self, rows):
            return RegexOracleEngine._Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)

        def detect_cells(self, cols, null_is_error, keep_lo, keep_hi, flag_bits=None):
            return DR.detect_cells(self.codes, cols, null_is_error, keep_lo, keep_hi, flag_bits)

    def upload(self, codes, n_codes):
        return RegexOracleEngine._Table(codes, n_codes)

    def upload_dictionaries(self, indices, remaps):
        t = RuleOracleEngine.upload_dictionaries(self, indices, remaps)
        return RegexOracleEngine._Table(t.codes, t.n_codes, t.values, t.kinds)

    def regex_structure(self, program, strings):
        RegexOracleEngine.regex_calls += 1
        return repair_values(program, strings)


RESIDENT = {"model.rule.resident": "true", "model.rule.regex.resident": "true"}


def both_paths(make, engine, monkeypatch, detected, repair_data=False):
    """(value-space frame, resident frame, resident model); the frames are equal cell for cell."""
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = make(None, **ON).run(repair_data=repair_data)
    monkeypatch.delenv("REPAIR_RESIDENT")
    fast = make(engine, **dict(ON, **RESIDENT))
    frame = fast.run(repair_data=repair_data)
    assert getattr(fast, "_last_resident_info", None) is not None, "the run did not take the resident path"
    assert fast._last_detection_on_device is detected
    pd.testing.assert_frame_equal(_sorted(slow, repair_data), _sorted(frame, repair_data), check_exact=True)
    return slow, frame, fast


NEW_VALUE = ((5, "32 patixxts"), (17, "77 patixxts"), (40, "x2 patixxts"), (41, "77 patienxx"), (60, None))


@pytest.mark.parametrize("setup", ["given", "detected", "new value", "new value detected"])
@pytest.mark.parametrize("repair_data", [False, True])
def test_resident_frame_equals_the_value_space_frame(oracle_backend, monkeypatch, setup, repair_data):
    detected = setup.endswith("detected")
    df = _frame(dirty=NEW_VALUE) if setup.startswith("new value") else _frame()
    dets = [NullErrorDetector(), RegExErrorDetector("sample", PATTERN)]
    cells = None if detected else pd.DataFrame([(r, "sample") for r in (5, 17, 40, 41, 60) if not isinstance(df.loc[r, "sample"], str)
                                                or not df.loc[r, "sample"].endswith(" patients")] + [(7, "ward")], columns=["tid", "attribute"])
    extra = {"error.value_detectors.resident": "true"} if detected else {}
    before = RegexOracleEngine.regex_calls
    slow, frame, fast = both_paths(lambda engine, **o: _model(df, cells, engine, dets, **dict(o, **extra)), RegexOracleEngine(), monkeypatch,
                                   detected, repair_data)
    assert RegexOracleEngine.regex_calls == before + 1            # one pool: the distinct strings of the attribute's cells
    info = fast._last_resident_info
    rc = _by_cell(info["regex_cells"])
    if setup.startswith("new value"):
        assert rc == {(5, "sample"): ("32 patixxts", "32 patients"), (17, "sample"): ("77 patixxts", "77 patients"),
                      (41, "sample"): ("77 patienxx", "77 patients")}
        assert info["regex_repairs"] == {"sample": 3}
    else:
        assert rc == {(5, "sample"): ("32 patixxts", "32 patients"), (17, "sample"): ("619 paxienxs", "619 patients")}
    if not repair_data:
        out = _by_cell(frame)
        assert all(out[k] == v for k, v in rc.items()) and (40, "sample") in out and out[(40, "sample")][1] != "x2 patixxts"


def test_with_only_one_of_the_two_options_the_run_is_not_resident(oracle_backend):
    df = _frame()
    cells = pd.DataFrame([(5, "sample"), (17, "sample"), (40, "sample")], columns=["tid", "attribute"])
    assert "model.rule.regex.resident" in RepairModel.option_keys
    assert RepairModel()._get_option_value(*RepairModel._opt_rule_regex_resident) is False
    for opts in ({"model.rule.resident": "true"}, {"model.rule.regex.resident": "true"}):
        m = _model(df, cells, RegexOracleEngine(), **dict(ON, **opts))
        m.run()
        assert getattr(m, "_last_resident_info", None) is None
    m = _model(df, cells, RegexOracleEngine(), **dict(ON, **RESIDENT))
    m.run()
    assert m._last_resident_info is not None
