"""-m gpu: rgbm_regex_structure (csrc/rgbm_regex.hip) against the statement repair.regex_structure -- states, offsets and code points,
all integers, so equality -- every case first asserting the route it took from info_out; then `RepairModel.run()` with regex-structure
repair through the HIP engine on the resident path against the value-space path."""
import os

import numpy as np
import pandas as pd
import pytest

from repair.regex_structure import ANCHOR_END, ANCHOR_START, Capture, Constant, Program, parse, program_arrays, repair_value
from tests.regex_cases import class_bits, pooled_cases

pytestmark = pytest.mark.gpu

WORD = 63                   # the last one-word length
DIGITS = class_bits("0123456789")
LOWER = class_bits("abcdefghijklmnopqrstuvwxyz")


ERR_ARG = -1                # RGBM_ERR_ARG


def _cap():
    """RGBM_RX_WAVE_MAX_CP as the header has it (the wrapper's copy is held to it)."""
    import re
    from repair import _native as N
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rgbm.h")) as f:
        cap = int(re.search(r"#define\s+RGBM_RX_WAVE_MAX_CP\s+(\d+)", f.read()).group(1))
    assert N.RX_WAVE_MAX_CP == cap and N.RX_WORD_MAX_CP == WORD
    return cap


def _routes(strings):
    cap = _cap()
    n = [len(s) for s in strings]
    return [sum(l <= WORD for l in n), sum(WORD < l <= cap for l in n), sum(l > cap for l in n)]


def _check(program, strings, routes=None):
    """Device output == statement for every string: state, offsets, code points; the route report == the lengths' (and `routes`)."""
    from repair import _native as N
    a = program_arrays(program)
    cp, off = N.pack_code_points(strings)
    state, out_off, out, info = N.regex_structure_raw(a["segs"], a["anchors"], a["const_cp"], cp, off)
    assert info[:3].tolist() == _routes(strings)
    if routes is not None:
        assert info[:3].tolist() == list(routes)
    cap = _cap()
    want = [None if len(s) > cap else repair_value(program, s) for s in strings]
    want_state = [2 if len(s) > cap else int(w is not None) for s, w in zip(strings, want)]
    assert state.tolist() == want_state
    assert int(info[3]) == sum(v == 1 for v in want_state)
    lens = [len(w) if w is not None else 0 for w in want]
    assert out_off.tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(np.int64).tolist()
    assert out.tolist() == [ord(ch) for w in want if w is not None for ch in w]
    # the wrapper: state 2 goes to the statement
    assert N.regex_structure(program, strings) == [repair_value(program, s) for s in strings]
    return want


PATIENTS = parse("^[0-9]{1,3} patients$")


@pytest.mark.parametrize("length", [0, 1, 62, 63, 64, 65, 127, 128, 129, "cap", "cap+1"])
def test_lengths_at_the_route_edges(length):
    cap = _cap()
    L = {"cap": cap, "cap+1": cap + 1}.get(length, length)
    route = [1, 0, 0] if L <= WORD else ([0, 1, 0] if L <= cap else [0, 0, 1])
    # unanchored, a run of letters to the very end: the capture ends at the last position
    p1 = Program(ANCHOR_END, (Capture(DIGITS, 0, -1), Constant("--"), Capture(LOWER, 0, -1)))
    s = (("12" * L)[:L // 3] + "#" + ("ab" * L)[:max(L - L // 3 - 1, 0)])[:L]
    assert len(s) == L
    want = _check(p1, [s], route)
    assert (want[0] is not None) == (1 <= L <= cap)
    # anchored on both sides, the whole string one class
    p2 = Program(ANCHOR_START | ANCHOR_END, (Capture(LOWER, 0, -1),))
    want = _check(p2, ["a" * L], route)
    assert L > cap or want[0] == "a" * L
    _check(p2, ["a" * (L - 1) + "1" if L else ""], route)


def test_runs_and_captures_across_word_boundaries():
    # a digit run that starts before position 64 / 128 and ends after it, found unanchored in a longer string; constants that straddle too
    p = Program(0, (Capture(DIGITS, 3, 40), Constant("ab"), Capture(LOWER, 2, -1)))
    strings = []
    for start in (60, 61, 62, 63, 64, 120, 126, 127, 128, 190):
        for run in (3, 5, 40, 45):
            strings.append("#" * start + "9" * run + "#" + "z" * 70 + "!")
            strings.append("#" * start + "9" * run + "##" + "zz")
            strings.append("#" * start + "9" * run + "##" + "z")           # the last capture needs two
    want = _check(p, strings, [0, len(strings), 0])
    assert sum(w is not None for w in want) > len(strings) // 2 and any(w is None for w in want)
    # the greedy pick has to come back across a boundary: digits {0,}, then exactly two digits, then `$`
    q = Program(ANCHOR_START | ANCHOR_END, (Capture(DIGITS, 0, -1), Constant("-"), Capture(DIGITS, 2, 2)))
    strings = ["1" * a + "." + "22" for a in (61, 62, 63, 64, 65, 125, 126, 127, 128)] + ["1" * 66, "1" * 130]
    want = _check(q, strings, [0, len(strings), 0])
    assert want[0] == "1" * 61 + "-22" and want[-1] == "1" * 127 + "-11"   # all digits: the constant takes one of them


@pytest.mark.parametrize("n_segs", [1, 32])
def test_segment_counts(n_segs):
    segs = tuple(Capture(DIGITS, 1, 2) if i % 2 == 0 else Constant("-") for i in range(n_segs))
    p = Program(ANCHOR_START, segs)
    short = ".".join(["12"] * 16)                 # 47 code points: 16 captures, 15 constants; the 32nd segment takes the last digit back
    full = short + ":"                            # ... and now it need not
    long_ = ".".join(["12"] * 16) + ":" + "#" * 100
    none = ".".join(["12"] * 15) + ".1"           # no way to give the 32nd segment a code point
    want = _check(p, [short, full, long_, "1", "", none], [5, 1, 0])
    if n_segs == 32:
        assert want[:3] == ["-".join(["12"] * 15) + "-1-", "-".join(["12"] * 16) + "-", "-".join(["12"] * 16) + "-"]
        assert want[3] is None and want[5] is None
    else:
        assert want[:4] == ["12", "12", "12", "1"] and want[4] is None and want[5] == "12"


def test_unbounded_max_on_one_long_run():
    cap = _cap()
    p = Program(ANCHOR_START | ANCHOR_END, (Capture(LOWER, 1, -1), Constant("!")))
    strings = ["q" * (cap - 1) + "?", "q" * cap, "q" * 63, "q" * 64, "q" * 62 + "?"]
    want = _check(p, strings, [2, 3, 0])
    assert want[0] == "q" * (cap - 1) + "!" and want[1] == "q" * (cap - 1) + "!" and want[2] == "q" * 62 + "!"


def test_constants_of_length_one_and_longer_than_the_string():
    p = Program(ANCHOR_START | ANCHOR_END, (Capture(DIGITS, 1, 3), Constant("%")))
    want = _check(p, ["33x", "x2%", "1234", "5", "55"], [5, 0, 0])
    assert want == ["33%", None, "123%", None, "5%"]
    p = Program(ANCHOR_START | ANCHOR_END, (Constant("a constant far longer than any string here" * 3),))
    want = _check(p, ["", "x", "xy", "z" * 70, "z" * 200], [3, 2, 0])
    assert want[0] is None and want[1] == want[2] == want[3] == p.segs[0].text and want[4] is None


def test_code_points_beyond_ascii_are_wildcards_never_class_members():
    every = (1 << 128) - 1
    p = Program(ANCHOR_START | ANCHOR_END, (Capture(every, 1, -1), Constant("_"), Capture(every, 0, -1)))
    specials = [chr(127), chr(128), chr(0xFFFF), chr(0x1F600)]
    strings = ["a" + ch + "b" for ch in specials] + [ch for ch in specials] + ["a" + ch for ch in specials]
    strings += ["a" * 70 + ch + "b" * 70 for ch in specials]
    want = _check(p, strings, [12, 4, 0])
    assert want[0] == "a\x7f_"                    # 127 is a class member: the greedy capture takes it, the constant takes the b
    assert want[1] == want[2] == want[3] == "a_b"  # the others end the capture and are the constant's
    assert want[4:8] == [None] * 4                # one code point: a capture and a constant need two
    assert want[8:12] == ["a_"] * 4
    assert want[12] == "a" * 70 + "\x7f" + "b" * 69 + "_" and want[13] == want[14] == want[15] == "a" * 70 + "_" + "b" * 70


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_pools_of_many_sizes_and_mixed_routes(n):
    cap = _cap()
    rng = np.random.default_rng(n)
    strings = []
    for i in range(n):
        k = int(rng.integers(0, 4))
        body = "%d patients" % int(rng.integers(0, 5000)) if k else "patients %d" % i
        if k == 2:
            body = body.replace("e", "x")
        if i % 97 == 5:
            body = body + " " * 100               # the wave route (the `$` then fails) ...
        if i % 97 == 6:
            body = "7" + " patients".ljust(120, "s")[:120]
        if i % 331 == 7:
            body = "#" * (cap + 1 + i % 3)        # ... and beyond it
        strings.append(body)
    want = _check(PATIENTS, strings)
    if n >= 63:
        assert any(w is not None for w in want) and any(w is None for w in want)
    if n == 1000:
        assert min(_routes(strings)) > 0
    # nothing matches: an empty output
    from repair import _native as N
    a = program_arrays(PATIENTS)
    cp, off = N.pack_code_points(["nothing here"] * n)
    state, out_off, out, info = N.regex_structure_raw(a["segs"], a["anchors"], a["const_cp"], cp, off)
    assert not state.any() and not out_off.any() and len(out) == 0 and info.tolist() == [n, 0, 0, 0]


def test_bad_arguments():
    import ctypes as C
    from repair import _native as N
    lib = N.lib()
    good = [(0, 1, 3, (0, 0x03FF0000, 0, 0), 0, 0), (1, 1, 2, (0, 0, 0, 0), 0, 2)]
    cp, off = N.pack_code_points(["12ab", "x"])

    def code(segs=good, anchors=3, const_cp=(97, 98), off_=off, n_segs=None, null=None):
        arr = (N.RxSeg * 40)()
        for i, (kind, mn, mx, cls, c_off, c_len) in enumerate(segs):
            arr[i] = N.RxSeg(kind, mn, mx, (C.c_uint32 * 4)(*cls), c_off, c_len)
        cc = np.asarray(const_cp, np.int32)
        o = np.asarray(off_, np.int64)
        n = len(o) - 1
        state, out_off, out, info = np.zeros(n + 1, np.uint8), np.zeros(n + 2, np.int64), np.zeros(64, np.int32), np.zeros(4, np.int64)
        args = dict(segs=arr, const_cp=N._p(cc, C.c_int32), cp=N._p(cp, C.c_int32), off=N._p(o, C.c_int64), state=N._p(state, C.c_uint8),
                    out_off=N._p(out_off, C.c_int64), out=N._p(out, C.c_int32), info=N._p(info, C.c_int64))
        if null:
            args[null] = None
        return lib.rgbm_regex_structure(C.c_int32(0), args["segs"], C.c_int32(len(segs) if n_segs is None else n_segs), C.c_int32(anchors),
                                        args["const_cp"], C.c_int32(len(cc)), args["cp"], args["off"], C.c_int64(n), args["state"],
                                        args["out_off"], args["out"], args["info"])

    err_arg = ERR_ARG
    assert code() == 0
    for k in ("segs", "cp", "off", "state", "out_off", "out", "info", "const_cp"):
        assert code(null=k) == err_arg, k
    assert code(n_segs=0) == err_arg and code(segs=good * 17) == err_arg and code(n_segs=-1) == err_arg
    assert code(anchors=4) == err_arg and code(anchors=-1) == err_arg
    cap = lambda mn, mx: [(0, mn, mx, (0, 0x03FF0000, 0, 0), 0, 0)]  # noqa: E731
    for mn, mx in [(-1, 3), (3, 2), (0, -2), (0, 65536), (65536, -1)]:
        assert code(segs=cap(mn, mx), const_cp=()) == err_arg, (mn, mx)
    assert code(segs=cap(0, -1), const_cp=()) == 0 and code(segs=cap(65535, 65535), const_cp=()) == 0
    con = lambda mn, mx, o, l: [(1, mn, mx, (0, 0, 0, 0), o, l)]  # noqa: E731
    for mn, mx, o, l in [(1, 2, 1, 2), (1, 2, -1, 2), (1, 0, 0, 0), (0, 2, 0, 2), (1, 1, 0, 2), (1, 3, 0, 3)]:
        assert code(segs=con(mn, mx, o, l)) == err_arg, (mn, mx, o, l)
    assert code(segs=con(1, 2, 0, 2) + con(1, 1, 1, 1)) == err_arg          # overlapping constants
    assert code(segs=[(2, 1, 1, (0, 0, 0, 0), 0, 0)]) == err_arg
    assert code(off_=[0, 4, 3]) == err_arg and code(off_=[1, 4, 5]) == err_arg
    assert code(off_=[0]) == 0                                              # n == 0 is legal


def test_random_cases_equal_the_statement():
    from repair import _native as N
    cases = pooled_cases()                        # 5 000 of the cases the CPU suite holds to `re.search`, eight strings to a program
    by_program = {}
    for prog, s in cases:
        by_program.setdefault(prog, []).append(s)
    assert len(cases) == 5000 and len(by_program) >= 500
    matched = 0
    # every hundredth program also sees a pool of all lengths up to the wave route
    pool = [s for _, s in cases[:100]] + [s * 9 for _, s in cases[:20]]
    for j, (prog, own) in enumerate(by_program.items()):
        strings = own + (pool if j % 100 == 0 else [])
        got = N.regex_structure(prog, strings)
        want = [repair_value(prog, s) for s in strings]
        assert got == want, prog
        matched += sum(w is not None for w in want[:len(own)])
    assert len(cases) // 5 <= matched <= 4 * len(cases) // 5


@pytest.mark.parametrize("detected", [False, True])
def test_run_through_the_hip_engine_equals_the_value_space_path(detected):
    from repair.engine import HipEngine
    from repair.errors import NullErrorDetector, RegExErrorDetector
    from repair.model import RepairModel
    rng = np.random.default_rng(11)
    n = 300
    g = rng.integers(0, 4, n)
    df = pd.DataFrame({"tid": np.arange(n), "size": np.array([["s", "m", "l", "xl"][v] for v in g], object),
                       "ward": np.array(["w%d" % ((v + rng.integers(0, 2)) % 3) for v in g], object),
                       "sample": np.array([["10 patients", "20 patients", "32 patients", "619 patients"][v] for v in g], object)})
    for r, v in ((5, "32 patixxts"), (17, "77 patixxts"), (40, "x2 patixxts"), (41, "77 patienxx"), (60, None)):
        df.loc[r, "sample"] = v
    cells = None if detected else pd.DataFrame([(r, "sample") for r in (5, 17, 40, 41, 60)] + [(7, "ward")], columns=["tid", "attribute"])

    def make(**opts):
        m = RepairModel().setInput(df).setRowId("tid").setRepairByRules(True).setTargets(["sample", "ward"]) \
            .setErrorDetectors([NullErrorDetector(), RegExErrorDetector("sample", "^[0-9]{1,3} patients$")])
        if cells is not None:
            m = m.setErrorCells(cells)
        base = {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2", "model.rule.repair_by_regex.disabled": ""}
        for k, v in dict(base, **opts).items():
            m = m.option(k, v)
        return m

    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        a = make().run()
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    fast = make(**{"model.rule.resident": "true", "model.rule.regex.resident": "true", "error.value_detectors.resident": "true"})
    fast._engine_override = HipEngine(0)
    b = fast.run()
    info = getattr(fast, "_last_resident_info", None)
    assert info is not None, "the run did not take the resident path"
    assert fast._last_detection_on_device is detected
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(a.sort_values(key).reset_index(drop=True), b.sort_values(key).reset_index(drop=True), check_exact=True)
    assert info["regex_repairs"] == {"sample": 3}
    got = {int(r[0]): r[3] for r in b[b["attribute"] == "sample"].to_numpy(dtype=object)}
    assert got[5] == "32 patients" and got[17] == got[41] == "77 patients" and got[40] != "x2 patixxts" and 60 in got
