"""CPU: the signature table of repair/_native.py is include/rgbm.h, type by type; the five struct mirrors have the layout the C
compiler gives the header's structs; and ctypes, armed with the table, refuses what the header does not declare."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rgbm.h")


def _header():
    """include/rgbm.h without comments and preprocessor lines."""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("#"))


def _ctype(text):
    """A C type in one spelling: 'const rgbm_model* const*', 'int64_t'."""
    return re.sub(r"\*(?=\w)", "* ", re.sub(r"\s*\*", "*", " ".join(text.split())))


def _prototypes():
    """{name: (return type, [parameter types])} of every `ret name(args);` of the header."""
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(rgbm_\w+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in out, name
        params = []
        for a in [a.strip() for a in args.split(",")]:
            if a == "void":
                assert args.strip() == "void"
                continue
            m = re.match(r"^(.*[\s\*])(\w+)$", a, flags=re.S)
            assert m, "parameter %r of %s has no name" % (a, name)
            params.append(_ctype(m.group(1)))
        out[name] = (_ctype(ret), params)
    return out


def _c_types():
    from repair import _native as N
    P = C.POINTER
    handle, handles = C.c_void_p, P(C.c_void_p)
    return {
        "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t,
        "const int32_t*": P(C.c_int32), "int32_t*": P(C.c_int32), "const int64_t*": P(C.c_int64), "int64_t*": P(C.c_int64),
        "const double*": P(C.c_double), "double*": P(C.c_double), "const uint8_t*": P(C.c_uint8), "uint8_t*": P(C.c_uint8),
        "uint64_t*": P(C.c_uint64), "size_t*": P(C.c_size_t),
        "const int32_t* const*": P(P(C.c_int32)), "const uint64_t* const*": P(P(C.c_uint64)),
        "void*": handle, "const void*": handle, "void**": handles,
        "rgbm_table*": handle, "const rgbm_table*": handle, "rgbm_model*": handle, "const rgbm_model*": handle,
        "rgbm_table**": handles, "rgbm_model**": handles, "const rgbm_table* const*": handles, "const rgbm_model* const*": handles,
        "const rgbm_params*": P(N.RgbmParams), "rgbm_train_stats*": P(N.RgbmTrainStats), "const rgbm_fit_spec*": P(N.RgbmFitSpec),
        "const rgbm_dc_pred*": P(N.DcPred), "const rgbm_rx_seg*": P(N.RxSeg),
    }


RETURN_TYPES = {"int": C.c_int, "void": None, "const char*": C.c_char_p}


def test_every_function_carries_the_signature_of_the_header():
    from repair import _native as N
    lib, protos, types = N.lib(), _prototypes(), _c_types()
    assert len(protos) >= 92
    assert sorted(protos) == sorted(N.SIGNATURES) == sorted(N.EXPORTED_SYMBOLS) and len(set(N.EXPORTED_SYMBOLS)) == len(N.EXPORTED_SYMBOLS)
    used = set()
    for name, (ret, params) in protos.items():
        for t in params:
            assert t in types, "%s: no ctypes type is known for the parameter type %r" % (name, t)
        assert ret in RETURN_TYPES, "%s: no ctypes type is known for the return type %r" % (name, ret)
        used.update(params)
        fn = getattr(lib, name)
        assert fn.argtypes is not None, "%s carries no argtypes" % name
        assert fn.restype == RETURN_TYPES[ret], (name, fn.restype, ret)
        assert tuple(fn.argtypes) == tuple(types[t] for t in params), (name, fn.argtypes, params)
        assert N.SIGNATURES[name] == (fn.restype, tuple(fn.argtypes)), name
    assert used == set(types), "the type dictionary holds types the header no longer uses: %s" % sorted(set(types) - used)


STRUCTS = {"rgbm_params": "RgbmParams", "rgbm_train_stats": "RgbmTrainStats", "rgbm_fit_spec": "RgbmFitSpec", "rgbm_dc_pred": "DcPred",
           "rgbm_rx_seg": "RxSeg"}


def _struct_fields():
    """{struct: [field names in order]} of the header's `typedef struct [tag] { .. } name;` blocks."""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _header()):
        fields = []
        for decl in [d.strip() for d in body.split(";") if d.strip()]:
            first, *more = decl.split(",")
            for d in [first.split()[-1]] + more:
                fields.append(re.sub(r"\[.*\]", "", d).replace("*", "").strip())
        out[name] = fields
    return out


def test_struct_mirrors_have_the_layout_of_the_header(tmp_path):
    from repair import _native as N
    cc = shutil.which(os.environ.get("CC", "cc")) or shutil.which("gcc")
    assert cc, "no host C compiler"
    fields = _struct_fields()
    assert sorted(fields) == sorted(STRUCTS)
    lines = ['#include <stdio.h>', '#include "rgbm.h"', "int main(void) {"]
    for s, names in fields.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in names:
            lines.append('    printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (s, f, s, f, s, f))
    lines += ["    return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.check_call([cc, "-I", os.path.dirname(HEADER), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")])
    got = subprocess.check_output([str(tmp_path / "layout")]).decode().split("\n")
    want = []
    for s, names in fields.items():
        cls = getattr(N, STRUCTS[s])
        assert [f[0] for f in cls._fields_] == names, s                     # order and count
        want.append("%s %d" % (s, C.sizeof(cls)))
        want += ["%s.%s %d %d" % (s, f, getattr(cls, f).offset, getattr(cls, f).size) for f in names]
    assert [l for l in got if l] == want


@pytest.fixture(scope="module")
def model():
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(0)
    X = rng.integers(0, 5, (3, 500)).astype(np.int32); y = (X[0] + X[1]) % 3
    return N.Model.load(O.train(X, [5, 5, 5], y, 3, objective=1, num_class=3, n_estimators=5, min_data_in_leaf=5).save())


def _deviceless_calls(model):
    """(name, well-formed arguments, position of an int32_t* argument) of entry points that need no device."""
    from repair import _native as N
    i32 = lambda n: N._p(np.zeros(n, np.int32), C.c_int32)  # noqa: E731
    plan = np.zeros(6 + 12 * 4096, np.float64)
    return [("rgbm_model_info", [model.h, i32(5)], 1),
            ("rgbm_model_predict_form", [model.h, i32(5)], 1),
            ("rgbm_level_pass_plan", [N._p(np.asarray([16, 32, 7], np.int32), C.c_int32), 3, 5000, 2, 7, 0, N._p(plan, C.c_double), len(plan), C.byref(C.c_int32(0))], 0),
            ("rgbm_table_fd_measures_report", [None, i32(2), 0], 1),
            ("rgbm_table_recode_report", [None, i32(1), 0], 1),
            ("rgbm_table_pair_counts_report", [None, N._p(np.zeros(6, np.int64), C.c_int64), i32(3), 0], 2)]


def test_a_pointer_or_scalar_of_another_type_is_refused(model):
    from repair import _native as N
    lib = N.lib()
    wrong = N._p(np.ones(8, np.int64), C.c_int64)                             # POINTER(c_int64) where int32_t* is declared
    for name, args, at in _deviceless_calls(model):
        fn = getattr(lib, name)
        assert fn(*args) == 0, name                                           # the well-formed call goes through
        with pytest.raises(C.ArgumentError):
            fn(*(args[:at] + [wrong] + args[at + 1:]))
    out = np.zeros(3, np.float64)
    assert lib.rgbm_model_importance(model.h, 1, N._p(out, C.c_double)) == 0
    with pytest.raises(C.ArgumentError):
        lib.rgbm_model_importance(model.h, 1, wrong)                          # int64_t* where double* is declared
    with pytest.raises(C.ArgumentError):
        lib.rgbm_model_importance(model.h, 1.0, N._p(out, C.c_double))        # a float where int32_t is declared
    p = N.make_params()
    assert lib.rgbm_distinct_view_eligible(1 << 20, 3, C.byref(p), 0, 0) == 1
    with pytest.raises(C.ArgumentError):
        lib.rgbm_distinct_view_eligible(1048576.0, 3, C.byref(p), 0, 0)       # a float where int64_t is declared
    with pytest.raises(C.ArgumentError):
        lib.rgbm_distinct_view_eligible(1 << 20, 3, wrong, 0, 0)              # int64_t* where rgbm_params* is declared


def test_a_call_with_an_argument_too_few_is_refused(model):
    from repair import _native as N
    lib = N.lib()
    for name, args, _ in _deviceless_calls(model):
        with pytest.raises(TypeError):
            getattr(lib, name)(*args[:-1])
    with pytest.raises(TypeError):
        lib.rgbm_model_importance(model.h, 1)
    with pytest.raises(TypeError):
        lib.rgbm_distinct_view_eligible(1 << 20, 3, C.byref(N.make_params()), 0)
    with pytest.raises(TypeError):
        N._call("rgbm_model_info", model.h)


def test_p_checks_what_it_casts():
    from repair import _native as N
    with pytest.raises(TypeError):
        N._p(np.zeros(3, np.int64), C.c_int32)
    with pytest.raises(TypeError):
        N._p(np.zeros(3, np.float32), C.c_double)
    with pytest.raises(TypeError):
        N._p(np.zeros(6, np.int32)[::2], C.c_int32)                           # a strided view
    with pytest.raises(TypeError):
        N._p(np.zeros((3, 4), np.int32).T, C.c_int32)                         # a transposed (Fortran-ordered) view
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert N._p(None, C.c_int32) is None and N._p(a, C.c_int32)[5] == 5 and N._p(a[1], C.c_int32)[0] == 4
    for t, d in ((C.c_int32, np.int32), (C.c_int64, np.int64), (C.c_double, np.float64), (C.c_uint8, np.uint8), (C.c_uint64, np.uint64)):
        assert isinstance(N._p(np.zeros(2, d), t), C.POINTER(t))


BIG_ROWS = (1 << 32) + 5000          # its low 32 bits are 5000


def test_64_bit_scalars_arrive_whole():
    from repair import _native as N
    assert BIG_ROWS & 0xFFFFFFFF == 5000
    plans = [N.level_pass_plan([16, 32, 7], rows, 2) for rows in (BIG_ROWS, np.int64(BIG_ROWS), 5000)]
    assert plans[0] == plans[1] and plans[0] != plans[2]
    # the modelled row-loop time of a root workgroup is rows / root_gx times a constant: it tells 2^32 + 5000 rows from 5000
    per_row = [p["root_t_rows_us"] * p["root_gx"] / rows for p, rows in zip(plans, (BIG_ROWS, BIG_ROWS, 5000))]
    assert per_row[0] == pytest.approx(per_row[2], rel=1e-12) and per_row[0] > 0
    # 5000 rows are below the view's default threshold of 2^20 rows, 2^32 + 5000 are not
    assert N.distinct_view_eligible(BIG_ROWS, 5) is True and N.distinct_view_eligible(np.int64(BIG_ROWS), 5) is True
    assert N.distinct_view_eligible(5000, 5) is False
    # ... and min_rows is the other int64_t: 2^32 + 5000 masked to 32 bits would let 6000 rows pass
    assert N.distinct_view_eligible(6000, 5, min_rows=BIG_ROWS) is False and N.distinct_view_eligible(6000, 5, min_rows=np.int64(BIG_ROWS)) is False
    assert N.distinct_view_eligible(6000, 5, min_rows=5000) is True


def test_a_symbol_the_library_lacks_is_named_when_it_is_called():
    from repair import _native as N
    assert not hasattr(N.lib(), "rgbm_no_such_entry")
    with pytest.raises(N.RepairGbmError, match="rgbm_no_such_entry") as ei:
        N._call("rgbm_no_such_entry", 1, 2)
    assert os.path.basename(N.lib()._name) in str(ei.value)
