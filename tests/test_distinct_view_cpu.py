"""CPU: the host side of the distinct-row view of rgbm_table_train.

1. `rgbm_distinct_view_eligible` -- may a fit of this shape train on the view -- against a restatement of what the multiplicity trainer
   honours, over depths, feature counts 1..33, bagging, flags, objectives, the table's own multiplicities and row counts on both sides of the
   floor;
2. the ABI: both new symbols are exported, the params struct keeps its 104 bytes, RGBM_FLAG_WHOLE_TABLE is bit 2 of `reserved`."""
import ctypes as C
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FLAG_ROW_SHARDED, FLAG_NO_MODEL, FLAG_WHOLE_TABLE = 1, 2, 4
DEFAULT_MIN_ROWS = 1 << 20


def may_use_view(rows, f, p, table_has_mult, min_rows):
    """The restatement: level grower, classifier, no bagging, whole-table call, a free byte 15 in the last record, enough rows."""
    if table_has_mult or p["reserved"] & (FLAG_ROW_SHARDED | FLAG_WHOLE_TABLE):
        return False
    if not 1 <= p["max_depth"] <= 7:
        return False
    if p["bagging_freq"] > 0 and p["bagging_fraction"] < 1.0:
        return False
    if p["objective"] not in (0, 1):
        return False
    if not 1 <= f <= 32 or f % 16 == 0:
        return False
    return rows >= (min_rows if min_rows > 0 else DEFAULT_MIN_ROWS)


def test_eligibility_equals_its_restatement():
    from repair import _native as N
    n_true = n = 0
    grid = itertools.product((-1, 0, 1, 7, 8), range(0, 34), ((0, 1.0), (1, 1.0), (1, 0.5), (0, 0.5)), (0, 1, 2, 4, 5), (0, 1, 2),
                             (False, True))
    for depth, f, (bfreq, bfrac), reserved, objective, has_mult in grid:
        for rows, min_rows in ((999, 1000), (1000, 1000), (1001, 1000), (1, 1), (DEFAULT_MIN_ROWS - 1, 0), (DEFAULT_MIN_ROWS, 0),
                               (DEFAULT_MIN_ROWS, -5), (1 << 31, 0)):
            p = dict(max_depth=depth, bagging_freq=bfreq, bagging_fraction=bfrac, reserved=reserved, objective=objective)
            got = N.distinct_view_eligible(rows, f, table_has_mult=has_mult, min_rows=min_rows, **p)
            want = may_use_view(rows, f, p, has_mult, min_rows)
            assert got == want, (rows, min_rows, f, p, has_mult)
            n += 1
            n_true += want
    assert n_true > 1000 and n - n_true > 1000                     # both answers are exercised


def test_whole_table_flag_and_bad_argument():
    from repair import _native as N
    assert N.make_params(whole_table=True).reserved == FLAG_WHOLE_TABLE == N.FLAG_WHOLE_TABLE
    assert N.make_params(whole_table=True, row_sharded=True).reserved == FLAG_WHOLE_TABLE | FLAG_ROW_SHARDED
    assert N.distinct_view_eligible(1 << 20, 15, max_depth=7) and not N.distinct_view_eligible(1 << 20, 15, max_depth=7, whole_table=True)
    assert N.lib().rgbm_distinct_view_eligible(C.c_int64(10), C.c_int32(3), None, C.c_int32(0), C.c_int64(1)) == -1     # RGBM_ERR_ARG
    assert N.lib().rgbm_table_distinct_view_info(None, None, None, None) == -1


def test_abi_new_symbols_and_params_size():
    from repair import _native as N
    lib = N.lib()
    for name in ("rgbm_table_distinct_view_info", "rgbm_distinct_view_eligible"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.RgbmParams) == 104
    src = open(os.path.join(ROOT, "include", "rgbm.h")).read()
    assert re.search(r"#define\s+RGBM_FLAG_WHOLE_TABLE\s+4\b", src)
    for name in ("rgbm_table_distinct_view_info", "rgbm_distinct_view_eligible"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src)
