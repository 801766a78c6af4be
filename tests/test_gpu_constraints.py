"""-m gpu: rgbm_table_detect_dc and rgbm_table_detect_row_bits (csrc/rgbm_dc.hip) against their numpy restatements
(tests/dc_restatement.py) -- integers, so equality of rows and columns, order included -- a 20 001-row table the host detector refuses,
and `RepairModel.run()` with `error.constraints.resident` through the HIP engine against the value-space path."""

import numpy as np
import pandas as pd
import pytest

from repair import detect_codes as DC
from tests import dc_restatement as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

G, A, B, C_ = 0, 1, 2, 3                       # columns: the group attribute, two ranked attributes, a small one
NA, NB, NC = 7, 65, 3


def _tiles():
    """(t1 rows per workgroup, t2 rows per LDS tile) of the pair kernel: the constants of the source, not copies of them."""
    return tuple(csrc_constant(k) for k in ("DC_T1", "DC_T2"))


def _groups(n, shape, rng):
    """Group id per row, in shuffled row order.  'mixed': groups of exactly the t1 tile, the LDS t2 tile and each +-1 as far as they fit
    (largest first), the rest in groups of 1, 2, 3, 5, 64, 65."""
    if shape == "singletons":
        return rng.permutation(n).astype(np.int32)
    if shape == "one":
        return np.zeros(n, np.int32)
    t1, t2 = _tiles()
    sizes, left = [], n
    for s in (t2 + 1, t2, t2 - 1, t1 + 1, t1, t1 - 1):
        if s <= left:
            sizes.append(s)
            left -= s
    small = [1, 2, 3, 5, 64, 65]
    k = 0
    while left > 0:
        s = min(small[k % len(small)], left)
        sizes.append(s)
        left -= s
        k += 1
    return rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)


def _table(n, shape, seed):
    """Random codes with 10 % NULLs in the three value columns (the group column: 10 % NULLs in the 'mixed' shape, where NULL is one more
    group); the value columns NULL at both ends and either side of every tile edge of the pair kernel."""
    rng = np.random.default_rng(seed)
    g = _groups(n, shape, rng)
    ng = int(g.max()) + 1
    cols = [g, rng.integers(0, NA, n), rng.integers(0, NB, n), rng.integers(0, NC, n)]
    codes = np.stack(cols).astype(np.int32)
    codes[1:][rng.random((3, n)) < 0.1] = -1
    if shape == "mixed":
        codes[0][rng.random(n) < 0.1] = -1
    t1, t2 = _tiles()
    edges = [r for r in (0, n - 1, t1 - 1, t1, t2 - 1, t2, 2 * t2 - 1, 2 * t2) if 0 <= r < n]
    codes[1:, edges] = -1
    return codes, [ng, NA, NB, NC]


def _ranks(seed):
    """Rank arrays with ties and "no number" entries for A and B, and a pair in one merged order for LT(A, B)."""
    rng = np.random.default_rng(seed)
    ra = rng.integers(-1, 4, NA).astype(np.int32)
    rb = rng.integers(-1, 20, NB).astype(np.int32)
    ra[0], rb[NB - 1] = -1, -1
    return ra, rb


def _pred_sets(seed):
    ra, rb = _ranks(seed)
    sixteen = [("EQ", G, G, None, None), ("IQ", C_, C_, None, None), ("LT", A, A, ra, ra), ("GT", B, B, None, None), ("LT", A, B, ra, rb),
               ("GT", B, A, rb, ra), ("IQ", A, A, None, None), ("LT", B, B, rb, rb), ("GT", A, A, None, None), ("IQ", B, B, None, None),
               ("LT", A, A, None, None), ("GT", B, B, rb, rb), ("EQ", G, G, None, None), ("LT", A, B, None, None), ("IQ", C_, C_, None, None),
               ("GT", B, A, None, None)]
    return {
        "2 IQ": [("IQ", A, A, None, None), ("IQ", C_, C_, None, None)],
        "EQ + 2 IQ": [("EQ", G, G, None, None), ("IQ", A, A, None, None), ("IQ", C_, C_, None, None)],
        "EQ, GT, LT": [("EQ", G, G, None, None), ("GT", A, A, None, None), ("LT", B, B, None, None)],
        "EQ, GT, LT ranked": [("EQ", G, G, None, None), ("GT", A, A, ra, ra), ("LT", B, B, rb, rb)],
        "EQ, LT across": [("EQ", G, G, None, None), ("LT", A, B, ra, rb)],
        "2 LT": [("LT", A, A, None, None), ("LT", B, B, rb, rb)],
        "2 LT nobody": [("LT", A, A, None, None), ("GT", A, A, None, None)],
        "EQ only": [("EQ", G, G, None, None), ("EQ", C_, C_, None, None)],
        "16": sixteen,
    }


def _check(tab, codes, n_codes, preds, cell_cols=()):
    want = R.detect_dc(codes, n_codes, preds, cell_cols)
    got = tab.detect_dc(preds, cell_cols=cell_cols)
    if len(cell_cols):
        assert got[0].dtype == np.int64 and got[1].dtype == np.int32
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    else:
        assert got.dtype == np.int64 and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 4097])
def test_detect_dc_equals_the_restatement(n):
    from repair import _native as N
    for shape in ("singletons", "one", "mixed"):
        codes, n_codes = _table(n, shape, seed=n)
        tab = N.Table(codes, n_codes)
        for name, preds in _pred_sets(n).items():
            got = _check(tab, codes, n_codes, preds)
            if name == "EQ only":
                assert len(got) == n                      # t2 = t1 satisfies every EQ
            if name == "2 LT nobody":
                assert len(got) == 0
        rows, cols = _check(tab, codes, n_codes, _pred_sets(n)["EQ, GT, LT"], cell_cols=[B, G])
        assert cols.tolist() == [B] * (len(rows) // 2) + [G] * (len(rows) // 2)


@pytest.mark.parametrize("shape", ["one", "mixed"])
def test_detect_dc_over_several_launches(monkeypatch, shape):
    """A per-launch pair budget of one LDS tile per workgroup: the t2 range is walked in many launches, the later ones starting from the
    rows already marked."""
    from repair import _native as N
    n = 4097
    monkeypatch.setenv("RGBM_DC_LAUNCH_PAIRS", str(n * _tiles()[1]))
    codes, n_codes = _table(n, shape, seed=5)
    tab = N.Table(codes, n_codes)
    sets = _pred_sets(5)
    for name in ("2 IQ", "EQ, GT, LT ranked", "2 LT", "2 LT nobody", "16"):
        _check(tab, codes, n_codes, sets[name])


def test_max_pairs_is_checked_before_any_pair(monkeypatch):
    from repair import _native as N
    codes, n_codes = _table(1000, "mixed", seed=9)
    tab = N.Table(codes, n_codes)
    preds = _pred_sets(9)["EQ, GT, LT"]
    pairs = R.group_pairs(codes, n_codes, preds)
    before = tab.detect_nulls([A, B])
    with pytest.raises(N.RepairGbmError) as e:
        tab.detect_dc(preds, cell_cols=[A], max_pairs=pairs - 1)
    assert e.value.code == -2                            # RGBM_ERR_PARAM
    kept = tab._fetch_cells(len(before[0]), True)        # the table's previous result is intact
    assert np.array_equal(kept[0], before[0]) and np.array_equal(kept[1], before[1])
    got = tab.detect_dc(preds, max_pairs=pairs)
    assert np.array_equal(got, R.detect_dc(codes, n_codes, preds))
    # no EQ predicate: one group, n^2 pairs
    alone = _pred_sets(9)["2 LT"]
    assert R.group_pairs(codes, n_codes, alone) == 1000 * 1000
    with pytest.raises(N.RepairGbmError) as e:
        tab.detect_dc(alone, max_pairs=1000 * 1000 - 1)
    assert e.value.code == -2
    assert np.array_equal(tab.detect_dc(alone, max_pairs=1000 * 1000), R.detect_dc(codes, n_codes, alone))


def test_detect_dc_argument_errors():
    from repair import _native as N
    codes, n_codes = _table(100, "mixed", seed=1)
    tab = N.Table(codes, n_codes)
    ra, rb = _ranks(1)
    for preds in ([("IQ", A, A, None, None)],                                           # fewer than two predicates
                  [("IQ", A, A, None, None)] * 17,
                  [("EQ", A, B, None, None), ("IQ", C_, C_, None, None)],               # EQ across two attributes
                  [("EQ", G, G, None, None), ("IQ", A, A, ra, ra)],                     # IQ with rank arrays
                  [("EQ", G, G, None, None), ("LT", A, 4, None, None)],                 # column out of range
                  [("EQ", G, G, None, None), ("LT", -1, A, None, None)]):
        with pytest.raises(N.RepairGbmError) as e:
            tab.detect_dc(preds)
        assert e.value.code == -1                        # RGBM_ERR_ARG


# ---------------------------------------------------------------------------------------------- single-tuple constraints
CODES = [1, 63, 64, 65, 129]                   # codes per column: with the NULL bit, the edges of the 64-bit bitset words


def _bit_table(n, seed):
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, k, n) for k in CODES]).astype(np.int32)
    codes[rng.random(codes.shape) < 0.1] = -1
    edges = [r for r in (0, n - 1, 4095, 4096, 8191, 8192) if 0 <= r < n]
    codes[:, edges] = -1
    codes[-1, edges] = CODES[-1] - 1
    return codes


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17])
def test_detect_row_bits_equals_the_restatement(n):
    from repair import _native as N
    codes = _bit_table(n, seed=n)
    tab = N.Table(codes, CODES)
    rng = np.random.default_rng(n + 1)
    every = list(range(len(CODES)))

    def bits(fill, null):
        out = []
        for k in CODES:
            f = np.ones(k, bool) if fill == "ones" else np.zeros(k, bool) if fill == "zeros" else rng.random(k) < 0.6
            out.append(DC.pack_bits(np.r_[f, bool(null)]))
        return out

    def check(cols, bs, cell_cols=()):
        want = R.detect_row_bits(codes, CODES, cols, bs, cell_cols)
        got = tab.detect_row_bits(cols, bs, cell_cols=cell_cols)
        if len(cell_cols):
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].dtype == np.int32
        else:
            assert got.dtype == np.int64 and np.array_equal(got, want)
        return got

    assert len(check(every, bits("ones", 1))) == n                                               # every bit set
    assert len(check(every, bits("ones", 0))) == int((codes >= 0).all(axis=0).sum())             # NULL bit off
    assert len(check(every, bits("zeros", 0))) == 0
    assert len(check(every, bits("zeros", 1))) == int((codes < 0).all(axis=0).sum())             # the NULL bit alone
    for null in (0, 1):
        check(every, bits("rand", null))
        for cols in ([3], [4, 0], [2, 1, 3]):
            bs = bits("rand", null)
            check(cols, [bs[c] for c in cols])
    bs = bits("rand", 1)
    rows, cols = check([1, 4], [bs[1], bs[4]], cell_cols=[4, 0, 1])
    assert cols.tolist() == [4] * (len(rows) // 3) + [0] * (len(rows) // 3) + [1] * (len(rows) // 3)
    for bad in ([1, 1], [len(CODES)], [-1]):
        with pytest.raises(N.RepairGbmError) as e:
            tab.detect_row_bits(bad, [bs[1]] * len(bad))
        assert e.value.code == -1


def _lds_bits():
    """The most bits of a bitset that is staged into LDS: the constant of the source, not a copy of it."""
    return csrc_constant("DET_LDS_WORDS") * 64


def test_row_bits_bitset_either_side_of_the_lds_bound():
    """One column whose bitset (codes + the NULL bit) just fits the LDS stage and one a bit beyond it (read from global memory): each
    alone and both in one call, the NULL bit on and off."""
    from repair import _native as N
    n = 4097
    ks = [_lds_bits() - 1, _lds_bits()]                  # 65 535 and 65 536 codes: 65 536 bits (staged), 65 537 bits (global)
    rng = np.random.default_rng(ks[1])
    codes = np.stack([rng.integers(0, k, n) for k in ks]).astype(np.int32)
    for j, k in enumerate(ks):
        must = [0, 63, 64, 65534, k - 1, -1]             # both ends of the first words, the last words' last bits, NULL
        codes[j, rng.permutation(n)[:2 * len(must)]] = must + must
        assert set(must) <= set(codes[j].tolist())
    tab = N.Table(codes, ks)
    for null in (0, 1):
        bs = [DC.pack_bits(np.r_[rng.random(k) < 0.5, bool(null)]) for k in ks]
        assert [len(b) for b in bs] == [(k + 1 + 63) // 64 for k in ks]
        for cols in ([0], [1], [0, 1], [1, 0]):
            want = R.detect_row_bits(codes, ks, cols, [bs[c] for c in cols])
            got = tab.detect_row_bits(cols, [bs[c] for c in cols])
            assert got.dtype == np.int64 and np.array_equal(got, want)
            assert 0 < len(want) < n


# ---------------------------------------------------------------------------------------------- the gap this closes
def test_a_table_the_host_detector_refuses():
    """20 001 rows, EQ(State) & GT(Salary) & LT(Tax) with groups of at most 64 rows: `_violating_rows` refuses the table, the device
    answers and equals the restatement."""
    from repair import _native as N
    from repair.dc_codes import lower_constraint
    from repair.errors import _violating_rows, parse_constraint
    from repair.pipeline import _merge_cells, detect_error_cells, encode_frame
    n = 20001
    rng = np.random.default_rng(20001)
    salary = rng.integers(20, 200, n).astype(np.float64) * 500
    salary[rng.random(n) < 0.02] = np.nan
    tax = np.round(salary * 0.2)
    odd = rng.random(n) < 0.01
    tax[odd] = rng.integers(0, 40000, int(odd.sum()))
    df = pd.DataFrame({"State": np.array(["s%03d" % (i % 400) for i in range(n)], object), "Salary": salary, "Tax": pd.array(tax, dtype="Int64")})
    cols = list(df.columns)
    preds = parse_constraint("t1&t2&EQ(t1.State,t2.State)&GT(t1.Salary,t2.Salary)&LT(t1.Tax,t2.Tax)")
    with pytest.raises(ValueError, match="table too large"):
        _violating_rows(df, preds)
    idx, remaps, dicts = encode_frame(df, cols)
    codes = np.stack([np.where(idx[j] >= 0, remaps[j][np.maximum(idx[j], 0)], -1) for j in range(3)]).astype(np.int32)
    n_codes = [len(d) for d in dicts]
    prog = lower_constraint(preds, cols, dicts, {c: df[c].dtype for c in cols})
    assert prog["kind"] == "dc" and prog["refs"] == [0, 1, 2]
    tab = N.Table(codes, n_codes)
    rows, ccols = detect_error_cells(tab, [1, 2], constraints=[prog], detect_nulls=False)
    want = _merge_cells(n, [R.detect_dc(codes, n_codes, prog["preds"], cell_cols=[1, 2])])
    assert len(rows) > 0 and np.array_equal(rows, want[0]) and np.array_equal(ccols, want[1])


# ---------------------------------------------------------------------------------------------- whole runs
def _run_both(monkeypatch, df, constraints, targets, thres):
    from repair.errors import ConstraintErrorDetector, NullErrorDetector
    from repair.model import RepairModel

    def model(on):
        m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(thres) \
            .setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints=constraints)])
        if targets:
            m = m.setTargets(targets)
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2",
                     "error.constraints.resident": "true" if on else "false"}.items():
            m = m.option(k, v)
        return m

    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = model(False).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = model(True)
    fast = fm.run()
    assert fm._last_detection_on_device is True
    key = ["tid", "attribute"]
    assert len(slow) > 0
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))


def test_run_adult_with_its_constant_constraints(monkeypatch):
    from tests.helpers import frame, load_golden
    g = load_golden("adult")
    df = frame(g["input"])
    _run_both(monkeypatch, df, ";".join(l for l in g["constraints"].splitlines() if l.strip()), [], 80)


def test_run_hospital_with_two_iqs_and_an_order_predicate(monkeypatch):
    from tests.helpers import frame, load_golden
    from tests.test_quality import HOSPITAL_TARGETS
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    cons = ("t1&t2&EQ(t1.HospitalName,t2.HospitalName)&IQ(t1.ZipCode,t2.ZipCode)&IQ(t1.City,t2.City);"
            "t1&t2&EQ(t1.City,t2.City)&GT(t1.ZipCode,t2.ZipCode)")
    _run_both(monkeypatch, df, cons, HOSPITAL_TARGETS, 400)
