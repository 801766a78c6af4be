"""-m gpu: rgbm_table_detect_cells (csrc/rgbm_prep.hip) against its numpy restatement (tests/detector_restatements.py) -- integers, so
equality of rows and columns, order included -- and one `RepairModel.run()` with the value detectors on the resident table through
the HIP engine against the value-space path."""

import numpy as np
import pandas as pd
import pytest

from repair import detect_codes as DC
from tests import detector_restatements as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu

CODES = [1, 63, 64, 65, 129]                 # codes per column: the edges of the 64-bit bitset words


def _lds_codes():
    """The most codes whose bitset is staged into LDS: the constant of the source, not a copy of it."""
    return csrc_constant("DET_LDS_WORDS") * 64


def _table(n, n_codes, seed):
    """Random codes with 10 % NULLs; every column NULL at row 0, at row n - 1 and either side of each 4096-row tile edge, except that
    the last column has its highest code there (so both ends of a range and the last bit of a bitset are met at the edges)."""
    rng = np.random.default_rng(seed)
    codes = np.stack([rng.integers(0, k, n) for k in n_codes]).astype(np.int32)
    codes[rng.random(codes.shape) < 0.1] = -1
    edges = [r for r in (0, n - 1, 4095, 4096, 8191, 8192) if 0 <= r < n]
    codes[:, edges] = -1
    codes[-1, edges] = n_codes[-1] - 1
    return codes


def _check(tab, codes, cols, null, lo, hi, bits):
    want = R.detect_cells(codes, cols, null, lo, hi, bits)
    got = tab.detect_cells(cols, null, lo, hi, bits)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    return got


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17])
def test_detect_cells_equals_the_restatement(n):
    from repair import _native as N
    codes = _table(n, CODES, seed=n)
    tab = N.Table(codes, CODES)
    rng = np.random.default_rng(n + 1)
    every = list(range(len(CODES)))
    zeros = [DC.pack_bits(np.zeros(k, bool)) for k in CODES]
    ones = [DC.pack_bits(np.ones(k, bool)) for k in CODES]
    rand = [DC.pack_bits(rng.random(k) < 0.4) for k in CODES]
    last = [DC.pack_bits(np.arange(k) == k - 1) for k in CODES]                 # the last bit of the last word alone
    no = [0] * len(CODES), [-1] * len(CODES)
    nn = int((codes >= 0).sum())
    for null in (0, 1):
        nulls = [null] * len(CODES)
        n_null = int((codes < 0).sum()) * null
        assert len(_check(tab, codes, every, nulls, *no, zeros)[0]) == n_null                       # bitset all zero
        assert len(_check(tab, codes, every, nulls, *no, ones)[0]) == nn + n_null                   # bitset all ones
        _check(tab, codes, every, nulls, *no, rand)                                                  # keep_lo > keep_hi: no range test
        _check(tab, codes, every, nulls, *no, last)
        _check(tab, codes, every, nulls, [k // 4 for k in CODES], [k // 2 for k in CODES], None)    # range only
        _check(tab, codes, every, nulls, [k // 4 for k in CODES], [k // 2 for k in CODES], rand)    # range + bitset (+ NULL)
        _check(tab, codes, every, nulls, [k - 1 for k in CODES], [k - 1 for k in CODES], [None, rand[1], None, rand[3], None])
        assert len(_check(tab, codes, every, nulls, [0] * len(CODES), [k - 1 for k in CODES], None)[0]) == n_null    # nothing outside
        assert len(_check(tab, codes, every, nulls, list(CODES), list(CODES), None)[0]) == nn + n_null               # everything outside
    # NULL detection alone is rgbm_table_detect_nulls
    for cols in (every, [3, 0, 4]):
        got = _check(tab, codes, cols, [1] * len(cols), [0] * len(cols), [-1] * len(cols), None)
        ref = tab.detect_nulls(cols)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # several columns, not in ascending order, each with another predicate
    cols = [3, 0, 4, 1]
    got = _check(tab, codes, cols, [1, 0, 0, 1], [0, 0, 10, 5], [-1, -1, 100, 4], [rand[3], ones[0], last[4], None])
    assert got[1].tolist() == sorted(got[1].tolist(), key=cols.index)
    for c in cols:
        assert (np.diff(got[0][got[1] == c]) > 0).all()
    # no column: no cell (and the table's last result is empty)
    got = tab.detect_cells([], [], [], [], [])
    assert len(got[0]) == 0 and len(got[1]) == 0


@pytest.mark.parametrize("which", ["lds", "lds+1"])
def test_bitset_either_side_of_the_lds_bound(which):
    """One column whose bitset just fits the LDS stage and one a word beyond it (read from global memory), in one call and alone."""
    from repair import _native as N
    k = _lds_codes() + (1 if which == "lds+1" else 0)
    n = 3 * k + 1001
    rng = np.random.default_rng(k)
    col = rng.permutation(np.r_[np.arange(k), rng.integers(0, k, n - k)]).astype(np.int32)      # every code occurs
    col[rng.random(n) < 0.05] = -1
    col[[0, n - 1]] = k - 1
    codes = np.stack([col, rng.integers(-1, 65, n).astype(np.int32)])
    tab = N.Table(codes, [k, 65])
    flags = rng.random(k) < 0.3
    flags[[0, k - 1, k - 2, 63, 64]] = [True, True, False, True, False]
    bits = DC.pack_bits(flags)
    assert len(bits) == (k + 63) // 64
    got = _check(tab, codes, [0], [0], [0], [-1], [bits])
    assert got[0][0] == 0 and got[0][-1] == n - 1
    _check(tab, codes, [1, 0], [1, 1], [3, k // 8], [60, k - k // 8], [DC.pack_bits(rng.random(65) < 0.5), bits])
    _check(tab, codes, [0], [0], [k // 8], [k - k // 8], None)                       # range only on the wide column


def test_bad_column_lists_are_argument_errors():
    from repair import _native as N
    codes = _table(100, CODES, seed=0)
    tab = N.Table(codes, CODES)
    for cols in ([1, 1], [0, 2, 0], [len(CODES)], [-1], [0, 99]):
        with pytest.raises(N.RepairGbmError) as e:
            tab.detect_cells(cols, [1] * len(cols), [0] * len(cols), [-1] * len(cols), None)
        assert e.value.code == -1                                                    # RGBM_ERR_ARG


def test_run_with_the_value_detectors_on_the_resident_table(monkeypatch):
    """Hospital with NULL, DomainValues(autofill), a regex and the outlier detector (ZipCode as the one continuous attribute): the run
    with `error.value_detectors.resident` detects on the device and ends with the frame of the value-space path."""
    from repair.errors import DomainValues, GaussianOutlierErrorDetector, NullErrorDetector, RegExErrorDetector
    from repair.model import RepairModel
    from tests.helpers import frame, load_golden
    from tests.test_quality import HOSPITAL_TARGETS
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    df["ZipCode"] = pd.to_numeric(df["ZipCode"], errors="coerce")

    def model(on):
        dets = [NullErrorDetector(), RegExErrorDetector("State", "^a[lk]$"), GaussianOutlierErrorDetector()]
        dets += [DomainValues(attr=c, autofill=True, min_count_thres=4) for c in ("City", "Condition", "MeasureCode", "HospitalOwner")]
        m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400).setTargets(HOSPITAL_TARGETS).setErrorDetectors(dets)
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2",
                     "error.value_detectors.resident": "true" if on else "false"}.items():
            m = m.option(k, v)
        return m

    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = model(False).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = model(True)
    fast = fm.run()
    assert fm._last_detection_on_device is True
    info = {d["attribute"]: d for d in fm._last_resident_info["value_detectors"]}
    assert info["State"]["kinds"] == ["null", "regex"] and info["ZipCode"]["kinds"] == ["null", "outlier"]
    assert info["City"]["kinds"] == ["null", "domain"] and info["City"]["cells"] > 0 and info["State"]["cells"] > 0
    key = ["tid", "attribute"]
    assert len(slow) > 0
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))
