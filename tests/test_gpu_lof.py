"""-m gpu: rgbm_lof_1d (csrc/rgbm_lof.hip: k_lof_window, k_lof_lrd, k_lof_score) against the numpy statement repair/lof_codes.py --
scores as uint64 views, flag words and both counters, so equality -- and one `RepairModel.run()` with LOFOutlierErrorDetector on the
resident table through the HIP engine against the value-space path."""
import numpy as np
import pandas as pd
import pytest

from repair import detect_codes as DC
from repair import lof_codes as L

pytestmark = pytest.mark.gpu

TILE = 256                                   # positions per workgroup (LOF_TILE of the source)
KS = [1, 20, 64]


def _values(d, seed, integers=False):
    """d ascending doubles without two equal differences (or the integers 0 .. d - 1: every inner value has a tie)."""
    if integers:
        return np.arange(d, dtype=np.float64)
    v = np.unique(np.random.default_rng(seed).normal(size=d))
    assert len(v) == d
    return v


def _check(values, counts, k):
    """Device == statement, bit for bit; returns the statement's tuple."""
    from repair import _native as N
    from repair.engine import HipEngine
    values, counts = np.asarray(values, np.float64), np.asarray(counts, np.int64)
    want = L.lof_codes(values, counts, k)
    score, bits, n_ties, n_near = N.lof_1d(values, counts, k=k)
    assert score.dtype == np.float64 and bits.dtype == np.uint64 and len(bits) == (len(values) + 63) // 64
    diff = np.flatnonzero(score.view(np.uint64) != want[0].view(np.uint64))
    assert len(diff) == 0, "scores differ at positions %s (of %d, k = %d)" % (diff[:8].tolist(), len(values), k)
    assert np.array_equal(bits, DC.pack_bits(want[1]))
    assert (n_ties, n_near) == (want[2], want[3])
    got = HipEngine(0).lof_codes(values, counts, k)
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)) and got[1].dtype == bool and np.array_equal(got[1], want[1])
    assert got[2:] == want[2:]
    none, bits2, _, _ = N.lof_1d(values, counts, k=k, want_scores=False)                  # the scores are optional
    assert none is None and np.array_equal(bits2, bits)
    return want


@pytest.mark.parametrize("d", [1, 2, 19, 20, 21, 22, 63, 64, 65, 255, 256, 257, 256 + 20, 512 + 1, 3 * 256 + 17])
def test_counts_all_one_and_random_counts(d):
    """Every size either side of the word, halo and tile edges, k at both ends of its range; n <= k exercises the k_ clamp."""
    rng = np.random.default_rng(d)
    v = _values(d, d)
    for k in KS:
        ones = np.ones(d, np.int64)
        if d == 1:
            ones[0] = 2                                                                   # n >= 2
        _check(v, ones, k)
        _check(v, rng.integers(1, 6, d), k)                                               # partial neighbours everywhere
    # two far values are flagged wherever the column holds a few times k values to compare them with
    if d >= 63:
        w = v.copy()
        w[-1] += 50.0
        w[0] -= 70.0
        assert _check(w, np.ones(d, np.int64), 20)[1][[0, d - 1]].all()


@pytest.mark.parametrize("copies", ["k-1", "k", "k+1", "1e6"])
@pytest.mark.parametrize("k", [20, 64])
def test_one_heavy_code_at_the_tile_edges_and_in_a_halo(copies, k):
    d = 3 * TILE + 17
    v = _values(d, 1000 + k)
    m = dict([("k-1", k - 1), ("k", k), ("k+1", k + 1), ("1e6", 10 ** 6)])[copies]
    rng = np.random.default_rng(k)
    for at in (TILE, TILE - 1, 2 * TILE - 1, 2 * TILE, TILE + 5, TILE - 5, 2 * TILE + k - 1, 0, d - 1):
        for base in (np.ones(d, np.int64), rng.integers(1, 4, d)):
            c = base.copy()
            c[at] = m
            _check(v, c, k)


def test_partial_neighbour_across_a_tile_edge_on_either_side():
    """Counts of 4 with k = 20: 3 copies of the value itself, four whole neighbours and one copy of a fifth; around the tile edge that
    one lies in the other tile."""
    d, k = 2 * TILE + 40, 20
    v = _values(d, 77)
    c = np.full(d, 4, np.int64)
    k_, m, self_taken, l, r, side, part, kdist, tie = L.lof_windows(v, c, k)
    pos = np.arange(d)
    left = (pos >= TILE) & (side == 1) & (l < TILE) & (part < m[l])                      # the partial neighbour is the last of the tile before
    right = (pos < TILE) & (side == 2) & (r >= TILE) & (part < m[r])                     # ... the first of the tile behind
    assert left.any() and right.any()
    _check(v, c, k)
    # and one copy each side of the edge with k = 64: windows that reach 64 positions into the neighbouring tile
    k_, m, self_taken, l, r, side, part, kdist, tie = L.lof_windows(v, np.ones(d, np.int64), 64)
    assert (pos - l).max() <= 64 and (r - pos).max() <= 64 and ((pos - l)[TILE:] > (pos - TILE)[TILE:]).any()
    _check(v, np.ones(d, np.int64), 64)


@pytest.mark.parametrize("k", KS)
def test_a_tied_column_counts_the_statements_ties(k):
    d = 2 * TILE + 9
    v = _values(d, 0, integers=True)
    rng = np.random.default_rng(k)
    want = _check(v, rng.integers(1, 4, d), k)
    assert want[2] > 0
    assert _check(v, np.ones(d, np.int64), 1)[2] == d - 2                                # every inner integer: either neighbour, one fits


def test_a_score_inside_the_band_is_counted():
    t = 1.5 + 0.5e-10
    assert _check([0.0, 1.0, 1.0 + t], [1, 1, 1], 1)[3] == 1


def test_argument_errors_come_back_as_errors():
    from repair import _native as N
    ok_v, ok_c = np.array([1.0, 2.0, 3.0]), np.array([1, 1, 1], np.int64)
    N.lof_1d(ok_v, ok_c, k=20)
    for v, c, k in ((ok_v, ok_c, 0), (ok_v, ok_c, 65), (ok_v, ok_c, -3), (np.zeros(0), np.zeros(0, np.int64), 20), (ok_v, [1, 0, 1], 20),
                    (ok_v, [1, -5, 1], 20), ([1.0], [1], 20), ([1.0, 1.0], [1, 1], 20), ([2.0, 1.0], [1, 1], 20), ([1.0, np.nan], [1, 1], 20),
                    ([1.0, np.inf], [1, 1], 20), ([-np.inf, 1.0], [1, 1], 20), ([-1.7e308, 1.7e308], [1, 1], 20)):
        with pytest.raises(N.RepairGbmError) as e:
            N.lof_1d(np.asarray(v, np.float64), np.asarray(c, np.int64), k=k)
        assert e.value.code == -1 and "rgbm_lof_1d" in str(e.value)                      # RGBM_ERR_ARG
    with pytest.raises(ValueError):
        N.lof_1d(ok_v, ok_c[:2])
    assert N.lof_1d([1.0], [2], k=20)[0].tolist() == [1.0]


def test_the_symbol_is_exported_and_declared():
    import os
    from repair import _native as N
    assert hasattr(N.lib(), "rgbm_lof_1d") and "rgbm_lof_1d" in N.EXPORTED_SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "int rgbm_lof_1d(" in open(os.path.join(root, "include", "rgbm.h")).read()


def test_run_with_the_lof_detector_on_the_resident_table(monkeypatch):
    """A few hundred rows, one tie-free continuous attribute with NULLs and outliers: the run with `error.lof.resident` detects on the
    device and ends with the frame of the value-space path."""
    pytest.importorskip("sklearn")
    from repair.errors import LOFOutlierErrorDetector, NullErrorDetector
    from repair.model import RepairModel
    rng = np.random.default_rng(7)
    n = 300
    g = rng.integers(0, 6, n)
    b = np.array(["b%d" % (v % 3) for v in g], object)
    x = g * 1.5 + rng.normal(0, 0.3, n)
    b[[40, 41]] = None
    x[[8, 120]] = [99.0, -50.0]
    x[[9, 200, 201]] = np.nan
    df = pd.DataFrame({"tid": np.arange(n), "a": np.array(["a%d" % v for v in g], object), "b": b, "x": x})

    def model(on):
        m = RepairModel().setInput(df).setRowId("tid").setTargets(["b", "x"]).setDiscreteThreshold(50) \
            .setErrorDetectors([NullErrorDetector(), LOFOutlierErrorDetector()])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2",
                     "error.lof.resident": "true" if on else "false"}.items():
            m = m.option(k, v)
        return m

    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = model(False).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = model(True)
    fast = fm.run()
    assert fm._last_detection_on_device is True
    info = {d["attribute"]: d for d in fm._last_resident_info["value_detectors"]}
    assert info["x"]["kinds"] == ["null", "lof"] and info["x"]["codes_flagged"] >= 2 and info["x"]["cells"] >= 5
    key = ["tid", "attribute"]
    assert {99.0, -50.0} <= set(slow.loc[slow["attribute"] == "x", "current_value"].dropna().astype(float))
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))
