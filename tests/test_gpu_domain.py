"""-m gpu: the device entries of the cell-domain analysis (csrc/rgbm_domain.hip: rgbm_table_pair_counts, rgbm_table_cell_domains)
against repair.domain -- counts exactly, flags / top values / probabilities bit for bit; their kernel edges are walked against a plain
restatement in tests/test_gpu_domain_edges.py -- and `run()` with
`error.domain_analysis.enabled` on the hospital fixture: the resident path ends with the cells of the value-space path."""
import numpy as np
import pandas as pd
import pytest

from tests.synth import make_table

pytestmark = pytest.mark.gpu


def _host_counts(codes, pairs, luts, n_bins):
    from repair import domain as D
    view = D.View(sorted(n_bins), n_bins, luts, [])
    return [j.dense() for j in D.HostBackend(codes, view).pair_counts(pairs)]


def _lut_table(n, seed):
    """6 discrete columns with NULLs, 2 'continuous' ones (500 / 37 codes) binned through LUTs (some LUT entries NULL) and a noisy copy of column 5."""
    from repair import domain as D
    rng = np.random.default_rng(seed)
    dirty, _, cards = make_table(n, 6, seed=seed, null_ratio=0.03)
    c6 = rng.integers(0, 500, n).astype(np.int32); c6[rng.random(n) < 0.02] = -1
    c7 = rng.integers(0, 37, n).astype(np.int32)
    # column 8: the last discrete column with 15 % of its cells redrawn -- strongly correlated, so that domains reach a high beta
    c8 = np.where(rng.random(n) < 0.15, rng.integers(0, int(cards[5]), n), np.maximum(dirty[5], 0)).astype(np.int32)
    c8[rng.random(n) < 0.02] = -1
    codes = np.vstack([dirty, c6[None], c7[None], c8[None]])
    n_codes = list(cards) + [500, 37, int(cards[5])]
    luts = {6: D.continuous_lut(np.sort(rng.normal(size=500)), 20), 7: D.continuous_lut(np.arange(37.0) ** 2, 9)}
    luts[7][5] = -1
    n_bins = {c: int(n_codes[c]) for c in range(6)}
    n_bins.update({6: 21, 7: 10, 8: int(cards[5])})
    return codes, n_codes, luts, n_bins


@pytest.mark.parametrize("n", [1, 511, 513, 100003])
def test_pair_counts_with_nulls_and_luts(n):
    from repair import _native as N
    codes, n_codes, luts, n_bins = _lut_table(n, seed=n)
    tab = N.Table(codes, n_codes)
    pairs = [(x, y) for x in range(9) for y in range(x + 1, 9)] + [(7, 0), (6, 2)]      # every column is used by 8+ pairs
    got = tab.pair_counts(pairs, luts=luts, n_bins=n_bins)
    want = _host_counts(codes, pairs, luts, n_bins)
    for p, g, w in zip(pairs, got, want):
        assert g.shape == w.shape and np.array_equal(g, w), p
        assert int(g.sum()) == n


def test_pair_counts_many_groups_and_the_global_variant():
    """66 pairs of 64-value columns (4225 cells each: several LDS groups, more than 16 distinct columns over the call), one pair whose
    dense table (301 x 301) does not fit the LDS, N not a multiple of the block."""
    from repair import _native as N
    n = 250_007
    rng = np.random.default_rng(2)
    dirty, _, cards = make_table(n, 18, seed=2, null_ratio=0.05, cards=[64] * 18)
    big = rng.integers(0, 300, (2, n)).astype(np.int32)
    big[0][rng.random(n) < 0.1] = -1
    codes = np.vstack([dirty, big])
    n_codes = list(cards) + [300, 300]
    tab = N.Table(codes, n_codes)
    pairs = [(x, y) for x in range(12) for y in range(x + 1, 12)] + [(17, c) for c in range(12, 17)] + [(18, 19), (19, 0)]
    got = tab.pair_counts(pairs)
    want = _host_counts(codes, pairs, {}, {c: int(n_codes[c]) for c in range(20)})
    for p, g, w in zip(pairs, got, want):
        assert np.array_equal(g, w), p
    assert got[-2].shape == (301, 301)


def test_pair_counts_above_the_dense_cap_is_a_parameter_error():
    from repair import _native as N
    codes = np.zeros((2, 10), np.int32)
    tab = N.Table(codes, [5000, 5000])
    with pytest.raises(N.RepairGbmError) as e:
        tab.pair_counts([(0, 1)])
    assert e.value.code == -2
    from repair.pipeline import NotResidentEligible, TableBackend
    from repair import domain as D
    with pytest.raises(NotResidentEligible):
        TableBackend(tab, D.View([0, 1], {0: 5000, 1: 5000}, {}, [])).pair_counts([(0, 1)])


@pytest.mark.parametrize("beta, alpha_cnt, freq_min", [(0.7, 0, 0), (0.3, 3, 0), (0.05, 0, 40)])
def test_cell_domains_bit_for_bit(beta, alpha_cnt, freq_min):
    from repair import _native as N
    from repair import domain as D
    n = 60_001
    codes, n_codes, luts, n_bins = _lut_table(n, seed=77)
    tab = N.Table(codes, n_codes)
    view = D.View(list(range(9)), n_bins, luts, [6, 7])
    host = D.HostBackend(codes, view)
    target = 5                                        # 12 values
    pairs = [(target, 3), (6, target), (target, 7), (0, target), (8, target)]
    dense = tab.pair_counts(pairs, luts=luts, n_bins=n_bins)
    ptab = D.PairTable(pairs, [D.Joint.from_dense(d) for d in dense])
    rng = np.random.default_rng(1)
    rows = np.sort(rng.choice(n, 5000, replace=False)).astype(np.int64)
    rows = np.concatenate([rows, np.flatnonzero(codes[6] < 0)[:50], np.flatnonzero(codes[target] < 0)[:50]])   # NULL correlated values / NULL cells
    single = ptab.single(target)
    ok = single[:12] > freq_min
    n_weak = n_empty = n_domain = 0
    for corr in ([3, 6], [6, 3, 7, 0], [7], [8], [8, 3], [6, 8]):
        min_cnt = [max(alpha_cnt, freq_min)] * len(corr)
        hw, ht, hp, hprobs = host.cell_domains(target, rows, corr, ptab, min_cnt, ok, beta, n, want_probs=True)
        # the precondition the comparison rests on: no host probability within 1e-9 of beta
        assert np.abs(hprobs - beta).min() > 1e-9
        pidx = [ptab.index[frozenset((c, target))] for c in corr]
        gw, gt, gp, gprobs = tab.cell_domains(target, rows, pidx, min_cnt, ok, beta, n, want_probs=True)
        assert np.array_equal(gw, hw) and np.array_equal(gt, ht)
        assert gp.tobytes() == hp.tobytes() and gprobs.tobytes() == hprobs.tobytes()
        n_weak, n_empty, n_domain = n_weak + int(hw.sum()), n_empty + int((ht < 0).sum()), n_domain + int((ht >= 0).sum())
    # the inputs exercise every outcome: weak labels, non-empty domains whose top is not the current value, empty domains
    assert n_weak > 1000 and n_empty > 100 and n_domain > n_weak


def test_run_hospital_same_cells_on_both_paths(monkeypatch):
    from tests.test_domain_analysis import _hospital_model
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _hospital_model(None).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = _hospital_model(None)
    fast = fm.run()
    assert fm._last_detection_on_device and fm._last_resident_info["weak_cells"] > 3000
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))
