"""-m gpu: the batched small-table trainer (rgbm_table_train_batch; csrc/rgbm_small.h, train_batch_small in csrc/rgbm.hip) at the edges of its
kernel paths.  Every assertion is equality: of a fit's row in rgbm_table_train_batch_report with what tests/batch_cases.py restates from the bins of
the CPU oracle's model (route, waves of the packed scan, chunks, LDS bytes) -- FIRST, so that a case meant for one route cannot pass on another --
then of the serialised model with the oracle's (oracle.oracle.train on the fit's training rows), and of validation labels / values with the
oracle model's prediction on the CPU.  No tolerances.  The tables come from tests/batch_cases.py; tests/test_batch_cases_cpu.py shows on the oracle
alone that each of them holds the edge it is named after.  2-3 boosting iterations at learning_rate 0.3 unless a case is about iterations.

What runs, by group:
  scan routes   Wn = 4 packed (four 254-bin features; sixteen 61..64-bin features = 256 lanes, a full chunk), one wave per feature (five 254-bin
                features; seventeen 61..64-bin features = five waves, two chunks), a feature that moves to the next wave (wide+narrow: 3 waves;
                two chunks: 2 waves, packed over two chunks), feature 0 with 254 value bins and with 253 + the NaN bin, feature 0 constant and all
                NULL; everything again under RGBM_SMALL_PACKED=0 (scan_waves 0, same bytes).
                (max_bin <= 255 leaves a feature at most 254 bins -- 254 value bins, or 253 and the NaN bin; a 256-bin feature cannot be built.)
  rows          n_train 1, 2, 39, 40, 41 (min_data_in_leaf 20), 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 16 383, 16 384, 16 385 with
                36 NULL-target rows each; n_train 65 535 in a table of 65 536 rows; 65 536 rows (route 1) and 65 537 rows (route 2) in the same batch.
  budgets       num_leaves 2, 255, 256 reached by every tree, 257 (route 2), max_depth 1; F = 1, 16, 17, 33, 255 (route 1, up to 16 chunks), 256 (route 2).
  classes       binary, K = 3, 64, 113, 219 and a regression fit (3 000 targets, max_bin 15) in one batch.
  bagging       bagging_freq 1, 2, 3 over 7 iterations, fractions 0.05 .. 0.95, 1 / 1 / 2 / 3 / 6 LCG blocks side by side, a fit that does not bag,
                feature_fraction 0.01.
  composition   n_estimators 1, 4, 9; a failing fit in the middle; F = 1 next to Wn = 4 (LDS 4 KB next to 60 KB); reversed; twice; every fit with a
                dummy; fits that freeze after 0, 1, 2, 3 iterations next to one that runs; one eligible fit (route 3).
  bins          two folds of one table with a code that has its own bin in one fold only, numeric and categorical columns set on the parent; a
                1 000-code Zipf column under max_bin 63.
  validation    n_valid 1, 255, 256, 257, 16 385 (larger than the training table), fits without validation rows in between, K = 64, regression, a
                two-chunk fit splitting on the second record, NULL / unseen / out-of-dictionary cells, want_model=False.

The LDS branches of train_batch_small have no case, because no eligible fit reaches them (F <= 255, num_leaves <= 256, sizeof(Leaf) = 96,
sizeof(Cand) = 48, HistBin 16 B, at most 254 bins per feature, 16 features per chunk):
  * `lds > 160 KB - 2048` (single-fit trainer, route 4).  One wave per feature: the histogram area is at most 16 features x 256 replicated slots x
    16 B = 65 536; + 256 x 96 = 24 576 of leaves; + 2 x 255 x 48 = 24 480 of candidates; + 64 = 114 656 < 161 792.  Packed: the bound below, 153 152.
  * `sm_lds_bytes <= 150 KB` (condition of the packed route).  Packed means at most 4 waves = 256 lanes per child.  A feature of l lanes has at
    most 4 l + 1 bins, and costs 96 B of candidates + 32 B per bin of the two compact histograms <= 256 l bytes (equality: one lane, five bins): at
    most 65 536 for all lanes.  The 16 features of the chunk that sets the histogram area add 16 B per replicated slot; over all feature shapes
    16 x slots - (256 l - 96 - 32 bins) is largest for 8 bins (256 slots, two lanes): 3 936.  So at most 65 536 + 16 x 3 936 + 24 576 + 64 = 153 152
    <= 153 600, met by 16 eight-bin and 224 five-bin features under num_leaves 256 -- 448 bytes short of the branch.  totbins <= 2048 cannot fail
    either (at most 256 x 4 + 255 bins).  tests/test_batch_cases_cpu.py::test_lds_branches_are_out_of_reach runs this sum over every shape.
"""
import functools

import numpy as np
import pytest

from tests import batch_cases as B

pytestmark = pytest.mark.gpu

scan_route_fits = functools.lru_cache(maxsize=None)(B.scan_route_fits)
row_fits = functools.lru_cache(maxsize=None)(B.row_fits)
composition_fits = functools.lru_cache(maxsize=None)(B.composition_fits)
dummy_fit = functools.lru_cache(maxsize=None)(B.dummy_fit)


def _table(tab, cache):
    """the device table of a Tab; gathers go through the parent's device table (Table.gather_rows), which carries the column values / kinds"""
    from repair import _native as N
    if id(tab) not in cache:
        if tab.parent is not None:
            t = _table(tab.parent, cache).gather_rows(tab.rows)
        else:
            t = N.Table(tab.codes, tab.cards)
            for col, v in tab.values.items():
                t.set_column_values(col, v)
            for col in tab.kinds:
                t.set_column_kind(col, True)
        cache[id(tab)] = t
    return cache[id(tab)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _run(fits, cache=None, **extra):
    """one rgbm_table_train_batch call -> (results, report rows)"""
    from repair import _native as N
    cache = {} if cache is None else cache
    specs = [f.spec(_table(f.tab, cache), _table(f.valid, cache) if f.valid is not None else None, **extra) for f in fits]
    out = N.train_batch(specs)
    return out, N.train_batch_report(len(fits))


def _blob(res):
    m = res[0] if isinstance(res, tuple) else res
    return m.save()


def _check(fits, out, rep, packed=True, want_model=True):
    """the report of every fit, THEN models and validation scores against the oracle"""
    from repair import _native as N
    assert len(out) == len(rep) == len(fits)
    alone = sum(1 for f in fits if B.eligible(f)) == 1
    for f, r in zip(fits, rep):
        assert r == B.expected_report(f, packed=packed, alone=alone), "%s: the report says %r" % (f.name, r)
        assert r["route"] == f.route or alone, "%s: built for route %d" % (f.name, f.route)
    for f, res in zip(fits, out):
        if f.fails:
            assert isinstance(res, N.RepairGbmError) and "no training rows" in str(res), "%s: %r" % (f.name, res)
            continue
        assert not isinstance(res, Exception), "%s failed: %r" % (f.name, res)
        if want_model or f.valid is None:
            assert _blob(res) == B.oracle_model(f).save(), "%s: the batched model differs from the oracle's" % f.name
        if f.valid is not None:
            assert isinstance(res, tuple), f.name
            assert want_model or res[0] is None, f.name
            lab, val = B.oracle_valid(f)
            assert np.array_equal(res[1], lab), "%s: validation labels differ from the oracle model's" % f.name
            assert np.array_equal(_bits(res[2]), _bits(val)), "%s: validation values differ from the oracle model's" % f.name


def _single(fit, cache):
    """Table.train for the same arguments"""
    t = _table(fit.tab, cache)
    return t.train(fit.target, fit.feats, y_value=fit.y_value, class_weight=fit.class_weight, **fit.params).save()


# ---- scan routes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "RGBM_SMALL_PACKED=0"])
def test_scan_routes(packed, monkeypatch):
    cases = scan_route_fits()
    if not packed:
        monkeypatch.setenv("RGBM_SMALL_PACKED", "0")
    fits = [c[0] for c in cases.values()]
    cache = {}
    out, rep = _run(fits, cache)
    for (name, (_, Wn, nchunk)), r in zip(cases.items(), rep):
        assert (r["route"], r["scan_waves"], r["nchunk"]) == (1, Wn if packed and 2 * Wn <= B.SM_WAVES else 0, nchunk), "%s: %r" % (name, r)
    _check(fits, out, rep, packed=packed)
    if packed:
        for name in ("four 254-bin features", "seventeen 61..64-bin features"):
            assert _single(cases[name][0], cache) == B.oracle_model(cases[name][0]).save(), name


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def test_row_count_edges_in_one_batch():
    fits = row_fits()
    out, rep = _run(fits)
    assert [r["route"] for r in rep[-3:]] == [1, 1, 2], "65 536 rows are the fused kernels' largest table: %r" % rep[-3:]
    _check(fits, out, rep)


# ---- budgets ------------------------------------------------------------------------------------------------------------------------
def test_leaf_budgets_and_feature_counts():
    fits = [f for f, _ in B.leaf_budget_fits()]
    out, rep = _run(fits)
    assert [r["route"] for r in rep] == [1, 1, 1, 2, 1], rep
    _check(fits, out, rep)
    fits = B.feature_count_fits()
    out, rep = _run(fits)
    assert [(r["route"], r["nchunk"]) for r in rep] == [(1, 1), (1, 1), (1, 2), (1, 3), (1, 16), (2, 0)], rep
    assert [r["scan_waves"] for r in rep[:5]] == [1, 1, 1, 1, 4], rep
    _check(fits, out, rep)


# ---- class counts -------------------------------------------------------------------------------------------------------------------
def test_class_counts_in_one_batch():
    fits = B.class_count_fits()
    out, rep = _run(fits)
    _check(fits, out, rep)


# ---- bagging ------------------------------------------------------------------------------------------------------------------------
def test_bagging_fits_of_different_block_counts():
    fits = B.bagging_fits()
    cache = {}
    out, rep = _run(fits, cache)
    _check(fits, out, rep)
    assert _single(fits[3], cache) == _blob(out[3])


# ---- composition --------------------------------------------------------------------------------------------------------------------
def test_composition_forward_reversed_and_twice():
    fits = composition_fits()
    cache = {}
    out, rep = _run(fits, cache)
    _check(fits, out, rep)
    assert rep[-1]["scan_waves"] == 4 and rep[-1]["lds_bytes"] > 2 * rep[-2]["lds_bytes"], rep
    first = [None if f.fails else _blob(o) for f, o in zip(fits, out)]
    out2, rep2 = _run(fits, cache)                                   # the same batch again
    assert rep2 == rep and [None if f.fails else _blob(o) for f, o in zip(fits, out2)] == first
    rev = fits[::-1]
    out3, rep3 = _run(rev, cache)
    _check(rev, out3, rep3)
    assert rep3 == rep[::-1] and [None if f.fails else _blob(o) for f, o in zip(rev, out3)] == first[::-1]


def test_every_fit_paired_with_a_dummy():
    cache = {}
    d = dummy_fit()
    for i, f in enumerate(x for x in composition_fits() if not x.fails):
        pair = [f, d] if i % 2 == 0 else [d, f]
        out, rep = _run(pair, cache)
        _check(pair, out, rep)


def test_fits_that_freeze_next_to_one_that_runs():
    from repair import _native as N
    fits = B.freeze_fits()
    out, rep = _run(fits)
    _check(fits, out, rep)
    assert [o[0].info()["n_iter"] for o in out] == [1, 1, 9, 2, 3, 3]


def test_one_eligible_fit_goes_to_the_single_fit_trainer():
    fits = [row_fits()[-1], dummy_fit()]                             # 65 537 rows: not eligible
    out, rep = _run(fits)
    assert [r["route"] for r in rep] == [2, 3], rep
    _check(fits, out, rep)


# ---- per-fit bins -------------------------------------------------------------------------------------------------------------------
def test_folds_bin_on_their_own_rows():
    fits = B.fold_fits() + [B.zipf_fit()]
    cache = {}
    out, rep = _run(fits, cache)
    _check(fits, out, rep)
    assert _single(fits[1], cache) == _blob(out[1])


# ---- validation scores --------------------------------------------------------------------------------------------------------------
def test_validation_scores_equal_the_oracle_models_prediction():
    fits = B.valid_fits() + [B.valid_two_chunk_fit(), B.valid_categorical_fit()]
    cache = {}
    out, rep = _run(fits, cache)
    _check(fits, out, rep)
    scored = [f for f in fits if f.valid is not None][1::2]
    out, rep = _run(scored, cache, want_model=False)
    _check(scored, out, rep, want_model=False)
