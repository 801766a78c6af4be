"""-m gpu: the probability-mode kernels where a lane-stride, tie-break or slice-offset mistake would hide.

k_top_k_pmf / k_weighted_pmf give one wave to a cell and lane l the classes c = l (mod 64): here K is 63, 64, 65, 128, 129 and 303, the
model is trained with label codes that no row carries (tests/prob_edges.py), so every cell holds tied probabilities -- also between two
classes of one lane -- and, from K = 128 on, probabilities that are exactly 0.0.  The probabilities come from the ORACLE model's predict
(after `save()` equality), the selection from oracle.prep.top_k_pmf and the per-cell Python loop of tests/test_prob_modes_cpu.py with its
explicit left-to-right sum; classes must be equal and probabilities, cur_prob, top1_cost equal byte for byte.  The conditions that make
the cases bite (ties among the selected classes, zeros, all-zero cells, a moved top-1) are asserted on the reference first.

rgbm_edit_distance: b pools of 65 535 / 65 536 / 70 000 strings (the second `j0` launch), texts of 5 000 and 100 000 code points, the
anti-diagonal kernel at 1 000-3 000 code points with every residue of ns + nt mod 3 and ns around the lane stride, patterns of 1 / 63 /
64 code points decided by their last position, code points 0, 0x10FFFF and lone surrogates, the host's offset checks -- against
repair.costs.edit_distance and a full-matrix numpy DP."""
import ctypes as C
import functools

import numpy as np
import pytest

from repair.costs import edit_distance
from tests import prob_edges as E
from tests.test_prob_modes_cpu import _select, _weighted_probs

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- the pmf kernels
@functools.lru_cache(maxsize=None)
def _case(K):
    """(device table, device model, NULL rows, the ORACLE's probabilities of those rows); the two models are equal byte for byte."""
    from repair import _native as N
    codes, cards = E.make_edge_table(K)
    tab = N.Table(codes, cards, device_id=0)
    mg = tab.train(E.N_FEATS, list(range(E.N_FEATS)), num_class=K, **E.TRAIN)
    mo = E.train_oracle(codes, cards, K)
    assert mg.save() == mo.save(), "K=%d: the device model differs from the oracle's; nothing below would test the pmf kernels" % K
    null_rows, proba = E.null_cell_probabilities(mo, codes)
    assert len(null_rows) >= 300
    E.check_probabilities(K, proba)
    return tab, mg, null_rows, proba


def _same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).reshape(len(got), -1).any(axis=1))
        raise AssertionError("%s: %d of %d cells differ, first cell %d: got %r, want %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def _same_but_nan(got, want, what):
    """NaN in the same cells, the same bytes everywhere else."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN in other cells, first %r" % (what, np.flatnonzero(np.isnan(got) != np.isnan(want))[:5].tolist())
    ok = ~np.isnan(want)
    _same_bytes(got[ok], want[ok], what)


def _same_classes(got, want, what):
    if not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(axis=1))
        raise AssertionError("%s: classes of %d of %d cells differ, first cell %d: got %r, want %r" % (what, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def _selections(K, p):
    """(top_k, threshold) pairs: padding and more selection rounds than lanes; -1.0 selects the zero-probability classes too, and one
    threshold is a probability that tied classes of `p` hold (`prob > threshold` must drop all of them)."""
    tied = E.tied_probability(p)
    assert tied is not None and tied > 0.0
    return [(top_k, thres) for top_k in (1, 64, K, K + 4) for thres in (-1.0, 0.0, tied, 0.2)]


@pytest.mark.parametrize("K", E.KS)
def test_top_k_pmf_beyond_one_chunk(K):
    from oracle import prep as P
    tab, mg, null_rows, proba = _case(K)
    feats = list(range(E.N_FEATS))
    cur = E.cur_codes(K, len(null_rows))
    want_cp = np.array([proba[i, c] if 0 <= c < K else 0.0 for i, c in enumerate(cur)], np.float64)
    for top_k, thres in _selections(K, proba):
        what = "repair_pmf K=%d top_k=%d threshold=%r" % (K, top_k, thres)
        want_cls, want_pr = P.top_k_pmf(proba, top_k, thres)
        rows, cls, pr, cp = tab.repair_pmf(mg, E.N_FEATS, feats, top_k=top_k, threshold=thres, cur_codes=cur)
        assert np.array_equal(rows, null_rows), what
        _same_classes(cls, want_cls, what)
        _same_bytes(pr, want_pr, what + " probabilities")
        _same_bytes(cp, want_cp, what + " cur_prob")


@pytest.mark.parametrize("K", E.KS)
def test_weighted_pmf_beyond_one_chunk(K):
    tab, mg, null_rows, proba = _case(K)
    feats = list(range(E.N_FEATS))
    m = len(null_rows)
    cur = E.cur_codes(K, m)
    plain_top1 = _select(proba, 1, -1.0, None, None, None)[0][:, 0]
    for name, (cost, special) in E.cost_matrices(K).items():
        crow = E.cost_rows(m, len(cost) - 1)
        for renorm in (False, True):
            for weight in E.WEIGHTS:
                p = _weighted_probs(proba, crow, cost, weight, renorm)
                E.check_weighted(K, p, crow, special, plain_top1)
                for top_k, thres in _selections(K, p):
                    what = "repair_pmf_weighted K=%d cost=%s renormalise=%r weight=%r top_k=%d threshold=%r" % (K, name, renorm, weight, top_k, thres)
                    wc, wp, wcp, wtc = _select(p, top_k, thres, cur, crow, cost)
                    rows, gc, gp, gcp, gtc = tab.repair_pmf_weighted(mg, E.N_FEATS, feats, top_k=top_k, threshold=thres, cur_codes=cur, cost_rows=crow,
                                                                     cost=cost, weight=weight, renormalise=renorm)
                    assert np.array_equal(rows, null_rows), what
                    _same_classes(gc, wc, what)
                    _same_bytes(gp, wp, what + " probabilities")
                    _same_bytes(gcp, wcp, what + " cur_prob")
                    _same_but_nan(gtc, wtc, what + " top1_cost")        # NaN: no top-1, or no cost for it
    # a cost matrix but no cost_rows: nothing is weighted, every top1_cost reads the self row
    cost, _ = E.cost_matrices(K)["integers"]
    p = _weighted_probs(proba, None, cost, 0.7, True)
    wc, wp, wcp, wtc = _select(p, 3, 0.0, cur, None, cost)
    _, gc, gp, gcp, gtc = tab.repair_pmf_weighted(mg, E.N_FEATS, feats, top_k=3, threshold=0.0, cur_codes=cur, cost=cost, weight=0.7, renormalise=True)
    _same_classes(gc, wc, "self row")
    _same_bytes(gp, wp, "self row probabilities"); _same_bytes(gcp, wcp, "self row cur_prob"); _same_but_nan(gtc, wtc, "self row top1_cost")
    assert np.array_equal(wtc[~np.isnan(wtc)], cost[-1][wc[:, 0]][~np.isnan(wtc)])


@pytest.mark.parametrize("K", E.KS)
def test_weighted_pmf_without_costs_is_the_plain_pmf(K):
    """No cost, no renormalisation: rgbm_table_repair_pmf bit for bit, and both equal to the oracle."""
    from oracle import prep as P
    tab, mg, null_rows, proba = _case(K)
    feats = list(range(E.N_FEATS))
    cur = E.cur_codes(K, len(null_rows))
    for top_k, thres in _selections(K, proba):
        what = "K=%d top_k=%d threshold=%r" % (K, top_k, thres)
        r0, c0, p0, cp0 = tab.repair_pmf(mg, E.N_FEATS, feats, top_k=top_k, threshold=thres, cur_codes=cur)
        r1, c1, p1, cp1, tc1 = tab.repair_pmf_weighted(mg, E.N_FEATS, feats, top_k=top_k, threshold=thres, cur_codes=cur)
        assert np.array_equal(r0, r1), what
        _same_classes(c1, c0, what)
        _same_bytes(p1, p0, what + " probabilities"); _same_bytes(cp1, cp0, what + " cur_prob")
        assert np.isnan(tc1).all(), what
        want_cls, want_pr = P.top_k_pmf(proba, top_k, thres)
        _same_classes(c1, want_cls, what + " (oracle)")
        _same_bytes(p1, want_pr, what + " probabilities (oracle)")


def test_run_hospital_wide_targets_equal_the_value_space_path():
    """`Sample` (303 classes) and `Score` (55): the targets of the hospital run that reach beyond one 64-class chunk (the six targets
    of test_run_hospital_equals_the_value_space_path stop at 44 classes)."""
    from repair import _native as N
    from repair.costs import Levenshtein
    from tests.test_gpu_prob_modes import _both_paths_hip, _equal
    from tests.test_prob_modes_cpu import _hospital_model
    for flags in (dict(compute_repair_prob=True), dict(compute_repair_score=True)):
        made = []

        def make():
            made.append(_hospital_model(Levenshtein(), delta=60).setTargets(["Score", "Sample"]).option("model.lgb.n_estimators", "12"))
            return made[-1]
        a, b = _both_paths_hip(make, **flags)
        info = made[-1]._last_resident_info
        wide = [info["columns"][t] for t, blob in info["models"].items() if N.Model.load(blob).info()["num_class"] > 64]
        assert wide and int(b["attribute"].isin(wide).sum()) >= 20, "no error cell of a target with more than 64 classes"
        _equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- edit distance
_dp = E.levenshtein_dp


def _rand(rng, n, alphabet="abc"):
    return "".join(rng.choice(list(alphabet), size=n))


def _three_ways(a, b):
    """Device == repair.costs.edit_distance == the numpy DP for every pair of the two pools."""
    from repair import _native as N
    got = N.edit_distance(a, b)
    want = np.array([[edit_distance(x, y) for y in b] for x in a], np.int32).reshape(len(a), len(b))
    dp = np.array([[_dp(x, y) for y in b] for x in a], np.int32).reshape(len(a), len(b))
    assert np.array_equal(want, dp), "repair.costs.edit_distance and the numpy DP disagree"
    assert got.shape == want.shape and np.array_equal(got, want), "pairs %r" % (np.argwhere(got != want)[:5].tolist(),)
    return got


@functools.lru_cache(maxsize=None)
def _big_pool():
    """70 000 short b strings over a three-letter alphabet (1 093 distinct ones, in random order), a few of more than 64 code points on
    both sides of index 65 535, and the a strings with their distances to every b string (repair.costs.edit_distance, memoised)."""
    rng = np.random.default_rng(65535)
    lens = rng.integers(0, 7, 70000)
    b = [_rand(rng, int(n)) for n in lens]
    for idx, n in ((7, 70), (65534, 65), (65535, 130), (65536, 66), (65600, 100), (69999, 129)):
        b[idx] = _rand(rng, n)
    a = ["", "cabba", _rand(rng, 64), _rand(rng, 70), "b", _rand(rng, 130), _rand(rng, 65)]
    dist = functools.lru_cache(maxsize=None)(edit_distance)
    want = np.array([[dist(x, y) for y in b] for x in a], np.int32)
    return a, b, want


@pytest.mark.parametrize("n_b", [65535, 65536, 70000])
def test_edit_distance_b_slices(n_b):
    """More than 65 535 b strings: the second launch (`j0` = 65 535) writes the columns from 65 535 on, for the bit-parallel kernel and
    -- both strings longer than 64 code points -- for the anti-diagonal one."""
    from repair import _native as N
    a, b, want = _big_pool()
    assert sum(len(x) > 64 for x in a) >= 3 and (n_b <= 65535 or any(len(y) > 64 for y in b[65535:n_b]))
    got = N.edit_distance(a, b[:n_b])
    assert got.shape == (len(a), n_b)
    bad = np.argwhere(got != want[:, :n_b])
    assert len(bad) == 0, "%d pairs differ, first (a, b) = %r: got %d, want %d" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    # the transposed call: the long pool on the a side (blockIdx.x), b strings as the LDS pattern or the text
    got_t = N.edit_distance(b[65000:n_b], a)
    assert np.array_equal(got_t, want[:, 65000:n_b].T)


def test_edit_distance_long_texts():
    """One side of at most 64 code points (the pattern), the other 5 000 and 100 000 (the text loop), on either side of the call."""
    from repair import _native as N
    rng = np.random.default_rng(5000)
    t5k, t100k = _rand(rng, 5000), _rand(rng, 100000)
    pats = ["", "c", _rand(rng, 63), _rand(rng, 64), t5k[100:164], t5k[:5]]
    want = np.array([[edit_distance(p, t5k)] for p in pats], np.int32)
    assert np.array_equal(want, np.array([[_dp(p, t5k)] for p in pats], np.int32))
    assert np.array_equal(N.edit_distance(pats, [t5k]), want) and np.array_equal(N.edit_distance([t5k], pats), want.T)
    pats = [t100k[70000:70005], _rand(rng, 64), t100k[31:95]]
    want = np.array([[edit_distance(p, t100k)] for p in pats], np.int32)
    assert np.array_equal(want, np.array([[_dp(p, t100k)] for p in pats], np.int32))
    assert want[2, 0] == 100000 - 64                    # a substring: only insertions
    assert np.array_equal(N.edit_distance(pats, [t100k]), want) and np.array_equal(N.edit_distance([t100k], pats), want.T)


def test_edit_distance_both_sides_long():
    """The anti-diagonal kernel: ns around the lane stride of a diagonal, ns + nt in every residue mod 3 (the three rotating
    diagonals), equal strings, a prefix, and 3 000 x 3 000."""
    rng = np.random.default_rng(3000)
    a = [_rand(rng, n, "ab") for n in (65, 127, 128, 129)]
    b = [_rand(rng, n, "ab") for n in (1000, 1001, 1002)]
    assert {(len(x) + len(y)) % 3 for x in a[:1] for y in b} == {0, 1, 2}
    _three_ways(a, b)
    _three_ways(b, a)
    s = _rand(rng, 1500)
    r1, r2 = _rand(rng, 1001), _rand(rng, 1001)
    pairs = [(s, s, 0), (s[:1000], s, 500), (s, s[:1000], 500), (r1, r2, None), (_rand(rng, 2000), _rand(rng, 2001), None),
             (_rand(rng, 3000, "ab"), _rand(rng, 3000, "ab"), None)]
    assert {(len(x) + len(y)) % 3 for x, y, _ in pairs} == {0, 1, 2}
    for x, y, known in pairs:
        got = _three_ways([x], [y])
        assert known is None or got[0, 0] == known


def test_edit_distance_patterns_decided_by_their_last_position():
    """Patterns of exactly 1, 63 and 64 code points whose last one decides the distance (the score follows bit m - 1; at m = 64 the
    vertical delta vector starts as all ones)."""
    a, b = [], []
    for m in (1, 63, 64):
        head = "x" * (m - 1)
        a += [head + "y", head + "z"]
        b += [head + "y", head + "z", head, head + "yy", "x" * 200 + "y", "x" * 200 + "z", "y" + head, ("x" * (m - 1) + "y") * 3]
    got = _three_ways(a, b)
    for k, m in enumerate((1, 63, 64)):
        assert got[2 * k, 8 * k] == 0 and got[2 * k, 8 * k + 1] == 1 and got[2 * k + 1, 8 * k] == 1 and got[2 * k, 8 * k + 2] == 1
    _three_ways(b, a)


def test_edit_distance_code_points_at_the_edges():
    """Code points 0, 0x10FFFF and lone surrogates (the binding encodes with `surrogatepass`), pools that begin or end with ''."""
    rng = np.random.default_rng(0x10FFFF)
    alphabet = ["\x00", "\U0010FFFF", "\ud800", "\udfff", "a", "\uffff", "\U00010000"]
    pool = ["".join(rng.choice(alphabet, size=int(n))) for n in rng.integers(0, 90, 24)]
    a = [""] + pool[:12] + ["\x00", ""]
    b = [""] + pool[12:] + ["\U0010FFFF" * 70, "\ud800", ""]
    got = _three_ways(a, b)
    assert got[0, 0] == 0 and got[-1, -1] == 0 and got[0, -3] == 70 and got[-2, -2] == 1


def test_edit_distance_three_ways_on_random_pairs():
    rng = np.random.default_rng(333)
    lengths = [0, 1, 2, 7, 31, 62, 63, 64, 65, 66, 100, 128, 129, 200]
    a = [_rand(rng, int(rng.choice(lengths)), "abcd") for _ in range(20)]
    b = [_rand(rng, int(rng.choice(lengths)), "abcd") for _ in range(15)]
    _three_ways(a, b)                                                    # 300 pairs


def test_edit_distance_host_checks():
    """Offsets that decrease or do not start at 0 and a missing code-point array are errors, not reads outside the pools."""
    from repair import _native as N

    def call(a_cp, a_off, b_cp, b_off):
        a_off, b_off = np.asarray(a_off, np.int64), np.asarray(b_off, np.int64)
        out = np.zeros((len(a_off) - 1, len(b_off) - 1), np.int32)
        N._check(N.lib().rgbm_edit_distance(C.c_int32(0), N._p(a_cp, C.c_int32), N._p(a_off, C.c_int64), C.c_int64(len(a_off) - 1),
                                            N._p(b_cp, C.c_int32), N._p(b_off, C.c_int64), C.c_int64(len(b_off) - 1), N._p(out, C.c_int32)),
                 "rgbm_edit_distance")
        return out
    cp = np.array([97, 98, 99, 100], np.int32)
    assert call(cp, [0, 2, 4], cp, [0, 1, 4]).tolist() == [[1, 3], [2, 1]]          # ab, cd against a, bcd
    for bad in ([0, 3, 2], [1, 2, 4], [0, 4, 3]):
        with pytest.raises(N.RepairGbmError):
            call(cp, bad, cp, [0, 1, 4])
        with pytest.raises(N.RepairGbmError):
            call(cp, [0, 2, 4], cp, bad)
    with pytest.raises(N.RepairGbmError):
        call(None, [0, 2, 4], cp, [0, 1, 4])
    with pytest.raises(N.RepairGbmError):
        call(cp, [0, 2, 4], None, [0, 1, 4])
    assert call(None, [0, 0, 0], cp, [0, 1, 4]).tolist() == [[1, 3], [1, 3]]        # empty strings need no code points
