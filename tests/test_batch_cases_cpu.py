"""CPU: the generators of tests/batch_cases.py do what tests/test_gpu_batch_edges.py needs them to do, shown on the oracle alone -- so that no
device test passes because its table missed the edge it is named after: the lane map gives the intended waves per child from the bins of the
oracle's model, the oracle's trees reach the leaf budgets, the rare code of the fold case has its own bin in one fold only, a fit of the freeze
case stops early, no bag is empty, and the validation rows of the categorical case hold what its name says."""
import numpy as np
import pytest

from tests import batch_cases as B


def test_lane_rule_on_hand_counts():
    assert B.lane_waves([254] * 4) == 4 and B.lane_waves([250] * 5) == 5
    assert B.lane_waves([64] * 16) == 4 and B.lane_waves([61] * 17) == 5
    assert B.lane_waves([0]) == 1 and B.lane_waves([1] * 64) == 1 and B.lane_waves([1] * 65) == 2
    assert B.lane_waves([3] * 17 + [224]) == 2            # 17 lanes, then 56 lanes that do not fit the first wave
    assert B.lane_waves([3] * 8 + [224]) == 1             # 8 + 56 lanes: exactly one wave
    assert B.lane_waves([2] * 255) == 4 and B.lane_waves([2] * 33) == 1


def test_scan_route_tables_give_the_intended_waves_and_chunks():
    for name, (fit, Wn, nchunk) in B.scan_route_fits().items():
        bins = B.blob_bins(B.oracle_model(fit).save())
        assert B.lane_waves([v for v, _ in bins]) == Wn, "%s: %d waves, bins %r" % (name, B.lane_waves([v for v, _ in bins]), bins)
        rep = B.expected_report(fit)
        assert rep["route"] == 1 and rep["nchunk"] == nchunk and rep["scan_waves"] == (Wn if 2 * Wn <= B.SM_WAVES else 0), (name, rep)
        assert B.expected_report(fit, packed=False)["scan_waves"] == 0
        assert (B.tree_leaves(B.oracle_model(fit).save()) >= 8).all(), name
    F = B.scan_route_fits()
    assert all(v >= 250 for v, _ in B.blob_bins(B.oracle_model(F["four 254-bin features"][0]).save()))
    assert all(v >= 250 for v, _ in B.blob_bins(B.oracle_model(F["five 254-bin features"][0]).save()))
    for name in ("sixteen 61..64-bin features", "seventeen 61..64-bin features"):
        assert all(61 <= v <= 64 for v, _ in B.blob_bins(B.oracle_model(F[name][0]).save())), name
    assert B.blob_bins(B.oracle_model(F["feature 0: 254 value bins"][0]).save())[0] == (254, 0)
    assert B.blob_bins(B.oracle_model(F["feature 0: 253 value bins + NaN"][0]).save())[0] == (253, 1)
    assert B.blob_bins(B.oracle_model(F["feature 0 constant"][0]).save())[0] == (1, 0)
    assert B.blob_bins(B.oracle_model(F["feature 0 all NULL"][0]).save())[0] == (0, 1)
    # the two-chunk table splits on the wide feature of its second record
    assert (B.tree_features(B.oracle_model(F["two chunks"][0]).save()) == 17).any()


def test_row_tables_hold_the_row_counts_and_routes():
    fits = B.row_fits()
    got = [int(f.train_rows().sum()) for f in fits]
    assert got[:len(B.ROW_COUNTS)] == B.ROW_COUNTS
    assert all(f.tab.n - n == 36 for f, n in zip(fits, got[:len(B.ROW_COUNTS) + 1]))
    assert [(f.tab.n, n) for f, n in zip(fits[-3:], got[-3:])] == [(65536, 65535), (65536, 65500), (65537, 65501)]
    assert [B.eligible(f) for f in fits[-3:]] == [True, True, False] and all(B.eligible(f) == (f.route == 1) for f in fits)
    L = {f.name: B.tree_leaves(B.oracle_model(f).save()) for f in fits}
    assert (L["n_train 1"] == 1).all() and (L["n_train 2"] == 1).all() and (L["n_train 39"] == 1).all()      # below 2 * min_data_in_leaf: no search
    assert (L["n_train 40"] > 1).any() and (L["n_train 41"] > 1).any()
    assert all((L[f.name] > 4).all() for f in fits if int(f.train_rows().sum()) >= 511)


def test_budget_tables_reach_their_budgets():
    for fit, leaves in B.leaf_budget_fits():
        L = B.tree_leaves(B.oracle_model(fit).save())
        assert (L == leaves).all(), "%s: %s" % (fit.name, L.tolist())
        assert B.eligible(fit) == (fit.route == 1)
    for fit, F in zip(B.feature_count_fits(), B.FEATURE_COUNTS):
        assert len(fit.feats) == F and B.eligible(fit) == (F <= 255) == (fit.route == 1)
        blob = B.oracle_model(fit).save()
        assert all(b == (2, 0) for b in B.blob_bins(blob)) and (B.tree_leaves(blob) >= 2).all()
        if fit.route == 1:
            assert B.expected_report(fit)["nchunk"] == (F + 15) // 16
        if F >= 17:
            assert (B.tree_features(blob) >= 16).any(), "F = %d: no split on a feature of a later record" % F


def test_class_count_tables():
    fits = B.class_count_fits()
    assert [f.K for f in fits] == [2, 3, 64, 113, 219, 0]
    assert [f.class_weight is not None for f in fits] == [False, True, False, True, False, False]
    for f in fits[:-1]:
        y = f.tab.codes[f.target]
        assert len(np.unique(y[y >= 0])) == f.K
        assert (B.tree_leaves(B.oracle_model(f).save()) > 1).any()
    r = fits[-1]
    y = r.tab.codes[r.target]
    assert len(np.unique(y[y >= 0])) >= 2990 and r.params["max_bin"] == 15
    assert max(v + nan for v, nan in B.blob_bins(B.oracle_model(r).save())) <= 15


def test_no_bag_is_empty():
    fits = B.bagging_fits()
    for f in fits:
        n = int(f.train_rows().sum())
        assert f.tab.n > n
        sizes = B.bag_sizes(f)
        assert sizes.shape[0] == 7 and (sizes > 0).all(), "%s: bags %s" % (f.name, sizes[:, 0].tolist())
        if f.params.get("bagging_freq", 0) > 0:
            assert (sizes < n).all(), f.name
            fr = f.params["bagging_freq"]
            assert all((sizes[i] == sizes[i - i % fr]).all() for i in range(7)) and len(set(sizes[:, 0].tolist())) > 1, f.name
        else:
            assert (sizes == n).all()
    blocks = [(int(f.train_rows().sum()) + 1023) // 1024 for f in fits if f.params.get("bagging_freq", 0) > 0]
    assert set(blocks) >= {1, 2, 3, 6}
    one = [f for f in fits if f.params.get("feature_fraction", 1.0) < 1.0][0]
    from repair import _native as N
    _, n_iter, trees = N.model_trees(B.oracle_model(one).save())
    assert all(len(set(t["feat"].tolist())) <= 1 for t in trees) and len(set(int(t["feat"][0]) for t in trees if len(t["feat"]))) > 1


def test_a_fit_of_the_freeze_case_stops_early():
    fits = B.freeze_fits()
    n_iter = [B.oracle_model(f).info()["n_iter"] for f in fits]
    leaves = [B.tree_leaves(B.oracle_model(f).save()).ravel().tolist() for f in fits]
    assert n_iter == [1, 1, 9, 2, 3, 3], n_iter
    assert leaves[0] == [1] and leaves[1] == [2] and leaves[3] == [2, 2]      # stopped with no tree at all / after one / after two iterations


def test_composition_case():
    fits = B.composition_fits()
    assert [f.params["n_estimators"] for f in fits if not f.fails][:3] == [1, 4, 9]
    assert fits[2].fails and not (fits[2].tab.codes[fits[2].target] >= 0).any() and 0 < 2 < len(fits) - 1
    assert B.expected_report(fits[-1])["scan_waves"] == 4 and len(fits[-2].feats) == 1
    assert B.expected_report(fits[-1])["lds_bytes"] > 2 * B.expected_report(fits[-2])["lds_bytes"]
    assert B.expected_report(B.dummy_fit(), alone=True)["route"] == 3


def test_rare_code_has_a_bin_in_one_fold_only():
    even, not3 = B.fold_fits()
    assert int((even.tab.codes[0] == B.RARE_CODE).sum()) == 4 and int((not3.tab.codes[0] == B.RARE_CODE).sum()) == 1
    ub_even, ub_not3 = (B.blob_upper_bounds(B.oracle_model(f).save(), 0) for f in (even, not3))
    assert B.RARE_CODE in ub_even and B.RARE_CODE - 1 in ub_even, ub_even          # its own bin: (16, 17]
    assert B.RARE_CODE not in ub_not3, ub_not3                                      # merged with the next code's
    # the numeric column's bounds sit at value midpoints, the categorical column is marked in the blob version
    assert even.tab.values and even.tab.kinds == (2,)


def test_zipf_column_has_more_codes_than_bins():
    f = B.zipf_fit()
    x = f.tab.codes[0][f.train_rows()]
    assert len(np.unique(x[x >= 0])) > 300
    V, nan = B.blob_bins(B.oracle_model(f).save())[0]
    assert nan == 1 and 20 <= V <= 61


def test_validation_tables():
    fits = B.valid_fits()
    nv = [f.valid.n for f in fits if f.valid is not None]
    assert nv[:5] == B.VALID_ROWS and any(f.valid is None for f in fits)
    big = [f for f in fits if f.valid is not None and f.valid.n == 16385][0]
    assert big.valid.n > big.tab.n
    for f in fits:
        if f.valid is not None:
            lab, val = B.oracle_valid(f)
            assert len(lab) == f.valid.n and np.isfinite(val).all()
            assert (lab == -1).all() if f.K == 0 else len(np.unique(lab)) > (1 if f.valid.n > 1 else 0)
    two = B.valid_two_chunk_fit()
    assert B.expected_report(two)["nchunk"] == 2 and (B.tree_features(B.oracle_model(two).save()) >= 16).any()
    cat = B.valid_categorical_fit()
    tr0, va0 = cat.tab.codes[0], cat.valid.codes[0]
    assert not (tr0 == B.UNSEEN_CODE).any() and (va0 == B.UNSEEN_CODE).any() and (va0 == B.OUT_OF_DICT).any() and B.OUT_OF_DICT >= cat.tab.cards[0]
    assert (va0 < 0).any() and (cat.valid.codes[1] < 0).any() and 0 in cat.tab.kinds
    assert (B.tree_features(B.oracle_model(cat).save()) == 0).any()


def test_lds_branches_are_out_of_reach():
    """The sum in the docstring of tests/test_gpu_batch_edges.py, searched over every feature shape instead of argued for one."""
    # one wave per feature: 16 features x 256 replicated slots x 16 B, 256 leaves, 255 features
    assert B.sm_lds_bytes(16 * 256 * 16, 256, 255) == 65536 + 24576 + 24480 + 64 == 114656 < 160 * 1024 - 2048
    # packed: at most 256 lanes.  A feature of l lanes has at most 4 l + 1 bins and costs 96 B of candidates + 32 B per bin <= 256 l bytes (equality: one
    # lane, five bins); the 16 features of the chunk that sets lds_hist add 16 B per replicated slot.  So the bytes are at most
    # 256 lanes x 256 + 16 x max over shapes of (16 slots - (256 l - 96 - 32 bins)) + 256 leaves x 96 + 64.
    extra = 0
    for V in range(0, 255):
        for nan in (0, 1):
            b, l = max(V + nan, 1), max(1, (V + 3) // 4)
            sh = 0
            while sh < 5 and (b << (sh + 1)) <= 256:
                sh += 1
            assert 96 + 32 * b <= 256 * l
            extra = max(extra, 16 * (b << sh) - (256 * l - 96 - 32 * b))
    bound = 256 * 256 + 16 * extra + 256 * B.SIZEOF_LEAF + 64
    assert extra == 16 * 256 + 96 + 32 * 8 - 2 * 256 == 3936 and bound == 65536 + 16 * 3936 + 24576 + 64 == 153152 <= 150 * 1024, (extra, bound)
    # ... and the bound is met: 16 eight-bin features (two lanes each) and 224 five-bin features (one lane each)
    assert B.sm_lds_bytes(16 * 256 * 16, 256, 240, 16 * 8 + 224 * 5) == 153152 < 160 * 1024 - 2048
