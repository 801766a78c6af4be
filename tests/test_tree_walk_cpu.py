"""CPU: the reference of tests/test_gpu_predictor_forms.py is held to the oracle, the library's choice of predictor form to a
restatement of its rule, and the model loader to "the child links form a tree".

* tests/tree_walk.py must give `OracleModel.predict`'s bits on every hand-built model of the GPU list (tests/predictor_form_cases.py),
  and the blobs it writes must come back byte for byte from the oracle and from the product: the GPU tests then only compare the
  device with the walk.
* `Model.predict_form()` (rgbm_model_predict_form: the rule `predict_device` launches from; it needs no device) must name the form each
  case is built to hit, and agree with a Python restatement of the rule for table sizes S on both sides of every turn-over, with and
  without RGBM_QS_FIXED=0 and RGBM_PREDICTOR=walk.
* rgbm_model_load must refuse a blob whose child links are in range and in order but do not form a tree: `device_model`'s in-order
  traversal of such a tree emits more than L leaves and writes past the tree's leaf block on the host.
"""
import struct

import numpy as np
import pytest

from tests import predictor_form_cases as PC
from tests import tree_walk as W

RGBM_ERR_FORMAT = -20


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("case", PC.CASES, ids=[c.name for c in PC.CASES])
def test_walk_gives_the_oracle_bits_and_the_case_hits_its_form(case):
    from oracle import oracle as O
    from repair import _native as N
    m, X = case.make()
    assert X.shape == (m["F"], PC.N_ROWS)
    b = W.blob(m)
    om = O.OracleModel.load(b)
    assert om.save() == b
    want = om.predict(X)
    got = W.predict(m, X)
    assert want.shape == got.shape and np.array_equal(_bits(want), _bits(got))
    pm = N.Model.load(b)
    assert pm.save() == b
    pf = pm.predict_form()
    assert (pf["form"], pf["MW"], pf["TW"], pf["tb"]) == case.form
    S, max_leaves = W.table_entries(m["feats"]), max(t["L"] for t in m["trees"])
    assert PC.restated_form(max_leaves, m["F"], S) == (pf["form"], pf["MW"], pf["TW"], pf["tb"], pf["lds"])


@pytest.mark.parametrize("L", [31, 32, 33, 63, 64, 65])
@pytest.mark.parametrize("kind", ["left", "right", "random"])
def test_leaf_cases_leave_at_the_edge_leaves(L, kind):
    """rows leave the L-leaf trees at in-order leaf 0, 31, 32, 63, 64 (those the tree has) and at the last one; a chain is L - 1 deep"""
    m, X = PC.BY_NAME["leaves L=%d %s" % (L, kind)].make()
    pos = W.exit_positions(m, X)
    for t in (0, 1):
        assert m["trees"][t]["L"] == L
        assert {p for p in (0, 31, 32, 63, 64, L - 1) if p < L} <= set(int(x) for x in np.unique(pos[t]))
        if kind == "left":
            assert (m["trees"][t]["left"][:-1] >= 0).all() and (m["trees"][t]["right"] < 0).all()
        if kind == "right":
            assert (m["trees"][t]["right"][:-1] >= 0).all() and (m["trees"][t]["left"] < 0).all()


def test_feature_probes_read_every_feature_and_rows_differ_in_one_feature_only():
    for F in (16, 17, 32, 33):
        m, X = PC.BY_NAME["feature probe F=%d" % F].make()
        assert [int(t["feat"][0]) for t in m["trees"]] == list(range(F))
        raw = W.raw_scores(m, X)[:, 0]
        went_left = raw.astype(np.int64)                     # exact: bit j = feature j went left
        assert np.array_equal(went_left.astype(np.float64), raw)
        seen = np.bitwise_or.reduce(went_left), np.bitwise_or.reduce(~went_left & ((1 << F) - 1))
        assert seen[0] == seen[1] == (1 << F) - 1            # every feature sends rows both ways
        # the one-feature probes: rows that differ from the base row (the first) in exactly one feature, for every feature
        differs = (X != X[:, :1])
        only = np.flatnonzero(differs.sum(axis=0) == 1)
        assert set(np.argmax(differs[:, only], axis=0).tolist()) == set(range(F))


def test_probe_rows_hold_nulls_out_of_dictionary_and_unseen_codes():
    m, X = PC.BY_NAME["thresholds dleft=1 unseen categories (blob version 2)"].make()
    assert struct.unpack_from("<2i", W.blob(m))[1] == 2
    for f, ft in enumerate(m["feats"]):
        col = X[f]
        assert (col == -1).any() and (col == ft["n_codes"]).any() and (col > ft["n_codes"]).any()
        assert (col == 0).any() and (col == ft["n_codes"] - 1).any()
        for c in ft["unseen"][:1]:
            assert (col == c).any()
    thetas = {(int(f), int(th)) for t in m["trees"] for f, th in zip(t["feat"], t["theta"])}
    assert {(0, -1), (0, 0), (1, -1), (1, 254), (4, 253)} <= thetas       # theta = -1 and theta = V - 1 (V = 1, 255, 254)


def _walked(name):
    m, X = PC.BY_NAME[name].make()
    want = W.predict(m, X)
    return (X, want) + W.label_top(m, want)


def test_ties_zero_scores_and_saturation_are_what_the_cases_say():
    """the walk's own answers on the score-conversion cases, so that the comparison on the device pins what they are built for: the first
    maximum on an exact tie, (0.5, 0.5) with label 0 at raw 0, and exponentials that saturate on both sides"""
    X, want, lab, top = _walked("exact ties between two and between all classes")
    b = np.minimum(X[0], 3)
    ok = (X[0] >= 0) & (X[0] < 5)
    assert (want[ok & (b == 0)] == want[ok & (b == 0)][:, :1]).all() and (lab[ok & (b == 0)] == 0).all()
    t1 = ok & (b == 1)
    assert (want[t1][:, 1] == want[t1][:, 2]).all() and (want[t1][:, 1] > want[t1][:, 0]).all() and (lab[t1] == 1).all()
    t2 = ok & (b == 2)
    assert (want[t2][:, 0] == want[t2][:, 2]).all() and (want[t2][:, 0] > want[t2][:, 1]).all() and (lab[t2] == 0).all()
    X, want, lab, top = _walked("binary raw score 0")
    assert (want == 0.5).all() and (lab == 0).all() and (top == 0.5).all()
    X, want, lab, top = _walked("saturation binary")
    assert {0.0, 1.0} <= set(np.unique(want).tolist()) and np.isfinite(want).all()
    X, want, lab, top = _walked("saturation multiclass")
    assert {0.0, 1.0} <= set(np.unique(want).tolist()) and np.isfinite(want).all()


# ---------------------------------------------------------------------------------------------------------------- form selection
def _one_tree_model(max_leaves, F, S, rng):
    feats = W.features_of_size(F, S)
    spec, _ = W.grow(W.shape(max_leaves, "random", rng), feats, rng)
    return W.model(2, 1, feats, [W.tree(spec, "random", rng)])


# S on both sides of every turn-over.  Fixed strides: S MW + MW <= TW, at S = 255 | 256, 511 | 512, 1023 | 1024.  Dynamic strides:
# tb (4 S MW + 256 MW + 4) <= (48 KB - 16) / 2 = 24568; MW 1: tb 8 -> 7 at S = 702 | 703, 2 -> 1 at 3006 | 3007, 1 -> the walk at
# 6077 | 6078; MW 2: 8 -> 7 at 319 | 320 (reached only with RGBM_QS_FIXED=0), 2 -> 1 at 1471 | 1472, 1 -> the walk at 3006 | 3007.
EDGES = [255, 256, 511, 512, 1023, 1024, 702, 703, 3006, 3007, 6077, 6078, 319, 320, 1471, 1472]
EXPECT_DEFAULT = {
    # (MW, F): {S: (form, TW, tb)} -- written out by hand from the rule, for the sizes the feature count can reach
    (1, 16): {255: ("fixed", 256, 8), 256: ("fixed", 512, 8), 511: ("fixed", 512, 8), 512: ("dynamic", 0, 8), 702: ("dynamic", 0, 8),
              703: ("dynamic", 0, 7), 3006: ("dynamic", 0, 2), 3007: ("dynamic", 0, 1)},
    (1, 32): {511: ("fixed", 512, 8), 512: ("fixed", 1024, 4), 1023: ("fixed", 1024, 4), 1024: ("dynamic", 0, 5), 3006: ("dynamic", 0, 2),
              3007: ("dynamic", 0, 1), 6077: ("dynamic", 0, 1), 6078: ("walk", 0, 0)},
    (2, 16): {255: ("fixed", 512, 8), 256: ("fixed", 1024, 4), 511: ("fixed", 1024, 4), 512: ("dynamic", 0, 5), 1471: ("dynamic", 0, 2),
              1472: ("dynamic", 0, 1), 3006: ("dynamic", 0, 1), 3007: ("walk", 0, 0)},
    (2, 32): {511: ("fixed", 1024, 4), 512: ("fixed", 2048, 2), 1023: ("fixed", 2048, 2), 1024: ("dynamic", 0, 2), 1471: ("dynamic", 0, 2),
              1472: ("dynamic", 0, 1), 3006: ("dynamic", 0, 1), 3007: ("walk", 0, 0)},
}
EXPECT_NO_FIXED = {   # RGBM_QS_FIXED=0: trees per stage of the dynamic scorer
    1: {255: 8, 256: 8, 511: 8, 702: 8, 703: 7}, 2: {255: 8, 256: 8, 319: 8, 320: 7, 511: 5},
}


@pytest.mark.parametrize("F", [16, 32], ids=["F<=16", "F 17-32"])
@pytest.mark.parametrize("MW", [1, 2])
def test_form_selection_at_every_turn_over(MW, F, monkeypatch):
    from repair import _native as N
    rng = np.random.default_rng(100 * MW + F)
    max_leaves = 32 if MW == 1 else 33
    seen = set()
    for S in EDGES:
        if not 2 * F <= S <= 256 * F:
            continue
        mdl = N.Model.load(W.blob(_one_tree_model(max_leaves, F, S, rng)))
        for env in ({}, {"RGBM_QS_FIXED": "0"}, {"RGBM_PREDICTOR": "walk"}, {"RGBM_QS_FIXED": "0", "RGBM_PREDICTOR": "walk"}, {"RGBM_QS_FIXED": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            pf = mdl.predict_form()
            got = (pf["form"], pf["MW"], pf["TW"], pf["tb"], pf["lds"])
            for k in env:
                monkeypatch.delenv(k)
            want = PC.restated_form(max_leaves, F, S, qs_fixed=env.get("RGBM_QS_FIXED") != "0", walk="RGBM_PREDICTOR" in env)
            assert got == want, (S, env)
            assert pf["lds"] <= 48 * 1024
            if "RGBM_PREDICTOR" in env:
                assert pf["form"] == "walk"
            elif env.get("RGBM_QS_FIXED") == "0":
                assert pf["form"] != "fixed"
                if S in EXPECT_NO_FIXED[MW]:
                    assert (pf["form"], pf["tb"]) == ("dynamic", EXPECT_NO_FIXED[MW][S])
            elif S in EXPECT_DEFAULT[(MW, F)]:
                form, TW, tb = EXPECT_DEFAULT[(MW, F)][S]
                assert (pf["form"], pf["TW"], pf["tb"]) == (form, TW, tb) and pf["MW"] == (0 if form == "walk" else MW)
                seen.add(S)
    assert seen == set(EXPECT_DEFAULT[(MW, F)])


def test_form_selection_at_the_leaf_and_feature_limits():
    from repair import _native as N
    rng = np.random.default_rng(7)

    def form(max_leaves, F, S):
        pf = N.Model.load(W.blob(_one_tree_model(max_leaves, F, S, rng))).predict_form()
        assert (pf["form"], pf["MW"], pf["TW"], pf["tb"], pf["lds"]) == PC.restated_form(max_leaves, F, S)
        return pf["form"], pf["MW"], pf["TW"]

    assert form(32, 4, 150) == ("fixed", 1, 256) and form(33, 4, 150) == ("fixed", 2, 512)          # one | two mask words
    assert form(64, 4, 150) == ("fixed", 2, 512) and form(65, 4, 150) == ("walk", 0, 0)              # 64 | 65 leaves
    assert form(20, 16, 300) == ("fixed", 1, 512) and form(20, 17, 510) == ("fixed", 1, 512)         # F <= 16 | 17-32 rows of the table
    assert form(20, 16, 520) == ("dynamic", 1, 0) and form(20, 17, 520) == ("fixed", 1, 1024)
    assert form(20, 32, 300) == ("fixed", 1, 512) and form(20, 33, 300) == ("walk", 0, 0)            # 32 | 33 features
    # a model of stumps has one-leaf trees: one mask word; a model without trees has nothing to stage: the walk
    assert N.Model.load(W.blob(W.model(2, 1, [W.feature(3)], [W.stump(1.5)]))).predict_form()["form"] == "fixed"
    assert N.Model.load(W.blob(W.model(2, 1, [W.feature(3)], []))).predict_form()["form"] == "walk"


# ---------------------------------------------------------------------------------------------------------------- the loader
def _raw_tree_blob(L, left, right):
    """a one-tree regression model over one 4-bin feature with the given child links, written without tree_walk's own checks"""
    n = L - 1
    out = [struct.pack("<7i", W.MAGIC, 1, 2, 1, 1, 1, 1), struct.pack("<3i", 4, 4, 0), np.asarray([0, 1, 2, W.INT32_MAX], "<i4").tobytes()]
    out.append(struct.pack("<i", L))
    for arr in (np.zeros(n), np.arange(n) % 3, np.zeros(n), left, right):
        out.append(np.asarray(arr, "<i4").tobytes())
    out.append(np.ones(n, "<f8").tobytes() + np.arange(L).astype("<f8").tobytes() + np.ones(L, "<i4").tobytes())
    return b"".join(out)


NOT_TREES = {
    # every link in range, every internal child above its parent
    "a shared leaf": (4, [1, ~0, ~2], [2, ~1, ~1]),
    "a shared leaf, another never referenced": (4, [1, ~0, ~2], [2, ~1, ~0]),
    "a shared internal node": (4, [1, 2, ~0], [2, ~1, ~2]),
    "a shared internal node and an unreferenced one": (5, [1, 3, ~0, ~1], [3, ~2, ~3, ~4]),
    "an unreferenced leaf": (3, [1, ~0], [~1, ~1]),
    "an unreferenced internal node": (4, [2, ~0, ~1], [~3, ~1, ~2]),
}


def test_the_writers_own_blobs_are_accepted_so_the_refusals_below_are_about_the_links():
    from repair import _native as N
    assert N.Model.load(_raw_tree_blob(4, [1, ~0, ~2], [2, ~1, ~3])).info()["n_iter"] == 1
    assert N.Model.load(_raw_tree_blob(1, [], [])).info()["n_iter"] == 1


@pytest.mark.parametrize("name", list(NOT_TREES))
def test_loader_refuses_child_links_that_do_not_form_a_tree(name):
    from repair import _native as N
    L, left, right = NOT_TREES[name]
    with pytest.raises(N.RepairGbmError, match="do not form a tree") as e:
        N.Model.load(_raw_tree_blob(L, left, right))
    assert e.value.code == RGBM_ERR_FORMAT


def test_loader_still_takes_trained_blobs():
    """models of the kinds the suite trains and loads (binary, multiclass, regression, categorical features with unseen categories =
    blob version 2, trees that stay stumps) load and come back byte for byte"""
    from oracle import oracle as O
    from repair import _native as N
    rng = np.random.default_rng(3)
    cards = [3, 5, 9, 17, 4, 6, 33, 2]
    X = np.stack([rng.integers(0, c, 1500) for c in cards]).astype(np.int32)
    X[rng.random(X.shape) < 0.02] = -1
    X[6][X[6] == 20] = 21                                    # a category no row holds
    y3 = ((X[0] * 3 + X[1] * 5 + X[4] * 7 + X[-1]) % 3).astype(np.int32)
    fits = [
        dict(y=y3, K=3, kw=dict(objective=1, num_class=3, n_estimators=6, num_leaves=31, learning_rate=0.2)),
        dict(y=y3, K=3, kw=dict(objective=1, num_class=3, n_estimators=4, num_leaves=100, max_depth=-1, min_data_in_leaf=3, learning_rate=0.2)),
        dict(y=(y3 > 0).astype(np.int32), K=2, kw=dict(objective=0, num_class=2, n_estimators=6, learning_rate=0.2)),
        dict(y=y3, K=3, kw=dict(objective=1, num_class=3, n_estimators=3, min_data_in_leaf=1400)),          # no split possible: stumps
        dict(y=y3, K=3, kw=dict(objective=1, num_class=3, n_estimators=4, learning_rate=0.2), categorical=[3, 6]),
        dict(y=y3, K=3, kw=dict(objective=2, n_estimators=5, learning_rate=0.2), y_value=True),
    ]
    versions = set()
    for fit in fits:
        extra = {}
        if fit.get("categorical"):
            extra["categorical"] = fit["categorical"]
        if fit.get("y_value"):
            extra["y_value"] = np.array([0.5, -1.25, 3.0])
        blob = O.train(X, np.asarray(cards, np.int32), fit["y"], fit["K"], **extra, **fit["kw"]).save()
        versions.add(struct.unpack_from("<2i", blob)[1])
        m = N.Model.load(blob)
        assert m.save() == blob
        assert m.predict_form()["form"] in ("fixed", "dynamic", "walk")
    assert versions == {1, 2}


# ---------------------------------------------------------------------------------------------------------------- the chain
def test_chain_walk_gives_the_oracle_chain():
    from oracle import oracle as O
    models, targets, feat_cols, class_codes, table = PC.chain_setup()
    om = [O.OracleModel.load(W.blob(m)) for m in models]
    for cc in (class_codes, [[2, 0], [1, 0]]):               # the full class lists; a list shorter than the classes, in another order
        a, b = table.copy(), table.copy()
        lab_o, top_o = O.repair_chain(om, targets, feat_cols, cc, a)
        lab_w, top_w = W.repair_chain(models, targets, feat_cols, cc, b)
        assert np.array_equal(lab_o, lab_w) and np.array_equal(_bits(top_o), _bits(top_w)) and np.array_equal(a, b)
        filled = (table[4] < 0) & (a[4] >= 0)
        assert filled.any() and np.array_equal(a[4][table[4] >= 0], table[4][table[4] >= 0])
        if len(cc[0]) == 2:
            assert ((lab_o[0] == 2) & (table[4] < 0)).any() and (a[4][(lab_o[0] == 2) & (table[4] < 0)] == -1).all()
        assert len(set(lab_o[0].tolist())) == 3 and len(set(lab_o[1].tolist())) == 2
