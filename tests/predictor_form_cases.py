"""The hand-built models of tests/test_gpu_predictor_forms.py, shared with tests/test_tree_walk_cpu.py (which holds tests/tree_walk.py to
the oracle on every one of them, and the library's form selection to the form each case names).  Python and numpy only.

A case is `Case(name, make, form)`: `make()` returns (model, X) -- a tests/tree_walk.py model and [F][1100] probe codes -- and `form` is
what `Model.predict_form()` must answer for it: (form, MW, TW, trees per stage).  The forms, per csrc/rgbm.hip `predict_form`, with
S = the sum over the features of (V + 1) mask entries and MW = 1 | 2 mask words for <= 32 | <= 64 leaves:

    fixed    the first (TW, TBN) of the model's (MW, F <= 16 | F <= 32) row with S * MW + MW <= TW:
             MW 1, F <= 16: (256, 8) (512, 8)    MW 1, F <= 32: (512, 8) (1024, 4)
             MW 2, F <= 16: (512, 8) (1024, 4)   MW 2, F <= 32: (1024, 4) (2048, 2)
    dynamic  else: the most trees per stage tb <= 8 with 2 tb (4 S MW + 256 MW + 4) + 16 <= 48 KB of LDS
    walk     no such tb, a tree of more than 64 leaves, or more than 32 features
"""
import collections
import functools
import zlib

import numpy as np

from tests import tree_walk as W

N_ROWS = 1100
Case = collections.namedtuple("Case", "name make form")
WALK = ("walk", 0, 0, 0)


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _case(name, form):
    def deco(fn):
        CASES.append(Case(name, functools.lru_cache(maxsize=None)(lambda: fn(_rng(name))), form))
        return fn
    return deco


CASES = []


def grown_model(rng, feats, leaves, objective=2, num_class=1, kinds=("random",), lo=-38, hi=2, aim=(0, 31, 32, 63, 64)):
    """one grown tree per entry of `leaves` (0 / 1: a stump), every tree with its leaf ids permuted; the first rows of X are aimed at the
    in-order leaves `aim` (and the last) of every tree"""
    trees, boxes = [], []
    for i, L in enumerate(leaves):
        if L <= 1:
            trees.append(W.stump(W.leaf_values(1, rng, lo, hi)[0]))
            continue
        spec, bx = W.grow(W.shape(L, kinds[i % len(kinds)], rng), feats, rng, values=W.leaf_values(L, rng, lo, hi))
        trees.append(W.tree(spec, "random", rng))
        boxes += [bx[p] for p in sorted(set(a for a in aim if a < L) | {L - 1})]
    m = W.model(objective, num_class, feats, trees)
    return m, W.probe_rows(m, N_ROWS, rng, boxes[:400])


# ---- feature probes: tree j splits only feature j, the left leaf is 2^j: the sum is exact and its set bits name the features that went left
def _feature_probe(F):
    def make(rng):
        feats = [W.feature(4, n_codes=5, unseen=(3,) if f % 5 == 4 else ()) for f in range(F)]
        trees = [W.tree((j, int(rng.integers(0, 3)), j & 1, float(2.0 ** j), 0.0)) for j in range(F)]
        m = W.model(2, 1, feats, trees)
        return m, W.probe_rows(m, N_ROWS, rng)
    return make


for F_, form_ in ((16, ("fixed", 1, 256, 8)), (17, ("fixed", 1, 512, 8)), (32, ("fixed", 1, 512, 8)), (33, WALK)):
    _case("feature probe F=%d" % F_, form_)(_feature_probe(F_))


# ---- leaf positions: rows leave at in-order leaf 0, 31, 32, 63, 64 of chains to the left, to the right and of random shapes
def _leaf_case(L, kind):
    def make(rng):
        feats = [W.feature(24, n_codes=26, has_nan=f & 1) for f in range(6)]
        return grown_model(rng, feats, [L, L, max(L - 7, 2)], kinds=(kind,))
    return make


for L_ in (31, 32, 33, 63, 64, 65):
    for kind_ in ("left", "right", "random"):
        _case("leaves L=%d %s" % (L_, kind_), ("fixed", 1, 256, 8) if L_ <= 32 else ("fixed", 2, 512, 8) if L_ <= 64 else WALK)(_leaf_case(L_, kind_))


# ---- stage edges: n_iter around the trees per stage of every fixed variant and of the dynamic scorer at 8, 3 and 1 trees per stage
STAGE_CONFIGS = [
    # MW, F, S, form
    (1, 8, 200, ("fixed", 1, 256, 8)), (1, 8, 400, ("fixed", 1, 512, 8)), (1, 20, 400, ("fixed", 1, 512, 8)), (1, 20, 800, ("fixed", 1, 1024, 4)),
    (2, 8, 200, ("fixed", 2, 512, 8)), (2, 8, 400, ("fixed", 2, 1024, 4)), (2, 20, 400, ("fixed", 2, 1024, 4)), (2, 20, 800, ("fixed", 2, 2048, 2)),
    (1, 8, 600, ("dynamic", 1, 0, 8)), (1, 8, 1700, ("dynamic", 1, 0, 3)), (2, 8, 1500, ("dynamic", 2, 0, 1)),
]


def _sized_case(MW, F, S, n_iter, K=1):
    def make(rng):
        feats = W.features_of_size(F, S)
        top = 32 if MW == 1 else 64
        leaves = [int(rng.integers(top // 2 + 1, top + 1))] + [int(rng.integers(2, top + 1)) for _ in range(n_iter * K - 1)]
        return grown_model(rng, feats, leaves, objective=2 if K == 1 else 1, num_class=K, kinds=("random", "left", "right"), aim=(0, 31, 32, 63))
    return make


for MW_, F_, S_, form_ in STAGE_CONFIGS:
    tbn = form_[3]
    for n_iter_ in sorted({1, tbn, tbn + 1, 2 * tbn, 2 * tbn + 1, 4 * tbn + 3}):
        _case("stages %s MW=%d F=%d S=%d n_iter=%d" % (form_[0], MW_, F_, S_, n_iter_), form_)(_sized_case(MW_, F_, S_, n_iter_))


# ---- size edges: S on both sides of every turn-over of the rule
SIZE_EDGES = [
    (1, 8, 255, ("fixed", 1, 256, 8)), (1, 8, 256, ("fixed", 1, 512, 8)), (1, 8, 511, ("fixed", 1, 512, 8)), (1, 8, 512, ("dynamic", 1, 0, 8)),
    (1, 20, 511, ("fixed", 1, 512, 8)), (1, 20, 512, ("fixed", 1, 1024, 4)), (1, 20, 1023, ("fixed", 1, 1024, 4)), (1, 20, 1024, ("dynamic", 1, 0, 5)),
    (2, 8, 255, ("fixed", 2, 512, 8)), (2, 8, 256, ("fixed", 2, 1024, 4)), (2, 8, 511, ("fixed", 2, 1024, 4)), (2, 8, 512, ("dynamic", 2, 0, 5)),
    (2, 20, 511, ("fixed", 2, 1024, 4)), (2, 20, 512, ("fixed", 2, 2048, 2)), (2, 20, 1023, ("fixed", 2, 2048, 2)), (2, 20, 1024, ("dynamic", 2, 0, 2)),
    (1, 8, 702, ("dynamic", 1, 0, 8)), (1, 8, 703, ("dynamic", 1, 0, 7)),                 # trees per stage 8 -> 7
    (1, 20, 3006, ("dynamic", 1, 0, 2)), (1, 20, 3007, ("dynamic", 1, 0, 1)),             # ... -> 1
    (1, 28, 6077, ("dynamic", 1, 0, 1)), (1, 28, 6078, WALK),                             # ... -> not even one: the silent fall to the walk
    (2, 8, 1471, ("dynamic", 2, 0, 2)), (2, 8, 1472, ("dynamic", 2, 0, 1)),
    (2, 16, 3006, ("dynamic", 2, 0, 1)), (2, 16, 3007, WALK),
]
for MW_, F_, S_, form_ in SIZE_EDGES:
    _case("size MW=%d F=%d S=%d" % (MW_, F_, S_), form_)(_sized_case(MW_, F_, S_, 3))


# ---- stumps
@_case("stumps only", ("fixed", 1, 256, 8))
def _stumps_only(rng):
    feats = [W.feature(5) for _ in range(4)]
    return grown_model(rng, feats, [1] * 11)


@_case("stumps between 64-leaf trees", ("fixed", 2, 512, 8))
def _stumps_between(rng):
    feats = [W.feature(24, n_codes=26) for _ in range(6)]
    return grown_model(rng, feats, [64, 1, 64, 1, 1, 64, 1, 64, 1], kinds=("random", "left", "right"))


@_case("one class tree of three is a stump", ("fixed", 1, 256, 8))
def _one_class_stump(rng):
    feats = [W.feature(9, n_codes=11) for _ in range(5)]
    return grown_model(rng, feats, [7, 1, 12] * 5, objective=1, num_class=3)


# ---- thresholds and default directions
def _threshold_case(dleft, unseen):
    def make(rng):
        feats = [W.feature(1, n_codes=3), W.feature(255, n_codes=300), W.feature(5, n_codes=7, unseen=(1, 4) if unseen else ()),
                 W.feature(2, has_nan=1), W.feature(254, n_codes=254, unseen=(0, 253) if unseen else ())]
        d, e = dleft, 1 - dleft
        v = iter(W.leaf_values(64, rng))
        nx = lambda: float(next(v))
        trees = [
            # theta = -1: only a missing value that defaults left goes left;  theta = V - 1: only a missing value that defaults right goes right
            W.tree((0, -1, d, nx(), (0, 0, d, nx(), nx())), "random", rng),
            W.tree((1, -1, d, (1, 254, d, nx(), nx()), (1, 253, e, (1, 0, d, nx(), nx()), nx())), "random", rng),
            W.tree((2, 4, d, (2, -1, e, nx(), (2, 0, d, nx(), (2, 3, d, nx(), nx()))), nx()), "random", rng),
            W.tree((3, 1, d, (3, 0, e, nx(), nx()), nx()), "random", rng),
            W.tree((4, 253, d, (4, 0, d, nx(), (4, 252, e, nx(), nx())), nx()), "random", rng),
            W.tree((1, 254, e, (4, -1, e, nx(), (0, 0, e, nx(), nx())), nx()), "random", rng),
        ]
        m = W.model(2, 1, feats, trees)
        return m, W.probe_rows(m, N_ROWS, rng)
    return make


# S = 2 + 256 + 6 + 3 + 255 = 522: one word, five features -> beyond both fixed variants of its row
for d_ in (0, 1):
    for u_ in (False, True):
        _case("thresholds dleft=%d%s" % (d_, " unseen categories (blob version 2)" if u_ else ""), ("dynamic", 1, 0, 8))(_threshold_case(d_, u_))


# ---- objectives
@_case("binary", ("fixed", 1, 256, 8))
def _binary(rng):
    feats = [W.feature(9, n_codes=11) for _ in range(5)]
    return grown_model(rng, feats, [9, 31, 2, 17, 5], objective=0, num_class=2)


def _multiclass(K, n_iter):
    def make(rng):
        feats = [W.feature(9, n_codes=11) for _ in range(5)]
        return grown_model(rng, feats, [int(x) for x in rng.integers(1, 9, K * n_iter)], objective=1, num_class=K, aim=(0,))
    return make


for K_ in (3, 64, 65, 303):
    _case("multiclass K=%d" % K_, ("fixed", 1, 256, 8))(_multiclass(K_, 2))


@_case("exact ties between two and between all classes", ("fixed", 1, 256, 8))
def _ties(rng):
    # feature 0 picks the pattern: bin 0 all three classes tie, bin 1 classes 1 and 2 tie above class 0, bin 2 classes 0 and 2 tie above
    # class 1, bin 3 no tie; feature 1 adds the same amount to every class
    feats = [W.feature(4, n_codes=5), W.feature(3)]
    a, b = float(np.ldexp(1.37, -3)), float(np.ldexp(1.11, 1))
    per_class = [(a, a, b, 0.25), (a, b, a, 0.5), (a, b, b, 0.125)]
    trees = []
    for it in range(2):
        for k in range(3):
            v = per_class[k]
            if it == 0:
                trees.append(W.tree((0, 1, 0, (0, 0, 1, v[0], v[1]), (0, 2, 0, v[2], v[3])), "random", rng))
            else:
                trees.append(W.tree((1, 0, 1, 0.3, (1, 1, 0, -0.7, 1e-3)), "random", rng))
    m = W.model(1, 3, feats, trees)
    return m, W.probe_rows(m, N_ROWS, rng)


@_case("binary raw score 0", ("fixed", 1, 256, 8))
def _binary_zero(rng):
    # raw 0 three ways: a stump of 0, +x and -x cancelling, and -0.0
    feats = [W.feature(3)]
    x = float(W.leaf_values(1, rng)[0])
    trees = [W.stump(0.0), W.tree((0, 0, 1, x, (0, 1, 0, -0.0, 0.5))), W.tree((0, 0, 1, -x, (0, 1, 0, -0.0, -0.5)))]
    m = W.model(0, 2, feats, trees)
    return m, W.probe_rows(m, N_ROWS, rng)


SATURATING = [700.0, -700.0, 710.0, -710.0, 750.0, -750.0, 709.0, -745.0]


def _saturation(objective):
    def make(rng):
        feats = [W.feature(len(SATURATING)), W.feature(2)]
        spec = SATURATING[-1]
        for b in range(len(SATURATING) - 2, -1, -1):
            spec = (0, b, b & 1, SATURATING[b], spec)          # a chain to the right: bin b leaves at leaf b
        K = 1 if objective == 0 else 3
        trees = []
        for k in range(K):
            trees.append(W.tree(spec if k == 0 else (1, 0, 0, 0.0, 0.5 * k), "random", rng))
        m = W.model(objective, 2 if objective == 0 else 3, feats, trees)
        return m, W.probe_rows(m, N_ROWS, rng)
    return make


_case("saturation binary", ("fixed", 1, 256, 8))(_saturation(0))
_case("saturation multiclass", ("fixed", 1, 256, 8))(_saturation(1))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the chain: two hand-built models on one table, the second reads the first one's target as a feature
def chain_setup():
    """(models, targets, feature lists, class codes, table [6][1100]): model 0 (3 classes) fills column 4 from columns (5, 0, 2); model 1
    (binary) fills column 1 from columns (3, 4, 0, 5) -- column 4 is model 0's target.  Feature lists are in no column order."""
    rng = _rng("chain")
    cards = [6, 2, 9, 7, 3, 5]
    targets = [4, 1]
    feat_cols = [[5, 0, 2], [3, 4, 0, 5]]
    models = []
    for t, (K, obj) in enumerate(((3, 1), (2, 0))):
        feats = [W.feature(cards[c]) for c in feat_cols[t]]
        leaves = [int(x) for x in rng.integers(2, 12, (K if obj == 1 else 1) * 4)]
        models.append(grown_model(rng, feats, leaves, objective=obj, num_class=K, lo=-39, hi=1)[0])
    table = np.stack([rng.integers(0, c, N_ROWS) for c in cards]).astype(np.int32)
    table[rng.random(table.shape) < 0.3] = -1
    table[4, :8] = [-1, 0, 1, 2, -1, -1, 2, 0]
    return models, targets, feat_cols, [[0, 1, 2], [0, 1]], np.ascontiguousarray(table)


# ---- a Python restatement of the rule (csrc/rgbm.hip predict_form), for the form-selection tests
FIXED = {(1, 16): ((256, 8), (512, 8)), (1, 32): ((512, 8), (1024, 4)), (2, 16): ((512, 8), (1024, 4)), (2, 32): ((1024, 4), (2048, 2))}
LDS_BYTES = 48 * 1024


def restated_form(max_leaves, F, S, n_trees=1, qs_fixed=True, walk=False):
    """(form, MW, TW, trees per stage, LDS bytes)"""
    if walk or max_leaves > 64 or F > 32 or n_trees == 0:
        return ("walk", 0, 0, 0, 0)
    MW = 1 if max_leaves <= 32 else 2

    def lds(tb, words):                                      # two buffers of tb trees: masks, 32 MW leaf values, the used-feature word
        return 2 * tb * (4 * words + 8 * 32 * MW + 4) + 16

    if qs_fixed:
        for TW, TBN in FIXED[(MW, 16 if F <= 16 else 32)]:
            if S * MW + MW <= TW:                            # the masks and one all-ones pad entry
                return ("fixed", MW, TW, TBN, lds(TBN, TW))
    for tb in range(8, 0, -1):
        if lds(tb, S * MW) <= LDS_BYTES:
            return ("dynamic", MW, 0, tb, lds(tb, S * MW))
    return ("walk", 0, 0, 0, 0)
