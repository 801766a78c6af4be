"""The tables of tests/test_gpu_split_edges.py: exact ties and exact limits of the split search and of the best-first order, importable
without a device (numpy only).  tests/test_split_cases_cpu.py holds the CPU oracle to tests/split_restatement.py on every case and
checks, through `holds`, that the edge a case is named after really decides its first tree.

Regression cases use h = 1 and dyadic targets of mean 0 in cells of 16 rows: the initial score is exactly 0, g = -y, every sum is an
exact double, and adding kEpsilon does not change a hessian sum of 16 or more.  Ties come from partitions that mirror each other, so the
two gains are the same double expression on the same operands.  min_data_in_bin = 1 and dense codes: a code is a bin.

A Case: X [F][n] codes (NULL = -1), cards, K (0 = regression), y_code, y_value, weights (or None), params (on top of BASE), `used`
(the features tree 0 may use, None = all), gh(k) -> the exact per-row (g, h) of class tree k in iteration 0, holds(tree, trace).
"""
import itertools
from fractions import Fraction as Fr

import numpy as np

R = 16                                       # rows per cell
BASE = dict(n_estimators=3, learning_rate=0.5, min_data_in_bin=1, min_data_in_leaf=8)
DEFAULTS = dict(num_leaves=31, max_depth=7, min_sum_hessian_in_leaf=1e-3, min_gain_to_split=0.0, lambda_l1=0.0, lambda_l2=0.0)
SMALL_MAX_LEAVES = 256                       # the batched trainer's largest num_leaves (csrc/rgbm_small.h)


def lane_map(V):
    """scan_lane_map's rule (csrc/rgbm_small.h) per feature: (first lane, lanes, moved) -- a lane owns 4 value bins of one feature, the
    features take lanes in order, and a feature that does not fit the rest of its 64-lane wave is moved to the start of the next"""
    out, lanes = [], 0
    for v in V:
        need = max(1, (int(v) + 3) // 4)
        moved = lanes % 64 + need > 64
        if moved:
            lanes += 64 - lanes % 64
        out.append((lanes, need, moved))
        lanes += need
    return out


class Case:
    def __init__(self, name, X, y, K=0, weights=None, used=None, holds=None, **params):
        """y: per-row Fractions (regression) or class codes"""
        self.name = name
        self.X = np.ascontiguousarray(X, np.int32)
        self.cards = (self.X.max(axis=1) + 1).astype(np.int32)
        self.K, self.used, self.holds = K, used, holds
        self.weights = None if weights is None else np.asarray([float(w) for w in weights], np.float64)
        self._w = None if weights is None else [Fr(w) for w in weights]
        if K == 0:
            self._y = [Fr(v) for v in y]
            vals = sorted(set(self._y))
            self.y_value = np.asarray([float(v) for v in vals], np.float64)
            self.y_code = np.asarray([vals.index(v) for v in self._y], np.int32)
            self.n_y = len(vals)
            wsum = sum((v * w for v, w in zip(self._y, self._w)), Fr(0)) if weights is not None else sum(self._y, Fr(0))
            assert wsum == 0, "%s: the targets do not have mean 0" % name
        else:
            self.y_code, self.y_value, self.n_y = np.asarray(y, np.int32), None, K
            assert (np.bincount(self.y_code, minlength=K) * K == len(self.y_code)).all(), "%s: the classes are not balanced" % name
        assert self.X.shape[1] == len(self.y_code)
        self.params = dict(BASE, objective=2 if K == 0 else (0 if K == 2 else 1), num_class=max(K, 2), **params)

    @property
    def n(self):
        return self.X.shape[1]

    def feats(self):
        """[(V, has_nan)] per feature: one bin per code"""
        return [(int(c), int((x < 0).any())) for c, x in zip(self.cards, self.X)]

    def bins(self):
        return [[int(b) if b >= 0 else int(c) for b in x] for c, x in zip(self.cards, self.X)]

    def class_trees(self):
        return 1 if self.K <= 2 else self.K

    def gh(self, k=0):
        if self.K == 0:
            w = self._w or [Fr(1)] * self.n
            return [-y * wi for y, wi in zip(self._y, w)], list(w)
        if self.K == 2:
            return [Fr(-1, 2) if c else Fr(1, 2) for c in self.y_code], [Fr(1, 4)] * self.n
        p = Fr(1, self.K)
        h32 = Fr(float(np.float32(self.K / (self.K - 1.0) * float(p) * (1.0 - float(p)))))
        return [p - 1 if c == k else p for c in self.y_code], [h32] * self.n

    def grower_params(self):
        d = dict(DEFAULTS, min_data_in_leaf=self.params["min_data_in_leaf"])
        d.update({k: v for k, v in self.params.items() if k in DEFAULTS})
        return d

    def table_codes(self):
        """[F + 1][n]: the features and the target's codes"""
        return np.ascontiguousarray(np.concatenate([self.X, self.y_code[None, :]], axis=0)), np.append(self.cards, max(self.n_y, 1)).astype(np.int32)

    def oracle(self, X=None, y_code=None):
        from oracle import oracle as O
        X = self.X if X is None else X
        return O.train(X, self.cards, self.y_code if y_code is None else y_code, self.n_y, y_value=self.y_value,
                       sample_weight=self.weights, **self.params)

    # routes of tests/test_gpu_split_edges.py
    def single_fit(self):
        return 1 <= self.params.get("max_depth", DEFAULTS["max_depth"]) <= 7

    def table_routes(self):
        return self.weights is None                    # Table.train and train_batch take no per-row weights

    def multiplicities(self):
        """a table with row multiplicities trains with at most two 16-feature chunks of which the last leaves byte 15 of its record free
        (train_table, csrc/rgbm.hip), and takes no per-row weights"""
        F = self.X.shape[0]
        return self.single_fit() and self.table_routes() and (F + 15) // 16 <= 2 and F % 16 != 0

    def batch(self):
        return self.table_routes() and self.params.get("num_leaves", DEFAULTS["num_leaves"]) <= SMALL_MAX_LEAVES

    def distinct_rows(self):
        """(codes [F + 1][m], multiplicities [m]) of the table's distinct rows; np.repeat gives the expanded table back up to row order"""
        T, _ = self.table_codes()
        u, cnt = np.unique(T, axis=1, return_counts=True)
        assert cnt.max() <= 255
        return np.ascontiguousarray(u), cnt.astype(np.uint8)


def _cells(cols, y, r=R):
    """every cell r times: cols [F][cells], y [cells]"""
    r = np.broadcast_to(np.asarray(r), (len(y),))
    return np.repeat(np.asarray(cols, np.int64), r, axis=1), [v for v, k in zip(y, r) for _ in range(int(k))]


def _root(trace):
    return trace["searches"][0]


# ---- threshold ties inside one feature ------------------------------------------------------------------------------------------
def end_isolating(V):
    """-1, 0, ..., 0, +1: thresholds 0 and V - 2 cut one end bin off and mirror each other"""
    return [Fr(-1)] + [Fr(0)] * (V - 2) + [Fr(1)], (0, V - 2)


def antisymmetric(V):
    """b - (V - 1) / 2 for odd V: the two thresholds next to the middle bin mirror each other"""
    return [Fr(b - (V - 1) // 2) for b in range(V)], ((V - 3) // 2, (V - 1) // 2)


def _threshold_tie_holds(f, tied, layout):
    def holds(case, tree, trace):
        best = set(_root(trace)["best"])
        lm = lane_map(case.cards)
        ok = {(f, tied[0], "r"), (f, tied[1], "r")} <= best and tree["feat"][0] == f and tree["theta"][0] == max(tied)
        if layout == "shared":
            ok = ok and not lm[f][2] and lm[f][0] % 64 != 0 and lm[f][0] // 64 == lm[f - 1][0] // 64
        if layout == "moved":
            ok = ok and lm[f][2] and lm[f][0] % 64 == 0 and lm[f][0] > 0
        return ok
    return holds


def threshold_tie_cases():
    out = []
    for prof, V in [(end_isolating, 5), (end_isolating, 9), (end_isolating, 130), (end_isolating, 254), (antisymmetric, 5), (antisymmetric, 9)]:
        y, tied = prof(V)
        name = "%s V=%d" % (prof.__name__.replace("_", " "), V)
        b = np.arange(V)
        X, yy = _cells([b], y)
        out.append(Case(name + " alone", X, yy, holds=_threshold_tie_holds(0, tied, None)))
        if V <= 130:                       # the second feature of a shared wave, behind a 3-bin feature
            X, yy = _cells([b % 3, b], y)
            out.append(Case(name + " shared wave", X, yy, holds=_threshold_tie_holds(1, tied, "shared")))
        # a feature the lane map moves to the next wave
        if V == 254:
            X, yy = _cells([b % 3, b], y)
        elif V == 130:
            X, yy = _cells([(b * 7 + 3) % 130, b], y)      # a bijection that keeps both end bins inside
        else:                              # behind a 249-bin feature (63 lanes) that scatters the rows
            r = 64 if V == 5 else 32
            X, yy = _cells([b, b], y, r)
            X[0] = (np.arange(X.shape[1]) * 101) % 249
        out.append(Case(name + " moved to the next wave", X, yy, holds=_threshold_tie_holds(1, tied, "moved")))
    return out


# ---- reverse against forward ----------------------------------------------------------------------------------------------------
def direction_cases():
    # value bins -3, -1, 1, 3 and a NaN bin of g = 0: (bins <= 1 + NaN | rest) mirrors (bins <= 1 | rest + NaN)
    X, y = _cells([[0, 1, 2, 3, -1]], [Fr(-3), Fr(-1), Fr(1), Fr(3), Fr(0)])

    def tie(case, tree, trace):
        return {(0, 1, "r"), (0, 1, "f")} <= set(_root(trace)["best"]) and (tree["theta"][0], tree["dleft"][0]) == (1, 1)

    # rows 32, 16, 16, 16 and 16 NaN: forward thresholds 0 and 2 mirror each other at gain 48, every reverse candidate is below 20
    X2, y2 = _cells([[0, 1, 2, 3, -1]], [Fr(-1), Fr(0), Fr(0), Fr(1), Fr(1)], [32, 16, 16, 16, 16])

    def forward(case, tree, trace):
        return (set(_root(trace)["best"]) == {(0, 0, "f"), (0, 2, "f")} and (tree["theta"][0], tree["dleft"][0]) == (0, 0)
                and tree["gain"][0] == 48.0)

    return [Case("reverse ties forward", X, y, holds=tie), Case("forward wins with a tie of its own", X2, y2, holds=forward)]


# ---- feature ties ---------------------------------------------------------------------------------------------------------------
PAIRS = [(0, 1), (15, 16), (31, 32), (0, 70), (64, 70)]
BASE_PROFILE = [Fr(-5), Fr(-4), Fr(1), Fr(2), Fr(3), Fr(3)]          # best threshold 1; mirrored: 3


def _feature_tie_table(i, j, kind, y_cells, seed):
    """a 6-bin feature at i and its copy / mirror at j among weak 3-bin fillers"""
    V = len(y_cells)
    X, y = _cells([np.arange(V)], y_cells)
    n = X.shape[1]
    rng = np.random.default_rng(seed)
    cols = rng.integers(0, 3, (j + 2, n))
    cols[:, :3] = np.arange(3)[None, :]                                 # every filler holds its three codes
    base, mirror = X[0], V - 1 - X[0]
    cols[i], cols[j] = {"copy": (base, base), "mirror": (base, mirror), "mirror first": (mirror, base)}[kind]
    return cols, y


def feature_tie_cases():
    out = []
    for (i, j), kind in itertools.product(PAIRS, ("copy", "mirror", "mirror first")):
        X, y = _feature_tie_table(i, j, kind, BASE_PROFILE, 7000 + 100 * i + j)
        ti, tj = {"copy": (1, 1), "mirror": (1, 3), "mirror first": (3, 1)}[kind]

        def holds(case, tree, trace, i=i, j=j, ti=ti, tj=tj):
            return {(i, ti, "r"), (j, tj, "r")} <= set(_root(trace)["best"]) and tree["feat"][0] == i and tree["theta"][0] == ti

        out.append(Case("feature %d and its %s at %d" % (i, kind, j), X, y, holds=holds))
    return out


# ---- a masked neighbour ---------------------------------------------------------------------------------------------------------
MASKED_SEED, MASKED_USED = 0, [True, False, True, False]      # found by search on the oracle (seeds 0, 1, 2, ...); `holds` checks it


def masked_case(seed, used):
    """feature 1 (y +-4) is the strongest, feature 2 (y +-2) the next; feature_fraction 0.5 and a seed that leaves 1 out of tree 0 and 2 in"""
    a, b = np.meshgrid(np.arange(2), np.arange(2), indexing="ij")
    a, b = a.ravel(), b.ravel()
    X, y = _cells([a, a, b, b], [Fr(4 * (2 * int(u) - 1) + 2 * (2 * int(v) - 1)) for u, v in zip(a, b)])
    rng = np.random.default_rng(7801)
    for f in (0, 3):
        X[f] = rng.integers(0, 2, X.shape[1])
        X[f, :2] = (0, 1)

    def holds(case, tree, trace):
        lm = lane_map(case.cards)
        return (not case.used[1] and case.used[2] and tree["feat"][0] == 2 and 1 not in tree["feat"]
                and lm[2][0] == lm[1][0] + lm[1][1] and lm[2][0] // 64 == lm[1][0] // 64)

    return Case("strongest feature masked below a used one", X, y, used=used, holds=holds, feature_fraction=0.5, seed=seed)


# ---- limits ---------------------------------------------------------------------------------------------------------------------
def _t3(mirror=False):
    """rows 16, 16, 32 with y -4, 0, 2: threshold 0 (gain 341.3) beats threshold 1 (256) where the 16-row child is allowed"""
    b = np.asarray([2, 1, 0] if mirror else [0, 1, 2])
    return _cells([b], [Fr(-4), Fr(0), Fr(2)], [16, 16, 32])


def _theta_is(t):
    return lambda case, tree, trace: len(tree["feat"]) >= 1 and tree["theta"][0] == t


def _leaves_are(k):
    return lambda case, tree, trace: len(tree["leaf_value"]) == k


def sym7(scale_half=None):
    """2^7 cells over seven binary features with weights 64, 32, ..., 1: every level's leaves tie on one feature.  scale_half = s: the
    part below feature 0 is multiplied by s where feature 0 is 0 (tied groups on both sides of leaf index 64)"""
    cells = np.asarray(list(itertools.product((0, 1), repeat=7))).T
    y = []
    for c in cells.T:
        rest = sum(Fr(2 ** (5 - k)) * (2 * int(c[k + 1]) - 1) for k in range(6))
        y.append(Fr(64) * (2 * int(c[0]) - 1) + (rest * scale_half if (scale_half is not None and c[0] == 0) else rest))
    return _cells(cells, y)


LIMIT_PAIRS = []


def limit_cases():
    out = []

    def pair(a, b):
        out.extend([a, b])
        LIMIT_PAIRS.append((a.name, b.name))

    for side, mirror, t_small, t_other in (("left", False, 0, 1), ("right", True, 1, 0)):
        X, y = _t3(mirror)
        pair(Case("min_data_in_leaf = the %s child's 16 rows" % side, X, y, holds=_theta_is(t_small), min_data_in_leaf=16),
             Case("min_data_in_leaf = the %s child's rows + 1" % side, X, y, holds=_theta_is(t_other), min_data_in_leaf=17))
    X, y = _cells([[0, 1]], [Fr(-1), Fr(1)], [32, 32])
    X1, y1 = _cells([[0, 1]], [Fr(-1), Fr(31, 32)], [31, 32])
    pair(Case("root rows = 2 min_data_in_leaf", X, y, holds=_leaves_are(2), min_data_in_leaf=32),
         Case("root rows = 2 min_data_in_leaf - 1", X1, y1, holds=_leaves_are(1), min_data_in_leaf=32))

    def children(ns):
        def holds(case, tree, trace):
            s = {e["leaf"]: e for e in trace["searches"][1:3]}
            return (tree["feat"][0] == 0 and [s[0]["n"], s[1]["n"]] == ns and [s[0]["searched"], s[1]["searched"]] == [k >= 32 for k in ns]
                    and len(tree["leaf_value"]) == 2 + sum(k >= 32 for k in ns))
        return holds

    X, y = _cells([[0, 0, 1, 1], [0, 1, 0, 1]], [Fr(-1) - Fr(15, 64), Fr(-1) + Fr(16, 64), Fr(1) + Fr(15, 64), Fr(1) - Fr(16, 64)], [16, 15, 16, 15])
    X1, y1 = _cells([[0, 0, 1, 1], [0, 1, 0, 1]], [Fr(-5, 4), Fr(-3, 4), Fr(17, 16), Fr(1)], [16, 16, 16, 15])
    pair(Case("both children at 2 min_data_in_leaf - 1 rows", X, y, holds=children([31, 31]), min_data_in_leaf=16, num_leaves=4),
         Case("one child at 2 min_data_in_leaf rows", X1, y1, holds=children([32, 31]), min_data_in_leaf=16, num_leaves=4))
    X, y = _t3()
    pair(Case("min_sum_hessian_in_leaf = a child's hessian", X, y, holds=_theta_is(0), min_data_in_leaf=1, min_sum_hessian_in_leaf=16.0),
         Case("min_sum_hessian_in_leaf = the next double above", X, y, holds=_theta_is(1), min_data_in_leaf=1,
              min_sum_hessian_in_leaf=float(np.nextafter(16.0, np.inf))))
    X, y = _t3(True)                                                   # the same limit on the side the reverse scan accumulates
    pair(Case("min_sum_hessian_in_leaf = the right child's hessian", X, y, holds=_theta_is(1), min_data_in_leaf=1, min_sum_hessian_in_leaf=16.0),
         Case("min_sum_hessian_in_leaf = the next double above the right child's", X, y, holds=_theta_is(0), min_data_in_leaf=1,
              min_sum_hessian_in_leaf=float(np.nextafter(16.0, np.inf))))
    X, y = _cells([[0, 1]], [Fr(-1), Fr(1, 2)], [32, 64])             # the one candidate has gain 1024 / 32 + 1024 / 64 = 48
    pair(Case("min_gain_to_split = the best gain", X, y, holds=_leaves_are(1), min_gain_to_split=48.0),
         Case("min_gain_to_split = the double below the best gain", X, y, holds=_leaves_are(2), min_gain_to_split=float(np.nextafter(48.0, 0.0))))
    X, y = _t3()                                                       # |G| of the children: 64 at both thresholds
    pair(Case("lambda_l1 = a child's |G|", X, y, holds=_leaves_are(1), lambda_l1=64.0),
         Case("lambda_l1 just below a child's |G|", X, y, holds=lambda case, tree, trace: len(tree["leaf_value"]) >= 2,
              lambda_l1=float(np.nextafter(64.0, 0.0))))
    X, y = sym7()
    pair(Case("max_depth 1", X, y, holds=_leaves_are(2), max_depth=1, num_leaves=128),
         Case("max_depth 3", X, y, holds=_leaves_are(8), max_depth=3, num_leaves=128))

    def cut(nl):
        def holds(case, tree, trace):
            # levels fill in leaf order: 64 leaves tie for the last level and the first nl - 64 of them are split
            last = trace["picks"][63:]
            return (len(tree["leaf_value"]) == nl and [bl for bl, _ in last] == list(range(nl - 64)) and all(f == 6 for f in tree["feat"][63:])
                    and (not last or last[0][1] == list(range(64))))
        return holds

    nls = [Case("symmetric 7 levels, num_leaves %d" % nl, X, y, holds=cut(nl), num_leaves=nl) for nl in (64, 65, 100, 128)]
    out.extend(nls)
    LIMIT_PAIRS.extend((a.name, b.name) for a, b in zip(nls, nls[1:]))
    return out


# ---- the count estimate at one half ---------------------------------------------------------------------------------------------
def count_half_cases():
    """64 rows of weights 0.5 and 1.5 (sum 64: cnt_factor = 1).  The top bin holds 17 rows of 0.5: h * cnt_factor = 8.5, 9 rows after rounding
    half up -- under min_data_in_leaf 9 the best threshold (1) is allowed only then"""
    X, y = _cells([[0, 1, 1, 2]], [Fr(-1, 2), Fr(-1), Fr(-1, 4), Fr(3)], [16, 15, 16, 17])
    w = [Fr(3, 2)] * 16 + [Fr(1, 2)] * 15 + [Fr(3, 2)] * 16 + [Fr(1, 2)] * 17

    def holds(theta):
        def h(case, tree, trace):
            _, hs = case.gh()
            top = sum(hs[-17:])
            return top == Fr(17, 2) and sum(hs) == case.n and (0, 2, "r") in _root(trace)["halves"] and tree["theta"][0] == theta
        return h

    a = Case("count estimate 8.5 under min_data_in_leaf 9", X, y, weights=w, holds=holds(1), min_data_in_leaf=9)
    b = Case("count estimate 8.5 under min_data_in_leaf 10", X, y, weights=w, holds=holds(0), min_data_in_leaf=10)
    LIMIT_PAIRS.append((a.name, b.name))
    return [a, b]


# ---- leaf ties ------------------------------------------------------------------------------------------------------------------
UNBALANCED_LEAVES = 100


def leaf_tie_cases():
    X, y = sym7(Fr(1, 64))

    def spans(case, tree, trace):
        groups = [tied for _, tied in trace["picks"] if len(tied) > 1 and min(tied) < 64 <= max(tied)]
        last_bl, last = trace["picks"][-1]
        # num_leaves cuts the last group: leaves of it are left unsplit
        return bool(groups) and len(tree["leaf_value"]) == UNBALANCED_LEAVES and len(last) > 1 and min(last) < 64 <= max(last)

    X2, y2 = _cells([[0, 1, 0, 1, 0, 1, 0, 1], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1]],
                    [Fr(-8) + (2 * b - 1) if c == 0 else Fr(8) + (2 * a - 1) for a, b, c in
                     zip([0, 1, 0, 1, 0, 1, 0, 1], [0, 0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 0, 1, 1, 1, 1])])

    def feature_first(case, tree, trace):
        s = {e["leaf"]: e for e in trace["searches"][1:3]}
        return (tree["feat"][:2] == [2, 0] and s[0]["gain"] == s[1]["gain"] and s[0]["best"][0][0] == 1 and s[1]["best"][0][0] == 0
                and trace["picks"][1] == (1, [0, 1]) and tree["right"][0] == 1)

    return [Case("unbalanced 7 levels, tied leaves on both sides of 64", X, y, holds=spans, num_leaves=UNBALANCED_LEAVES),
            Case("two leaves tie, the higher leaf owns the smaller feature", X2, y2, holds=feature_first, num_leaves=3)]


# ---- classification -------------------------------------------------------------------------------------------------------------
def _labels(counts):
    """per bin (a cell of 16 rows) the rows of every class: counts [K][V] -> bins, labels"""
    counts = np.asarray(counts)
    assert (counts.sum(axis=0) == R).all()
    V = counts.shape[1]
    lab = np.concatenate([np.repeat(np.arange(counts.shape[0]), counts[:, b]) for b in range(V)])
    return np.repeat(np.arange(V), R), lab


def classification_cases():
    out = []
    ones = np.asarray([0, 4, 8, 12, 16])
    anti = {2: [16 - ones, ones], 4: [[0, 2, 4, 6, 8], [8, 6, 4, 2, 0], [4] * 5, [4] * 5]}
    o6 = np.asarray([2, 3, 6, 10, 12, 15])
    copy = {2: [16 - o6, o6], 4: [[8, 6, 4, 3, 2, 1], [1, 2, 3, 4, 6, 8], [4] * 6, [3, 4, 5, 5, 4, 3]]}
    for K in (2, 4):
        b, lab = _labels(anti[K])
        out.append(Case("antisymmetric V=5, K=%d" % K, [b], lab, K=K,
                        holds=lambda case, tree, trace: {(0, 1, "r"), (0, 2, "r")} <= set(_root(trace)["best"]) and tree["theta"][0] == 2))
        b, lab = _labels(copy[K])
        out.append(Case("feature 0 and its copy at 1, K=%d" % K, [b, b], lab, K=K,
                        holds=lambda case, tree, trace: {f for f, _, _ in _root(trace)["best"]} == {0, 1} and tree["feat"][0] == 0))
    return out


def all_cases():
    LIMIT_PAIRS.clear()
    cases = (threshold_tie_cases() + direction_cases() + feature_tie_cases() + [masked_case(MASKED_SEED, MASKED_USED)] + limit_cases()
             + count_half_cases() + leaf_tie_cases() + classification_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = None


def cases():
    global CASES
    if CASES is None:
        CASES = all_cases()
    return CASES


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---- the routes of tests/test_gpu_split_edges.py ----------------------------------------------------------------------------------
HOST_ROUTES = [
    ("leafwise", dict(RGBM_GROWER="leafwise")),
    ("level", dict(RGBM_GROWER="level")),
    ("level, scan out of the pool", dict(RGBM_GROWER="level", RGBM_STEP_READBACK=1)),
]
BATCH_IDS = ["packed", "RGBM_SMALL_PACKED=0"]


def host_nodes():
    return [(r, c.name) for r, _ in HOST_ROUTES for c in cases() if c.single_fit()]


def mult_nodes():
    return [c.name for c in cases() if c.multiplicities()]


def batch_names():
    return [c.name for c in cases() if c.batch()]


def gpu_node_ids():
    """every node of tests/test_gpu_split_edges.py, as pytest names it"""
    f = "tests/test_gpu_split_edges.py::"
    return ([f + "test_single_fit_route_gives_the_oracle_model[%s-%s]" % n for n in host_nodes()]
            + [f + "test_level_grower_with_row_multiplicities_gives_the_oracle_model_of_the_expanded_table[%s]" % n for n in mult_nodes()]
            + [f + "test_fused_batch_gives_the_oracle_models[%s]" % i for i in BATCH_IDS])
