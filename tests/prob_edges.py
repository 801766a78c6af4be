"""Deterministic inputs for the probability-mode kernels beyond one 64-class chunk (k_top_k_pmf / k_weighted_pmf give one wave to a
cell and lane l the classes c = l (mod 64)): a small table whose target has K classes of which a few are carried by no training row --
the model then gives those classes one common score, so every cell holds tied probabilities, and for large K probabilities that are
exactly 0.0 -- and cost matrices with the rows a lane-stride or guard mistake would trip over.  tests/test_prob_edges_cpu.py asserts
on the oracle that the inputs have these properties; a device test built on them compares with the oracle's probabilities."""
import numpy as np

KS = (63, 64, 65, 128, 129, 303)
N_ROWS, N_FEATS, NULL_EVERY = 4000, 7, 8          # 500 NULL target cells
TRAIN = dict(objective=1, n_estimators=4, learning_rate=0.2)
WEIGHTS = (0.1, 0.7)


def absent_classes(K):
    """Label codes without a training row: on both sides of the 64-class chunk edges where K reaches them, the last class, and
    for K > 64 classes that share a lane of the one-wave-per-cell kernels (0 / 64 / 128 / 192 / 256, 1 / 65, 63 / 127)."""
    return sorted({c for c in (0, 1, 5, 62, 63, 64, 65, 127, 128, 192, 256, K // 2, K - 2, K - 1) if c < K})


def make_edge_table(K, seed=0):
    """(codes [F + 1][n] int32 with the target in the last column and NULL in every NULL_EVERY-th row, cards [F + 1])."""
    rng = np.random.default_rng(1000 + K + seed)
    cards = np.array([12, 9, 7, 5, 11, 6, 4][:N_FEATS] + [K], np.int32)
    X = np.stack([rng.integers(0, int(cards[f]), N_ROWS) for f in range(N_FEATS)]).astype(np.int32)
    present = np.array([c for c in range(K) if c not in set(absent_classes(K))], np.int32)
    y = present[(5 * X[0] + 3 * X[1] + 7 * X[4] + rng.integers(0, 3, N_ROWS)) % len(present)]
    y[::NULL_EVERY] = -1
    return np.ascontiguousarray(np.vstack([X, y[None, :]]), np.int32), cards


def train_oracle(codes, cards, K):
    from oracle import oracle as O
    t = N_FEATS
    rows = codes[t] >= 0
    return O.train(np.ascontiguousarray(codes[:t][:, rows]), cards[:t], codes[t][rows], K, num_class=K, **TRAIN)


def null_cell_probabilities(model, codes):
    null_rows = np.flatnonzero(codes[N_FEATS] < 0)
    return null_rows, np.asarray(model.predict(np.ascontiguousarray(codes[:N_FEATS][:, null_rows])), np.float64)


def cur_codes(K, m):
    """Current values that hit class 0, 63, 64, K - 1, no class (-1) and codes beyond the classes, then a fixed scramble."""
    pat = np.array([0, 63, 64, K - 1, -1, K, K + 5, 1, K // 2], np.int64)
    cur = pat[np.arange(m) % len(pat)]
    tail = np.arange(m) >= 6 * len(pat)
    cur[tail] = (np.arange(m)[tail] * 37) % (K + 2) - 1
    return cur.astype(np.int32)


# rows of the cost matrices, by name; the self row (each class against itself) is the last row of a matrix
SPECIAL_ROWS = ("inf", "huge_alternating", "nan", "negative")


def cost_matrices(K):
    """{name: (cost [R + 1][K] float64, {special row name: row index})}.  Both matrices hold an all-+inf row (every class weighted to
    exactly 0: norm == 0, no top-1 above 0), a row with 1e308 on every second class, an all-NaN row (None costs: the cell is left
    alone) and a row of negative costs -7.5 / -3.25 / -0.5 / 1.5: with the weights 0.1 and 0.7 the denominators 1 + weight * cost are
    0.25, 0.675, 0.95, 1.15 and -4.25, -1.275, 0.65, 2.05 -- never 0, some negative, as the Python loop computes them too."""
    out = {}
    for name, seed, lo, hi in (("integers", 1, 0, 12), ("steep", 2, 0, 400)):
        rng = np.random.default_rng(7000 + 10 * K + seed)
        R0 = 6
        rows = [rng.integers(lo, hi, K).astype(np.float64) for _ in range(R0)]
        for r in rows:
            r[rng.random(K) < 0.2] = np.nan
        special = {}
        special["inf"] = len(rows); rows.append(np.full(K, np.inf))
        special["huge_alternating"] = len(rows); rows.append(np.where(np.arange(K) % 2 == 0, 1e308, 0.0))
        special["nan"] = len(rows); rows.append(np.full(K, np.nan))
        special["negative"] = len(rows); rows.append(np.array([-7.5, -3.25, -0.5, 1.5])[rng.integers(0, 4, K)])
        self_row = np.arange(K) * 0.5 + (1.0 if name == "steep" else 0.0)
        self_row[rng.random(K) < 0.3] = np.nan
        rows.append(self_row)
        out[name] = (np.ascontiguousarray(np.stack(rows), np.float64), special)
    return out


def cost_rows(m, n_rows):
    """Per cell: every row of the matrix in turn, and -1 (leave the cell alone; top1_cost then reads the self row)."""
    return ((np.arange(m) * 5) % (n_rows + 1) - 1).astype(np.int32)


def has_tie(values):
    v = np.sort(np.asarray(values, np.float64))
    return bool((v[1:] == v[:-1]).any())


def tied_probability(p, above=0.0):
    """The most frequent probability > `above` that at least two classes of one cell share (None if there is none)."""
    best, count = None, 0
    for row in p:
        v, c = np.unique(row[row > above], return_counts=True)
        if len(v) and c.max() >= 2 and c.max() > count:
            best, count = float(v[np.argmax(c)]), int(c.max())
    return best


def same_lane_tie(row, selected=None):
    """Two classes c != c' with c = c' (mod 64) -- one lane of the one-wave-per-cell kernels owns both -- and equal probability."""
    row = np.asarray(row, np.float64)
    for lane in range(min(64, len(row))):
        v = row[lane::64] if selected is None else row[lane::64][selected[lane::64]]
        if len(v) > 1 and has_tie(v):
            return True
    return False


def check_probabilities(K, proba):
    """The conditions that keep the K-class case from degenerating, asserted on the reference probabilities: ties among the classes a
    threshold of 0.0 selects (a tenth of the cells at least), for K > 64 ties inside one lane, for K >= 128 exact zeros."""
    m = len(proba)
    assert sum(has_tie(r[r > 0.0]) for r in proba) >= m // 10, "K=%d: no tied probabilities above 0.0" % K
    assert tied_probability(proba) is not None
    if K > 64:
        assert sum(same_lane_tie(r) for r in proba) >= m // 10, "K=%d: no tie between two classes of one lane" % K
    if K >= 128:
        assert (proba == 0.0).any(), "K=%d: no probability is exactly 0.0" % K
        assert sum(same_lane_tie(r, r == 0.0) for r in proba) >= 1, "K=%d: no two zero-probability classes in one lane" % K


def check_weighted(K, p, crow, special, plain_top1):
    """The same for the final probabilities `p` of one cost matrix / weight / renormalise setting: an all-zero cell (the +inf row:
    norm == 0, no top-1 above 0), a cell whose top-1 moved away from the unweighted one, ties that survive in the cells the costs
    leave alone (cost row -1 and the all-NaN row)."""
    zero = (p == 0.0).all(axis=1)
    assert zero.any() and zero[crow == special["inf"]].all(), "K=%d: no all-zero cell" % K
    moved = (np.argmax(p, axis=1) != plain_top1) & ~zero
    assert moved.any(), "K=%d: the costs move no top-1" % K
    alone = (crow == -1) | (crow == special["nan"])
    assert alone.any() and sum(has_tie(r[r > 0.0]) for r in p[alone]) >= 1, "K=%d: no tied probabilities after the weighting" % K
    assert tied_probability(p) is not None


def levenshtein_dp(a, b):
    """Levenshtein distance by the full (len(a) + 1) x (len(b) + 1) matrix in numpy, row by row:
    D[i][j] = min(D[i-1][j] + 1, D[i-1][j-1] + [a_i != b_j], D[i][j-1] + 1); the dependency on the left neighbour is a running
    minimum of D[i][j] - j.  A second opinion next to repair.costs.edit_distance."""
    s = np.array([ord(c) for c in a], np.int64)
    t = np.array([ord(c) for c in b], np.int64)
    j = np.arange(len(t) + 1, dtype=np.int32)
    D = np.zeros((len(s) + 1, len(t) + 1), np.int32)
    D[0] = j
    for i in range(1, len(s) + 1):
        best = np.minimum(D[i - 1, 1:] + 1, D[i - 1, :-1] + (t != s[i - 1]))
        D[i] = np.minimum.accumulate(np.concatenate(([i], best)).astype(np.int32) - j) + j
    return int(D[len(s), len(t)])
