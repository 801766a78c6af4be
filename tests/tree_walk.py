"""A plain tree walk over hand-built models: the reference of tests/test_tree_walk_cpu.py and tests/test_gpu_predictor_forms.py.

Python and numpy only; nothing here imports the product library.  Three parts:

* the blob writer: the byte format of `serialise_into` / `rgbm_model_load` (csrc/rgbm.hip), with the loader's rules asserted here as
  well (`check_model`), so that a model built by a test is one the product accepts;
* the tree builder: a tree is a nested spec -- a leaf is a float, an internal node is `(feat, theta, dleft, left, right)` -- of any
  shape (`shape`: left chain, right chain, random), grown so that every leaf can be reached (`grow`), with any leaf id at any in-order
  position;
* the walk: GBDT::PredictRaw as oracle/rgbm_oracle.c states it, and the output conversion in the expression order of `orc_predict`
  with the oracle's exponential (`orc_exp`), so that `predict` gives `OracleModel.predict`'s bits (test_tree_walk_cpu.py holds it to
  that on every model of the GPU list).
"""
import struct

import numpy as np

MAGIC = 0x4D424752
INT32_MAX = 2 ** 31 - 1
MISSING = 255


# ---------------------------------------------------------------------------------------------------------------- features
def feature(V, n_codes=None, has_nan=0, unseen=()):
    """A feature of V bins over n_codes codes (default: one bin per code).  Code c sits in bin min(c, V - 1): ub = 0, 1, ..., V - 2, INT32_MAX.
    `unseen`: codes no training row held (blob version 2): missing at prediction time."""
    n_codes = V if n_codes is None else n_codes
    assert 1 <= V <= 255 and n_codes >= 1
    ub = list(range(V - 1)) + [INT32_MAX]
    return dict(n_codes=int(n_codes), V=int(V), has_nan=int(has_nan), ub=ub, unseen=sorted(int(c) for c in unseen))


def features_of_size(F, S, **kw):
    """F features whose scoring tables hold exactly S mask entries: S = sum of (V + 1), the value bins and the missing entry."""
    base, rem = divmod(S, F)
    vs = [base - 1 + (1 if f < rem else 0) for f in range(F)]
    assert sum(v + 1 for v in vs) == S and min(vs) >= 1 and max(vs) <= 255, (F, S)
    return [feature(v, **kw) for v in vs]


def table_entries(feats):
    return sum(max(f["V"], 1) + 1 for f in feats)


def code_to_bin(ft, codes):
    """first b with ub[b] >= c; NULL, a code >= n_codes and an unseen code are bin 255"""
    codes = np.asarray(codes, np.int64)
    bins = np.searchsorted(np.asarray(ft["ub"], np.int64), codes, side="left")
    miss = (codes < 0) | (codes >= ft["n_codes"])
    if ft["unseen"]:
        miss |= np.isin(codes, ft["unseen"])
    return np.where(miss, MISSING, bins).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- trees
def shape(L, kind, rng=None):
    """A tree shape of exactly L leaves: None is a leaf, (left, right) an internal node.  kind: "left" / "right" = a chain of depth L - 1
    towards that side, "random" = a random split of the leaves at every node."""
    if L == 1:
        return None
    if kind == "left":
        return (shape(L - 1, kind), None)
    if kind == "right":
        return (None, shape(L - 1, kind))
    a = int(rng.integers(1, L))
    return (shape(a, kind, rng), shape(L - a, kind, rng))


def leaf_values(n, rng, lo=-38, hi=2):
    """random mantissas times 2^e, e over hi - lo + 1 >= 40 binades: any change in the order of a sum changes its bits"""
    assert hi - lo + 1 >= 40
    return np.ldexp(rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n), rng.integers(lo, hi + 1, n))


def grow(shp, feats, rng, values=None, dleft=None, use=None):
    """Fill a shape with splits so that EVERY leaf can be reached by in-dictionary codes: a node splits a feature whose bins, narrowed by
    the splits above it, still number two or more.  Returns (spec, boxes): boxes[p] = {feature: (lo, hi)}, the bins that lead to the
    p-th leaf from the left.  `use`: the features to split on (default all); `dleft`: 0 / 1 / None = random per node."""
    use = list(range(len(feats))) if use is None else list(use)
    n_leaves = [0]
    boxes = []

    def count(s):
        return 1 if s is None else count(s[0]) + count(s[1])

    def rec(s, box, L):
        if s is None:
            p = n_leaves[0]
            n_leaves[0] += 1
            boxes.append(dict(box))
            return float(values[p]) if values is not None else float(leaf_values(1, rng)[0])
        # a subtree of L leaves may be a chain of L - 1 splits, each of which takes a bin from the box: keep room for both sides
        span = {f: box.get(f, (0, feats[f]["V"] - 1)) for f in use}
        R = sum(hi - lo for lo, hi in span.values())
        assert R >= L - 1, "too few bins for a tree of this many leaves: give it more features or more bins"
        room = [f for f in use if span[f][1] > span[f][0]]
        f = int(room[int(rng.integers(len(room)))])
        lo, hi = span[f]
        a, w = count(s[0]), hi - lo
        x = int(rng.integers(max(0, a - 1 - R + w), min(w - 1, R - L + a) + 1))
        theta = lo + x                                       # lo <= theta <= hi - 1: both sides keep a bin
        d = int(rng.integers(2)) if dleft is None else int(dleft)
        lbox = dict(box); lbox[f] = (lo, theta)
        rbox = dict(box); rbox[f] = (theta + 1, hi)
        left = rec(s[0], lbox, a)
        right = rec(s[1], rbox, L - a)
        return (f, theta, d, left, right)

    return rec(shp, {}, count(shp)), boxes


def tree(spec, leaf_order=None, rng=None):
    """The arrays of a tree from its nested spec.  Internal nodes are numbered in pre-order (a child's index is greater than its
    parent's); the leaf at in-order position p gets id leaf_order[p] (default: p; "random": a random permutation), as a trained tree's
    leaf ids are in no particular order either.  t["pos"][leaf id] = its in-order position."""
    def count(s):
        return 1 if not isinstance(s, tuple) else count(s[3]) + count(s[4])

    L = count(spec)
    if leaf_order is None:
        leaf_order = list(range(L))
    elif isinstance(leaf_order, str):
        leaf_order = [int(x) for x in rng.permutation(L)]
    assert sorted(leaf_order) == list(range(L))
    n = L - 1
    t = dict(L=L, feat=np.zeros(n, np.int32), theta=np.zeros(n, np.int32), dleft=np.zeros(n, np.int32), left=np.zeros(n, np.int32),
             right=np.zeros(n, np.int32), gain=np.zeros(n, np.float64), leaf_value=np.zeros(L, np.float64), leaf_count=np.zeros(L, np.int32),
             pos=np.zeros(L, np.int32))
    nxt = [0, 0]          # next node index, next in-order leaf position

    def rec(s):
        if not isinstance(s, tuple):
            p = nxt[1]; nxt[1] += 1
            leaf = leaf_order[p]
            t["leaf_value"][leaf] = s
            t["leaf_count"][leaf] = 1 + p
            t["pos"][leaf] = p
            return ~leaf
        j = nxt[0]; nxt[0] += 1
        t["feat"][j], t["theta"][j], t["dleft"][j] = s[0], s[1], s[2]
        t["gain"][j] = 1.0 + j
        t["left"][j] = rec(s[3])
        t["right"][j] = rec(s[4])
        return j

    root = rec(spec)
    assert root == (0 if L > 1 else ~leaf_order[0])
    return t


def stump(value):
    return tree(float(value))


# ---------------------------------------------------------------------------------------------------------------- models and blobs
def model(objective, num_class, feats, trees, K=None):
    """trees in (iteration, class tree) order; K class trees per iteration (objective 1: num_class, else 1)"""
    K = (num_class if objective == 1 else 1) if K is None else K
    assert len(trees) % K == 0
    m = dict(objective=int(objective), num_class=int(num_class), K=int(K), n_iter=len(trees) // K, F=len(feats), feats=list(feats), trees=list(trees))
    check_model(m)
    return m


def check_model(m):
    """what rgbm_model_load enforces"""
    assert m["objective"] in (0, 1, 2) and m["num_class"] >= 1
    assert m["K"] == (m["num_class"] if m["objective"] == 1 else 1)
    assert m["objective"] != 0 or m["num_class"] == 2
    assert 0 <= m["F"] <= 65535 and len(m["trees"]) == m["K"] * m["n_iter"]
    for ft in m["feats"]:
        assert 0 < ft["V"] <= 255 and len(ft["ub"]) == ft["V"] and ft["ub"][-1] == INT32_MAX
        assert all(a < b for a, b in zip(ft["ub"], ft["ub"][1:]))
        assert all(0 <= c < ft["n_codes"] for c in ft["unseen"])
    for t in m["trees"]:
        L, n = t["L"], t["L"] - 1
        assert 1 <= L <= 32767
        refs = np.zeros(n + L, np.int64)                       # nodes, then leaves
        for j in range(n):
            assert 0 <= t["feat"][j] < m["F"] and -1 <= t["theta"][j] <= 254
            for ch in (int(t["left"][j]), int(t["right"][j])):
                if ch < 0:
                    assert ~ch < L                              # a leaf child is ~leaf
                    refs[n + ~ch] += 1
                else:
                    assert j < ch < n                           # an internal child's index is greater than its parent's
                    refs[ch] += 1
        if n:
            assert refs[0] == 0 and (refs[1:] == 1).all()       # every leaf and every node but the root: referenced exactly once


def blob(m):
    """the bytes of rgbm_model_save: version 2 (with every feature's unseen-category bitmap) when a feature has unseen codes, else 1"""
    check_model(m)
    ver = 2 if any(ft["unseen"] for ft in m["feats"]) else 1
    out = [struct.pack("<7i", MAGIC, ver, m["objective"], m["num_class"], m["K"], m["n_iter"], m["F"])]
    for ft in m["feats"]:
        out.append(struct.pack("<3i", ft["n_codes"], ft["V"], ft["has_nan"]))
        out.append(np.asarray(ft["ub"], "<i4").tobytes())
        if ver == 2:
            words = np.zeros((ft["n_codes"] + 31) // 32 if ft["unseen"] else 0, np.uint32)
            for c in ft["unseen"]:
                words[c >> 5] |= np.uint32(1 << (c & 31))
            out.append(struct.pack("<i", len(words)) + words.astype("<u4").tobytes())
    for t in m["trees"]:
        out.append(struct.pack("<i", t["L"]))
        for name in ("feat", "theta", "dleft", "left", "right"):
            out.append(np.asarray(t[name], "<i4").tobytes())
        out.append(np.asarray(t["gain"], "<f8").tobytes())
        out.append(np.asarray(t["leaf_value"], "<f8").tobytes())
        out.append(np.asarray(t["leaf_count"], "<i4").tobytes())
    return b"".join(out)


# ---------------------------------------------------------------------------------------------------------------- the walk
def bins_of(m, X):
    X = np.asarray(X)
    assert X.shape[0] == m["F"]
    return [code_to_bin(ft, X[f]) for f, ft in enumerate(m["feats"])]


def exit_leaves(t, bins, n):
    """leaf id every row leaves tree t at: bin 255 follows dleft, any other bin goes left when bin <= theta"""
    if t["L"] <= 1:
        return np.zeros(n, np.int64)
    node = np.zeros(n, np.int64)                                # >= 0: at that internal node; < 0: ~leaf
    feat, theta, dleft = t["feat"].astype(np.int64), t["theta"].astype(np.int64), t["dleft"]
    left, right = t["left"].astype(np.int64), t["right"].astype(np.int64)
    B = np.stack(bins) if len(bins) else np.zeros((0, n), np.int64)
    rows = np.arange(n)
    while True:
        live = node >= 0
        if not live.any():
            return ~node
        j = node[live]
        b = B[feat[j], rows[live]]
        go_left = np.where(b == MISSING, dleft[j] != 0, b <= theta[j])
        node[live] = np.where(go_left, left[j], right[j])


def raw_scores(m, X):
    """[n][K] float64: the leaf values added in iteration order"""
    X = np.asarray(X)
    n = X.shape[1]
    bins = bins_of(m, X)
    K = m["K"]
    raw = np.zeros((n, K), np.float64)
    for it in range(m["n_iter"]):
        for k in range(K):
            t = m["trees"][it * K + k]
            raw[:, k] = raw[:, k] + t["leaf_value"][exit_leaves(t, bins, n)]
    return raw


def exit_positions(m, X):
    """[trees][n]: the in-order position (0 = leftmost) of every row's exit leaf"""
    X = np.asarray(X)
    bins = bins_of(m, X)
    return np.stack([t["pos"][exit_leaves(t, bins, X.shape[1])] for t in m["trees"]])


_exp = None


def oracle_exp(x):
    """the oracle's exponential (rg_exp), elementwise"""
    global _exp
    if _exp is None:
        from oracle import oracle as O
        _exp = O.lib().orc_exp
    x = np.asarray(x, np.float64)
    u, inv = np.unique(x, return_inverse=True)
    return np.array([_exp(float(v)) for v in u], np.float64)[inv].reshape(x.shape)


def convert(m, raw):
    """orc_predict's output conversion, in its expression order: [n][ncol]"""
    if m["objective"] == 2:
        return raw[:, :1].copy()
    if m["objective"] == 0:
        pr = 1.0 / (1.0 + oracle_exp(-raw[:, 0]))
        return np.stack([1.0 - pr, pr], axis=1)
    wmax = raw[:, 0].copy()
    for k in range(1, m["K"]):
        wmax = np.where(raw[:, k] > wmax, raw[:, k], wmax)
    e = oracle_exp(raw - wmax[:, None])
    wsum = np.zeros(len(raw), np.float64)
    for k in range(m["K"]):
        wsum = wsum + e[:, k]
    return e / wsum[:, None]


def predict(m, X):
    return convert(m, raw_scores(m, X))


def label_top(m, proba):
    """the chain's label (first maximum; -1 for a regression target) and its probability (the raw value for a regression target)"""
    if m["objective"] == 2:
        return np.full(len(proba), -1, np.int32), proba[:, 0].copy()
    lab = np.argmax(proba, axis=1).astype(np.int32)            # numpy: the first maximum
    return lab, proba[np.arange(len(proba)), lab]


def repair_chain(models, target_col, feat_cols, class_codes, table):
    """RepairModel._repair's chain on a [C][n] table, in place: model t scores every row from its feature columns, then only the NULL
    cells of its target column take class_codes[t][label] (a label beyond that list leaves the cell NULL)."""
    n = table.shape[1]
    labs, tops = np.zeros((len(models), n), np.int32), np.zeros((len(models), n), np.float64)
    for t, m in enumerate(models):
        labs[t], tops[t] = label_top(m, predict(m, table[list(feat_cols[t])]))
        if m["objective"] == 2:
            continue
        cc = np.asarray(class_codes[t], np.int32)
        fill = (table[target_col[t]] < 0) & (labs[t] < len(cc))
        table[target_col[t]][fill] = cc[labs[t][fill]]
    return labs, tops


# ---------------------------------------------------------------------------------------------------------------- probe rows
def codes_in_bin(ft, b):
    """the in-dictionary, seen codes of bin b"""
    lo = 0 if b == 0 else ft["ub"][b - 1] + 1
    hi = min(ft["ub"][b], ft["n_codes"] - 1)
    return [c for c in range(lo, hi + 1) if c not in ft["unseen"]]


def row_for_box(m, box, rng):
    """a row of codes inside a leaf's box (see grow); the features the box leaves free take a random code"""
    row = np.zeros(m["F"], np.int32)
    for f, ft in enumerate(m["feats"]):
        lo, hi = box.get(f, (0, ft["V"] - 1))
        cand = [c for b in range(lo, hi + 1) for c in codes_in_bin(ft, b)]
        row[f] = cand[int(rng.integers(len(cand)))]
    return row


def probe_rows(m, n, rng, boxes=()):
    """[F][n] codes.  First the rows aimed at `boxes`; then, around one base row and changing ONE feature at a time, every feature's
    bin 0, its last bin, theta and theta + 1 of (some of) the nodes that split it, a NULL, the codes n_codes and n_codes + 3 and an
    unseen category; the rest random with NULLs and out-of-dictionary codes sprinkled in."""
    F = m["F"]
    rows = [row_for_box(m, b, rng) for b in boxes]
    base = np.array([int(rng.integers(ft["n_codes"])) for ft in m["feats"]], np.int32)
    rows.append(base.copy())
    thetas = [set() for _ in range(F)]
    for t in m["trees"]:
        for f, th in zip(t["feat"], t["theta"]):
            thetas[int(f)].add(int(th))
    for f, ft in enumerate(m["feats"]):
        vals = [0, ft["n_codes"] - 1, -1, ft["n_codes"], ft["n_codes"] + 3] + ft["unseen"][:1]
        V = ft["V"]
        vals += [c for c in range(max(V - 1, 0), min(V + 1, ft["n_codes"]))]        # the last bin's first codes
        th = sorted(thetas[f])
        for x in (th[:1] + th[-1:] + ([th[len(th) // 2]] if th else [])):
            vals += [c for c in (x, x + 1) if 0 <= c < ft["n_codes"]]                 # code c sits in bin min(c, V - 1)
        for v in dict.fromkeys(vals):
            r = base.copy(); r[f] = v
            rows.append(r)
    rows = rows[:n]
    X = np.stack(rows, axis=1).astype(np.int32) if rows else np.zeros((F, 0), np.int32)
    k = n - X.shape[1]
    R = np.stack([rng.integers(0, ft["n_codes"], k) for ft in m["feats"]]).astype(np.int32) if F else np.zeros((0, k), np.int32)
    u = rng.random(R.shape)
    R[u < 0.05] = -1
    over = (u >= 0.05) & (u < 0.08)
    R[over] = (np.array([ft["n_codes"] for ft in m["feats"]], np.int32)[:, None] + rng.integers(0, 4, R.shape).astype(np.int32))[over]
    return np.ascontiguousarray(np.concatenate([X, R], axis=1))
