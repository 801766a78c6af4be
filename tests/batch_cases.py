"""The tables and fit specs of tests/test_gpu_batch_edges.py (the batched small-table trainer, csrc/rgbm_small.h), importable without a device:
seeded numpy only.  tests/test_batch_cases_cpu.py holds every generator to its purpose on the CPU oracle, so that a device test cannot
pass on a table that misses the edge it names.

A `Tab` is a code table ([C][N] int32, NULL = -1) or a row gather of one (`parent`, `rows`); a `Fit` is one entry of a batch: the table,
target, features, the training arguments, optionally a validation table -- and `route`, the entry of rgbm_table_train_batch_report the
fit is built for.  `oracle_model` trains the CPU oracle on the fit's training rows; `expected_report` restates, from the bins of the
oracle's model, what the report must say (route, waves of the packed scan, 16-feature chunks, LDS bytes).
"""
import struct

import numpy as np

SM_WAVES = 8            # csrc/rgbm_small.h: 512 threads
SMALL_ROWS = 65536      # RGBM_SMALL_ROWS default: the largest TABLE (rows, not training rows) the fused kernels take
SM_MAX_LEAVES, SM_MAX_FEATS = 256, 255
SIZEOF_LEAF, SIZEOF_CAND, SIZEOF_HISTBIN = 96, 48, 16
ROUTE_NONE, ROUTE_FUSED, ROUTE_NOT_ELIGIBLE, ROUTE_ALONE, ROUTE_LDS = 0, 1, 2, 3, 4
BASE = dict(n_estimators=3, learning_rate=0.3)


# ---------------------------------------------------------------------------------------------------------------------------------
# restatements of the host rules of the batched trainer
# ---------------------------------------------------------------------------------------------------------------------------------
def lane_waves(V):
    """scan_lane_map's rule (csrc/rgbm_small.h): a lane of the packed threshold scan owns 4 value bins of ONE feature (a feature without
    value bins still takes a lane); the features take lanes in order; a feature that does not fit the rest of its 64-lane wave starts
    the next wave.  V: value bins per feature (without the NaN bin).  Returns the waves one child needs."""
    lanes = 0
    for v in V:
        need = max(1, (int(v) + 3) // 4)
        if lanes % 64 + need > 64:
            lanes += 64 - lanes % 64
        lanes += need
    return (lanes + 63) // 64


def lds_layout(bins, num_leaves):
    """(totbins, nchunk, lds_hist) of fit_setup (csrc/rgbm.hip): a feature has max(V + has_nan, 1) bins; the histogram of a 16-feature
    chunk keeps 2^sh replicas of every bin, sh the largest shift <= 5 with bins << sh <= 256, 16 bytes each; lds_hist = the largest chunk."""
    nb = [max(v + nan, 1) for v, nan in bins]
    lds_hist = 0
    for ch in range(0, len(nb), 16):
        slots = 0
        for b in nb[ch:ch + 16]:
            sh = 0
            while sh < 5 and (b << (sh + 1)) <= 256:
                sh += 1
            slots += b << sh
        lds_hist = max(lds_hist, slots * 16)
    return sum(nb), (len(nb) + 15) // 16, lds_hist


def sm_lds_bytes(lds_hist, num_leaves, F, packed_totbins=0):
    """sm_lds_bytes (csrc/rgbm_small.h): histogram area (at least num_leaves doubles), leaves, two candidate rows, the two compact child
    histograms of the packed scan, 64 spare bytes; every part rounded up to 16."""
    r16 = lambda x: (x + 15) & ~15
    b = r16(max(lds_hist, num_leaves * 8))
    b = r16(b + num_leaves * SIZEOF_LEAF)
    b = r16(b + 2 * F * SIZEOF_CAND)
    return b + 2 * packed_totbins * SIZEOF_HISTBIN + 64


def blob_bins(blob):
    """[(V, has_nan)] per feature out of a serialised model (the header of rgbm_model_save / orc_model_save)"""
    ver, F = struct.unpack_from("7i", blob, 0)[1], struct.unpack_from("7i", blob, 0)[6]
    p, out = 28, []
    for _ in range(F):
        _, V, nan = struct.unpack_from("3i", blob, p); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
        out.append((V, nan))
    return out


def blob_upper_bounds(blob, feature):
    """the upper code of every value bin of one feature"""
    ver = struct.unpack_from("7i", blob, 0)[1]
    p = 28
    for f in range(feature + 1):
        _, V, _ = struct.unpack_from("3i", blob, p)
        ub = np.frombuffer(blob, np.int32, V, p + 12); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
    return ub


def tree_leaves(blob):
    """leaves of every tree, [iteration][class tree]"""
    hdr = struct.unpack_from("7i", blob, 0)
    ver, K, n_iter, F = hdr[1], hdr[4], hdr[5], hdr[6]
    p = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("3i", blob, p); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
    L = []
    for _ in range(K * n_iter):
        l, = struct.unpack_from("i", blob, p)
        p += 4 + (l - 1) * (5 * 4 + 8) + l * 12
        L.append(l)
    return np.asarray(L, np.int64).reshape(n_iter, K)


def tree_features(blob):
    """the split features of all trees, concatenated"""
    hdr = struct.unpack_from("7i", blob, 0)
    ver, K, n_iter, F = hdr[1], hdr[4], hdr[5], hdr[6]
    p = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("3i", blob, p); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
    out = []
    for _ in range(K * n_iter):
        l, = struct.unpack_from("i", blob, p)
        out.append(np.frombuffer(blob, np.int32, l - 1, p + 4))
        p += 4 + (l - 1) * (5 * 4 + 8) + l * 12
    return np.concatenate(out) if out else np.zeros(0, np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# tables and fits
# ---------------------------------------------------------------------------------------------------------------------------------
class Tab:
    def __init__(self, codes=None, cards=None, parent=None, rows=None, values=None, kinds=()):
        self.parent, self.rows = parent, None if rows is None else np.ascontiguousarray(rows, np.int64)
        if parent is not None:
            codes, cards, values, kinds = np.ascontiguousarray(parent.codes[:, self.rows]), parent.cards, parent.values, parent.kinds
        self.codes = np.ascontiguousarray(codes, np.int32)
        self.cards = np.ascontiguousarray(cards, np.int32)
        self.values = dict(values or {})          # column -> ascending values behind its codes (Table.set_column_values)
        self.kinds = tuple(kinds)                 # categorical columns (Table.set_column_kind)

    @property
    def n(self):
        return self.codes.shape[1]


class Fit:
    def __init__(self, name, tab, target, feats, K, route=ROUTE_FUSED, y_value=None, class_weight=None, valid=None, fails=False, **params):
        self.name, self.tab, self.target, self.feats, self.K = name, tab, int(target), [int(f) for f in feats], K      # K = 0: regression
        self.route, self.y_value, self.class_weight, self.valid, self.fails = route, y_value, class_weight, valid, fails
        self.params = dict(BASE, objective=2 if K == 0 else (0 if K == 2 else 1), num_class=max(K, 2), **params)
        self._oracle = None

    def train_rows(self):
        return self.tab.codes[self.target] >= 0

    def spec(self, table, valid_table=None, **extra):
        """the dict repair._native.train_batch takes, on device tables"""
        d = dict(table=table, target_col=self.target, feat_cols=self.feats, y_value=self.y_value, class_weight=self.class_weight, **self.params)
        if valid_table is not None:
            d["valid_table"] = valid_table
        d.update(extra)
        return d


def eligible(fit):
    """small_fit_eligible (csrc/rgbm.hip) for the fits of this module (no multiplicities, not row-sharded)"""
    return fit.tab.n <= SMALL_ROWS and fit.params.get("num_leaves", 31) <= SM_MAX_LEAVES and len(fit.feats) <= SM_MAX_FEATS


def oracle_model(fit):
    """the CPU oracle's model of the fit's training rows (cached on the fit); None for a fit that must fail"""
    from oracle import oracle as O
    if fit.fails:
        return None
    if fit._oracle is None:
        t = fit.tab
        rows = fit.train_rows()
        fv = {j: t.values[c] for j, c in enumerate(fit.feats) if c in t.values}
        cat = [j for j, c in enumerate(fit.feats) if c in t.kinds]
        fit._oracle = O.train(np.ascontiguousarray(t.codes[fit.feats][:, rows]), t.cards[fit.feats], t.codes[fit.target][rows], int(t.cards[fit.target]),
                              y_value=fit.y_value, class_weight=fit.class_weight, feature_values=fv or None, categorical=cat or None, **fit.params)
    return fit._oracle


def oracle_valid(fit):
    """(labels, values) the oracle's model gives the rows of the fit's validation table: arg-max class and its probability; regression: -1 and the value"""
    from oracle import oracle as O
    m, v = oracle_model(fit), fit.valid
    t = v.codes.copy()
    cc = [] if fit.K == 0 else list(range(int(fit.tab.cards[fit.target])))
    lab, val = O.repair_chain([m], [fit.target], [fit.feats], [cc], t)
    return lab[0], val[0]


def expected_report(fit, packed=True, alone=False):
    """the row of rgbm_table_train_batch_report this fit must get: `packed` False under RGBM_SMALL_PACKED=0, `alone` when it is the only
    eligible fit of its batch.  The bins are those of the ORACLE's model."""
    zero = dict(scan_waves=0, nchunk=0, lds_bytes=0)
    if not eligible(fit):
        return dict(route=ROUTE_NOT_ELIGIBLE, **zero)
    if alone:
        return dict(route=ROUTE_ALONE, **zero)
    if fit.fails:
        return dict(route=ROUTE_NONE, **zero)
    bins = blob_bins(oracle_model(fit).save())
    NL, F = fit.params.get("num_leaves", 31), len(fit.feats)
    totbins, nchunk, lds_hist = lds_layout(bins, NL)
    Wn = lane_waves([v for v, _ in bins])
    W = Wn if (packed and 2 * Wn <= SM_WAVES and totbins <= 2048 and sm_lds_bytes(lds_hist, NL, F, totbins) <= 150 * 1024) else 0
    return dict(route=ROUTE_FUSED, scan_waves=W, nchunk=nchunk, lds_bytes=sm_lds_bytes(lds_hist, NL, F, totbins if W else 0))


def _nulls(col, rng, ratio, first=0):
    col = col.copy()
    m = rng.random(col.shape[0]) < ratio
    m[:first] = False
    col[m] = -1
    return col


def signal_table(seed, n, cards, K, null_cols=(), null_targets=0, every_code=0, noise=0.25):
    """[F + 1][n + null_targets] codes, the target last: a latent z drives the label and, through a per-column affine map, every feature; `noise` of
    the cells are uniform.  every_code = k: the first k * card rows of a column walk its codes, so that each holds at least k training rows (its own bin
    from k = min_data_in_bin on).  null_cols: 5 % NULL cells (after those rows).  null_targets: further rows with a NULL target."""
    rng = np.random.default_rng(seed)
    cards = np.asarray(cards, np.int32)
    N = n + null_targets
    z = rng.integers(0, 254, N)
    if K == 0:
        y = z.copy()
    else:
        y = (((z // 9 if K < 28 else z) + rng.integers(0, 2, N)) % K).astype(np.int32)
    X = np.empty((len(cards) + 1, N), np.int32)
    for j, c in enumerate(cards):
        c = int(c)
        sig = (z * (2 * (j % 5) + 1) + (y if K else 0) * (j % 3)) % c
        X[j] = np.where(rng.random(N) >= noise, sig, rng.integers(0, c, N))
        if every_code:
            X[j, :every_code * c] = np.tile(np.arange(c), every_code)[:N]
        if j in null_cols:
            X[j] = _nulls(X[j], rng, 0.05, first=every_code * c)
    X[-1] = y
    if null_targets:
        X[-1, n:] = -1
    return np.ascontiguousarray(X), np.append(cards, max(K, 1) if K else 254).astype(np.int32)


def _fit(name, codes, cards, K, **kw):
    F = codes.shape[0] - 1
    return Fit(name, Tab(codes, cards), F, range(F), K, **kw)


# ---- scan routes --------------------------------------------------------------------------------------------------------------------
def scan_route_fits():
    """name -> (fit, waves per child the table is built for, chunks).  About 6 000 rows, K = 3 (the two imported tables: 20 000 rows, K = 3 and 4)."""
    from tests.test_gpu_level_step import two_chunks, wide_narrow
    out = {}

    def add(name, fit, Wn, nchunk):
        out[name] = (fit, Wn, nchunk)

    add("four 254-bin features", _fit("four 254-bin features", *signal_table(2101, 6000, [254] * 4, 3, every_code=4), K=3), 4, 1)
    add("five 254-bin features", _fit("five 254-bin features", *signal_table(2102, 6000, [254] * 5, 3, every_code=4), K=3), 5, 1)
    add("sixteen 61..64-bin features", _fit("sixteen 61..64-bin features", *signal_table(2103, 6000, [61, 62, 63, 64] * 4, 3, every_code=4), K=3), 4, 1)
    add("seventeen 61..64-bin features", _fit("seventeen 61..64-bin features", *signal_table(2104, 6000, [61, 62, 63, 64] * 4 + [61], 3, every_code=4), K=3), 5, 2)
    for name, gen, Wn, nchunk in (("wide+narrow", wide_narrow, 3, 1), ("two chunks", two_chunks, 2, 2)):
        X, cards, y, K = gen()
        add(name, _fit(name, np.concatenate([X, y[None, :]], axis=0), np.append(cards, K), K), Wn, nchunk)
    # feature 0 at the largest bin counts max_bin <= 255 allows: 254 value bins; 253 value bins + the NaN bin (the last of the 64 lanes that sum the root's
    # totals from feature 0 holds bins 252 and 253 and must leave out 254 and 255)
    add("feature 0: 254 value bins", _fit("feature 0: 254 value bins", *signal_table(2105, 6000, [254, 5, 3, 9], 3, every_code=4), K=3), 2, 1)
    add("feature 0: 253 value bins + NaN", _fit("feature 0: 253 value bins + NaN", *signal_table(2106, 6000, [253, 5, 3, 9], 3, every_code=4, null_cols=(0, 2)), K=3), 2, 1)
    c, cards = signal_table(2107, 6000, [6, 40, 3, 9], 3)
    c[0] = 4
    add("feature 0 constant", _fit("feature 0 constant", c, cards, K=3), 1, 1)
    c, cards = signal_table(2108, 6000, [6, 40, 3, 9], 3, null_cols=(1,))
    c[0] = -1
    add("feature 0 all NULL", _fit("feature 0 all NULL", c, cards, K=3), 1, 1)
    return out


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = [1, 2, 39, 40, 41, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4097, 16383, 16384, 16385]


def row_fits():
    """F = 4, K = 3 fits (and one binary) with n_train at the workgroup, partition-tile and grid-stride edges, 36 NULL-target rows in every table (N != n_train);
    n_train 39 / 40 / 41 with min_data_in_leaf 20 (the root is searched from 40 rows on); then the eligibility edge, which is about the TABLE's rows:
    n_train 65 535 in a table of 65 536 rows (one NULL target: the fused kernels' largest table), 65 536 rows with 36 NULL targets, and 65 537 rows (not eligible)."""
    fits = []
    for i, n in enumerate(ROW_COUNTS):
        kw = dict(min_data_in_leaf=20) if n <= 65 else dict()
        fits.append(_fit("n_train %d" % n, *signal_table(2200 + i, n, [5, 3, 7, 4], 3, null_cols=(1,), null_targets=36), K=3, **kw))
    fits.append(_fit("n_train 2049, binary", *signal_table(2230, 2049, [5, 3, 7, 4], 2, null_cols=(1,), null_targets=36), K=2))
    fits.append(_fit("n_train 65535 of 65536 rows", *signal_table(2231, 65535, [5, 3, 7, 4], 3, null_cols=(1,), null_targets=1), K=3))
    fits.append(_fit("65536 rows", *signal_table(2232, 65500, [5, 3, 7, 4], 3, null_cols=(1,), null_targets=36), K=3))
    fits.append(_fit("65537 rows", *signal_table(2233, 65501, [5, 3, 7, 4], 3, null_cols=(1,), null_targets=36), K=3, route=ROUTE_NOT_ELIGIBLE))
    return fits


# ---- budgets ------------------------------------------------------------------------------------------------------------------------
def leaf_budget_fits():
    """num_leaves 2, 255, 256 (fused) and 257 (single-fit trainer) on one table whose trees reach them: max_depth -1, min_data_in_leaf 1;
    max_depth 1 on the same table.  -> [(fit, leaves every oracle tree must have, or None)]"""
    codes, cards = signal_table(2301, 5000, [40, 37, 29, 23, 31], 3, null_cols=(2,), null_targets=30, noise=0.4)
    tab = Tab(codes, cards)
    out = []
    for nl in (2, 255, 256, 257):
        out.append((Fit("num_leaves %d" % nl, tab, 5, range(5), 3, route=ROUTE_FUSED if nl <= 256 else ROUTE_NOT_ELIGIBLE,
                        num_leaves=nl, max_depth=-1, min_data_in_leaf=1, n_estimators=2), nl))
    out.append((Fit("max_depth 1", tab, 5, range(5), 3, max_depth=1), 2))
    return out


FEATURE_COUNTS = [1, 16, 17, 33, 255, 256]


def feature_count_fits():
    """F two-code features, 3 000 rows, K = 3; F = 256 is not eligible"""
    fits = []
    for i, F in enumerate(FEATURE_COUNTS):
        codes, cards = signal_table(2320 + i, 3000, [2] * F, 3, null_targets=20, noise=0.35)
        fits.append(_fit("F = %d" % F, codes, cards, K=3, route=ROUTE_FUSED if F <= 255 else ROUTE_NOT_ELIGIBLE, num_leaves=8))
    return fits


# ---- class counts -------------------------------------------------------------------------------------------------------------------
def class_count_fits():
    """binary, K = 3, 64, 113, 219 (K = 3 and 113 with balanced class weights) and a regression fit with ~3 000 distinct targets under max_bin 15, in one batch"""
    fits = []
    for i, K in enumerate((2, 3, 64, 113, 219)):
        rng = np.random.default_rng(2400 + i)
        n = 4000
        y = rng.integers(0, K, n).astype(np.int32)
        y[:K] = np.arange(K)
        cards = [12, 7, 30, 5]
        X = np.stack([np.where(rng.random(n) < 0.7, (y * (j + 1) + j) % c, rng.integers(0, c, n)) for j, c in enumerate(cards)] + [y]).astype(np.int32)
        X[1] = _nulls(X[1], rng, 0.05)
        X[4, -25:] = -1
        cnt = np.bincount(y[:-25], minlength=K)
        cw = (n - 25) / (K * np.maximum(cnt, 1)) if K in (3, 113) else None          # balanced class weights on two of the fits
        fits.append(_fit("K = %d" % K, X, cards + [K], K=K, class_weight=cw, num_leaves=7, n_estimators=2))
    rng = np.random.default_rng(2410)
    n = 4000
    cards = [60, 9, 200, 5]
    z = rng.integers(0, 3000, n)
    z[:3000] = np.arange(3000)
    X = np.stack([np.where(rng.random(n) < 0.8, (z // (3000 // c + 1)) % c, rng.integers(0, c, n)) for c in cards] + [z]).astype(np.int32)
    X[2] = _nulls(X[2], rng, 0.05)
    X[4, -25:] = -1
    yv = np.cumsum(rng.random(3000) + 0.01) * 0.37 - 100.0
    fits.append(_fit("regression, 3000 targets, max_bin 15", X, cards + [3000], K=0, y_value=yv, max_bin=15))
    return fits


# ---- bagging ------------------------------------------------------------------------------------------------------------------------
def bagging_fits():
    """7 iterations.  bagging_freq 1 and 3, bagging_fraction 0.05 and 0.95, n_train 1023 / 1024 / 1025 / 2049 (one LCG per 1024 training-row positions:
    1, 1, 2 and 3 blocks), NULL targets everywhere; a fit that does not bag and one drawing one feature per tree (feature_fraction 0.01) between them;
    a 6 000-row fit (6 blocks) as the neighbour with more blocks."""
    fits = []
    spec = [(1023, 1, 0.95), (1024, 3, 0.05), (1025, 1, 0.05), (2049, 3, 0.95), (1024, 1, 0.5)]
    for i, (n, freq, frac) in enumerate(spec):
        codes, cards = signal_table(2500 + i, n, [9, 4, 30, 6, 3], 3, null_cols=(0,), null_targets=40)
        fits.append(_fit("n_train %d, freq %d, fraction %.2f" % (n, freq, frac), codes, cards, K=3, n_estimators=7, bagging_freq=freq, bagging_fraction=frac,
                         min_data_in_leaf=3))
    codes, cards = signal_table(2510, 3000, [9, 4, 30, 6, 3], 3, null_targets=40)
    fits.insert(2, _fit("no bagging", codes, cards, K=3, n_estimators=7))
    codes, cards = signal_table(2511, 6000, [9, 4, 30, 6, 3], 2, null_targets=40)
    fits.insert(4, _fit("n_train 6000, binary, freq 2, fraction 0.70", codes, cards, K=2, n_estimators=7, bagging_freq=2, bagging_fraction=0.7))
    codes, cards = signal_table(2512, 2500, [9, 4, 30, 6, 3], 3, null_targets=40)
    fits.append(_fit("feature_fraction 0.01, freq 1, fraction 0.60", codes, cards, K=3, n_estimators=7, bagging_freq=1, bagging_fraction=0.6, feature_fraction=0.01))
    return fits


def bag_sizes(fit):
    """rows in the bag, [iteration][class tree], read off the oracle's model: the root of a tree holds the bag of its iteration, so the tree's leaf
    counts sum to the bag's size"""
    blob = oracle_model(fit).save()
    hdr = struct.unpack_from("7i", blob, 0)
    ver, K, n_iter, F = hdr[1], hdr[4], hdr[5], hdr[6]
    p = 28
    for _ in range(F):
        _, V, _ = struct.unpack_from("3i", blob, p); p += 12 + 4 * V
        if ver == 2:
            nw, = struct.unpack_from("i", blob, p); p += 4 + 4 * nw
    sizes = []
    for _ in range(K * n_iter):
        l, = struct.unpack_from("i", blob, p)
        p += 4 + (l - 1) * (5 * 4 + 8) + l * 8
        sizes.append(int(np.frombuffer(blob, np.int32, l, p).sum()))
        p += 4 * l
    return np.asarray(sizes).reshape(n_iter, K)


# ---- composition --------------------------------------------------------------------------------------------------------------------
FREEZE_SEEDS = (1, 5, 8, 17, 46)


def freeze_fits():
    """One informative feature among noise, min_gain_to_split high enough that noise never splits, two of six features per tree: a fit stops at the
    first iteration whose trees draw no informative feature (tests/test_gpu_batch.py) -- seeds that stop after 0, 1, 2 and 3 iterations -- next to a fit
    without those limits that runs all its iterations; validation rows every fourth row."""
    rng = np.random.default_rng(5)
    n = 6000
    codes = np.empty((7, n), np.int32)
    codes[1] = rng.integers(0, 4, n)
    codes[0] = ((codes[1] >= 2) ^ (rng.random(n) < 0.1)).astype(np.int32)
    for c in range(2, 7):
        codes[c] = rng.integers(0, 5, n)
    cards = np.asarray([2, 4, 5, 5, 5, 5, 5], np.int32)
    parent = Tab(codes, cards)
    va = np.arange(0, n, 4)
    tr = np.setdiff1d(np.arange(n), va)
    ttab, vtab = Tab(parent=parent, rows=tr), Tab(parent=parent, rows=va)
    fits = [Fit("freeze, seed %d" % sd, ttab, 0, range(1, 7), 2, valid=vtab, n_estimators=9, feature_fraction=0.34, min_gain_to_split=25.0,
                min_data_in_leaf=50, seed=sd) for sd in FREEZE_SEEDS]
    fits.insert(2, Fit("runs all 9 iterations", ttab, 0, range(1, 7), 2, valid=vtab, n_estimators=9, min_data_in_leaf=50))
    return fits


def composition_fits():
    """n_estimators 1, 4 and 9 together, a fit whose target is all NULL in the middle (fails alone), a tiny F = 1 fit and the Wn = 4 fit"""
    fits = []
    for i, ne in enumerate((1, 4, 9)):
        codes, cards = signal_table(2600 + i, 3000 + 500 * i, [9, 4, 30, 6], 3, null_cols=(2,), null_targets=30)
        fits.append(_fit("n_estimators %d" % ne, codes, cards, K=3, n_estimators=ne))
    codes, cards = signal_table(2610, 2000, [9, 4], 3)
    codes[2] = -1
    fits.insert(2, _fit("no training rows", codes, cards, K=3, fails=True, route=ROUTE_NONE))
    codes, cards = signal_table(2611, 300, [3], 3, null_targets=5)
    fits.append(_fit("tiny, F = 1", codes, cards, K=3, min_data_in_leaf=5))
    fits.append(scan_route_fits()["four 254-bin features"][0])
    return fits


def dummy_fit():
    codes, cards = signal_table(2620, 700, [4, 4], 2)
    return _fit("dummy", codes, cards, K=2, n_estimators=1)


# ---- per-fit bins -------------------------------------------------------------------------------------------------------------------
RARE_CODE = 17


def fold_fits():
    """Two folds gathered from one table.  Code 17 of column 0 sits in 4 rows, all of them even: the fold of the even rows holds 4 of them (its own bin under
    min_data_in_bin 3), the fold of rows 0 mod 3 != 0 holds 2 (merged with code 18's bin).  Column 1 is numeric (set_column_values on the parent: uneven
    gaps move the bin bounds' midpoints), column 2 categorical (set_column_kind)."""
    codes, cards = signal_table(2701, 6000, [30, 12, 8, 5], 3, null_cols=(3,), null_targets=30)
    c0 = codes[0]
    c0[c0 == RARE_CODE] = RARE_CODE + 1
    c0[[0, 6, 12, 20]] = RARE_CODE          # even rows; rows 0, 6, 12 are 0 mod 3
    vals = np.cumsum(np.asarray([1, 1, 7, 1, 30, 2, 2, 11, 1, 1, 5, 3], np.float64))
    parent = Tab(codes, cards, values={1: vals}, kinds=(2,))
    N = parent.n
    even = np.flatnonzero(np.arange(N) % 2 == 0)
    not3 = np.flatnonzero(np.arange(N) % 3 != 0)
    return [Fit("fold of the even rows", Tab(parent=parent, rows=even), 4, range(4), 3, min_data_in_leaf=5),
            Fit("fold of the rows != 0 mod 3", Tab(parent=parent, rows=not3), 4, range(4), 3, min_data_in_leaf=5)]


def zipf_fit():
    """a 1 000-code column with Zipf frequencies under max_bin 63 (greedy_find_bin's second branch: more distinct codes than bins), next to small columns"""
    rng = np.random.default_rng(2710)
    n = 8000
    w = 1.0 / np.arange(1, 1001)
    z = rng.choice(1000, n, p=w / w.sum())
    perm = rng.permutation(1000)
    y = ((perm[z] // 37 + rng.integers(0, 2, n)) % 3).astype(np.int32)
    X = np.stack([perm[z], rng.integers(0, 6, n), (y + rng.integers(0, 2, n)) % 4, y]).astype(np.int32)
    X[0] = _nulls(X[0], rng, 0.03)
    X[3, -30:] = -1
    return _fit("zipf, 1000 codes, max_bin 63", X, [1000, 6, 4, 3], K=3, max_bin=63)


# ---- validation scores --------------------------------------------------------------------------------------------------------------
VALID_ROWS = [1, 255, 256, 257, 16385]


def _valid_pair(seed, n, nv, cards, K, **kw):
    codes, cards2 = signal_table(seed, n + nv, cards, K, null_cols=(1,), noise=0.3)
    parent = Tab(codes, cards2)
    rng = np.random.default_rng(seed + 1)
    perm = rng.permutation(n + nv)
    return Tab(parent=parent, rows=np.sort(perm[:n])), Tab(parent=parent, rows=np.sort(perm[n:]))


def valid_fits():
    """n_valid 1, 255, 256, 257 and 16 385 (the last: larger than its 3 000-row training table, past 64 tiles of 256 rows), K = 64, a regression fit, fits
    without validation rows between them, one fit with want_model=False"""
    fits = []
    for i, nv in enumerate(VALID_ROWS):
        ttab, vtab = _valid_pair(2800 + 2 * i, 3000, nv, [9, 4, 30, 6], 3)
        fits.append(Fit("n_valid %d" % nv, ttab, 4, range(4), 3, valid=vtab))
        if i in (1, 3):
            codes, cards = signal_table(2820 + i, 1500, [9, 4], 2, null_targets=10)
            fits.append(_fit("no validation rows (%d)" % i, codes, cards, K=2))
    ttab, vtab = _valid_pair(2830, 4000, 700, [12, 7, 30, 5], 64)
    fits.append(Fit("K = 64, n_valid 700", ttab, 4, range(4), 64, valid=vtab, num_leaves=7, n_estimators=2))
    rng = np.random.default_rng(2840)
    n = 3600
    x = np.stack([rng.integers(0, 20, n), rng.integers(0, 5, n), rng.integers(0, 40, n)])
    y = np.clip(x[0] + 3 * x[1] + rng.integers(0, 4, n), 0, 49)
    parent = Tab(np.concatenate([x, y[None]]).astype(np.int32), [20, 5, 40, 50])
    fits.append(Fit("regression, n_valid 600", Tab(parent=parent, rows=np.arange(3000)), 3, range(3), 0, y_value=np.arange(50) * 0.37, valid=Tab(parent=parent, rows=np.arange(3000, n))))
    return fits


def valid_two_chunk_fit():
    """twenty features; the label follows features 17 and 19 (the second 16-byte record of a row) -- and feature 3, so that both records are read"""
    rng = np.random.default_rng(2850)
    n, nv = 4000, 900
    X = rng.integers(0, 4, (20, n + nv)).astype(np.int32)
    y = ((X[17] + 2 * X[19] + (X[3] >= 2) + (rng.random(n + nv) < 0.1)) % 3).astype(np.int32)
    X[18] = _nulls(X[18], rng, 0.05)
    X[17] = _nulls(X[17], rng, 0.03)
    parent = Tab(np.concatenate([X, y[None]]), [4] * 20 + [3])
    return Fit("two chunks, n_valid 900", Tab(parent=parent, rows=np.arange(n)), 20, range(20), 3, valid=Tab(parent=parent, rows=np.arange(n, n + nv)))


UNSEEN_CODE, OUT_OF_DICT = 7, 8


def valid_categorical_fit():
    """Column 0 is categorical with 8 codes; code 7 occurs in validation rows only (missing for the model); validation row 5 holds code 8, outside the
    dictionary of the training table, and the validation rows hold NULLs in columns 0 and 1.  Training and validation table are separate tables here
    (the validation table's dictionary is one code longer)."""
    rng = np.random.default_rng(2860)
    n, nv = 3000, 500
    c0 = rng.integers(0, 7, n + nv)
    c1 = rng.integers(0, 6, n + nv)
    y = ((c0 * 2 + c1 + (rng.random(n + nv) < 0.15)) % 3).astype(np.int32)
    X = np.stack([c0, c1, rng.integers(0, 3, n + nv), y]).astype(np.int32)
    tr, va = np.ascontiguousarray(X[:, :n]), np.ascontiguousarray(X[:, n:])
    va[0, 10:40] = UNSEEN_CODE
    va[0, 5] = OUT_OF_DICT
    va[0, 50:70] = -1
    va[1, 60:90] = -1
    ttab = Tab(tr, [8, 6, 3, 3], kinds=(0,))
    vtab = Tab(va, [9, 6, 3, 3], kinds=(0,))
    return Fit("categorical: unseen, NULL, out of dictionary", ttab, 3, range(3), 3, valid=vtab)
