"""Cell-domain analysis and weak labels: the second half of the reference's `ErrorModel.detect`
(python/repair/errors.py:488-578; RepairApi.scala:126-149 `discretizeTable`, 231-477 `computeFreqStats` / `computePairwiseStats` /
`computeAttrStats`, 479-675 `computeDomainInErrorCells`), re-stated on code matrices: int32 codes, -1 = NULL.

This module is the value-space implementation and DEFINES the result; the device entries (`Table.pair_counts`,
`Table.cell_domains`, csrc/rgbm_domain.hip) must equal it -- counts exactly, probabilities bit for bit.  The entropy / selection
code (`candidate_pairs`, `pairwise_stats`, `analyse`) is shared by both paths: it only sees integer counts.

Stated deviations from the reference (DESIGN.md "Cell-domain analysis"):
  * the candidate filter counts the non-empty joint cells of (x, y) exactly; the reference uses a HyperLogLog sketch;
  * the score of a domain element is ONE division, b / rowCount, which is what exp(ln(cnt/R) + ln(b/cnt)) evaluates to
    mathematically: correctly rounded, so host and device agree bit for bit;
  * probability ties in a domain are ordered by ascending code (unspecified in the reference).
Kept quirk: the per-attribute element lists are folded with  IF(ISNOTNULL(domain), CONCAT(domain, d), d)  -- a NULL `d` (the
cell's correlated value is NULL or matches no group) after a non-NULL domain wipes the domain.
"""
import math
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

OPTION_DEFAULTS = {
    "error.attr_freq_ratio_threshold": 0.0, "error.pairwise_freq_ratio_threshold": 0.05, "error.max_attrs_to_compute_pairwise_stats": 3,
    "error.max_attrs_to_compute_domains": 2, "error.domain_threshold_alpha": 0.0, "error.domain_threshold_beta": 0.70,
}


class Joint:
    """Joint counts of an ordered attribute pair (x, y), sparse: `keys` ascending, key = bx * (dy + 1) + by with the NULL of
    either side in slot dx / dy; `cnt` the rows of each non-empty cell."""

    def __init__(self, dx: int, dy: int, keys: Any, cnt: Any) -> None:
        self.dx, self.dy = int(dx), int(dy)
        self.keys, self.cnt = np.asarray(keys, np.int64), np.asarray(cnt, np.int64)

    @classmethod
    def from_dense(cls, dense: Any) -> "Joint":
        dense = np.asarray(dense, np.int64)
        flat = dense.reshape(-1)
        keys = np.flatnonzero(flat)
        return cls(dense.shape[0] - 1, dense.shape[1] - 1, keys, flat[keys])

    @classmethod
    def from_bins(cls, bx: Any, by: Any, dx: int, dy: int) -> "Joint":
        """Sparse counting of two bin vectors (-1 = NULL)."""
        kx = np.where((bx < 0) | (bx >= dx), dx, bx).astype(np.int64)
        ky = np.where((by < 0) | (by >= dy), dy, by).astype(np.int64)
        keys, cnt = np.unique(kx * (dy + 1) + ky, return_counts=True)
        return cls(dx, dy, keys, cnt)

    def transposed(self) -> "Joint":
        kx, ky = self.keys // (self.dy + 1), self.keys % (self.dy + 1)
        k = ky * (self.dx + 1) + kx
        o = np.argsort(k, kind="stable")
        return Joint(self.dy, self.dx, k[o], self.cnt[o])

    def dense(self) -> Any:
        out = np.zeros((self.dx + 1) * (self.dy + 1), np.int64)
        out[self.keys] = self.cnt
        return out.reshape(self.dx + 1, self.dy + 1)


def _marginal(j: Joint) -> Any:
    """Rows per bin of x (slot dx = NULL): exact integer sums."""
    out = np.zeros(j.dx + 1, np.int64)
    np.add.at(out, j.keys // (j.dy + 1), j.cnt)
    return out


# ---------------------------------------------------------------------------------------------- discretised view
def continuous_lut(values: Any, discrete_thres: int) -> Any:
    """Look-up table code -> bin of a continuous attribute: `values` are the ascending distinct values behind the codes;
    bin = int((v - min) / (max - min) * discrete_thres), truncated toward zero (v = max gives bin `discrete_thres`); max = min gives
    NULL (the SQL division by zero)."""
    v = np.asarray(values, np.float64)
    if len(v) == 0:
        return np.zeros(0, np.int32)
    mn, mx = float(np.min(v)), float(np.max(v))
    if not mx > mn:
        return np.full(len(v), -1, np.int32)
    return np.trunc((v - mn) / (mx - mn) * float(discrete_thres)).astype(np.int64).astype(np.int32)


class View:
    """The discretised table (RepairApi.discretizeTable): which columns it keeps, their bins and the LUTs of the continuous ones."""

    def __init__(self, cols: List[int], n_bins: Dict[int, int], luts: Dict[int, Any], continuous: Sequence[int]) -> None:
        self.cols, self.n_bins, self.luts, self.continuous = list(cols), dict(n_bins), dict(luts), set(continuous)

    def bins(self, col: int, codes: Any) -> Any:
        codes = np.asarray(codes, np.int32)
        lut = self.luts.get(col)
        if lut is None:
            return codes
        out = np.full(len(codes), -1, np.int32)
        ok = (codes >= 0) & (codes < len(lut))
        out[ok] = lut[codes[ok]]
        return out


def discretised_view(n_codes: Sequence[int], domain_stats: Sequence[int], continuous: Dict[int, Any], discrete_thres: int) -> View:
    """`continuous`: {column: ascending distinct values}.  A discrete attribute with 1 < |domain| <= discrete_thres keeps its codes,
    a continuous one is binned through its LUT, every other attribute is dropped (a continuous attribute without any value too: the
    reference cannot state its min / max)."""
    cols, n_bins, luts = [], {}, {}
    for c in range(len(n_codes)):
        if c in continuous:
            if len(continuous[c]) == 0:
                continue
            luts[c] = continuous_lut(continuous[c], discrete_thres)
            n_bins[c] = int(discrete_thres) + 1
            cols.append(c)
        elif 1 < int(domain_stats[c]) <= int(discrete_thres):
            n_bins[c] = int(n_codes[c])
            cols.append(c)
    return View(cols, n_bins, luts, [c for c in cols if c in continuous])


# ---------------------------------------------------------------------------------------------- frequency statistics
def freq_min_count(row_count: int, attr_freq_ratio_threshold: float) -> int:
    """Groups are kept iff cnt > this (HAVING cnt > int(rowCount * threshold) when the threshold is positive)."""
    return int(row_count * attr_freq_ratio_threshold) if attr_freq_ratio_threshold > 0.0 else 0


def all_pairs(targets: Sequence[int], attrs: Sequence[int]) -> List[Tuple[int, int]]:
    """Every unordered (target, other) pair once, as (first, second) in the order met."""
    seen, out = set(), []
    for x in targets:
        for y in attrs:
            if y != x and frozenset((x, y)) not in seen:
                seen.add(frozenset((x, y)))
                out.append((int(x), int(y)))
    return out


class PairTable:
    """Joint tables of unordered pairs, readable in either orientation."""

    def __init__(self, pairs: Sequence[Tuple[int, int]], joints: Sequence[Joint]) -> None:
        self.index = {frozenset(p): i for i, p in enumerate(pairs)}
        self.pairs, self.joints = list(pairs), list(joints)
        self._t: Dict[int, Joint] = {}

    def has(self, x: int, y: int) -> bool:
        return frozenset((x, y)) in self.index

    def get(self, x: int, y: int) -> Joint:
        i = self.index[frozenset((x, y))]
        if self.pairs[i][0] == x:
            return self.joints[i]
        if i not in self._t:
            self._t[i] = self.joints[i].transposed()
        return self._t[i]

    def single(self, a: int) -> Any:
        for i, p in enumerate(self.pairs):
            if a in p:
                return _marginal(self.get(a, p[1] if p[0] == a else p[0]))
        raise KeyError(a)


def candidate_pairs(targets: Sequence[int], attrs: Sequence[int], table: PairTable, domain_stats: Any, max_attrs: int,
                    ratio_threshold: float) -> List[Tuple[int, int]]:
    """RepairApi.scala:429-448 with the exact number of non-empty joint cells in place of approx_count_distinct."""
    out: List[Tuple[int, int]] = []
    for x in targets:
        cands = [y for y in attrs if y != x]
        if len(cands) > max_attrs:
            scored = []
            for y in cands:
                co = (len(table.get(x, y).keys) + 0.0) / (int(domain_stats[x]) * int(domain_stats[y])) if int(domain_stats[x]) * int(domain_stats[y]) else math.inf
                scored.append((co, y))
            scored = [s for s in scored if s[0] < ratio_threshold]
            scored.sort(key=lambda s: s[0])                       # stable
            cands = [y for _, y in scored[:max_attrs]]
        out += [(x, y) for y in cands]
    return out


def _log2(v: float) -> float:
    return math.log(v) / math.log(2.0)


def entropy(kept_counts: Any, row_count: int, space: int) -> float:
    """-sum p log2 p over the kept groups (p = cnt / rowCount) plus the reference's correction term when the kept counts sum to
    less than rowCount (RepairApi.scala:306-325): the missing mass spread evenly over the groups that may exist."""
    cnt = np.asarray(kept_counts, np.int64)
    p = cnt.astype(np.float64) / float(row_count)
    terms = p * (np.log(p) / math.log(2.0))
    h = -(float(np.cumsum(terms)[-1]) if len(terms) else 0.0)       # sequential sum, ascending key order
    total = int(cnt.sum())
    if row_count > total:
        ub = max(int(space) - len(cnt), 1)
        avg = max((row_count - total + 0.0) / ub, 1.0)
        h = h + (-ub * (avg / row_count) * _log2(avg / row_count))
    return h


def pairwise_stats(row_count: int, pairs: Sequence[Tuple[Any, Any]], joint_counts: Dict[Any, Any], single_counts: Dict[Any, Any],
                   domain_stats: Dict[Any, int], targets: Sequence[Any] = ()) -> Dict[Any, List[Tuple[Any, float]]]:
    """computePairwiseStats: H(x|y) = H(x,y) - H(y) for the ordered pairs; per x the list [(y, H)] ascending (stable).
    `joint_counts[frozenset((x, y))]` / `single_counts[a]`: the counts of the groups the frequency filter kept, NULL groups included."""
    hxy = {frozenset(p): entropy(joint_counts[frozenset(p)], row_count, int(domain_stats[p[0]]) * int(domain_stats[p[1]])) for p in pairs}
    hy = {a: entropy(single_counts[a], row_count, int(domain_stats[a])) for a in {a for p in pairs for a in p}}
    out: Dict[Any, List[Tuple[Any, float]]] = {t: [] for t in targets}
    for x, y in pairs:
        out.setdefault(x, []).append((y, hxy[frozenset((x, y))] - hy[y]))
    for x in out:
        out[x].sort(key=lambda e: e[1])
    return out


# ---------------------------------------------------------------------------------------------- cell domains
def tau_of(alpha: float, row_count: int, dom_c: int, dom_a: int) -> int:
    """long(alpha * (rowCount // (dom(c) * dom(a)))): the inner division is integer division, as in the Scala."""
    prod = int(dom_c) * int(dom_a)
    return int(alpha * (row_count // prod)) if prod > 0 else 0


def cell_domains(cur: Any, corr_bins: Sequence[Any], joints: Sequence[Joint], min_cnt: Sequence[int], single_ok: Any, beta: float,
                 row_count: int, want_probs: bool = True) -> Tuple[Any, Any, Any, Optional[Any]]:
    """Domains of the error cells of ONE discrete target.

    cur        [m] the cells' current codes (-1 = NULL);  corr_bins[j] [m] the cells' rows' bins of correlated attribute j
    joints[j]  joint counts oriented (attribute j, target);  min_cnt[j]: an element exists iff cnt > min_cnt[j] (tau and the frequency
               filter);  single_ok [d_a]: the single-attribute group of the value survived the frequency filter
    Returns (weak [m] uint8, top [m] int32 (-1 = empty domain), top_prob [m], probs [m][d_a] or None); probs are 0 outside the scored values.
    """
    cur = np.asarray(cur, np.int32)
    m = len(cur)
    d_a = len(single_ok)
    single_ok = np.asarray(single_ok, bool)
    score = np.zeros((m, d_a), np.float64)
    R = float(row_count)
    for j, jt in enumerate(joints):
        assert jt.dy == d_a
        vc = np.asarray(corr_bins[j], np.int64)
        kc, ka = jt.keys // (d_a + 1), jt.keys % (d_a + 1)
        keep = (kc < jt.dx) & (ka < d_a) & (jt.cnt > int(min_cnt[j]))
        keys, cnt = jt.keys[keep], jt.cnt[keep]
        ok = (vc >= 0) & (vc < jt.dx)
        lo = np.searchsorted(keys, np.where(ok, vc, 0) * (d_a + 1))
        hi = np.searchsorted(keys, np.where(ok, vc, 0) * (d_a + 1) + d_a)
        num = np.where(ok, hi - lo, 0)
        # a NULL element list (no value / no group) wipes whatever the fold holds; the next non-NULL list starts afresh
        score[num == 0] = 0.0
        cell = np.repeat(np.arange(m), num)
        at = np.repeat(lo - np.concatenate([[0], np.cumsum(num)[:-1]]), num) + np.arange(int(num.sum())) if m else np.zeros(0, np.int64)
        b = np.maximum(cnt[at].astype(np.float64) - 1.0, 0.1)
        score[cell, keys[at] % (d_a + 1)] = score[cell, keys[at] % (d_a + 1)] + b / R
    score[:, ~single_ok] = 0.0                                     # the score is NULL without the value's single-attribute group
    den = np.zeros(m, np.float64)
    for n in range(d_a):                                           # fixed order: ascending code
        den = den + score[:, n]
    with np.errstate(divide="ignore", invalid="ignore"):
        probs = np.where(den[:, None] > 0.0, score / den[:, None], 0.0)
    top = np.full(m, -1, np.int32)
    top_prob = np.zeros(m, np.float64)
    for n in range(d_a):                                           # first maximum: ties by ascending code
        better = probs[:, n] > top_prob
        top[better] = n
        top_prob[better] = probs[better, n]
    valid = top_prob > beta
    top[~valid] = -1
    top_prob[~valid] = 0.0
    weak = ((cur >= 0) & (top == cur) & valid).astype(np.uint8)
    return weak, top, top_prob, (probs if want_probs else None)


def literal_probs(cur_dummy: Any, corr_bins: Sequence[Any], joints: Sequence[Joint], min_cnt: Sequence[int], single_cnt: Any, single_ok: Any,
                  row_count: int) -> Any:
    """The reference's literal formula  exp(ln(cnt_a / R) + ln(b / cnt_a))  summed and normalised with numpy: what the tests hold
    `cell_domains` against (1e-12 relative)."""
    m, d_a = len(corr_bins[0]) if corr_bins else 0, len(single_ok)
    score = np.zeros((m, d_a), np.float64)
    for j, jt in enumerate(joints):
        dense = jt.dense()
        for i in range(m):
            v = int(corr_bins[j][i])
            row = dense[v, :d_a] if 0 <= v < jt.dx else np.zeros(d_a, np.int64)
            el = row > int(min_cnt[j])
            if not el.any():
                score[i] = 0.0
                continue
            for n in np.flatnonzero(el):
                if single_ok[n]:
                    ca = float(single_cnt[n])
                    score[i, n] += math.exp(math.log(ca / row_count) + math.log(max(float(row[n]) - 1.0, 0.1) / ca))
    den = score.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, score / den, 0.0)


# ---------------------------------------------------------------------------------------------- the whole step
class HostBackend:
    """Counts and cell domains on a host code matrix [C][N] (the value-space path)."""

    def __init__(self, codes: Any, view: View) -> None:
        self.codes, self.view = codes, view
        self._bins: Dict[int, Any] = {}

    def bins(self, c: int) -> Any:
        if c not in self._bins:
            self._bins[c] = self.view.bins(c, self.codes[c])
        return self._bins[c]

    def pair_counts(self, pairs: Sequence[Tuple[int, int]]) -> List[Joint]:
        return [Joint.from_bins(self.bins(x), self.bins(y), self.view.n_bins[x], self.view.n_bins[y]) for x, y in pairs]

    def cell_domains(self, target: int, rows: Any, corr: Sequence[int], table: PairTable, min_cnt: Sequence[int], single_ok: Any, beta: float,
                     row_count: int, want_probs: bool = False) -> Tuple[Any, Any, Any, Optional[Any]]:
        rows = np.asarray(rows, np.int64)
        return cell_domains(self.bins(target)[rows], [self.bins(c)[rows] for c in corr], [table.get(c, target) for c in corr], min_cnt,
                            single_ok, beta, row_count, want_probs)


def analyse(backend: Any, n_rows: int, view: View, targets: Sequence[int], domain_stats: Sequence[int], cell_rows: Any, cell_cols: Any,
            options: Dict[str, Any], want_weak: bool = True, cell_counts: Optional[Dict[int, int]] = None) -> Dict[str, Any]:
    """computeAttrStats + computeDomainInErrorCells + the weak-label rule on any backend with `pair_counts` / `cell_domains`.

    targets: the repairable (noisy, discretised) columns, in order.  Returns dict(pairwise={target: [(attr column, H(target|attr))]},
    weak [cells] bool, top [cells] int32, top_prob [cells]).

    cell_counts: {column: its error cells} -- the cells stay WITH THE BACKEND (the cell set of a resident table) and `cell_rows` /
    `cell_cols` are None: per target with cells, `backend.drop_weak(target, corr, table, min_cnt, single_ok, beta, n_rows)` -> (cells
    examined, cells pruned) applies the weak-label rule where the cells lie.  The result then holds `weak_counts` {target: cells pruned}
    (a target that is not examined has none) and no `weak` / `top` / `top_prob`."""
    g = lambda k: options.get(k, OPTION_DEFAULTS[k])  # noqa: E731
    if cell_counts is not None:
        cell_rows, cell_cols = np.zeros(0, np.int64), np.zeros(0, np.int32)
    cell_rows, cell_cols = np.asarray(cell_rows, np.int64), np.asarray(cell_cols, np.int32)
    weak = np.zeros(len(cell_rows), bool)
    top = np.full(len(cell_rows), -1, np.int32)
    top_prob = np.zeros(len(cell_rows), np.float64)
    targets = [int(t) for t in targets if int(t) in view.n_bins]
    out: Dict[str, Any] = dict(pairwise={t: [] for t in targets}, weak=weak, top=top, top_prob=top_prob)
    if cell_counts is not None:
        out = dict(pairwise=out["pairwise"], weak_counts={})
    if not targets or len(view.cols) <= 1:
        return out
    pairs = all_pairs(targets, view.cols)
    table = PairTable(pairs, backend.pair_counts(pairs))
    cand = candidate_pairs(targets, view.cols, table, domain_stats, int(g("error.max_attrs_to_compute_pairwise_stats")),
                           float(g("error.pairwise_freq_ratio_threshold")))
    fmin = freq_min_count(n_rows, float(g("error.attr_freq_ratio_threshold")))
    singles = {a: table.single(a) for a in view.cols}
    kept_single = {a: s[s > fmin] for a, s in singles.items()}
    kept_joint = {}
    for x, y in cand:
        c = table.get(x, y).cnt
        kept_joint[frozenset((x, y))] = c[c > fmin]
    stats = pairwise_stats(n_rows, cand, kept_joint, kept_single, {c: int(domain_stats[c]) for c in view.cols}, targets)
    out["pairwise"] = stats
    if not want_weak:
        return out
    k = int(g("error.max_attrs_to_compute_domains"))
    alpha, beta = float(g("error.domain_threshold_alpha")), float(g("error.domain_threshold_beta"))
    for t in targets:
        corr = [y for y, _ in stats[t][:k]]
        sel = np.flatnonzero(cell_cols == t)
        if t in view.continuous or not corr or (len(sel) == 0 if cell_counts is None else int(cell_counts.get(t, 0)) == 0):
            continue
        min_cnt = [max(tau_of(alpha, n_rows, domain_stats[c], domain_stats[t]), fmin, 0) for c in corr]
        ok = singles[t][:view.n_bins[t]] > fmin
        if cell_counts is not None:
            examined, pruned = backend.drop_weak(t, corr, table, min_cnt, ok, beta, n_rows)
            assert int(examined) == int(cell_counts[t]), "the cell set holds %d cells of column %d, not %d" % (examined, t, cell_counts[t])
            out["weak_counts"][t] = int(pruned)
            continue
        w, tp, pr, _ = backend.cell_domains(t, cell_rows[sel], corr, table, min_cnt, ok, beta, n_rows)
        weak[sel], top[sel], top_prob[sel] = np.asarray(w, bool), tp, pr
    return out


# ---------------------------------------------------------------------------------------------- given frequency tables (tests)
def stats_from_rows(attrs: Sequence[str], rows: Sequence[Sequence[Any]]) -> Dict[str, Any]:
    """A frequency table in the reference's own shape -- rows (value_0, group_0, value_1, group_1, ..., cnt) with group = 1 where
    the attribute is grouped out -- as code-space statistics: dictionaries (ascending distinct values), single counts and joint
    tables.  A row belongs to the single-attribute groups of `a` iff only a's group flag is 0, to the pair (a, b) iff both flags
    are 0 and every other attribute is NULL."""
    A = len(attrs)
    vals = [[r[2 * i] for r in rows] for i in range(A)]
    flags = np.array([[int(r[2 * i + 1]) for r in rows] for i in range(A)], np.int64).reshape(A, len(rows))
    cnt = np.array([int(r[2 * A]) for r in rows], np.int64)
    dicts = [sorted({str(v) for v in vals[i] if v is not None}) for i in range(A)]
    code = [np.array([dicts[i].index(str(v)) if v is not None else -1 for v in vals[i]], np.int64) for i in range(A)]
    single, joint = {}, {}
    for i, a in enumerate(attrs):
        d = len(dicts[i])
        s = np.zeros(d + 1, np.int64)
        for r in range(len(rows)):
            if flags[i, r] == 0 and all(flags[k, r] == 1 for k in range(A) if k != i):
                s[code[i][r] if code[i][r] >= 0 else d] = max(s[code[i][r] if code[i][r] >= 0 else d], cnt[r])
        single[a] = s
    for i in range(A):
        for j in range(i + 1, A):
            di, dj = len(dicts[i]), len(dicts[j])
            dense = np.zeros((di + 1, dj + 1), np.int64)
            for r in range(len(rows)):
                if flags[i, r] == 0 and flags[j, r] == 0 and all(code[k][r] < 0 for k in range(A) if k not in (i, j)):
                    dense[code[i][r] if code[i][r] >= 0 else di, code[j][r] if code[j][r] >= 0 else dj] += cnt[r]
            joint[(attrs[i], attrs[j])] = Joint.from_dense(dense)
    return dict(dicts=dict(zip(attrs, dicts)), single=single, joint=joint)


def freq_rows(attrs: Sequence[str], dicts: Dict[str, Sequence[Any]], single: Dict[str, Any], joint: Dict[Tuple[str, str], Joint],
              min_count: int = 0) -> List[Tuple[Any, ...]]:
    """The inverse: the kept groups as the reference's rows (value, group flag, ..., cnt), in no particular order."""
    out = []
    pos = {a: i for i, a in enumerate(attrs)}

    def row(parts: Dict[str, Any], cnt: int) -> Tuple[Any, ...]:
        r: List[Any] = []
        for a in attrs:
            r += [parts[a], 0] if a in parts else [None, 1]
        return tuple(r + [int(cnt)])

    for a in attrs:
        d = len(dicts[a])
        for b, c in enumerate(single[a]):
            if c > min_count:
                out.append(row({a: dicts[a][b] if b < d else None}, c))
    for (x, y), jt in joint.items():
        assert pos[x] != pos[y]
        for key, c in zip(jt.keys, jt.cnt):
            bx, by = int(key) // (jt.dy + 1), int(key) % (jt.dy + 1)
            if c > min_count:
                out.append(row({x: dicts[x][bx] if bx < jt.dx else None, y: dicts[y][by] if by < jt.dy else None}, c))
    return out


def domains_from_rows(attrs: Sequence[str], rows: Sequence[Sequence[Any]], row_count: int, domain_stats: Dict[str, int], pairwise: Dict[str, Any],
                      continuous: Sequence[str], cells: Sequence[Tuple[Dict[str, Any], str, Any]], max_attrs: int, alpha: float,
                      beta: float) -> List[List[Tuple[Any, float]]]:
    """computeDomainInErrorCells on a GIVEN frequency table: `cells` are (the cell's row as {attr: value}, attribute, current value);
    returns each cell's domain [(value, prob)], descending."""
    st = stats_from_rows(attrs, rows)
    out = []
    for rowvals, attr, _cur in cells:
        corr = [a for a, _ in pairwise.get(attr, [])][:max_attrs]
        if attr in continuous or not corr:
            out.append([])
            continue
        da = len(st["dicts"][attr])
        joints, bins, mins = [], [], []
        for c in corr:
            jt = st["joint"][(c, attr)] if (c, attr) in st["joint"] else st["joint"][(attr, c)].transposed()
            joints.append(jt)
            v = rowvals.get(c)
            bins.append(np.array([st["dicts"][c].index(str(v)) if v is not None and str(v) in st["dicts"][c] else -1], np.int64))
            mins.append(max(tau_of(alpha, row_count, domain_stats[c], domain_stats[attr]), 0))
        ok = st["single"][attr][:da] > 0
        _, _, _, probs = cell_domains(np.array([-1], np.int32), bins, joints, mins, ok, beta, row_count)
        dom = [(st["dicts"][attr][n], float(probs[0, n])) for n in range(da) if probs[0, n] > beta]
        dom.sort(key=lambda e: -e[1])
        out.append(dom)
    return out
