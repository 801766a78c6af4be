"""`LOFOutlierErrorDetector` (scikit-learn's `LocalOutlierFactor(novelty=False)` on one continuous attribute whose NULLs are replaced
by the median, repair/errors.py `ScikitLearnBackedErrorDetector._detect_impl`) as a function of a column's DICTIONARY CODES -- the
statement `rgbm_lof_1d` (csrc/rgbm_lof.hip) computes bit for bit, and what `detect_codes.build_descriptors` turns into `flag_bits`.

A continuous column's dictionary is its distinct values in ascending order and `count_codes` gives the rows per code.  In one
dimension the k nearest neighbours of a value are the other copies of itself plus a contiguous window of at most k neighbouring
dictionary positions, and all copies of a value share one k-distance, one local reachability density and one LOF: the detector is D
evaluations with neighbour reads inside a +-k halo of the sorted dictionary, not N k-d-tree queries.

scikit-learn's formulas, per position c with count m_c, k_ = max(1, min(k, n - 1)), n = the sum of the counts:
  neighbours  min(m_c - 1, k_) copies of itself at distance 0, then the nearest positions outward by |v_c - v_j| (float64), each taken
              whole until k_ is reached, the last one partially;  kdist[c] = the distance of the last neighbour taken
  lrd[c]      1.0 / (sum_j taken_j * max(kdist[j], |v_c - v_j|) / k_ + 1e-10)
  lof[c]      (sum_j taken_j * (lrd[j] / lrd[c])) / k_;  flagged when -lof < -1.5 (`offset_` of contamination='auto')
Both sums run left to right over the window's positions in ascending order, own position included, each term float64(taken) * x with
no fused multiply-add.  scikit-learn sums its k neighbours pairwise in distance order: the scores agree to rounding (measured:
DESIGN.md 5j), not to the bit, which is what the guard band of `n_near` is for.

Where two different values lie at exactly the same distance on either side of a point and only one of them fits into the k
neighbours, scikit-learn's choice is implementation-defined.  Such ties are resolved to the LEFT here, so that the function is total,
and counted (`n_ties`); the lowering refuses a column with any.  Plain numpy: both engines (and the tests) use it."""
import numpy as np

from repair.detect_codes import order_statistics

THRESHOLD = 1.5                      # -offset_ of LocalOutlierFactor(contamination='auto')
NEAR_BAND = 2.0 ** -40               # relative guard band around the threshold: 2^10 times the deviation measured against scikit-learn
MAX_K = 64


def median_from_counts(values, counts):
    """`float(np.median(expanded))` of the multiset that holds values[c] counts[c] times, bit for bit: the two middle order statistics,
    added and then halved (one of them when n is odd)."""
    values = np.asarray(values, np.float64)
    n = int(np.sum(np.asarray(counts, np.int64)))
    if n < 1:
        raise ValueError("no value")
    lo, hi = order_statistics(counts, [(n - 1) // 2, n // 2])
    if lo == hi:
        return float(values[lo])
    return float((values[lo] + values[hi]) / 2.0)


def filled_multiset(values, counts, n_null):
    """The column after `fillna(median)` as (values ascending, counts, position of the median, position of every dictionary code).

    Codes without a row (count 0) are not part of the multiset: their position is -1.  The median's count grows by `n_null` when the
    median is a dictionary value, otherwise one value is inserted (nothing when there is no NULL: the position of the median is then
    -1 unless a dictionary value equals it).  Without any non-NULL value the median is 0.0."""
    values = np.asarray(values, np.float64)
    counts = np.asarray(counts, np.int64)
    n_null = int(n_null)
    live = counts > 0
    v, m = values[live], counts[live].copy()
    med = median_from_counts(v, m) if len(v) else 0.0
    at = int(np.searchsorted(v, med, side="left"))
    hit = at < len(v) and v[at] == med
    shift = 0
    if hit:
        m[at] += n_null
    elif n_null > 0:
        v, m, shift = np.insert(v, at, med), np.insert(m, at, n_null), 1
    else:
        at = -1
    pos = np.full(len(values), -1, np.int64)
    p = np.arange(int(live.sum()), dtype=np.int64)
    if shift:
        p[p >= at] += 1
    pos[live] = p
    return v, m, at, pos


def _check(values, counts, k):
    v = np.ascontiguousarray(values, np.float64)
    m = np.ascontiguousarray(counts, np.int64)
    if v.ndim != 1 or m.shape != v.shape or len(v) < 1:
        raise ValueError("values and counts must be two non-empty vectors of one length")
    if int(k) != k or not 1 <= int(k) <= MAX_K:
        raise ValueError("k must be in 1 .. %d" % MAX_K)
    if not np.isfinite(v).all() or not np.isfinite(v[-1] - v[0]):
        raise ValueError("values must be finite")
    if (np.diff(v) <= 0).any():
        raise ValueError("values must be ascending")
    if (m < 1).any():
        raise ValueError("counts must be >= 1")
    if int(m.sum()) < 2:
        raise ValueError("LOF needs two values at least")
    return v, m


def lof_windows(values, counts, k=20):
    """The neighbour windows: (k_, m, self_taken, l, r, side, part, kdist, tie) -- window [l, r] of positions, the last neighbour
    taken lies at l (side 1) or r (side 2; 0: the copies of itself suffice) with `part` copies taken, `m` = the counts clamped to
    k_ + 1 (a count above k_ never acts differently from k_ + 1)."""
    v, cnt = _check(values, counts, k)
    D = len(v)
    k_ = max(1, min(int(k), int(cnt.sum()) - 1))
    m = np.minimum(cnt, k_ + 1)
    self_taken = np.minimum(m - 1, k_)
    need = k_ - self_taken
    c = np.arange(D, dtype=np.int64)
    l, r = c.copy(), c.copy()
    kdist = np.zeros(D, np.float64)
    side = np.zeros(D, np.int8)
    part = np.zeros(D, np.int64)
    tie = np.zeros(D, bool)
    for _ in range(k_):                                        # every step takes one copy at least
        act = need > 0
        if not act.any():
            break
        has_l, has_r = act & (l > 0), act & (r < D - 1)
        jl, jr = np.maximum(l - 1, 0), np.minimum(r + 1, D - 1)
        dl, dr = np.abs(v - v[jl]), np.abs(v - v[jr])
        go_l = has_l & (~has_r | (dl <= dr))                   # ties to the left
        go = go_l | has_r
        tie |= has_l & has_r & (dl == dr) & (need < m[jl] + m[jr])
        j = np.where(go_l, jl, jr)
        take = np.minimum(need, m[j])
        need = np.where(go, need - take, need)
        kdist = np.where(go, np.where(go_l, dl, dr), kdist)
        side = np.where(go, np.where(go_l, 1, 2), side).astype(np.int8)
        part = np.where(go, take, part)
        l = np.where(go_l, jl, l)
        r = np.where(go & ~go_l, jr, r)
    return k_, m, self_taken, l, r, side, part, kdist, tie


def _window_sum(k_, m, self_taken, l, r, side, part, term):
    """sum over j = l .. r ascending of float64(taken_j) * term(j), one addition per position."""
    D = len(m)
    c = np.arange(D, dtype=np.int64)
    last = np.where(side == 1, l, np.where(side == 2, r, -1))
    s = np.zeros(D, np.float64)
    for o in range(-k_, k_ + 1):
        j = c + o
        inside = (j >= l) & (j <= r)
        if not inside.any():
            continue
        jj = np.clip(j, 0, D - 1)
        taken = np.where(jj == c, self_taken, np.where(jj == last, part, m[jj])).astype(np.float64)
        s = np.where(inside, s + taken * term(jj), s)
    return s


def lof_codes(values, counts, k=20):
    """(lof float64 [D], flagged bool [D], n_ties, n_near) of the multiset that holds values[c] (ascending, finite) counts[c] (>= 1)
    times.  n_ties: positions whose window depends on the tie rule (see the header); n_near: positions with
    |lof - 1.5| <= 1.5 * 2^-40.  ValueError: fewer than two values in all (scikit-learn raises there), non-finite or unordered values,
    k outside 1 .. 64."""
    v = np.ascontiguousarray(values, np.float64)
    k_, m, self_taken, l, r, side, part, kdist, tie = lof_windows(values, counts, k)
    kf = np.float64(k_)
    s = _window_sum(k_, m, self_taken, l, r, side, part, lambda jj: np.maximum(kdist[jj], np.abs(v - v[jj])))
    lrd = 1.0 / (s / kf + 1e-10)
    s = _window_sum(k_, m, self_taken, l, r, side, part, lambda jj: lrd[jj] / lrd)
    lof = s / kf
    flagged = -lof < -THRESHOLD
    near = np.abs(lof - THRESHOLD) <= THRESHOLD * NEAR_BAND
    return lof, flagged, int(tie.sum()), int(near.sum())
