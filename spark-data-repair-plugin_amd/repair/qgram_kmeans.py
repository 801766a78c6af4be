"""k-means over bag-of-q-gram features, in CODE SPACE: the statement behind `RepairMisc.splitInputTable`
(reference RepairMiscApi.scala:52-153 `computeQgram` / `splitInputTableInto`, python/repair/misc.py:182-213).

The reference builds an N x V sparse matrix (one bag of q-grams per row, `CountVectorizer`) and hands it to Spark's k-means.  On a
dictionary-encoded table the bag of a row is the sum of the bags of its dictionary entries, one per attribute, so with
E [d_tot][V] = the bag of every distinct value (d_tot = all dictionary entries of the target attributes, V = the pooled vocabulary)

    x . c_k  =  sum_j  E[off_j + code_j] . c_k

and one Lloyd iteration needs  P = -2 E C^T  ([d_tot][k]) and  h_k = |c_k|^2  only: the score of a row is h_k plus one row of P per
attribute (|x|^2 is the same for every centre and drops out of the arg-min), and the new centres follow from the integer counts
counts[k][d_tot] of the codes each cluster holds:  C_k = counts[k] . E / n_k.  The assignment step is the only pass over the rows; it
is `assign_step` here (numpy) and `rgbm_table_kmeans_assign` on the device, and both compute the same float64 additions in the same
order, so their labels are equal, not close.

numpy / scipy only; `split_rows` is the entry, `lloyd` the loop both paths run.  `split_rows(alg="bisecting")` runs the bisecting k-means
of repair/qgram_bisect.py on the same encoding and the same E instead.
"""
import logging
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np
import pandas as pd
from scipy import sparse

_logger = logging.getLogger(__name__)

INIT_SAMPLE_ROWS = 4096       # k-means++ runs on this many rows at most
STEP_BLOCK_ROWS = 1 << 18     # rows the numpy step scores at a time (N x k float64 scores are never whole in memory)


def qgrams(s: Optional[str], q: int) -> List[str]:
    """`computeQgram` for one string (RepairMiscApi.scala:52-72): the len - q + 1 substrings of length q when len > q, else the string
    itself (also the empty string); None gives nothing.  Length counts Python code points here, UTF-16 units in the reference (Scala's
    String.length): a character outside the Basic Multilingual Plane is one position here and two there."""
    if q <= 0:
        raise ValueError("`q` must be positive, but %d got" % q)
    if s is None:
        return []
    if len(s) > q:
        return [s[i:i + q] for i in range(len(s) - q + 1)]
    return [s]


class Encoded:
    """The target attributes as codes: codes int32 [c][N] (-1 = NULL), dicts[j] = ascending distinct strings of attribute j, off[j] = its
    start among the d_tot entries of all dictionaries."""

    def __init__(self, codes: np.ndarray, dicts: List[List[str]]) -> None:
        self.codes = codes
        self.dicts = dicts
        self.n_codes = np.asarray([len(d) for d in dicts], np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.n_codes[:-1], dtype=np.int64)]).astype(np.int64)
        self.d_tot = int(self.n_codes.sum())


def encode(df: pd.DataFrame, attrs: Sequence[str]) -> Encoded:
    """Every attribute as a discrete column of its `CAST(.. AS STRING)` values (`array(attrs)` casts to string in the reference)."""
    from repair.errors import _to_sql_string
    codes = np.full((len(attrs), len(df)), -1, np.int32)
    dicts = []
    for j, a in enumerate(attrs):
        idx, uniq = pd.factorize(df[a].to_numpy(dtype=object), use_na_sentinel=True)
        strs = np.asarray([_to_sql_string(v) for v in uniq], dtype=object)
        if len(strs):
            values, inv = np.unique(strs, return_inverse=True)           # ascending; two values may share a string
            codes[j] = np.where(idx >= 0, inv[np.maximum(idx, 0)], -1)
            dicts.append([str(v) for v in values])
        else:
            dicts.append([])
    return Encoded(codes, dicts)


def bag_matrix(dicts: List[List[str]], q: int) -> Tuple[sparse.csr_matrix, List[str]]:
    """E [d_tot][V]: the q-gram counts of every dictionary entry.  The vocabulary is pooled over the attributes (the reference fits ONE
    CountVectorizer on the row's q-grams) and ordered by first appearance: attribute, then code, then position."""
    vocab, rows, cols = {}, [], []
    r = 0
    for d in dicts:
        for s in d:
            for g in qgrams(s, q):
                rows.append(r)
                cols.append(vocab.setdefault(g, len(vocab)))
            r += 1
    e = sparse.coo_matrix((np.ones(len(rows), np.float64), (rows, cols)), shape=(r, max(len(vocab), 1))).tocsr()
    e.sum_duplicates()
    return e, list(vocab)


def dense_rows(enc: Encoded, e: sparse.csr_matrix, rows: np.ndarray) -> np.ndarray:
    """The bags of the given rows, dense [len(rows)][V]."""
    x = np.zeros((len(rows), e.shape[1]), np.float64)
    for j in range(len(enc.dicts)):
        v = enc.codes[j, rows]
        ok = np.flatnonzero(v >= 0)
        if len(ok):
            x[ok] += e[enc.off[j] + v[ok]].toarray()
    return x


def initial_centres(enc: Encoded, e: sparse.csr_matrix, k: int, seed: int) -> np.ndarray:
    """k-means++ (Arthur & Vassilvitskii 2007) on min(N, 4096) rows drawn by np.random.RandomState(seed), dense on the host."""
    n = enc.codes.shape[1]
    rng = np.random.RandomState(seed)
    m = min(n, INIT_SAMPLE_ROWS)
    pos = np.sort(rng.choice(n, m, replace=False)) if m < n else np.arange(n)
    x = dense_rows(enc, e, pos)
    centres = np.zeros((k, x.shape[1]), np.float64)
    centres[0] = x[rng.randint(m)]
    d2 = ((x - centres[0]) ** 2).sum(axis=1)
    for i in range(1, k):
        tot = d2.sum()
        pick = rng.randint(m) if not tot > 0.0 else min(int(np.searchsorted(np.cumsum(d2), rng.random_sample() * tot, side="right")), m - 1)
        centres[i] = x[pick]
        d2 = np.minimum(d2, ((x - centres[i]) ** 2).sum(axis=1))
    return centres


def assign_step(codes: np.ndarray, n_codes: np.ndarray, off: np.ndarray, p: np.ndarray, h: np.ndarray,
                prev: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """The assignment step, stated in numpy.  Score of a row for cluster k, float64, in this order:  s_k = h_k, then for every attribute j
    in order with code_j inside [0, n_codes[j])  s_k = s_k + p[off_j + code_j][k]  -- additions only.  Label = the lowest k with the least
    score.  Returns (assign int32 [N], counts int64 [k][d_tot], sizes int64 [k], n_changed); prev None = first step, every row changed."""
    c, n = codes.shape
    d_tot, k = p.shape
    assign = np.empty(n, np.int32)
    counts = np.zeros(k * d_tot, np.int64)
    for b in range(0, n, STEP_BLOCK_ROWS):
        blk = codes[:, b:b + STEP_BLOCK_ROWS]
        s = np.repeat(h[None, :], blk.shape[1], axis=0)
        for j in range(c):
            ok = np.flatnonzero((blk[j] >= 0) & (blk[j] < n_codes[j]))
            s[ok] = s[ok] + p[off[j] + blk[j, ok]]
        lab = np.argmin(s, axis=1)                   # the first minimum: strict <
        assign[b:b + STEP_BLOCK_ROWS] = lab
        for j in range(c):
            ok = np.flatnonzero((blk[j] >= 0) & (blk[j] < n_codes[j]))
            counts += np.bincount(lab[ok] * d_tot + off[j] + blk[j, ok], minlength=k * d_tot)
    sizes = np.bincount(assign, minlength=k).astype(np.int64)
    n_changed = n if prev is None else int((assign != prev).sum())
    return assign, counts.reshape(k, d_tot), sizes, n_changed


def lloyd(e: sparse.csr_matrix, centres: np.ndarray, step: Callable[[np.ndarray, np.ndarray, bool], Tuple[np.ndarray, np.ndarray, int]],
          max_iter: int = 20, tol: float = 1e-4, on_step: Optional[Callable[..., None]] = None) -> int:
    """The loop.  `step(p, h, first)` -> (counts, sizes, n_changed) assigns every row (and keeps the labels); then
    C_k = counts[k] . E / sizes[k] (an empty cluster keeps its centre).  Stops when no row changed, when the largest squared centre
    shift is <= tol^2, or after max_iter steps (Spark's KMeans defaults: 20, 1e-4).  Returns the steps taken."""
    c = np.array(centres, np.float64)
    et = e.T.tocsr()
    for it in range(max_iter):
        h = (c * c).sum(axis=1)
        p = np.ascontiguousarray(-2.0 * np.asarray(e @ c.T), np.float64)
        counts, sizes, n_changed = step(p, h, it == 0)
        if on_step is not None:
            on_step(it, c, p, h, counts, sizes, n_changed)
        new = c.copy()
        nz = np.flatnonzero(sizes > 0)
        new[nz] = np.asarray(et @ counts[nz].T.astype(np.float64)).T / sizes[nz, None].astype(np.float64)
        shift = float(((new - c) ** 2).sum(axis=1).max())
        c = new
        if n_changed == 0 or shift <= tol * tol:
            return it + 1
    return max_iter


def cluster(enc: Encoded, k: int, q: int = 2, seed: int = 0, max_iter: int = 20, tol: float = 1e-4, engine: Any = None,
            centres: Optional[np.ndarray] = None, on_step: Optional[Callable[..., None]] = None) -> np.ndarray:
    """Labels int32 [N] of the encoded attributes.  With an engine the codes are uploaded once, every step runs on the device and the
    labels are read once; when the engine refuses (any error of its calls) the numpy step runs from the start, the reason in the log."""
    e, _ = bag_matrix(enc.dicts, q)
    if centres is None:
        centres = initial_centres(enc, e, k, seed)
    if enc.d_tot == 0:                          # nothing but NULLs: every score is h_k
        return np.full(enc.codes.shape[1], int(np.argmin((centres * centres).sum(axis=1))), np.int32)
    if engine is not None:
        try:
            table = engine.upload(enc.codes, enc.n_codes)
            cols = np.arange(len(enc.dicts), dtype=np.int32)
            lloyd(e, centres, lambda p, h, first: engine.kmeans_assign(table, cols, enc.off, p, h, first), max_iter, tol, on_step)
            return np.asarray(engine.kmeans_read(table), np.int32)
        except Exception as ex:  # noqa: BLE001 - a refusal (RGBM_ERR_PARAM: k > 64, d_tot * k > 2^27, ...) or no device: the numpy step
            _logger.info("q-gram k-means runs its numpy step: %s" % ex)
    state = {"assign": None}

    def step(p: np.ndarray, h: np.ndarray, first: bool) -> Tuple[np.ndarray, np.ndarray, int]:
        state["assign"], counts, sizes, n_changed = assign_step(enc.codes, enc.n_codes, enc.off, p, h, None if first else state["assign"])
        return counts, sizes, n_changed

    lloyd(e, centres, step, max_iter, tol, on_step)
    return state["assign"]


def split_rows(df: pd.DataFrame, row_id: str, attrs: Sequence[str], k: int, q: int = 2, seed: int = 0, max_iter: int = 20, tol: float = 1e-4,
               engine: Any = None, alg: str = "kmeans") -> pd.DataFrame:
    """`splitInputTableInto`: the frame [row_id, "k"], one row per input row in frame order, k = the row's cluster as int.  alg "kmeans": the
    Lloyd loop of this module; "bisecting": the tree of repair/qgram_bisect.py (k up to 1024, possibly fewer groups than k, `tol` not read)."""
    if alg not in ("kmeans", "bisecting"):
        raise ValueError("alg must be 'kmeans' or 'bisecting', but %r found" % (alg,))
    if k < 2:
        raise ValueError("k must be 2 or more, but %d found" % k)
    if q <= 0:
        raise ValueError("`q` must be positive, but %d got" % q)
    if len(df) == 0:
        return pd.DataFrame({row_id: df[row_id].to_numpy(), "k": np.zeros(0, np.int64)})
    if alg == "bisecting":
        from repair import qgram_bisect
        labels = qgram_bisect.cluster(encode(df, list(attrs)), k, q=q, seed=seed, max_iter=max_iter, engine=engine)
    else:
        labels = cluster(encode(df, list(attrs)), k, q=q, seed=seed, max_iter=max_iter, tol=tol, engine=engine)
    return pd.DataFrame({row_id: df[row_id].to_numpy(), "k": labels.astype(np.int64)})
