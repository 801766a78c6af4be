"""Bisecting k-means over bag-of-q-gram features, in CODE SPACE: `clustering_alg="bisecting"` of `RepairMisc.splitInputTable`, modelled on
MLlib's `BisectingKMeans.run` (the reference builds it in RepairMiscApi.scala:127-152).  The code-space trick is that of
repair/qgram_kmeans.py: with E [d_tot][V] = the bag of every dictionary entry, a centre is counts . E / size for the integer counts of the
codes a node holds, and a row is scored through  P = -2 E C^T  and  h = |c|^2  alone.

The tree.  Node ids are allocated in creation order, the root is 0; a level splits its chosen leaves in ascending id order and each takes the
next two ids (left, right).  A leaf is DIVISIBLE iff it is not final, holds two rows or more, and some dictionary entry e has
0 < counts[e] < size (an integer test for "its rows differ in some attribute"; it stands in for Spark's cost > EPSILON * size, which would need
|x|^2 per row).  Per level: needed = k - leaves; the needed largest divisible leaves are chosen (ties: the lower id); each gets the two centres
c -/+ 1e-4 * |c| * noise, noise = rng.random_sample(V) (Spark's `splitCenter`), and at most `max_iter` passes follow, a pass after the first
that changes no row ending the level (exactly: nothing could change afterwards).  `tol` is not read.

One pass (`bisect_step` in numpy, `rgbm_table_kmeans_bisect` on the device; equal labels, not close ones).  The chosen nodes are the slots
s = 0 .. m-1 in ascending id order, C = [left_0, right_0, left_1, ...].  A row whose label is the parent or either child of slot s computes
s0 = h[2s], then for j in attribute order with 0 <= code_j < n_codes  s0 = s0 + P[off_j + code_j][2s],  s1 the same at 2s + 1 -- float64,
additions only, in this order -- and takes the right child iff s1 < s0 (a tie goes left).  Every other row keeps its label and is counted
nowhere.  Returned: counts [2m][d_tot], sizes [2m], n_changed = the rows of the slots whose label differs from before the pass.

After the level a slot with both children non-empty turns them into leaves; a slot that left one child empty is a VOID split: the other child
replaces the parent as a leaf and is final, the leaf count does not grow (Spark likewise may return fewer than k clusters).  The group of a row
is the rank of its leaf among the leaves in ascending node id.
"""
import logging
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
from scipy import sparse

from repair.qgram_kmeans import STEP_BLOCK_ROWS, Encoded, bag_matrix

_logger = logging.getLogger(__name__)

SPLIT_NOISE = 1e-4            # Spark's splitCenter: level = 1e-4 * |c|
MAX_SLOTS = 512               # slots of one pass: k <= 1024 gives at most k / 2 of them
MAX_K = 1024

Step = Callable[[np.ndarray, np.ndarray, np.ndarray, np.ndarray, bool], Tuple[np.ndarray, np.ndarray, int]]


def bisect_step(codes: np.ndarray, n_codes: np.ndarray, off: np.ndarray, p: np.ndarray, h: np.ndarray, slot_of: np.ndarray, child: np.ndarray,
                labels: Optional[np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """One pass, stated in numpy (the module's docstring).  labels None = there are none yet, every row is node 0.  Returns (labels int32 [N],
    counts int64 [2m][d_tot], sizes int64 [2m], n_changed); the given labels are not written."""
    c, n = codes.shape
    d_tot, k2 = p.shape
    slot_of, child = np.asarray(slot_of, np.int64), np.asarray(child, np.int32)
    out = np.zeros(n, np.int32) if labels is None else np.array(labels, np.int32)
    counts = np.zeros(k2 * d_tot, np.int64)
    sizes = np.zeros(k2, np.int64)
    n_changed = 0
    for b in range(0, n, STEP_BLOCK_ROWS):
        lab = out[b:b + STEP_BLOCK_ROWS]
        named = (lab >= 0) & (lab < len(slot_of))
        slot = np.where(named, slot_of[np.where(named, lab, 0)], -1)
        rows = np.flatnonzero(slot >= 0)
        if not len(rows):
            continue
        s2 = 2 * slot[rows]
        s0, s1 = h[s2], h[s2 + 1]
        for j in range(c):
            v = codes[j, b + rows]
            ok = np.flatnonzero((v >= 0) & (v < n_codes[j]))
            s0[ok] = s0[ok] + p[off[j] + v[ok], s2[ok]]
            s1[ok] = s1[ok] + p[off[j] + v[ok], s2[ok] + 1]
        side = s2 + (s1 < s0)                        # strict: a tie goes left
        for j in range(c):
            v = codes[j, b + rows]
            ok = np.flatnonzero((v >= 0) & (v < n_codes[j]))
            counts += np.bincount(side[ok] * d_tot + off[j] + v[ok], minlength=k2 * d_tot)
        sizes += np.bincount(side, minlength=k2)
        new = child[side]
        n_changed += int((new != lab[rows]).sum())
        lab[rows] = new
    return out, counts.reshape(k2, d_tot), sizes, n_changed


def divisible(size: int, counts: np.ndarray, final: bool) -> bool:
    return (not final) and size >= 2 and bool(((counts > 0) & (counts < size)).any())


def choose(candidates: Sequence[Tuple[int, int]], needed: int) -> List[int]:
    """(node id, size) of the divisible leaves -> the ids this level splits, ascending: all of them, or the `needed` largest (ties: lower id)."""
    ids = [i for i, _ in candidates]
    if len(ids) > needed:
        ids = [i for i, _ in sorted(candidates, key=lambda t: (-t[1], t[0]))[:needed]]
    return sorted(ids)


class Tree:
    """What the loop built: per node `size`, `counts`, `centre`, `final`; `leaves` (ascending ids); `passes` per level; `void` = the void splits."""

    def __init__(self) -> None:
        self.size: List[int] = []
        self.counts: List[np.ndarray] = []
        self.centre: List[np.ndarray] = []
        self.final: List[bool] = []
        self.leaves: List[int] = []
        self.passes: List[int] = []
        self.void: List[int] = []

    def add(self, size: int, counts: np.ndarray, centre: np.ndarray) -> int:
        self.size.append(int(size)); self.counts.append(counts); self.centre.append(centre); self.final.append(False)
        return len(self.size) - 1

    def group_of_node(self) -> np.ndarray:
        """int32 [n_nodes]: the rank of a leaf among the leaves, -1 for every other node."""
        g = np.full(len(self.size), -1, np.int32)
        g[np.asarray(sorted(self.leaves), np.int64)] = np.arange(len(self.leaves), dtype=np.int32)
        return g


def _centre(et: sparse.csr_matrix, counts: np.ndarray, size: int) -> np.ndarray:
    return np.asarray(et @ counts.astype(np.float64)).reshape(-1) / float(size)


def grow(e: sparse.csr_matrix, root_counts: np.ndarray, n_rows: int, k: int, step: Step, seed: int = 0, max_iter: int = 20,
         on_pass: Optional[Callable[..., None]] = None, early_end: bool = True) -> Tree:
    """The loop both paths run.  `step(p, h, slot_of, child, first)` -> (counts, sizes, n_changed) runs one pass and keeps the labels.
    `on_pass(level, it, nodes, centres, p, h, slot_of, child, counts, sizes, n_changed)` sees every pass (nodes = the chosen ids).
    early_end False runs all `max_iter` passes of every level (the labels are the same: a test holds the two against each other)."""
    et = e.T.tocsr()
    max_iter = max(int(max_iter), 1)
    rng = np.random.RandomState(seed)
    tree = Tree()
    tree.add(n_rows, np.asarray(root_counts, np.int64), _centre(et, np.asarray(root_counts, np.int64), max(n_rows, 1)))
    tree.leaves = [0]
    first = True
    while True:
        needed = k - len(tree.leaves)
        cand = [(i, tree.size[i]) for i in sorted(tree.leaves) if divisible(tree.size[i], tree.counts[i], tree.final[i])]
        if needed <= 0 or not cand:
            break
        nodes = choose(cand, needed)
        m = len(nodes)
        centres = np.zeros((2 * m, e.shape[1]), np.float64)
        child = np.zeros(2 * m, np.int32)
        for s, node in enumerate(nodes):
            c = tree.centre[node]
            noise = rng.random_sample(e.shape[1])
            lvl = SPLIT_NOISE * np.sqrt(c.dot(c))
            centres[2 * s], centres[2 * s + 1] = c - lvl * noise, c + lvl * noise
            child[2 * s] = tree.add(0, np.zeros_like(tree.counts[0]), centres[2 * s])
            child[2 * s + 1] = tree.add(0, np.zeros_like(tree.counts[0]), centres[2 * s + 1])
        slot_of = np.full(len(tree.size), -1, np.int32)
        for s, node in enumerate(nodes):
            slot_of[[node, child[2 * s], child[2 * s + 1]]] = s
        level = len(tree.passes)
        for it in range(max_iter):
            h = (centres * centres).sum(axis=1)
            p = np.ascontiguousarray(-2.0 * np.asarray(e @ centres.T), np.float64)
            counts, sizes, n_changed = step(p, h, slot_of, child, first)
            first = False
            if on_pass is not None:
                on_pass(level, it, nodes, centres, p, h, slot_of, child, counts, sizes, n_changed)
            nz = np.flatnonzero(sizes > 0)
            centres[nz] = np.asarray(et @ counts[nz].T.astype(np.float64)).T / sizes[nz, None].astype(np.float64)
            if early_end and it > 0 and n_changed == 0:
                break
        tree.passes.append(it + 1)
        for s, node in enumerate(nodes):
            tree.leaves.remove(node)
            kids = [int(child[2 * s]), int(child[2 * s + 1])]
            for j, kid in enumerate(kids):
                tree.size[kid], tree.counts[kid], tree.centre[kid] = int(sizes[2 * s + j]), counts[2 * s + j].copy(), centres[2 * s + j].copy()
            full = [kid for kid in kids if tree.size[kid] > 0]
            tree.leaves += full
            if len(full) == 1:                                   # a void split: the leaf count does not grow, the leaf is final
                tree.final[full[0]] = True
                tree.void.append(node)
        tree.leaves.sort()
    if tree.void:
        _logger.info("bisecting k-means: %d void split(s), %d of %d groups" % (len(tree.void), len(tree.leaves), k))
    return tree


def numpy_step(enc: Encoded, state: Dict[str, Any]) -> Step:
    """The numpy pass over the encoded attributes; the labels live in state["labels"]."""
    def step(p: np.ndarray, h: np.ndarray, slot_of: np.ndarray, child: np.ndarray, first: bool) -> Tuple[np.ndarray, np.ndarray, int]:
        state["labels"], counts, sizes, n_changed = bisect_step(enc.codes, enc.n_codes, enc.off, p, h, slot_of, child,
                                                                None if first else state["labels"])
        return counts, sizes, n_changed
    return step


def root_counts(enc: Encoded) -> np.ndarray:
    out = np.zeros(enc.d_tot, np.int64)
    for j in range(len(enc.dicts)):
        v = enc.codes[j]
        out[enc.off[j]:enc.off[j] + enc.n_codes[j]] = np.bincount(v[(v >= 0) & (v < enc.n_codes[j])], minlength=enc.n_codes[j])
    return out


def cluster(enc: Encoded, k: int, q: int = 2, seed: int = 0, max_iter: int = 20, engine: Any = None,
            on_pass: Optional[Callable[..., None]] = None, early_end: bool = True, tree_out: Optional[List[Tree]] = None) -> np.ndarray:
    """Group ids int32 [N] (0 .. k'-1, k' <= k) of the encoded attributes.  With an engine the codes are uploaded once, the root counts and
    every pass run on the device and the labels (node ids) are read once; when the engine refuses (any error of its calls: more than 2048
    tree nodes after void splits, d_tot * 2m > 2^27, no device, ...) the numpy pass runs the same loop from the start, the reason in the log."""
    if not 2 <= k <= MAX_K:
        raise ValueError("k must be 2 .. %d for the bisecting k-means, but %d found" % (MAX_K, k))
    n = enc.codes.shape[1]
    if enc.d_tot == 0:                          # nothing but NULLs: the root is not divisible
        return np.zeros(n, np.int32)
    e, _ = bag_matrix(enc.dicts, q)
    tree = None
    if engine is not None:
        try:
            table = engine.upload(enc.codes, enc.n_codes)
            cols = np.arange(len(enc.dicts), dtype=np.int32)
            root = np.concatenate([np.asarray(engine.count_codes(table, j), np.int64) for j in range(len(enc.dicts))])
            tree = grow(e, root, n, k, lambda p, h, slot_of, child, first: engine.kmeans_bisect(table, cols, enc.off, slot_of, child, p, h, first),
                        seed, max_iter, on_pass, early_end)
            nodes = np.asarray(engine.kmeans_read(table), np.int32) if tree.passes else np.zeros(n, np.int32)
        except Exception as ex:  # noqa: BLE001 - a refusal (RGBM_ERR_PARAM) or no device: the numpy pass
            _logger.info("bisecting q-gram k-means runs its numpy pass: %s" % ex)
            tree = None
    if tree is None:
        state: Dict[str, Any] = {"labels": np.zeros(n, np.int32)}
        tree = grow(e, root_counts(enc), n, k, numpy_step(enc, state), seed, max_iter, on_pass, early_end)
        nodes = state["labels"]
    if tree_out is not None:
        tree_out.append(tree)
    return tree.group_of_node()[nodes]
