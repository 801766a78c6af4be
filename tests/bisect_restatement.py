"""An independent, dense statement of one pass of the bisecting k-means over bag-of-q-gram features: the explicit N x V bag matrix built
from the ROW STRINGS (tests/kmeans_restatement.py builds it), an explicit tree of node ids, and squared distances |x - c|^2 to the two
child centres of a row's own node.  tests/test_bisect_cpu.py holds repair.qgram_bisect (code space: h + rows of P) against it."""
import numpy as np

from tests.kmeans_restatement import bag_matrix, random_frame, row_strings  # noqa: F401  (the frames and the matrix of the k-means restatement)


class DenseTree:
    """Node ids and who splits into whom: children[node] = (left, right)."""

    def __init__(self):
        self.children = {}

    def split(self, node, left, right):
        assert node not in self.children and left not in self.children and right not in self.children
        self.children[int(node)] = (int(left), int(right))

    def family(self, node):
        """The labels a row of this split may carry during its level: the parent before the first pass, a child afterwards."""
        return (int(node),) + self.children[int(node)]


def dense_pass(x, labels, tree, nodes, centre_of):
    """One pass over the dense rows.  nodes: the nodes being split; centre_of[node id] = the centre of a child, float64 [V].
    Returns (new labels, margin = | |x - right|^2 - |x - left|^2 | per row (inf for a row of no split), touched = the rows of the splits)."""
    new = np.array(labels, np.int32)
    margin = np.full(len(labels), np.inf)
    touched = np.zeros(len(labels), bool)
    for node in nodes:
        left, right = tree.children[int(node)]
        rows = np.flatnonzero(np.isin(labels, tree.family(node)))
        d_left = ((x[rows] - centre_of[left][None, :]) ** 2).sum(axis=1)
        d_right = ((x[rows] - centre_of[right][None, :]) ** 2).sum(axis=1)
        new[rows] = np.where(d_right < d_left, right, left)
        margin[rows] = np.abs(d_right - d_left)
        touched[rows] = True
    return new, margin, touched


def counts_of(labels, touched, child, codes, n_codes, off, d_tot):
    """counts [len(child)][d_tot] and sizes [len(child)] of the touched rows by the child their label names (-1 / out of range = NULL)."""
    place = {int(c): i for i, c in enumerate(child)}
    idx = np.asarray([place.get(int(l), -1) for l in labels])
    idx[~touched] = -1
    assert (idx[touched] >= 0).all()
    counts = np.zeros((len(child), d_tot), np.int64)
    for j in range(codes.shape[0]):
        ok = touched & (codes[j] >= 0) & (codes[j] < n_codes[j])
        np.add.at(counts, (idx[ok], off[j] + codes[j][ok]), 1)
    sizes = np.zeros(len(child), np.int64)
    np.add.at(sizes, idx[touched], 1)
    return counts, sizes
