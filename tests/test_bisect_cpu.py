"""CPU: the bisecting k-means of repair/qgram_bisect.py (`clustering_alg="bisecting"` of `RepairMisc.splitInputTable`): its numpy pass
against the dense restatement of tests/bisect_restatement.py on every pass of every level, the loop on frames built by hand, the option
names, and an engine that refuses."""
import logging

import numpy as np
import pandas as pd
import pytest

from tests import bisect_restatement as B
from tests.helpers import frame, load_golden

MARGIN = 1e-9            # rows whose dense margin | |x - right|^2 - |x - left|^2 | is not above it are left out of the label comparison
LEFT_OUT_CAP = 0.01      # at most this share of a pass's rows


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setenv("REPAIR_RESIDENT", "0")


def _register(name, df):
    from repair.api import Delphi
    Delphi.register_table(name, df)


def _adult():
    return frame(load_golden("adult")["input"])


def _hospital_strings():
    df = frame(load_golden("hospital")["input"])
    keep = ["tid"] + [c for c in df.columns if c != "tid" and df[c].dtype == object]
    return df[keep]


# (frame, k, seed): seeds for which the restatement alone leaves at most 1 % of a pass's rows without a clear margin
FRAMES = {"adult": (_adult, 6, 0), "hospital": (_hospital_strings, 7, 0), "random": (lambda: B.random_frame(5000), 9, 0)}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_numpy_pass_equals_dense_restatement(name):
    """Every pass of every level, fed the loop's own centres through the hook: labels equal on every row of the split nodes whose dense
    margin is clear (at most 1 % of the pass's rows left out), every other row untouched, counts / sizes equal as integers to those the
    restatement derives from the labels, n_changed = the rows that moved."""
    from repair import qgram_bisect as QB
    from repair import qgram_kmeans as Q
    make, k, seed = FRAMES[name]
    df = make()
    attrs = [c for c in df.columns if c != "tid"]
    q = 2
    enc = Q.encode(df, attrs)
    e, vocab = Q.bag_matrix(enc.dicts, q)
    x, vocab_r = B.bag_matrix(df, attrs, q)
    assert sorted(vocab) == sorted(vocab_r)
    to_r = np.asarray([vocab.index(g) for g in vocab_r])          # restatement column -> column of E
    state = {"labels": np.zeros(len(df), np.int32)}
    prev = {"labels": np.zeros(len(df), np.int32)}
    tree_r, seen = B.DenseTree(), []

    def on_pass(level, it, nodes, centres, p, h, slot_of, child, counts, sizes, n_changed):
        if it == 0:
            for s, node in enumerate(nodes):
                tree_r.split(node, child[2 * s], child[2 * s + 1])
        centre_of = {int(c): centres[i][to_r] for i, c in enumerate(child)}
        want, margin, touched = B.dense_pass(x, prev["labels"], tree_r, nodes, centre_of)
        got = state["labels"]
        clear = touched & (margin > MARGIN)
        left_out = int((touched & ~clear).sum())
        print("%s level %d pass %d: %d nodes, %d rows, %d left out, %d changed" % (name, level, it, len(nodes), int(touched.sum()), left_out, n_changed))
        assert left_out <= LEFT_OUT_CAP * touched.sum()
        np.testing.assert_array_equal(got[clear], want[clear])
        np.testing.assert_array_equal(got[~touched], prev["labels"][~touched])
        assert np.isin(got[touched], child).all()
        counts_r, sizes_r = B.counts_of(got, touched, child, enc.codes, enc.n_codes, enc.off, enc.d_tot)
        np.testing.assert_array_equal(counts, counts_r)
        np.testing.assert_array_equal(sizes, sizes_r)
        assert counts.dtype == np.int64 and sizes.dtype == np.int64 and got.dtype == np.int32
        assert n_changed == int((got != prev["labels"]).sum())
        if it == 0:
            assert n_changed == int(touched.sum())
        prev["labels"] = got.copy()
        seen.append((level, it))

    tree = QB.grow(e, QB.root_counts(enc), len(df), k, QB.numpy_step(enc, state), seed=seed, on_pass=on_pass)
    assert len(tree.leaves) == k and len(seen) == sum(tree.passes) and len(tree.passes) >= 2
    np.testing.assert_array_equal(QB.cluster(enc, k, q=q, seed=seed), tree.group_of_node()[state["labels"]])


def _frame(rows, cols=("a", "b")):
    df = pd.DataFrame(rows, columns=list(cols))
    df.insert(0, "tid", np.arange(len(df)))
    return df


def _cluster(df, k, **kw):
    from repair import qgram_bisect as QB
    from repair import qgram_kmeans as Q
    trees = []
    labels = QB.cluster(Q.encode(df, [c for c in df.columns if c != "tid"]), k, tree_out=trees, **kw)
    return labels, trees[0]


DISTINCT = [("alpha", "one"), ("alpine", "once"), ("beta", "two"), ("betamax", "twofold"), ("gamma", "three"), ("gamut", "threes"),
            ("delta", "four"), ("deltoid", "fourth")]


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_exactly_k_groups_with_contiguous_ids(k):
    labels, tree = _cluster(_frame(DISTINCT * 3), k)
    assert sorted(set(labels.tolist())) == list(range(k)) and len(tree.leaves) == k and not tree.void
    by_row = {}
    for r, l in zip(DISTINCT * 3, labels.tolist()):
        assert by_row.setdefault(r, l) == l                       # equal rows, equal group
    assert labels.dtype == np.int32


def test_choose_largest_first_with_tie_break():
    from repair.qgram_bisect import choose
    cand = [(1, 5), (2, 7), (3, 7), (4, 2)]
    assert choose(cand, 4) == [1, 2, 3, 4] and choose(cand, 9) == [1, 2, 3, 4]
    assert choose(cand, 3) == [1, 2, 3]
    assert choose(cand, 2) == [2, 3]
    assert choose(cand, 1) == [2]                                 # 7 rows each: the lower id


@pytest.mark.parametrize("reps", [(3, 3, 3, 3), (2, 2, 3, 3), (4, 4, 1, 2)])
def test_the_loop_splits_the_largest_leaf_first(reps):
    """k = 3: the root splits into nodes 1 and 2, then ONE more split is needed: it goes to the larger of the two, to node 1 when they tie."""
    rows = [("aaaa", "b"), ("aaab", "b"), ("zzzz", "y"), ("zzzy", "y")]
    df = _frame([r for r, n in zip(rows, reps) for _ in range(n)])
    labels, tree = _cluster(df, 3)
    assert len(tree.passes) == 2 and len(tree.leaves) == 3
    assert tree.size[1] + tree.size[2] == len(df) and min(tree.size[1], tree.size[2]) >= 2
    want = 1 if tree.size[1] >= tree.size[2] else 2
    assert sorted(tree.leaves) == sorted([3 - want, 3, 4])
    if reps == (3, 3, 3, 3):
        assert tree.size[1] == tree.size[2] == 6 and want == 1


def test_a_node_of_identical_rows_is_never_chosen():
    df = _frame([("same", "row")] * 5 + [("other", "thing"), ("quite", "different")])
    labels, tree = _cluster(df, 5)
    assert len(set(labels[:5].tolist())) == 1 and len(tree.leaves) == 3 and not tree.void
    assert sorted(set(labels.tolist())) == [0, 1, 2]
    same = [i for i in tree.leaves if tree.size[i] == 5]
    assert len(same) == 1 and not tree.final[same[0]]            # not final, not divisible: 0 < counts[e] < size holds for no entry
    from repair.qgram_bisect import divisible
    assert not divisible(5, np.asarray([5, 0, 5]), False) and divisible(5, np.asarray([5, 1, 4]), False)
    assert not divisible(1, np.asarray([1, 0]), False) and not divisible(5, np.asarray([5, 1, 4]), True)


def test_a_void_split_marks_its_leaf_final_and_the_loop_ends(caplog):
    """("ab", "cd") and ("cd", "ab") differ as codes and have the same bag (strings no longer than q are their own q-gram, the vocabulary is
    pooled): their node is divisible by the integer test and cannot be split, whatever the noise."""
    df = _frame([("ab", "cd"), ("cd", "ab")] * 3 + [("xyxy", "zzzz")] * 2)
    with caplog.at_level(logging.INFO, logger="repair.qgram_bisect"):
        labels, tree = _cluster(df, 4)
    assert len(tree.void) == 1 and len(tree.leaves) == 2
    assert sorted(set(labels.tolist())) == [0, 1]                  # fewer than k groups, ids contiguous
    assert len(set(labels[:6].tolist())) == 1 and labels[6] == labels[7] != labels[0]
    kept = [i for i in tree.leaves if tree.size[i] == 6]
    assert len(kept) == 1 and tree.final[kept[0]] and kept[0] > tree.void[0]
    assert sum("void split" in r.getMessage() for r in caplog.records) == 1


def test_early_end_of_a_level_gives_the_labels_of_all_passes():
    df = _frame(DISTINCT * 3)
    early, tree = _cluster(df, 6, max_iter=8)
    full, tree_full = _cluster(df, 6, max_iter=8, early_end=False)
    assert set(tree_full.passes) == {8} and max(tree.passes) < 8 and min(tree.passes) >= 2
    np.testing.assert_array_equal(early, full)
    assert tree.leaves == tree_full.leaves and tree.size == tree_full.size


def test_seed():
    df = B.random_frame(600)
    a, _ = _cluster(df, 6, seed=0)
    b, _ = _cluster(df, 6, seed=0)
    c, _ = _cluster(df, 6, seed=5)
    np.testing.assert_array_equal(a, b)
    assert a.tolist() != c.tolist()


def test_names(no_device):
    from repair import qgram_kmeans as Q
    from repair.misc import RepairMisc
    df = B.random_frame(1500)
    _register("rnd_bisect", df)
    attrs = [c for c in df.columns if c != "tid"]
    base = {"table_name": "rnd_bisect", "row_id": "tid", "k": "5"}
    got = RepairMisc().options(dict(base, clustering_alg="bisecting", seed="3")).splitInputTable()
    want = Q.split_rows(df, "tid", attrs, 5, seed=3, alg="bisecting")
    assert list(got.columns) == ["tid", "k"] and got["tid"].tolist() == df["tid"].tolist()
    assert got["k"].tolist() == want["k"].tolist() and sorted(set(got["k"])) == [0, 1, 2, 3, 4]
    assert all(isinstance(v, int) for v in got["k"].tolist())
    big = RepairMisc().options(dict(base, clustering_alg="bisecting", k="1024")).splitInputTable()
    assert sorted(set(big["k"])) == list(range(big["k"].max() + 1)) and 64 < big["k"].max() + 1 <= 1024
    with pytest.raises(ValueError, match="1024 or less"):
        RepairMisc().options(dict(base, clustering_alg="bisecting", k="1025")).splitInputTable()
    a = RepairMisc().options(dict(base)).splitInputTable()
    b = RepairMisc().options(dict(base, clustering_alg="kmeans++")).splitInputTable()
    c = RepairMisc().options(dict(base, clustering_alg="bisect-kmeans")).splitInputTable()
    assert a["k"].tolist() == b["k"].tolist() == c["k"].tolist() == Q.split_rows(df, "tid", attrs, 5)["k"].tolist()
    assert a["k"].tolist() != got["k"].tolist()
    with pytest.raises(ValueError, match="Unknown clustering algorithm found: dbscan"):
        RepairMisc().options(dict(base, clustering_alg="dbscan")).splitInputTable()


class _RefusingEngine:
    """Uploads and counts, then refuses the pass as the library refuses an argument (RGBM_ERR_PARAM = -2)."""
    name = "refusing"

    def __init__(self):
        self.calls = 0

    def upload(self, codes, n_codes):
        self.codes, self.n_codes = codes, n_codes
        return object()

    def count_codes(self, table, col):
        v = self.codes[col]
        return np.bincount(v[v >= 0], minlength=int(self.n_codes[col])).astype(np.int64)

    def kmeans_bisect(self, table, cols, code_off, slot_of, child, p, h, first):
        self.calls += 1
        err = RuntimeError("rgbm_table_kmeans_bisect failed (-2): m must be 1 .. 512")
        err.code = -2
        raise err


def test_engine_refusal_falls_back_to_numpy(no_device, caplog):
    from repair.misc import RepairMisc
    _register("adult_bisect", _adult())
    opts = {"table_name": "adult_bisect", "row_id": "tid", "k": "4", "clustering_alg": "bisecting"}
    want = RepairMisc().options(opts).splitInputTable()
    misc = RepairMisc().options(opts)
    misc._engine_override = _RefusingEngine()
    with caplog.at_level(logging.INFO, logger="repair.qgram_bisect"):
        got = misc.splitInputTable()
    assert misc._engine_override.calls == 1
    assert got["tid"].tolist() == want["tid"].tolist() and got["k"].tolist() == want["k"].tolist()
    assert any("m must be 1 .. 512" in r.getMessage() for r in caplog.records)
