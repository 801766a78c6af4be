"""CPU: `RepairMisc.splitInputTable` / `toHistogram` / `toErrorMap` (mirrors of the reference's python/repair/tests/test_misc.py:82-86,
146-174) and the code-space k-means of repair/qgram_kmeans.py against the dense restatement of tests/kmeans_restatement.py."""
import logging

import numpy as np
import pandas as pd
import pytest

from tests import kmeans_restatement as R
from tests.helpers import frame, load_golden

MARGIN = 1e-9            # rows whose dense margin is below MARGIN * max(1, |best|) are left out of the label comparison
LEFT_OUT_CAP = 0.01      # at most this share of the rows, per iteration


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setenv("REPAIR_RESIDENT", "0")


def _register(name, df):
    from repair.api import Delphi
    Delphi.register_table(name, df)


def _adult():
    return frame(load_golden("adult")["input"])


def test_split_input_table_adult():
    """test_misc.py:82-86: k = 3 on adult gives one row per tid and exactly the ids 0, 1, 2."""
    from repair.misc import RepairMisc
    df = _adult()
    _register("adult", df)
    out = RepairMisc().options({"table_name": "adult", "row_id": "tid", "k": "3"}).splitInputTable()
    assert list(out.columns) == ["tid", "k"]
    assert out["tid"].tolist() == df["tid"].tolist()
    assert sorted(out["k"].unique().tolist()) == [0, 1, 2]
    assert all(isinstance(v, int) for v in out["k"].tolist())


def test_to_histogram():
    """test_misc.py:146-155: the numeric attribute v2 gives no row."""
    from repair.misc import RepairMisc
    _register("tempView", pd.DataFrame([(1, "a", 1), (2, "a", 1), (3, "a", 1), (4, "a", 2)], columns=["tid", "v1", "v2"]))
    out = RepairMisc().options({"table_name": "tempView", "targets": "v1,v2"}).toHistogram()
    assert list(out.columns) == ["attribute", "histogram"]
    assert out.sort_values("attribute").values.tolist() == [["v1", [{"value": "a", "cnt": 4}]]]
    _register("tempView", pd.DataFrame({"tid": [1, 2, 3], "v": ["x", None, "y"]}))
    out = RepairMisc().options({"table_name": "tempView", "targets": "v,missing"}).toHistogram()
    assert out.values.tolist() == [["v", [{"value": "x", "cnt": 1}, {"value": "y", "cnt": 1}]]]
    with pytest.raises(ValueError, match="Required options not found: table_name, targets"):
        RepairMisc().options({"table_name": "tempView"}).toHistogram()


def test_to_error_map():
    """test_misc.py:157-174."""
    from repair.misc import RepairMisc
    _register("tempView", pd.DataFrame([(1, "a", 1), (2, "b", 1), (3, "c", 1), (4, "d", 2)], columns=["tid", "v1", "v2"]))
    _register("errorCells", pd.DataFrame([(1, "v1"), (2, "v2"), (4, "v1"), (4, "v2")], columns=["tid", "attribute"]))
    misc = RepairMisc().options({"table_name": "tempView", "row_id": "tid", "error_cells": "errorCells"})
    assert misc.toErrorMap().sort_values("tid").values.tolist() == [[1, "*-"], [2, "-*"], [3, "--"], [4, "**"]]
    _register("errorCells", pd.DataFrame([(1, "v1")], columns=["tid", "attr"]))
    with pytest.raises(ValueError, match="Table 'errorCells' must have 'tid' and 'attribute' columns"):
        misc.toErrorMap()
    with pytest.raises(ValueError, match="Required options not found: table_name, row_id, error_cells"):
        RepairMisc().options({"table_name": "tempView", "row_id": "tid"}).toErrorMap()


def test_qgrams():
    from repair.qgram_kmeans import qgrams
    assert qgrams("abc", 2) == ["ab", "bc"]
    assert qgrams("ab", 2) == ["ab"]
    assert qgrams("a", 2) == ["a"]
    assert qgrams("", 2) == [""]
    assert qgrams(None, 2) == []
    assert qgrams("abcd", 3) == ["abc", "bcd"]
    with pytest.raises(ValueError):
        qgrams("abc", 0)


def _hospital_strings():
    df = frame(load_golden("hospital")["input"])
    keep = ["tid"] + [c for c in df.columns if c != "tid" and df[c].dtype == object]
    return df[keep]


FRAMES = {"adult": (_adult, 3), "hospital": (_hospital_strings, 4), "random": (lambda: R.random_frame(5000), 4)}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_numpy_step_equals_dense_restatement(name):
    """Every iteration of the loop until it stops, from the same initial centres: labels equal on every row whose dense margin is clear,
    at most 1 % of the rows left out, and the integer counts / sizes equal to those the restatement derives from the labels."""
    from repair import qgram_kmeans as Q
    make, k = FRAMES[name]
    df = make()
    attrs = [c for c in df.columns if c != "tid"]
    q = 2
    enc = Q.encode(df, attrs)
    e, vocab = Q.bag_matrix(enc.dicts, q)
    x, vocab_r = R.bag_matrix(df, attrs, q)
    assert sorted(vocab) == sorted(vocab_r)
    to_r = np.asarray([vocab.index(g) for g in vocab_r])          # restatement column -> column of E
    np.testing.assert_array_equal(Q.dense_rows(enc, e, np.arange(len(df)))[:, to_r], x)
    centres = Q.initial_centres(enc, e, k, seed=0)
    state, seen = {"assign": None}, []

    def step(p, h, first):
        state["assign"], counts, sizes, n_changed = Q.assign_step(enc.codes, enc.n_codes, enc.off, p, h, None if first else state["assign"])
        return counts, sizes, n_changed

    def on_step(it, c, p, h, counts, sizes, n_changed):
        lab, margin, best = R.assign(x, c[:, to_r])
        clear = margin > MARGIN * np.maximum(1.0, best)
        left_out = 1.0 - clear.mean()
        print("%s iteration %d: %d rows left out, %d changed" % (name, it, int((~clear).sum()), n_changed))
        assert left_out <= LEFT_OUT_CAP
        np.testing.assert_array_equal(state["assign"][clear], lab[clear])
        counts_r, sizes_r = R.counts_of(state["assign"], enc.codes, enc.n_codes, enc.off, enc.d_tot, k)
        np.testing.assert_array_equal(counts, counts_r)
        np.testing.assert_array_equal(sizes, sizes_r)
        assert counts.dtype == np.int64 and sizes.dtype == np.int64 and state["assign"].dtype == np.int32
        assert n_changed == (len(df) if it == 0 else int((state["assign"] != seen[-1]).sum()))
        seen.append(state["assign"].copy())

    steps = Q.lloyd(e, centres, step, max_iter=20, tol=1e-4, on_step=on_step)
    assert steps == len(seen) >= 1
    np.testing.assert_array_equal(Q.cluster(enc, k, q=q, seed=0), seen[-1])


def test_random_frame_has_the_cases_it_is_for():
    from repair import qgram_kmeans as Q
    df = R.random_frame(5000)
    attrs = [c for c in df.columns if c != "tid"]
    enc = Q.encode(df, attrs)
    assert enc.n_codes[-1] == 0 and (enc.codes[-1] == -1).all()                         # the all-NULL attribute
    assert (enc.codes[:-1] < 0).any() and any(len(s) < 2 for d in enc.dicts for s in d)  # NULLs, strings shorter than q
    grams = [set(g for s in d for g in Q.qgrams(s, 2)) for d in enc.dicts[:-1]]
    assert len(set.intersection(*grams)) > 0                                            # the attributes share q-grams


def test_option_handling(no_device):
    from repair import qgram_kmeans as Q
    from repair.misc import RepairMisc
    df = R.random_frame(5000)
    _register("rnd", df)
    base = {"table_name": "rnd", "row_id": "tid", "k": "4"}
    with pytest.raises(ValueError, match="Unknown clustering algorithm found: dbscan"):
        RepairMisc().options(dict(base, clustering_alg="dbscan")).splitInputTable()
    with pytest.raises(ValueError, match="Columns 'nope' do not exist in 'rnd'"):
        RepairMisc().options(dict(base, target_attr_list="a0,nope")).splitInputTable()
    with pytest.raises(ValueError):
        RepairMisc().options(dict(base, k="1")).splitInputTable()
    attrs = [c for c in df.columns if c != "tid"]
    out3 = RepairMisc().options(dict(base, q="3")).splitInputTable()
    assert out3["k"].tolist() == Q.split_rows(df, "tid", attrs, 4, q=3)["k"].tolist()
    assert set(out3["k"]) <= {0, 1, 2, 3} and len(out3) == len(df)
    a = RepairMisc().options(dict(base, seed="0")).splitInputTable()
    b = RepairMisc().options(dict(base, seed="0", clustering_alg="kmeans++")).splitInputTable()
    c = RepairMisc().options(dict(base, seed="5")).splitInputTable()
    assert a["k"].tolist() == b["k"].tolist()
    assert a["k"].tolist() != c["k"].tolist()
    sub = RepairMisc().options(dict(base, target_attr_list="a1,a0")).splitInputTable()
    assert sub["k"].tolist() == Q.split_rows(df, "tid", ["a1", "a0"], 4)["k"].tolist()


class _RefusingEngine:
    """Uploads, then refuses the step as the library refuses an argument (RGBM_ERR_PARAM = -2)."""
    name = "refusing"

    def __init__(self):
        self.calls = 0

    def upload(self, codes, n_codes):
        return object()

    def kmeans_assign(self, table, cols, code_off, p, h, first):
        self.calls += 1
        err = RuntimeError("rgbm_table_kmeans_assign failed (-2): k must be 2 .. 64")
        err.code = -2
        raise err


def test_engine_refusal_falls_back_to_numpy(no_device, caplog):
    from repair.misc import RepairMisc
    _register("adult", _adult())
    opts = {"table_name": "adult", "row_id": "tid", "k": "3"}
    want = RepairMisc().options(opts).splitInputTable()
    misc = RepairMisc().options(opts)
    misc._engine_override = _RefusingEngine()
    with caplog.at_level(logging.INFO, logger="repair.qgram_kmeans"):
        got = misc.splitInputTable()
    assert misc._engine_override.calls == 1
    assert got["k"].tolist() == want["k"].tolist()
    assert any("k must be 2 .. 64" in r.getMessage() for r in caplog.records)
