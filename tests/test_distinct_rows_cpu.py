"""CPU: training on the distinct rows of a resident table (rgbm_table_distinct_rows, `repair_table(distinct_training_rows=..)`,
`model.train.distinct_rows`): the numpy restatement of the device entry, the two options, and the pipeline hook on a CPU engine whose table
offers `distinct_rows()` from the restatement and whose `train` expands a distinct table back through the inverse -- so every model must
be the whole table's, and the hook only shows in `distinct_rows` of the result.
Reference semantics pinned: the models of python/repair/model.py:768-815 (every row of the frame); the reference has no distinct-row variant."""
import numpy as np
import pandas as pd
import pytest

from repair.model import RepairModel
from tests import distinct_restatement as DR
from tests.helpers import OracleEngine
from tests.synth import make_table

PARAMS = dict(n_estimators=4, learning_rate=0.2, num_leaves=31, max_depth=7)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _tables():
    rng = np.random.default_rng(7)
    a, _, ca = make_table(3000, 5, seed=11, null_ratio=0.05, cards=[2, 3, 4, 2, 3])
    yield a, ca
    b = np.ascontiguousarray(np.concatenate([a, a[:, :700], np.repeat(a[:, 5:8], 300, axis=1)], axis=1)[:, rng.permutation(3000 + 700 + 900)])
    yield b, ca                                                                    # groups of more than 255 rows
    c = rng.integers(-1, 1000, (12, 2000)).astype(np.int32)
    c[:, 1000:] = c[:, :1000]
    yield c, np.full(12, 1000, np.int32)                                           # a key of more than one word
    yield np.zeros((3, 600), np.int32), np.ones(3, np.int32)                       # one group, three copies
    yield np.array([[0, -1, 0, -1], [-1, 0, -1, 0]], np.int32), np.ones(2, np.int32)   # rows that differ only in which cell is NULL


@pytest.mark.parametrize("case", range(5))
def test_restatement_agrees_with_the_host_dedup_up_to_the_order_of_groups(case):
    from repair.pipeline import distinct_rows
    codes, n_codes = list(_tables())[case]
    N = codes.shape[1]
    dist, mult, inv = DR.distinct_rows(codes)
    assert np.array_equal(dist[:, inv], codes) and int(mult.astype(np.int64).sum()) == N and mult.min() >= 1
    hd, hm, hi = distinct_rows(codes, n_codes)
    assert dist.shape == hd.shape
    as_rows = lambda d, m: sorted(map(tuple, np.vstack([d, m.astype(np.int32)[None]]).T.tolist()))   # noqa: E731
    assert as_rows(dist, mult) == as_rows(hd, hm)
    # first-occurrence order: the first copies' first rows ascend, the copies of a group are consecutive, 255s first
    first_copy = np.unique(inv)
    first_row = np.array([np.flatnonzero(inv == p)[0] for p in first_copy[:50]])
    assert (np.diff(first_row) > 0).all() and first_copy[0] == 0
    cnt = np.bincount(inv, minlength=dist.shape[1])
    for p in first_copy:
        k = (int(cnt[p]) + 254) // 255
        assert (mult[p:p + k - 1] == 255).all() and int(mult[p + k - 1]) == int(cnt[p]) - 255 * (k - 1)
        assert (dist[:, p:p + k] == dist[:, [p]]).all()
    assert np.array_equal(DR.expand(dist, inv), codes)


def test_restatement_of_a_tiny_table_by_hand():
    codes = np.array([[1, 0, 1, 1, 0, -1], [2, 2, 2, 2, 2, 2]], np.int32)
    dist, mult, inv = DR.distinct_rows(codes, max_mult=2)
    assert dist.tolist() == [[1, 1, 0, -1], [2, 2, 2, 2]] and mult.tolist() == [2, 1, 2, 1] and inv.tolist() == [0, 2, 0, 0, 2, 3]


# ---- the options ----------------------------------------------------------------------------------------------------------------
def test_options_are_registered_parsed_and_validated():
    on, ratio = "model.train.distinct_rows", "model.train.distinct_rows.max_ratio"
    assert on in RepairModel.option_keys and ratio in RepairModel.option_keys
    m = RepairModel()
    assert m._get_option_value(*RepairModel._opt_train_distinct_rows) is False
    assert m._get_option_value(*RepairModel._opt_train_distinct_rows_max_ratio) == 0.5
    m = m.option(on, "true").option(ratio, "0.25")
    assert m._get_option_value(*RepairModel._opt_train_distinct_rows) is True
    assert m._get_option_value(*RepairModel._opt_train_distinct_rows_max_ratio) == 0.25
    assert RepairModel().option(ratio, "1.0")._get_option_value(*RepairModel._opt_train_distinct_rows_max_ratio) == 1.0
    for bad in ("0.0", "1.5", "-1"):
        with pytest.raises(ValueError, match="should be in"):
            RepairModel().option(ratio, bad)._get_option_value(*RepairModel._opt_train_distinct_rows_max_ratio)
    with pytest.raises(ValueError, match="Failed to cast"):
        RepairModel().option(ratio, "half")._get_option_value(*RepairModel._opt_train_distinct_rows_max_ratio)
    with pytest.raises(ValueError, match="Non-existent key"):
        RepairModel().option("model.train.distinct_row", "true")


# ---- the pipeline hook ----------------------------------------------------------------------------------------------------------
class DistinctOracleEngine(OracleEngine):
    """OracleEngine whose tables offer `distinct_rows()` (the restatement); `train` expands a distinct table through its inverse."""

    def __init__(self, small=50):
        self.small, self.calls, self.trained_on_distinct, self.closed = small, 0, [], 0

    class _Table(OracleEngine._Table):
        inverse, engine = None, None

        def _like(self, codes):
            t = type(self)(codes, self.n_codes, self.values, self.kinds)
            t.engine = self.engine
            return t

        def gather_rows(self, rows):
            return self._like(self.codes[:, np.asarray(rows, np.int64)])

        def distinct_rows(self):
            dist, mult, inv = DR.distinct_rows(self.codes)
            t = self._like(dist)
            t.mult, t.inverse = mult, inv
            self.engine.calls += 1
            return t

        def close(self):
            if self.inverse is not None:
                self.engine.closed += 1

    def small_rows(self):
        return self.small

    def _own(self, t):
        o = DistinctOracleEngine._Table(t.codes, t.n_codes, t.values, t.kinds)
        o.engine = self
        return o

    def upload(self, codes, n_codes):
        return self._own(OracleEngine.upload(self, codes, n_codes))

    def upload_dictionaries(self, indices, remaps):
        return self._own(OracleEngine.upload_dictionaries(self, indices, remaps))

    def train(self, table, target, feats, class_weight, params, y_value=None, want_stats=False):
        if getattr(table, "inverse", None) is not None:
            self.trained_on_distinct.append(int(target))
            table = table._like(DR.expand(table.codes, table.inverse))
        return OracleEngine.train(self, table, target, feats, class_weight, params, y_value=y_value, want_stats=want_stats)


class NoDistinctEngine(DistinctOracleEngine):
    class _Table(OracleEngine._Table):
        engine = None

    def _own(self, t):
        return NoDistinctEngine._Table(t.codes, t.n_codes, t.values, t.kinds)


def _frame(n=600, seed=23):
    dirty, _, _ = make_table(n, 5, seed=seed, null_ratio=0.04, cards=[2, 3, 4, 2, 3])
    df = pd.DataFrame({"tid": np.arange(n)})
    for c in range(5):
        df["c%d" % c] = [None if v < 0 else "v%d" % v for v in dirty[c]]
    return df


TARGETS = ["c1", "c2", "c4"]


def _run(engine, df, **kw):
    from repair.pipeline import repair_frame
    return repair_frame(engine, df, "tid", targets=TARGETS, base_params=dict(PARAMS, **kw.pop("params", {})), want_details=True, **kw)


@pytest.fixture(scope="module")
def baseline():
    df = _frame()
    frame, info = _run(DistinctOracleEngine(), df)
    assert "distinct_rows" not in info and len(frame) > 20
    return df, frame, info


def _same(a, b):
    pd.testing.assert_frame_equal(a[0], b[0])
    assert a[1]["models"] == b[1]["models"]


def test_hook_trains_every_target_on_the_distinct_rows_and_changes_nothing(baseline):
    df, frame, info = baseline
    eng = DistinctOracleEngine()
    got = _run(eng, df, distinct_training_rows=dict(max_ratio=1.0))
    _same(got, (frame, info))
    d = got[1]["distinct_rows"]
    assert d["used_for"] == TARGETS and d["skipped"] == {} and d["rows"] == len(df) and 50 < d["distinct"] < len(df)
    assert eng.calls == 1 and sorted(eng.trained_on_distinct) == [1, 2, 4] and eng.closed == 1


def test_a_sampled_target_keeps_its_sample(baseline):
    df = baseline[0]
    pick = lambda a, rows: rows[::2] if a == "c2" else None   # noqa: E731
    off = _run(DistinctOracleEngine(), df, train_rows=pick)
    eng = DistinctOracleEngine()
    on = _run(eng, df, train_rows=pick, distinct_training_rows=dict(max_ratio=1.0))
    _same(on, off)
    d = on[1]["distinct_rows"]
    assert d["used_for"] == ["c1", "c4"] and list(d["skipped"]) == ["c2"] and "sample" in d["skipped"]["c2"]
    assert sorted(eng.trained_on_distinct) == [1, 4]


def test_a_search_keeps_the_whole_table(baseline):
    df = baseline[0]
    opts = {"model.hp.max_evals": "2", "model.cv.n_splits": "3", "model.hp.no_progress_loss": "1"}
    off = _run(DistinctOracleEngine(), df, search_opts=opts)
    eng = DistinctOracleEngine()
    on = _run(eng, df, search_opts=opts, distinct_training_rows=dict(max_ratio=1.0))
    _same(on, off)
    d = on[1]["distinct_rows"]
    assert d["used_for"] == [] and sorted(d["skipped"]) == TARGETS and all("search" in w for w in d["skipped"].values())
    assert eng.calls == 0 and eng.trained_on_distinct == [] and d["distinct"] is None


@pytest.mark.parametrize("small,ratio,word", [(100000, 1.0, "batched trainer"), (300, 1.0, "batched trainer"), (50, 0.05, "max_ratio")])
def test_small_tables_and_tables_of_mostly_distinct_rows_keep_the_whole_table(baseline, small, ratio, word):
    df, frame, info = baseline
    eng = DistinctOracleEngine(small=small)
    on = _run(eng, df, distinct_training_rows=dict(max_ratio=ratio))
    _same(on, (frame, info))
    d = on[1]["distinct_rows"]
    assert d["used_for"] == [] and sorted(d["skipped"]) == TARGETS and all(word in w for w in d["skipped"].values())
    assert eng.trained_on_distinct == []
    if small == 100000:
        assert eng.calls == 0                                  # N <= small_rows: nothing is computed
    else:
        assert eng.calls == 1 and eng.closed == 1 and small < d["rows"] and (d["distinct"] <= small or d["distinct"] > ratio * d["rows"])


def test_an_engine_without_distinct_rows_keeps_the_whole_table(baseline):
    df, frame, info = baseline
    on = _run(NoDistinctEngine(), df, distinct_training_rows=dict(max_ratio=1.0))
    _same(on, (frame, info))
    d = on[1]["distinct_rows"]
    assert d["used_for"] == [] and all("no distinct_rows" in w for w in d["skipped"].values()) and sorted(d["skipped"]) == TARGETS


@pytest.mark.parametrize("params,word", [(dict(bagging_fraction=0.5, bagging_freq=1), "bagging"), (dict(max_depth=9), "level grower")])
def test_parameters_the_variant_cannot_honour_keep_the_whole_table(baseline, params, word):
    df = baseline[0]
    off = _run(DistinctOracleEngine(), df, params=params)
    eng = DistinctOracleEngine()
    on = _run(eng, df, params=params, distinct_training_rows=dict(max_ratio=1.0))
    _same(on, off)
    d = on[1]["distinct_rows"]
    assert d["used_for"] == [] and all(word in w for w in d["skipped"].values()) and eng.calls == 0


def test_repair_model_option_reaches_the_pipeline(baseline, oracle_backend):
    from repair.errors import NullErrorDetector
    df = baseline[0]

    def model(on):
        m = RepairModel().setInput(df).setRowId("tid").setTargets(TARGETS).setErrorDetectors([NullErrorDetector()])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2", "model.max_training_row_num": "100000",
                     "model.train.distinct_rows": "true" if on else "false", "model.train.distinct_rows.max_ratio": "1.0"}.items():
            m = m.option(k, v)
        m._engine_override = DistinctOracleEngine()
        return m

    a, b = model(False), model(True)
    fa, fb = a.run(), b.run()
    assert a._last_resident_info is not None and "distinct_rows" not in a._last_resident_info
    d = b._last_resident_info["distinct_rows"]
    assert d["used_for"] and not d["skipped"] and b._engine_override.trained_on_distinct
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(fa.sort_values(key).reset_index(drop=True), fb.sort_values(key).reset_index(drop=True))
    assert a._last_resident_info["models"] == b._last_resident_info["models"]


class RefusingEngine(DistinctOracleEngine):
    """The trainer refuses the distinct table for some targets with RGBM_ERR_PARAM, as rgbm_table_train does for a fit whose bins cannot carry
    the multiplicity (17 to 31 features that do not fit the one-pass forms); `other` raises something else instead."""

    def __init__(self, refuse, code=-2):
        DistinctOracleEngine.__init__(self)
        self.refuse, self.code = set(refuse), code

    def train(self, table, target, feats, class_weight, params, y_value=None, want_stats=False):
        if getattr(table, "inverse", None) is not None and int(target) in self.refuse:
            e = RuntimeError("rgbm_table_train failed (%d): a two-chunk table with row multiplicities needs the one-pass level form" % self.code)
            e.code = self.code
            raise e
        return DistinctOracleEngine.train(self, table, target, feats, class_weight, params, y_value=y_value, want_stats=want_stats)


def test_a_fit_the_trainer_refuses_on_the_distinct_table_trains_on_the_whole_table(baseline):
    df, frame, info = baseline
    eng = RefusingEngine([2, 4])
    on = _run(eng, df, distinct_training_rows=dict(max_ratio=1.0))
    _same(on, (frame, info))
    d = on[1]["distinct_rows"]
    assert d["used_for"] == ["c1"] and sorted(d["skipped"]) == ["c2", "c4"] and all("one-pass level form" in w for w in d["skipped"].values())
    assert eng.trained_on_distinct == [1] and eng.closed == 1
    with pytest.raises(RuntimeError, match="rgbm_table_train failed"):           # any other failure of a fit surfaces as before
        _run(RefusingEngine([2], code=-11), df, distinct_training_rows=dict(max_ratio=1.0))
