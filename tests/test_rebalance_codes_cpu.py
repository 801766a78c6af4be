"""CPU: rebalancing in code space (`repair.rebalance_codes`) against the value-space statement (`repair.train.rebalance_training_data`),
and the case generators of tests/test_gpu_rebalance.py held to their purpose on the statement alone."""
import logging

import numpy as np
import pandas as pd
import pytest

from tests import rebalance_cases as RC
from tests.helpers import csrc_constant

from repair.rebalance_codes import check_dictionary_order, rebalance_plan, rebalanced_codes, smoten_codes  # noqa: E402
from repair.train import rebalance_training_data, smoten_resample  # noqa: E402


def _code_space(X, y, train_rows=None):
    codes, n_codes, dicts, cols = RC.encode(X, y)
    c = len(cols)
    rows = np.arange(codes.shape[1]) if train_rows is None else np.asarray(train_rows, np.int64)
    feats = list(range(c - 1))
    plan = rebalance_plan(codes[c - 1, rows], (codes[:c - 1, rows] < 0).any(axis=0), target="t", class_names=dicts[c - 1])
    return RC.decode(rebalanced_codes(codes, n_codes, c - 1, feats, rows, plan), dicts), plan


def _same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = [(i, j, got[i, j], want[i, j]) for i in range(got.shape[0]) for j in range(got.shape[1]) if got[i, j] != want[i, j]]
    assert not bad, "%d cells differ, e.g. %s" % (len(bad), bad[:5])


@pytest.mark.parametrize("name", sorted(RC.VALUE_FRAMES))
def test_code_space_gives_the_value_space_rows_in_order(name):
    X, y = RC.VALUE_FRAMES[name]()
    Xr, yr = rebalance_training_data(X.copy(), y.copy(), "t")
    got, plan = _code_space(X, y)
    _same(got, RC.frame_values(Xr, yr))
    hist = y.value_counts()
    median = int(np.median(hist.values))
    assert plan["median"] == median
    assert bool(len(plan["classes"])) == (name not in ("balanced", "none_below", "too_few_clean"))
    if name == "none_above":
        assert (plan["order"] == np.arange(len(plan["order"]))).all() and len(plan["classes"]) == 1
    if name == "none_below":
        assert len(got) == 3 * median and len(plan["picks"]) == 0


def test_too_few_clean_rows_warns_like_the_value_space(caplog):
    X, y = RC.too_few_clean_rows_frame()
    with caplog.at_level(logging.WARNING):
        _, plan = _code_space(X, y)
    msgs = [r.getMessage() for r in caplog.records if "Over-sampling of" in r.getMessage()]
    assert sorted(msgs) == ["Over-sampling of 'c' in y='t' failed because the number of the clean rows is too small: 4",
                            "Over-sampling of 'd' in y='t' failed because the number of the clean rows is too small: 5"]
    assert len(plan["classes"]) == 0


def test_the_samplers_shuffled_order_is_the_frames():
    """Above `model.max_training_row_num` the value-space frame holds the sample in the sampler's order (`DataFrame.sample(n,
    random_state=42)`); the resident sampler draws the same positions (`RepairModel._training_row_sampler`): the plan takes them unsorted."""
    X, y = RC.four_class_frame(seed=4, n=700)
    max_rows = 300
    df = pd.concat([X, y], axis=1)
    sample = df.sample(n=max_rows, random_state=42)
    rows = np.arange(len(df))[np.random.RandomState(42).choice(len(df), max_rows, replace=False)]
    assert sample.index.tolist() == rows.tolist() and not (np.diff(rows) > 0).all()
    Xr, yr = rebalance_training_data(sample[list(X.columns)], sample["t"], "t")
    got, _ = _code_space(X, y, train_rows=rows)
    _same(got, RC.frame_values(Xr, yr))
    with pytest.raises(AssertionError):                  # and the order matters: the sorted rows give another frame
        _same(_code_space(X, y, train_rows=np.sort(rows))[0], RC.frame_values(Xr, yr))


@pytest.mark.parametrize("seed,F,V,K", [(0, 3, 3, 3), (1, 15, 6, 16), (2, 5, 300, 4), (3, 7, 40, 66)])
def test_smoten_codes_is_smoten_resample_on_random_tables(seed, F, V, K):
    codes, n_codes = RC.random_table(seed, 260, [V] * F, K)
    X = pd.DataFrame({"f%02d" % j: codes[j].astype(object) for j in range(F)})
    y = pd.Series(codes[F], name="t")
    cnt = np.bincount(codes[F], minlength=K)
    grow = [c for c in range(K) if cnt[c] > 5][:3]
    targets = {c: int(cnt[c]) + 7 + c for c in grow}
    Xn, yn = smoten_resample(X, y, dict(targets), k_neighbors=5, random_state=42)
    res = smoten_codes(codes, n_codes, F, list(range(F)), np.arange(codes.shape[1]), targets)
    synth = np.concatenate([r["synth"] for r in res])
    assert [r["klass"] for r in res] == grow
    assert (Xn.iloc[len(X):].to_numpy().astype(np.int64) == synth[:, :F]).all() and (yn.iloc[len(X):].to_numpy() == synth[:, F]).all()


def test_the_tie_case_ties():
    codes, n_codes = RC.tie_table()
    m = int((codes[3] == 0).sum())
    assert 60 <= m <= 100
    assert RC.tie_share(codes, n_codes, 0, 5) >= 0.5


def test_the_identical_case_has_distance_zero_and_the_first_k_neighbours():
    codes, n_codes = RC.identical_table()
    assert RC.tie_share(codes, n_codes, 0, 5) == 1.0
    m = int((codes[3] == 0).sum())
    r, = smoten_codes(codes, n_codes, 3, [0, 1, 2], np.arange(codes.shape[1]), {0: m + 3})
    want = np.asarray([[j for j in range(7) if j != q][:5] for q in range(m)])
    assert (r["nn"] == want).all() and (r["synth"] == [1, 2, 0, 0]).all()


def test_the_large_v_case_straddles_the_table_limit():
    lim = csrc_constant("VDM_TABLE_CODES")
    codes, n_codes = RC.large_v_table(lim)
    assert (n_codes[:-1] > lim).any() and (n_codes[:-1] <= lim).any() and lim in n_codes[:-1] and lim + 1 in n_codes[:-1]
    assert all(len(np.unique(codes[j])) > min(n_codes[j], 2) - 1 for j in range(len(n_codes) - 1))
    assert len(np.unique(codes[0])) > lim // 2                      # the feature above the limit really holds that many codes


def test_mixed_type_dictionaries_are_refused():
    from repair.pipeline import NotResidentEligible
    check_dictionary_order(np.asarray(["a", "b", "c"], object))
    check_dictionary_order(np.asarray([0.5, 1.0, 7.0]))
    check_dictionary_order(np.asarray([1, 2, 10], object))
    with pytest.raises(NotResidentEligible, match="mixed types"):
        check_dictionary_order(np.asarray([1, "a", 2.5], object), "`f2`")
    with pytest.raises(NotResidentEligible, match="not in the order"):
        check_dictionary_order(np.asarray(["b", "a"], object))


def _run_model(df, engine, resident, **opts):
    from repair.errors import NullErrorDetector
    from repair.model import RepairModel
    m = RepairModel().setInput(df).setRowId("tid").setErrorDetectors([NullErrorDetector()]).setTargets(["y"])
    m = m.setTrainingDataRebalancingEnabled(True)
    for k, v in dict({"model.hp.max_evals": "1", "model.lgb.n_estimators": "10", "model.lgb.learning_rate": "0.2",
                      "model.rebalance.resident": "true" if resident else "false"}, **opts).items():
        m = m.option(k, str(v))
    m._engine_override = engine
    return m


@pytest.mark.parametrize("max_rows", [10000, 300])
def test_run_with_rebalancing_takes_the_resident_path_and_gives_the_same_cells(oracle_backend, max_rows):
    """`RepairModel.run()` with rebalancing on the oracle engine: `model.rebalance.resident` keeps the run on the resident path, and the
    cells are those of the value-space path (same arithmetic on both sides), with and without the row sample."""
    df = RC.skewed_run_frame()
    opts = {"model.max_training_row_num": max_rows}
    slow = _run_model(df, RC.oracle_engine(), False, **opts)
    a = slow.run()
    assert getattr(slow, "_last_resident_info", None) is None           # the option is opt-in: without it the run leaves the resident path
    fast = _run_model(df, RC.oracle_engine(), True, **opts)
    b = fast.run()
    info = getattr(fast, "_last_resident_info", None)
    assert info is not None, "the run did not take the resident path"
    assert info["rebalanced"]["y"]["synthetic"] > 0 and info["rebalanced"]["y"]["rows"] == 4 * info["rebalanced"]["y"]["median"]
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(a.sort_values(key).reset_index(drop=True), b.sort_values(key).reset_index(drop=True))
    assert len(a) >= 40


def test_a_multi_rank_job_keeps_the_value_space_path(oracle_backend, monkeypatch):
    """Rebalancing inside the row-sharded job is out of scope: the plan refuses it (the reason is logged) and `repair_table` would too."""
    from repair import dist
    from repair.pipeline import NotResidentEligible, repair_frame
    df = RC.skewed_run_frame()
    monkeypatch.setattr(dist, "world", lambda: (0, 2))
    m = _run_model(df, RC.oracle_engine(), True)
    assert m._resident_plan(df, ["y"], [], {"y": 4}, False, False) is None
    with pytest.raises(NotResidentEligible, match="multi-rank"):
        repair_frame(RC.oracle_engine(), df, "tid", targets=["y"], base_params=dict(n_estimators=2), rebalance=dict(k=5, random_state=42))


def test_the_distinct_row_variant_skips_rebalanced_targets_with_a_reason():
    from repair.pipeline import distinct_training_tables

    class Tab:
        n, c = 1000, 4

        def distinct_rows(self):
            raise AssertionError("no target qualifies")

    class Eng:
        def small_rows(self):
            return 10

    tabs = {0: object(), 1: object()}
    dtab, info = distinct_training_tables(Eng(), Tab(), [0, 1], dict(max_depth=7), dict(max_ratio=0.5), tabs, rebalanced={1: {}})
    assert dtab is None and info["skipped"] == {0: "trained on a row sample (train_rows)", 1: "trained on a rebalanced table (rebalance)"}
