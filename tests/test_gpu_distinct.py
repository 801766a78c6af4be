"""-m gpu: rgbm_table_distinct_rows (`_native.Table.distinct_rows`), the pipeline hook `distinct_training_rows` and the option
`model.train.distinct_rows` on the HIP engine.

1. the entry equals its numpy restatement (tests/distinct_restatement.py) -- codes, multiplicities, inverse, row count, inherited column kinds
   and values -- at the wave and 4096-row tile edges, for keys of one and of several words, and for the duplicate structures that stress it;
2. training on `Table.distinct_rows()` gives byte for byte the whole table's model and the host-dedup table's (tests/test_gpu_multiplicity.py);
3. `repair_frame` and `RepairModel.run()` with the hook on end with the frames and models of the hook off;
4. parameters the multiplicity trainer cannot honour fall back to the whole table inside the pipeline.
Every comparison is of exact integers or bytes.  Reference semantics pinned: the models of python/repair/model.py:768-815 (every row)."""
import numpy as np
import pandas as pd
import pytest

from tests import distinct_restatement as DR
from tests.synth import make_table, balanced_weights

pytestmark = pytest.mark.gpu


def _read(tab):
    return np.stack([tab.read_column(c) for c in range(tab.c)])


def _check(codes, cards):
    """distinct_rows() of the uploaded table against the restatement; returns (distinct table, restated codes)."""
    from repair import _native as N
    codes = np.ascontiguousarray(codes, np.int32)
    tab = N.Table(codes, cards)
    d, inv = tab.distinct_rows(want_inverse=True)
    dist, mult, rinv = DR.distinct_rows(codes)
    assert d.n == dist.shape[1] and d.c == codes.shape[0]
    assert np.array_equal(d.n_codes, np.asarray(cards, np.int32))
    assert np.array_equal(_read(d), dist)
    assert np.array_equal(d.row_multiplicity(), mult)
    assert np.array_equal(inv, rinv)
    assert np.array_equal(_read(tab), codes)                      # the source is untouched and carries no multiplicities
    assert (tab.row_multiplicity() == 1).all()
    return d, dist


def _pooled(rng, n, cards, null_ratio=0.0):
    """n rows drawn from a pool of n // 3 + 1 random rows: most rows occur more than once."""
    cards = np.asarray(cards, np.int32)
    pool = np.stack([rng.integers(0, k, n // 3 + 1) for k in cards]).astype(np.int32)
    if null_ratio:
        pool[rng.random(pool.shape) < null_ratio] = -1
    return np.ascontiguousarray(pool[:, rng.integers(0, pool.shape[1], n)]), cards


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 12289])
def test_entry_equals_restatement_at_the_wave_and_tile_edges(n):
    rng = np.random.default_rng(1000 + n)
    _check(*_pooled(rng, n, [5]))                                                        # C = 1
    for ratio in (0.01, 0.3):                                                            # C = 3 with NULLs
        codes, cards = _pooled(rng, n, [3, 2, 4], null_ratio=ratio)
        if n >= 2:
            codes[:, 0], codes[:, n - 1] = [1, -1, 2], [-1, 1, 2]                        # differ only in which cell is NULL
        _check(codes, cards)
    _check(*_pooled(rng, n, [2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 2, 3, 4, 6, 8], null_ratio=0.02))    # C = 16: a one-word key
    _check(*_pooled(rng, n, [1000] * 12, null_ratio=0.02))                               # C = 12 x 1000 codes: two words
    _check(*_pooled(rng, n, [2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64] * 3, null_ratio=0.02))   # C = 33: two words
    _check(*_pooled(rng, n, [1000] * 33, null_ratio=0.02))                               # C = 33 x 1000 codes: six words


def test_all_rows_distinct():
    n = 200000
    i = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(3)
    codes = np.stack([i % 1000, i // 1000, np.zeros(n, np.int64)]).astype(np.int32)[:, rng.permutation(n)]
    d, _ = _check(codes, [1000, 200, 1])
    assert d.n == n


def test_all_rows_identical():
    n = 70000
    codes = np.tile(np.array([[3], [-1], [0], [7]], np.int32), (1, n))
    d, _ = _check(codes, [4, 2, 1, 8])
    assert d.n == 275 and d.row_multiplicity().tolist() == [255] * 274 + [130]


def test_groups_at_the_edges_of_the_split_interleaved():
    rng = np.random.default_rng(17)
    sizes = [1, 254, 255, 256, 510, 511] * 7
    gid = np.repeat(np.arange(len(sizes)), sizes)[rng.permutation(sum(sizes))]
    codes = np.stack([gid % 6, gid // 6, np.where(gid % 5 == 0, -1, 1)]).astype(np.int32)
    d, dist = _check(codes, [6, 7, 2])
    assert d.n == sum((s + 254) // 255 for s in sizes)


def test_a_block_repeated_four_times():
    rng = np.random.default_rng(29)
    block, cards = _pooled(rng, 6001, [16, 24, 3, 48], null_ratio=0.05)
    codes = np.ascontiguousarray(np.tile(block, (1, 4)))
    from repair import _native as N
    d, dist = _check(codes, cards)
    _, inv = N.Table(codes, cards).distinct_rows(want_inverse=True)
    assert np.array_equal(inv[:6001], inv[6001:12002]) and np.array_equal(inv[:6001], inv[18003:])
    assert d.n == len(np.unique(inv))                             # no group passes 255 rows here: one copy each


def test_column_kinds_and_values_are_inherited():
    """Kinds and values have no reader; each is shown to change the whole table's model on its own, and the distinct table's model must equal
    the whole table's under each."""
    from repair import _native as N
    dirty, _, cards = make_table(30000, 6, seed=41, null_ratio=0.01)
    dirty[3][dirty[3] == 5] = 4            # a category no row holds: missing for the model of a CATEGORICAL column
    dirty[4][dirty[4] == 3] = 2            # a value no row holds, next to its upper neighbour in value and midway in rank: another bin bound
    values = np.array([0, 1, 2, 9.9, 10, 11, 12, 13], np.float64)
    t, feats = 1, [0, 2, 3, 4, 5]
    kw = dict(objective=1, num_class=int(cards[t]), class_weight=balanced_weights(dirty[t], int(cards[t])), n_estimators=3, learning_rate=0.2)

    def table(kind, vals):
        tab = N.Table(dirty, cards)
        if kind:
            tab.set_column_kind(3, True)
        if vals:
            tab.set_column_values(4, values)
        return tab
    plain = table(False, False).train(t, feats, **kw).save()
    for kind, vals in ((True, False), (False, True), (True, True)):
        whole = table(kind, vals).train(t, feats, **kw).save()
        assert whole != plain, (kind, vals)
        assert table(kind, vals).distinct_rows().train(t, feats, **kw).save() == whole, (kind, vals)


def test_a_table_that_carries_multiplicities_is_refused():
    from repair import _native as N
    dirty, _, cards = make_table(5000, 4, seed=43)
    d = N.Table(dirty, cards).distinct_rows()
    with pytest.raises(N.RepairGbmError) as e:
        d.distinct_rows()
    assert e.value.code == -2                                                            # RGBM_ERR_PARAM
    d.set_row_multiplicity(None)
    assert d.distinct_rows().n == d.n


def test_models_of_the_distinct_table_equal_the_whole_tables_byte_for_byte():
    from repair import _native as N
    from repair.pipeline import distinct_rows
    dirty, _, cards = make_table(100000, 8, seed=97, null_ratio=0.01)
    dirty = np.ascontiguousarray(np.concatenate([dirty, dirty[:, :9000], np.repeat(dirty[:, :3], 400, axis=1)], axis=1))
    whole = N.Table(dirty, cards)
    dev = N.Table(dirty, cards).distinct_rows()
    dist, mult, inv = distinct_rows(dirty, cards)
    host = N.Table(dist, cards)
    host.set_row_multiplicity(mult)
    assert dev.n == host.n < dirty.shape[1] and int(dev.row_multiplicity().astype(np.int64).sum()) == dirty.shape[1]
    for t in (0, 7):                                              # K = 2 and K = 24
        K, feats = int(cards[t]), [c for c in range(8) if c != t]
        kw = dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=balanced_weights(dirty[t], K), n_estimators=5, learning_rate=0.2)
        a = whole.train(t, feats, **kw).save()
        assert dev.train(t, feats, **kw).save() == a, t
        assert host.train(t, feats, **kw).save() == a, t


# ---- through the pipeline -----------------------------------------------------------------------------------------------------------
def _frame(n=100000, base=76000, seed=31):
    """n rows of which the last n - base repeat the first ones; four independent columns keep most base rows distinct (more distinct rows than
    the batched trainer takes), NULL cells in every column."""
    dirty, _, cards = make_table(base, 8, seed=seed, null_ratio=0.01)
    rng = np.random.default_rng(seed)
    for c in (4, 5, 6, 7):
        v = rng.integers(0, cards[c], base).astype(np.int32)
        v[dirty[c] < 0] = -1
        dirty[c] = v
    dirty = np.concatenate([dirty, dirty[:, :n - base]], axis=1)
    df = pd.DataFrame({"tid": np.arange(n)})
    for c in range(8):
        names = np.array([None] + ["v%02d" % v for v in range(int(cards[c]))], object)
        df["c%d" % c] = names[dirty[c] + 1]
    return df


TARGETS = ["c0", "c1", "c3"]
PARAMS = dict(n_estimators=5, learning_rate=0.2, num_leaves=31, max_depth=7)


@pytest.fixture(scope="module")
def frame_and_baseline():
    from repair.engine import HipEngine
    from repair.pipeline import repair_frame
    df = _frame()
    off = repair_frame(HipEngine(), df, "tid", targets=TARGETS, base_params=PARAMS, want_details=True)
    assert len(off[0]) > 1000 and "distinct_rows" not in off[1]
    return df, off


def test_repair_frame_with_the_hook_equals_the_hook_off(frame_and_baseline):
    from repair.engine import HipEngine
    from repair.pipeline import repair_frame
    df, (frame, info) = frame_and_baseline
    got, ginfo = repair_frame(HipEngine(), df, "tid", targets=TARGETS, base_params=PARAMS, want_details=True,
                              distinct_training_rows=dict(max_ratio=1.0))
    d = ginfo["distinct_rows"]
    print("distinct rows:", d)
    assert d["used_for"] == TARGETS and not d["skipped"] and d["rows"] == len(df) and HipEngine.small_rows() < d["distinct"] < len(df)
    pd.testing.assert_frame_equal(got, frame)
    assert ginfo["models"] == info["models"]


def test_repair_model_run_with_the_option_equals_the_option_off(frame_and_baseline):
    from repair.errors import NullErrorDetector
    from repair.model import RepairModel
    df = frame_and_baseline[0]

    def model(on):
        m = RepairModel().setInput(df).setRowId("tid").setTargets(TARGETS).setErrorDetectors([NullErrorDetector()])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "5", "model.lgb.learning_rate": "0.2",
                     "model.max_training_row_num": "200000", "model.train.distinct_rows": "true" if on else "false",
                     "model.train.distinct_rows.max_ratio": "1.0"}.items():
            m = m.option(k, v)
        return m

    a, b = model(False), model(True)
    fa, fb = a.run(), b.run()
    assert a._last_resident_info is not None and "distinct_rows" not in a._last_resident_info
    d = b._last_resident_info["distinct_rows"]
    print("distinct rows:", d)
    assert d["used_for"] == TARGETS and not d["skipped"]
    key = ["tid", "attribute"]
    assert len(fa) > 1000
    pd.testing.assert_frame_equal(fa.sort_values(key).reset_index(drop=True), fb.sort_values(key).reset_index(drop=True))
    assert a._last_resident_info["models"] == b._last_resident_info["models"]


def test_parameters_the_variant_cannot_honour_fall_back_to_the_whole_table(frame_and_baseline):
    from repair.engine import HipEngine
    from repair.pipeline import repair_frame
    df = frame_and_baseline[0]
    params = dict(PARAMS, bagging_fraction=0.5, bagging_freq=1)
    off = repair_frame(HipEngine(), df, "tid", targets=["c0"], base_params=params, want_details=True)
    on = repair_frame(HipEngine(), df, "tid", targets=["c0"], base_params=params, want_details=True, distinct_training_rows=dict(max_ratio=1.0))
    d = on[1]["distinct_rows"]
    assert d["used_for"] == [] and "bagging" in d["skipped"]["c0"]
    pd.testing.assert_frame_equal(on[0], off[0])
    assert on[1]["models"] == off[1]["models"]


def test_a_fit_the_trainer_refuses_on_the_distinct_table_falls_back_inside_the_pipeline():
    """20 columns of 20 values: 19 features in two chunks that do not pack into 15 joint-bin groups, so rgbm_table_train refuses the distinct
    table's multiplicities (RGBM_ERR_PARAM); the run must train that target on the whole table and say so."""
    from repair import _native as N
    from repair.engine import HipEngine
    from repair.pipeline import repair_frame
    rng = np.random.default_rng(61)
    base, n = 70000, 80000
    codes = rng.integers(0, 20, (20, base)).astype(np.int32)
    codes[1] = (codes[2] + codes[3]) % 20
    codes = np.concatenate([codes, codes[:, :n - base]], axis=1)
    names = np.array([None] + ["v%02d" % v for v in range(20)], object)
    df = pd.DataFrame({"tid": np.arange(n)})
    for c in range(20):
        col = codes[c].copy()
        if c == 1:
            col[rng.random(n) < 0.01] = -1
        df["c%02d" % c] = names[col + 1]
    tab = N.Table(codes, [20] * 20).distinct_rows()
    with pytest.raises(N.RepairGbmError) as e:                                           # the premise: the trainer refuses this fit
        tab.train(1, [c for c in range(20) if c != 1], objective=1, num_class=20, n_estimators=1)
    assert e.value.code == -2
    params = dict(PARAMS, n_estimators=3)
    off = repair_frame(HipEngine(), df, "tid", targets=["c01"], base_params=params, want_details=True)
    on = repair_frame(HipEngine(), df, "tid", targets=["c01"], base_params=params, want_details=True, distinct_training_rows=dict(max_ratio=1.0))
    d = on[1]["distinct_rows"]
    print("distinct rows:", d)
    assert d["used_for"] == [] and "refused" in d["skipped"]["c01"] and d["distinct"] > HipEngine.small_rows()
    assert len(off[0]) > 500
    pd.testing.assert_frame_equal(on[0], off[0])
    assert on[1]["models"] == off[1]["models"]
