"""-m gpu: the distinct-row view of rgbm_table_train (`_native.Table.train`).  The library deduplicates a table by itself and
trains every eligible fit on the distinct rows with multiplicities; the model must be the whole table's, byte for byte.

1. model bytes, view against RGBM_FLAG_WHOLE_TABLE, for every gradient kernel and record layout (one case also against the oracle);
2. every fallback returns the whole table's model without an error, and `distinct_view_info()` says what happened;
3. every kind of write to the table drops the view: the next fit equals a freshly uploaded table's;
4. six threads on one fresh table build the view once;
5. the statistics of a view fit count the rows its kernels streamed.
The tables are small, so the view is reached with RGBM_DISTINCT_MIN_ROWS=1.  Every comparison is of bytes or exact integers.
Reference semantics pinned: the models of python/repair/model.py:768-815 (every row)."""
import threading

import numpy as np
import pytest

from tests.synth import make_table, balanced_weights

pytestmark = pytest.mark.gpu

NE = 10
CARDS8 = [2, 5, 4, 6, 8, 12, 16, 24]
CARDS16 = CARDS8 + [3, 4, 2, 6, 3, 8, 2, 4]                               # 15 features
CARDS21 = CARDS8[:5] + [2, 3, 4, 2, 3, 4, 6, 2, 3, 4, 2, 3, 6, 2, 3, 4]   # 20 features: two chunks that take the one-pass form


@pytest.fixture(autouse=True)
def _reach_the_view(monkeypatch):
    monkeypatch.setenv("RGBM_DISTINCT_MIN_ROWS", "1")
    monkeypatch.delenv("RGBM_DISTINCT", raising=False)
    monkeypatch.delenv("RGBM_DISTINCT_MAX_RATIO", raising=False)


def _table(cards, seed, n=20000, pool=3000, big=1000):
    """n rows drawn from `pool` distinct ones, one of them `big` times (the 255-split), NULLs in every column."""
    rng = np.random.default_rng(seed)
    src, _, cards = make_table(pool, len(cards), seed=seed, null_ratio=0.02, cards=cards)
    idx = np.concatenate([rng.integers(0, pool, n - big), np.full(big, 7)])
    return np.ascontiguousarray(src[:, rng.permutation(idx)]), cards


def _kw(codes, cards, t, n_estimators=NE):
    K = int(cards[t])
    return dict(objective=0 if K == 2 else 1, num_class=max(K, 2), class_weight=balanced_weights(codes[t], K), n_estimators=n_estimators,
                learning_rate=0.2)


def _feats(c, t):
    return [j for j in range(c) if j != t]


def _view_rows(codes, t):
    """Training rows of the view: distinct rows with a label, a group of cnt rows kept as ceil(cnt / 255) copies."""
    _, cnt = np.unique(codes[:, codes[t] >= 0], axis=1, return_counts=True)
    return int(((cnt + 254) // 255).sum())


def _train_both(tab, codes, cards, t, **over):
    """(model through the default path, its stats, model under RGBM_FLAG_WHOLE_TABLE)"""
    kw = dict(_kw(codes, cards, t), **over)
    feats = _feats(len(cards), t)
    m, st = tab.train(t, feats, want_stats=True, **kw)
    w = tab.train(t, feats, whole_table=True, **kw)
    return m.save(), st, w.save()


@pytest.mark.parametrize("cards,t", [(CARDS8, 0), (CARDS8, 1), (CARDS8, 7), (CARDS16, 1), (CARDS21, 1)],
                         ids=["K2", "K5", "K24", "K5-15-features", "K5-20-features"])
def test_model_through_the_view_equals_the_whole_tables(cards, t):
    from repair import _native as N
    codes, cards = _table(cards, seed=200 + len(cards))
    tab = N.Table(codes, cards)
    got, st, whole = _train_both(tab, codes, cards, t)
    info = tab.distinct_view_info()
    print("view:", info, "root_rows", st["root_rows"])
    assert info["state"] == "built" and info["builds"] == 1 and info["rows"] < codes.shape[1] // 2
    K = 1 if int(cards[t]) == 2 else int(cards[t])
    assert st["root_rows"] == NE * K * _view_rows(codes, t)          # the fit did stream the view, not the table
    assert got == whole
    if (len(cards), t) == (8, 1):
        from oracle import oracle as O
        feats, rows = _feats(8, t), codes[t] >= 0
        kw = _kw(codes, cards, t)
        ref = O.train(np.ascontiguousarray(codes[feats][:, rows]), cards[feats], codes[t][rows], int(cards[t]), **kw)
        assert got == ref.save()


def _whole_rows(codes, t, K, ne):
    return ne * K * int((codes[t] >= 0).sum())


def test_fallbacks_return_the_whole_tables_model(monkeypatch):
    from repair import _native as N
    codes, cards = _table(CARDS8, seed=31)
    n = codes.shape[1]

    # all rows distinct: one pass, "not worth it", no table kept
    i = np.arange(n)
    uniq = codes.copy()
    uniq[5], uniq[6], uniq[7] = i % 12, (i // 12) % 16, (i // 192) % 24
    uniq[4] = (i // 4608) % 8
    tab = N.Table(uniq, cards)
    got, st, whole = _train_both(tab, uniq, cards, 1, n_estimators=3)
    assert got == whole and st["root_rows"] == _whole_rows(uniq, 1, 5, 3)
    assert tab.distinct_view_info() == {"state": "not worth it", "rows": n, "builds": 1}
    tab.train(0, _feats(8, 0), **_kw(uniq, cards, 0, 2))
    assert tab.distinct_view_info()["builds"] == 1                    # decided without a second pass

    # 16 features: no free byte in the record
    c17, k17 = _table(CARDS16 + [3], seed=32)
    tab = N.Table(c17, k17)
    got, st, whole = _train_both(tab, c17, k17, 1, n_estimators=3)
    assert got == whole and st["root_rows"] == _whole_rows(c17, 1, 5, 3)
    assert tab.distinct_view_info() == {"state": "none", "rows": 0, "builds": 0}

    # bagging; a regression target
    tab = N.Table(codes, cards)
    got, st, whole = _train_both(tab, codes, cards, 1, n_estimators=3, bagging_fraction=0.5, bagging_freq=1)
    assert got == whole and tab.distinct_view_info()["builds"] == 0
    reg = dict(objective=2, n_estimators=3, learning_rate=0.2)
    yv = np.arange(int(cards[3]), dtype=np.float64) * 1.5
    a = tab.train(3, _feats(8, 3), y_value=yv, **reg).save()
    assert a == tab.train(3, _feats(8, 3), y_value=yv, whole_table=True, **reg).save() and tab.distinct_view_info()["builds"] == 0

    # RGBM_DISTINCT=0
    monkeypatch.setenv("RGBM_DISTINCT", "0")
    got, st, whole = _train_both(tab, codes, cards, 1, n_estimators=3)
    assert got == whole and st["root_rows"] == _whole_rows(codes, 1, 5, 3) and tab.distinct_view_info()["state"] == "none"
    monkeypatch.delenv("RGBM_DISTINCT")

    # a table with multiplicities of its own
    own = N.Table(codes, cards).distinct_rows()
    a = own.train(1, _feats(8, 1), **_kw(codes, cards, 1, 3)).save()
    assert a == whole and own.distinct_view_info() == {"state": "none", "rows": 0, "builds": 0}


def test_a_fit_the_trainer_refuses_on_the_view_trains_the_whole_table():
    """20 columns of 20 values: 19 features in two chunks that do not pack into 15 joint-bin groups.  The view is built, the multiplicity trainer
    refuses it (RGBM_ERR_PARAM on the distinct table itself), and the same call returns the whole table's model."""
    from repair import _native as N
    rng = np.random.default_rng(61)
    base = rng.integers(0, 20, (20, 3000)).astype(np.int32)
    base[1] = (base[2] + base[3]) % 20
    codes = np.ascontiguousarray(base[:, rng.integers(0, 3000, 20000)])
    codes[1][rng.random(20000) < 0.01] = -1
    cards = np.full(20, 20, np.int32)
    kw = dict(objective=1, num_class=20, n_estimators=2, learning_rate=0.2)
    with pytest.raises(N.RepairGbmError) as e:                        # the premise
        N.Table(codes, cards).distinct_rows().train(1, _feats(20, 1), **kw)
    assert e.value.code == -2
    tab = N.Table(codes, cards)
    m, st = tab.train(1, _feats(20, 1), want_stats=True, **kw)
    assert tab.distinct_view_info()["state"] == "built" and tab.distinct_view_info()["builds"] == 1
    assert st["root_rows"] == _whole_rows(codes, 1, 20, 2)
    assert m.save() == tab.train(1, _feats(20, 1), whole_table=True, **kw).save()
    m2 = tab.train(2, _feats(20, 2), **kw)                            # another target of the same shape: straight to the whole table
    assert m2.save() == tab.train(2, _feats(20, 2), whole_table=True, **kw).save()
    assert tab.distinct_view_info()["builds"] == 1


def test_every_write_drops_the_view():
    from repair import _native as N
    codes, cards = _table(CARDS8, seed=77)
    t, feats = 1, _feats(8, 1)
    tab = N.Table(codes, cards)

    def fresh(c, kind=False):
        f = N.Table(c, cards)
        if kind:
            f.set_column_kind(3, True)
        return f.train(t, feats, whole_table=True, **_kw(c, cards, t)).save()

    def current():
        return np.stack([tab.read_column(c) for c in range(8)])

    assert tab.train(t, feats, **_kw(codes, cards, t)).save() == fresh(codes)
    assert tab.distinct_view_info()["state"] == "built"

    # write_cells: two equal rows now differ, and a label changes
    _, inv, cnt = np.unique(codes, axis=1, return_inverse=True, return_counts=True)
    rows = np.flatnonzero(np.ravel(inv) == cnt.argmax())
    assert len(rows) >= 1000
    r0, r1 = int(rows[0]), int(rows[1])
    new_feat = (int(codes[4][r1]) + 1) % int(cards[4])
    new_lab = (max(int(codes[t][r0]), 0) + 1) % int(cards[t])
    tab.write_cells([r1, r0], [4, t], [new_feat, new_lab])
    assert tab.distinct_view_info()["state"] == "none"
    c1 = codes.copy()
    c1[4][r1], c1[t][r0] = new_feat, new_lab
    assert np.array_equal(current(), c1)
    assert tab.train(t, feats, **_kw(c1, cards, t)).save() == fresh(c1)
    assert tab.distinct_view_info() == dict(tab.distinct_view_info(), state="built", builds=2)

    # repair_chain fills the NULL cells of a feature column
    m2 = tab.train(4, _feats(8, 4), **_kw(c1, cards, 4, 3))
    tab.repair_chain([m2], [4], [_feats(8, 4)])
    assert tab.distinct_view_info()["state"] == "none"
    c2 = current()
    assert (c2[4] >= 0).all() and (c1[4] < 0).any()
    assert tab.train(t, feats, **_kw(c2, cards, t)).save() == fresh(c2)
    assert tab.distinct_view_info()["state"] == "built"

    # a column's kind
    c3 = c2.copy()
    gone = c3[3] == 5
    assert gone.any()
    tab.write_cells(np.flatnonzero(gone), np.full(int(gone.sum()), 3), np.full(int(gone.sum()), 4))   # a category no row holds
    c3[3][gone] = 4
    plain = tab.train(t, feats, **_kw(c3, cards, t)).save()
    assert plain == fresh(c3) and tab.distinct_view_info()["state"] == "built"
    tab.set_column_kind(3, True)
    assert tab.distinct_view_info()["state"] == "none"
    kinded = tab.train(t, feats, **_kw(c3, cards, t)).save()
    assert kinded == fresh(c3, kind=True) and kinded != plain


def test_six_threads_build_one_view():
    from repair import _native as N
    codes, cards = _table(CARDS8, seed=55)
    targets = [0, 1, 2, 3, 4, 7]
    seq_tab = N.Table(codes, cards)
    seq = [seq_tab.train(t, _feats(8, t), **_kw(codes, cards, t, 5)).save() for t in targets]
    tab = N.Table(codes, cards)
    out, errs = [None] * 6, []
    gate = threading.Barrier(6)

    def work(i):
        try:
            gate.wait()
            out[i] = tab.train(targets[i], _feats(8, targets[i]), **_kw(codes, cards, targets[i], 5)).save()
        except Exception as e:              # noqa: BLE001 -- reported below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    info = tab.distinct_view_info()
    assert info["state"] == "built" and info["builds"] == 1
    assert out == seq


def test_statistics_count_the_rows_streamed():
    from repair import _native as N
    codes, cards = _table(CARDS8, seed=91)
    tab = N.Table(codes, cards)
    for t in (0, 7):
        K = 1 if int(cards[t]) == 2 else int(cards[t])
        kw = _kw(codes, cards, t)
        _, st = tab.train(t, _feats(8, t), want_stats=True, **kw)
        _, sw = tab.train(t, _feats(8, t), want_stats=True, whole_table=True, **kw)
        mv, mw = _view_rows(codes, t), int((codes[t] >= 0).sum())
        assert st["root_rows"] == NE * K * mv and sw["root_rows"] == NE * K * mw
        assert st["root_rows"] <= st["hist_rows"] < sw["hist_rows"]
        assert st["hist_bytes"] == st["hist_rows"] * (7 + 8)
