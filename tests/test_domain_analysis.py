"""CPU: the cell-domain analysis of the reference's ErrorModel.detect re-stated in repair.domain (RepairApi.scala:231-675) -- the golden
rows of the reference's own suite (tests/golden/domain_analysis.json), the kept CONCAT-NULL quirk, tau's integer division, the literal
exp(ln + ln) formula, and `RepairModel.run()` with `error.domain_analysis.enabled` on both paths."""
import json
import os

import numpy as np
import pandas as pd
import pytest

from repair.errors import ConstraintErrorDetector, ErrorModel, NullErrorDetector
from repair.model import RepairModel
from tests.helpers import OracleEngine

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "domain_analysis.json")))
SPELLINGS = [("tid", "xx", "yy", "zz"), ("t i d", "x x", "y y", "z z")]


def _codes(rows, ncol):
    """Value rows -> (codes [ncol][n] int32, dictionaries): ascending distinct values, None = NULL."""
    dicts, codes = [], []
    for j in range(ncol):
        v = [r[j + 1] for r in rows]
        d = sorted({str(x) for x in v if x is not None})
        dicts.append(d)
        codes.append([d.index(str(x)) if x is not None else -1 for x in v])
    return np.asarray(codes, np.int32), dicts


@pytest.mark.parametrize("thr, key", [(0.0, "freq_rows_0.0"), (0.3, "freq_rows_0.3")])
@pytest.mark.parametrize("names", SPELLINGS)
def test_frequency_rows_of_the_reference_suite(thr, key, names):
    from repair import domain as D
    codes, dicts = _codes(GOLD["freq_input"], 2)
    x, y = names[1], names[2]
    view = D.discretised_view([3, 4], [3, 4], {}, 80)
    be = D.HostBackend(codes, view)
    tab = D.PairTable([(0, 1)], be.pair_counts([(0, 1)]))
    rows = D.freq_rows([x, y], {x: dicts[0], y: dicts[1]}, {x: tab.single(0), y: tab.single(1)}, {(x, y): tab.get(0, 1)},
                       min_count=D.freq_min_count(9, thr))
    assert sorted(map(repr, rows)) == sorted(repr(tuple(r)) for r in GOLD[key])


def test_pairwise_stats_without_any_frequency_row():
    from repair import domain as D
    st = D.pairwise_stats(1000, [("x", "y"), ("y", "x")], {frozenset(("x", "y")): []}, {"x": [], "y": []}, {"tid": 9, "x": 2, "y": 4})
    assert st == {"x": [("y", 1.0)], "y": [("x", 2.0)]}            # the worst-case values, exactly


@pytest.mark.parametrize("names", SPELLINGS)
def test_pairwise_stats_on_the_given_frequency_table(names):
    from repair import domain as D
    x, y = names[1], names[2]
    st = D.stats_from_rows([x, y], GOLD["pairwise_freq_rows"])
    jt = st["joint"][(x, y)]
    out = D.pairwise_stats(9, [(x, y), (y, x)], {frozenset((x, y)): jt.cnt}, {a: s[s > 0] for a, s in st["single"].items()}, {names[0]: 9, x: 3, y: 4})
    assert set(out) == {x, y}
    assert [a for a, _ in out[x]] == [y] and out[x][0][1] > 0.0
    assert [a for a, _ in out[y]] == [x] and out[y][0][1] > 0.0


@pytest.mark.parametrize("names", SPELLINGS)
def test_attr_stats_inequalities(names):
    """computeAttrStats (RepairSuite.scala:367-427): H <= 1 with every group kept, and dropping every group (threshold 1.0) makes it larger."""
    from repair import domain as D
    codes, _ = _codes(GOLD["freq_input"], 2)
    view = D.discretised_view([3, 4], [3, 4], {}, 80)

    def run(thr):
        opts = {"error.attr_freq_ratio_threshold": thr, "error.pairwise_freq_ratio_threshold": 1.0, "error.max_attrs_to_compute_pairwise_stats": 256}
        return D.analyse(D.HostBackend(codes, view), 9, view, [0, 1], [3, 4], [], [], opts, want_weak=False)["pairwise"]
    a, b = run(0.0), run(1.0)
    assert set(a) == set(b) == {0, 1}
    assert a[0][0][0] == 1 and a[0][0][1] <= 1.0 and a[1][0][0] == 0 and a[1][0][1] <= 1.0
    assert b[0][0][0] == 1 and b[1][0][0] == 0
    assert a[0][0][1] < b[0][0][1] and a[1][0][1] < b[0][0][1]


@pytest.mark.parametrize("names", SPELLINGS)
def test_domain_rows_of_the_reference_suite(names):
    from repair import domain as D
    tid, x, y, z = names
    ren = {"x": x, "y": y, "z": z}
    rows_in = {r[0]: {x: r[1], y: r[2], z: r[3]} for r in GOLD["domain_input"]}
    cells = [(rows_in[t], ren[a], cur) for t, a, cur in GOLD["domain_error_cells"]]
    pw = {ren[k]: [(ren[a], h) for a, h in v] for k, v in GOLD["domain_pairwise"].items()}     # 0.8469... is an INPUT here
    ds = {tid: 9, x: 3, y: 4, z: 3}
    doms = D.domains_from_rows([x, y, z], GOLD["domain_freq_rows"], 9, ds, pw, [z], cells, 4, 0.0, 0.01)
    got = sorted([t, ren[a], cur, n] for (t, a, cur), dom in zip(GOLD["domain_error_cells"], doms) for n, _ in dom)
    assert got == sorted([t, ren[a], cur, n] for t, a, cur, n in GOLD["domain_expected_beta_0.01"])
    for dom in doms:
        assert [p for _, p in dom] == sorted((p for _, p in dom), reverse=True)


def _hand_made():
    """Target a (3 values), correlated c1, c2 (2 values each) on 40 rows."""
    from repair import domain as D
    rng = np.random.default_rng(5)
    a = rng.integers(0, 3, 40); c1 = (a + rng.integers(0, 2, 40)) % 2; c2 = rng.integers(0, 2, 40)
    j1, j2 = D.Joint.from_bins(c1, a, 2, 3), D.Joint.from_bins(c2, a, 2, 3)
    return a, j1, j2, np.bincount(a, minlength=3)


def test_concat_null_quirk_is_kept():
    """IF(ISNOTNULL(domain), CONCAT(domain, d), d): a NULL list after a non-NULL domain wipes it; a NULL list first is replaced."""
    from repair import domain as D
    a, j1, j2, single = _hand_made()
    ok = np.ones(3, bool)
    cur = np.array([0, 0, 0], np.int32)
    # cell 0: both values known; cell 1: c2 NULL (second list NULL -> domain wiped); cell 2: c1 NULL (first list NULL -> only c2 counts)
    _, top, _, probs = D.cell_domains(cur, [np.array([0, 0, -1]), np.array([1, -1, 1])], [j1, j2], [0, 0], ok, 0.0, 40)
    assert probs[0].sum() > 0 and top[0] >= 0
    assert np.all(probs[1] == 0.0) and top[1] == -1
    _, _, _, only2 = D.cell_domains(cur[:1], [np.array([1])], [j2], [0], ok, 0.0, 40)
    assert np.array_equal(probs[2], only2[0])
    _, _, _, both = D.cell_domains(cur[:1], [np.array([0]), np.array([1])], [j1, j2], [0, 0], ok, 0.0, 40)
    assert np.array_equal(probs[0], both[0]) and not np.array_equal(probs[0], only2[0])


def test_tau_uses_integer_division_and_thresholds_the_joint_counts():
    from repair import domain as D
    assert D.tau_of(0.5, 100, 7, 3) == 2            # long(0.5 * (100 // 21)) = long(0.5 * 4); a float division would give long(2.38) = 2 as well ...
    assert D.tau_of(0.9, 100, 6, 3) == 4            # ... here it would not: 0.9 * (100 // 18) = 4.5 -> 4, 0.9 * (100 / 18) = 5.0 -> 5
    assert D.tau_of(0.99, 5, 3, 2) == 0
    a, j1, _, _ = _hand_made()
    dense = j1.dense()
    tau = int(np.sort(dense[0, :3])[1])              # the middle count of row c1 = 0: elements need cnt > tau
    _, _, _, probs = D.cell_domains(np.array([0], np.int32), [np.array([0])], [j1], [tau], np.ones(3, bool), 0.0, 40)
    assert np.array_equal(probs[0] > 0, dense[0, :3] > tau)


def test_probabilities_agree_with_the_literal_formula():
    from repair import domain as D
    rng = np.random.default_rng(9)
    n = 5000
    a = rng.integers(0, 7, n); c1 = (a * 3 + rng.integers(0, 3, n)) % 11; c2 = rng.integers(0, 5, n)
    c1[rng.random(n) < 0.05] = -1
    j1, j2 = D.Joint.from_bins(c1, a, 11, 7), D.Joint.from_bins(c2, a, 5, 7)
    single = np.bincount(a, minlength=7)
    rows = rng.choice(n, 300, replace=False)
    ok = np.ones(7, bool); ok[3] = False
    _, _, _, probs = D.cell_domains(a[rows].astype(np.int32), [c1[rows], c2[rows]], [j1, j2], [2, 2], ok, 0.1, n)
    lit = D.literal_probs(None, [c1[rows], c2[rows]], [j1, j2], [2, 2], single, ok, n)
    assert (probs > 0).sum() > 500
    np.testing.assert_allclose(probs, lit, rtol=1e-12, atol=0.0)


def test_continuous_lut():
    from repair import domain as D
    lut = D.continuous_lut([1.0, 2.0, 2.5, 5.0], 8)
    assert lut.tolist() == [0, 2, 3, 8]                                    # v = max gives bin discrete_thres
    assert D.continuous_lut([4.0], 8).tolist() == [-1]                      # max = min: NULL
    assert D.continuous_lut([-3.0, -1.0, 1.0], 3).tolist() == [0, 1, 3]


# ------------------------------------------------------------------ the option and run()
def test_option_is_registered_and_checked():
    key = "error.domain_analysis.enabled"
    assert key in ErrorModel.option_keys and key in RepairModel.option_keys
    em = ErrorModel("tid", [], 80, [], None, {key: "true", "error.domain_threshold_beta": "0.5"})
    assert em._checked_options()[key] is True
    assert ErrorModel("tid", [], 80, [], None, {})._checked_options()[key] is False
    with pytest.raises(ValueError):
        ErrorModel("tid", [], 80, [], None, {key: "true", "error.domain_threshold_beta": "1.5"})._checked_options()


def _fd_frame(n_groups=30, per=12, seed=3):
    """k -> v holds in every group except for ONE deviating row in each of the first 10 groups; w is a feature correlated with v."""
    rng = np.random.default_rng(seed)
    k = np.repeat(np.arange(n_groups), per)
    v = k % 5
    w = (v * 2 + (rng.random(len(k)) < 0.1)) % 10
    odd = [g * per + 3 for g in range(10)]
    v = v.copy()
    v[odd] = (v[odd] + 1 + np.arange(10) % 3) % 5
    df = pd.DataFrame({"tid": np.arange(len(k)), "k": ["k%02d" % i for i in k], "v": ["v%d" % i for i in v], "w": ["w%d" % i for i in w]})
    return df, set(odd)


def _fd_model(df, on, engine=None):
    m = RepairModel().setInput(df).setRowId("tid").setTargets(["v"]).setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints="k->v")])
    for key, val in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2", "error.max_attrs_to_compute_pairwise_stats": "2",
                     "error.domain_threshold_beta": "0.5"}.items():
        m = m.option(key, val)
    if on:
        m = m.option("error.domain_analysis.enabled", "true")
    m._engine_override = engine
    return m


def test_run_keeps_the_majority_cells_out(oracle_backend, monkeypatch):
    df, odd = _fd_frame()
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    off = _fd_model(df, False).run(detect_errors_only=True)
    on = _fd_model(df, True).run(detect_errors_only=True)
    assert len(off) == 10 * 12 and set(off["attribute"]) == {"v"}                         # today: every row of a violating group
    assert set(on["tid"]) == odd                                                         # the majority value is a weak label
    rep = _fd_model(df, True).run()
    assert set(rep["tid"]) <= odd and len(rep) >= 8
    truth = {t: "v%d" % ((t // 12) % 5) for t in odd}
    assert np.mean([truth[r.tid] == r.repaired for r in rep.itertuples()]) >= 0.8


class _DomainTable(OracleEngine._Table):
    """The oracle engine's table with the two analysis entries of `_native.Table`, served by repair.domain on the host."""

    def pair_counts(self, pairs, luts=None, n_bins=None):
        from repair import domain as D
        view = D.View(sorted(n_bins), n_bins, luts or {}, [])
        self._view = view
        self._pairs = [tuple(map(int, p)) for p in pairs]
        self._joints = D.HostBackend(self.codes, view).pair_counts(self._pairs)
        return [j.dense() for j in self._joints]

    def cell_domains(self, target_col, rows, pair_idx, min_cnt, single_ok, beta, row_count, want_probs=False):
        from repair import domain as D
        tab = D.PairTable(self._pairs, self._joints)
        corr = [[c for c in self._pairs[p] if c != target_col][0] for p in pair_idx]
        return D.HostBackend(self.codes, self._view).cell_domains(target_col, rows, corr, tab, min_cnt, single_ok, beta, row_count, want_probs)

    def gather_rows(self, rows):
        return OracleEngine._Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)


class _DomainEngine(OracleEngine):
    def upload_dictionaries(self, indices, remaps):
        t = OracleEngine.upload_dictionaries(self, indices, remaps)
        return _DomainTable(t.codes, t.n_codes, t.values, t.kinds)


def test_resident_and_value_space_paths_give_the_same_cells(oracle_backend, monkeypatch):
    df, odd = _fd_frame()
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _fd_model(df, True).run()
    slow_all = _fd_model(df, False).run()
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = _fd_model(df, True, _DomainEngine())
    fast = fm.run()
    assert fm._last_detection_on_device and fm._last_resident_info is not None
    info = fm._last_resident_info
    assert info["noisy_cells"] == 120 and info["weak_cells"] == 110 and [a for a, _ in info["pairwise_attr_stats"]["v"]] != []
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))
    fo = _fd_model(df, False, _DomainEngine())
    pd.testing.assert_frame_equal(slow_all.sort_values(key).reset_index(drop=True), fo.run().sort_values(key).reset_index(drop=True))
    assert "pairwise_attr_stats" not in fo._last_resident_info


def _hospital_model(engine, on=True):
    from tests.helpers import frame, load_golden
    from tests.test_quality import HOSPITAL_TARGETS
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)
    m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400).setTargets(HOSPITAL_TARGETS).setErrorDetectors(
        [NullErrorDetector(), ConstraintErrorDetector(constraints=";".join(ln for ln in g["constraints"].splitlines() if ln.strip()))])
    for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "4", "model.lgb.learning_rate": "0.2",
                 "error.domain_analysis.enabled": "true" if on else "false"}.items():
        m = m.option(k, v)
    m._engine_override = engine
    return m


def test_hospital_constraints_same_cells_on_both_paths(oracle_backend, monkeypatch):
    """The hospital fixture with its 13 denial constraints: the analysis turns most cells of the violating groups into weak labels,
    and the resident path (analysis through the table entries) ends with the cells of the value-space path."""
    monkeypatch.setenv("REPAIR_RESIDENT", "0")
    slow = _hospital_model(None).run()
    n_off = len(_hospital_model(None, on=False).run(detect_errors_only=True))
    n_on = len(_hospital_model(None).run(detect_errors_only=True))
    monkeypatch.delenv("REPAIR_RESIDENT")
    fm = _hospital_model(_DomainEngine())
    fast = fm.run()
    assert fm._last_detection_on_device
    assert fm._last_resident_info["noisy_cells"] == n_off and n_off - fm._last_resident_info["weak_cells"] == n_on < n_off // 4
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(slow.sort_values(key).reset_index(drop=True), fast.sort_values(key).reset_index(drop=True))
