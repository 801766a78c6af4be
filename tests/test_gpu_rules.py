"""-m gpu: the device entries of the rule-based repairs (csrc/rgbm_rules.hip: rgbm_table_fd_map, rgbm_table_rule_fill,
rgbm_nearest_values) against their numpy restatements (tests/rule_restatements.py) -- integers, so equality -- and
`RepairModel.run()` with `setRepairByRules(True)` and `model.rule.resident` through the HIP engine against the value-space path."""
import os

import numpy as np
import pandas as pd
import pytest

from tests import rule_restatements as R
from tests.helpers import csrc_constant

pytestmark = pytest.mark.gpu


def _lds_codes():
    """The largest n_codes[x] whose (lo, hi) tables stay in LDS: the constant of the source, not a copy of it."""
    return csrc_constant("FD_LDS_CODES")


N_ROWS = 200_003            # 25 workgroups of 8192 rows; not a multiple of the 2048-row load tile


def _fd_table(nx, ny, seed, n=N_ROWS):
    """x -> y = (7 x + 3) mod ny, except: codes with x % 5 == 1 occur with random y values (conflicts), codes with x % 5 == 2 only next to
    a NULL y, 2 % of either column is NULL, and the code `lone` occurs in the first and the last row only, with y = 0 and y = ny - 1."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, nx, n).astype(np.int32)
    y = ((x.astype(np.int64) * 7 + 3) % ny).astype(np.int32)
    y[x % 5 == 1] = rng.integers(0, ny, int((x % 5 == 1).sum()))
    y[x % 5 == 2] = -1
    x[rng.random(n) < 0.02] = -1
    y[rng.random(n) < 0.02] = -1
    lone = nx - 1 if (nx - 1) % 5 not in (1, 2) else nx - 3
    if nx >= 8:
        x[x == lone] = -1
        x[0], y[0], x[-1], y[-1] = lone, 0, lone, ny - 1
    return np.stack([x, y, rng.integers(0, 3, n).astype(np.int32)]), [nx, ny, 3], lone


@pytest.mark.parametrize("nx", [1, 2, 1000, "lds", "lds+1"])
def test_fd_map(nx):
    from repair import _native as N
    nx = {"lds": _lds_codes(), "lds+1": _lds_codes() + 1}.get(nx, nx)
    ny = 3 if nx <= 2 else 257
    codes, n_codes, lone = _fd_table(nx, ny, seed=nx)
    if nx == 2:
        codes[1] = np.where(codes[0] == 0, 0, np.where(codes[0] == 1, ny - 1, -1))        # the sentinels' neighbours: y codes 0 and ny - 1
        codes[1][::17] = -1
    got = N.Table(codes, n_codes).fd_map(0, 1)
    want = R.fd_map(codes, n_codes, 0, 1)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    if nx == 2:
        assert got.tolist() == [0, ny - 1]
    if nx >= 8:
        assert got[lone] == -1 and (got[np.arange(nx) % 5 == 2] == -1).all() and (got >= 0).sum() > nx // 3
        assert got[(np.arange(nx) * 7 + 3) % ny == 0].max() == 0 and got.max() == ny - 1
        # the other direction too (y -> x): many x per y, almost every code in conflict
        assert np.array_equal(N.Table(codes, n_codes).fd_map(1, 0), R.fd_map(codes, n_codes, 1, 0))


def test_fd_map_single_code_and_empty_groups():
    from repair import _native as N
    n = 70_001
    x = np.zeros(n, np.int32)
    y = np.full(n, 4, np.int32)
    y[::3] = -1
    tab = N.Table(np.stack([x, y]), [1, 6])
    assert tab.fd_map(0, 1).tolist() == [4]
    y2 = y.copy(); y2[0], y2[-1] = 0, 5                  # the two other values sit in the first and the last row only
    assert N.Table(np.stack([x, y2]), [1, 6]).fd_map(0, 1).tolist() == [-1]
    assert N.Table(np.stack([x, np.full(n, -1, np.int32)]), [1, 6]).fd_map(0, 1).tolist() == [-1]      # y always NULL
    assert N.Table(np.stack([np.full(n, -1, np.int32), y]), [3, 6]).fd_map(0, 1).tolist() == [-1, -1, -1]


@pytest.mark.parametrize("row_begin,n_rows", [(0, None), (1000, 5003), (10_006, 1)])
def test_rule_fill(row_begin, n_rows):
    from repair import _native as N
    n = 10_007
    rng = np.random.default_rng(7)
    codes = rng.integers(-1, 40, (3, n)).astype(np.int32)
    codes[1] = np.where(rng.random(n) < 0.3, -1, rng.integers(0, 9, n)).astype(np.int32)
    n_codes = [40, 9, 40]
    n_rows = n - row_begin if n_rows is None else n_rows
    lut = rng.integers(-1, 9, 37).astype(np.int32)      # shorter than the dictionary: codes 37..39 have no entry
    lut[[0, 5, 36]] = -1
    for x, l in ((0, lut), (-1, np.array([6], np.int32)), (-1, np.array([-1], np.int32))):
        tab = N.Table(codes, n_codes)
        want = codes.copy()
        want_pred = R.rule_fill(want, 1, x, l, row_begin, n_rows)
        got_pred = tab.rule_fill(1, x, l, row_begin, n_rows)
        assert np.array_equal(got_pred, want_pred)
        for c in range(3):
            assert np.array_equal(tab.read_column(c), want[c]), (x, c)
        was_null = codes[1] < 0
        assert np.array_equal(want[1][~was_null], codes[1][~was_null])               # only NULL cells change
        if x == 0:
            assert (want[1][row_begin:row_begin + n_rows] < 0).any() or n_rows == 1    # lut entries of -1 leave the cell NULL
        assert tab.rule_fill(1, x, l, row_begin, n_rows, want_labels=False) is None
    with pytest.raises(N.RepairGbmError):
        N.Table(codes, n_codes).rule_fill(1, 0, np.array([9], np.int32))                # a code outside the target's dictionary
    with pytest.raises(N.RepairGbmError):
        N.Table(codes, n_codes).rule_fill(1, 0, lut, n - 5, 6)                          # past the last row


def _pools(n_b, seed):
    """(a, b): b holds n_b distinct strings -- short ones plus, from 4 on, strings of 64, 65 and 200 code points; a holds copies of b's first
    and last string (minimum 0 in the first / last position), strings one edit from two of b (ties), strings of 0, 1, 64, 65 and 203 code
    points and random short ones."""
    rng = np.random.default_rng(seed)
    abc = "abcdé日"
    word = lambda k: "".join(abc[i] for i in rng.integers(0, len(abc), k))      # noqa: E731
    b = []
    while len(b) < n_b:
        w = word(int(rng.integers(1, 9)))
        if w not in b:
            b.append(w)
    if n_b >= 4:
        b[1], b[2], b[n_b // 2] = "x" + word(63), "y" + word(64), "z" + word(199)
    if n_b >= 2:
        b[0], b[-1] = "qqqq1", "qqqq2"
    a = [word(int(rng.integers(1, 9))) for _ in range(20)] + ["", "q", "x" + word(63), "y" + word(64), "z" + word(202), "qqqq3", "qqqq"]
    if n_b:
        a += [b[0], b[-1], b[0] + "!", b[-1][:-1], b[n_b // 2], b[n_b // 2] + "ab", b[1 % n_b][1:]]
    return a, b


@pytest.fixture(scope="module", params=[0, 1, 63, 64, 65, 130])
def pools(request):
    a, b = _pools(request.param, seed=request.param)
    from repair.costs import edit_distance
    return a, b, np.array([[edit_distance(x, y) for y in b] for x in a], np.float64).reshape(len(a), len(b))


def test_nearest_values_of_string_pools(pools):
    from repair import _native as N
    a, b, dist = pools
    seen = set()
    for thr in (0.0, 1.0, 2.0, 2.5, 1e9):
        got = N.nearest_values(a, b, threshold=thr)
        want = R.nearest(dist, thr) if len(b) else np.full(len(a), -1, np.int32)
        assert got.dtype == np.int32 and np.array_equal(got, want), thr
        seen |= set(got.tolist())
    if len(b) == 0:
        assert seen == {-1}
    if len(b) >= 2:
        assert {-1, 0, len(b) - 1} <= seen                      # no merge, the first and the last position all occur
        m = dist.min(axis=1)
        assert ((dist == m[:, None]).sum(axis=1) > 1).any()      # a tie at the minimum
        assert (m == 2.0).any() and (m == 1.0).any() and (m > 2.5).any()    # minima equal to a threshold and just above one
    assert np.array_equal(N.edit_distance(a, b).astype(np.float64), dist) or len(b) == 0


@pytest.mark.parametrize("n_b", [1, 63, 64, 65, 130])
def test_nearest_values_of_a_cost_matrix(n_b):
    from repair import _native as N
    rng = np.random.default_rng(n_b)
    cost = rng.integers(0, 50, (300, n_b)).astype(np.float64) / 4.0
    cost[rng.random(cost.shape) < 0.2] = np.nan
    cost[0] = np.nan                                           # no pair has a cost
    cost[1] = 7.0; cost[1, 0] = 1.0                            # the minimum in the first position
    cost[2] = 7.0; cost[2, -1] = 1.0                           # ... in the last
    cost[3] = 7.0; cost[3, 0] = 2.0                            # equal to the threshold
    cost[4] = 7.0; cost[4, -1] = 2.25                          # just above it
    cost[5] = 1.0                                              # a tie everywhere (unique only when n_b is 1)
    cost[6] = np.nan; cost[6, n_b // 2] = 0.5                  # one pair with a cost
    if n_b > 64:
        cost[7] = 7.0; cost[7, 0] = cost[7, 64] = 1.0          # a tie across two lanes' strides
        cost[8] = 7.0; cost[8, 63] = cost[8, 64] = 1.0         # ... across the wave boundary
    got = N.nearest_values(cost=cost, threshold=2.0)
    want = R.nearest(cost, 2.0)
    assert np.array_equal(got, want)
    assert got[:5].tolist() == [-1, 0, n_b - 1, 0, -1] and got[5] == (0 if n_b == 1 else -1) and got[6] == n_b // 2
    assert np.array_equal(N.nearest_values(cost=cost, threshold=-1.0), np.full(300, -1, np.int32))


def _both_paths(make):
    from repair.engine import HipEngine
    os.environ["REPAIR_RESIDENT"] = "0"
    try:
        a = make().run()
    finally:
        os.environ.pop("REPAIR_RESIDENT", None)
    fast = make().option("model.rule.resident", "true")
    fast._engine_override = HipEngine(0)
    b = fast.run()
    assert getattr(fast, "_last_resident_info", None) is not None, "the run did not take the resident path"
    key = ["tid", "attribute"]
    pd.testing.assert_frame_equal(a.sort_values(key).reset_index(drop=True), b.sort_values(key).reset_index(drop=True), check_exact=True)
    return b, fast


def test_run_with_fd_rules_equals_the_value_space_path():
    from repair.errors import ConstraintErrorDetector, NullErrorDetector
    from repair.model import RepairModel
    df, cells = R.fd_frame()

    def make():
        m = RepairModel().setInput(df).setRowId("tid").setErrorCells(cells).setRepairByRules(True) \
            .setErrorDetectors([NullErrorDetector(), ConstraintErrorDetector(constraints=R.FD_CONSTRAINTS)])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "8", "model.lgb.learning_rate": "0.2"}.items():
            m = m.option(k, v)
        return m

    b, fast = _both_paths(make)
    steps = {s["target"]: s for s in fast._last_resident_info["rule_steps"]}
    assert steps["c1"]["mapped"] > 0 and steps["c1"]["conflict"] > 0 and steps["c1"]["unseen"] > 0 and steps["c2"]["kind"] == "fd"
    assert b[b["attribute"] == "c1"]["repaired"].isna().any()


def test_run_with_nearest_values_equals_the_value_space_path():
    from repair.costs import Levenshtein
    from repair.model import RepairModel
    from tests.helpers import GOLDEN
    import json
    with open(os.path.join(GOLDEN, "rule_repairs.json"), encoding="utf-8") as f:
        g = json.load(f)["nearest_values"]
    df = pd.DataFrame(g["rows"], columns=g["columns"])
    cells = pd.DataFrame(g["error_cells"], columns=["tid", "attribute"])

    def make():
        m = RepairModel().setInput(df).setRowId("tid").setErrorCells(cells).setRepairByRules(True).setTargets(g["targets_run"]) \
            .setUpdateCostFunction(Levenshtein(targets=g["cost_targets"])).option("model.hp.max_evals", "1")
        for k, v in g["options"].items():
            m = m.option(k, v)
        return m

    b, fast = _both_paths(make)
    rows = b.sort_values(["tid", "attribute"])[["tid", "attribute", "current_value", "repaired"]].to_numpy(dtype=object).tolist()
    assert rows == g["expected_targets_run"] and fast._last_resident_info["nearest_values"] == {"v0": 3, "v1": 3}


def test_hospital_run_with_its_constraints_equals_the_value_space_path():
    from repair.errors import ConstraintErrorDetector, NullErrorDetector
    from repair.model import RepairModel
    from tests.helpers import frame, load_golden
    from tests.test_quality import HOSPITAL_TARGETS
    g = load_golden("hospital")
    df = frame(g["input"], dtypes=False)
    df["tid"] = df["tid"].astype(int)

    def make():
        m = RepairModel().setInput(df).setRowId("tid").setDiscreteThreshold(400).setTargets(HOSPITAL_TARGETS).setRepairByRules(True).setErrorDetectors(
            [NullErrorDetector(), ConstraintErrorDetector(constraints=";".join(ln for ln in g["constraints"].splitlines() if ln.strip()))])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": "10", "model.lgb.learning_rate": "0.2"}.items():
            m = m.option(k, v)
        return m

    b, fast = _both_paths(make)
    assert fast._last_detection_on_device and len(b) > 1000
    steps = fast._last_resident_info["rule_steps"]
    assert len(steps) >= 4 and all(s["kind"] == "fd" for s in steps) and sum(s["mapped"] for s in steps) > 0
