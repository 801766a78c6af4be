"""The cases of tests/test_repair_frame_pinned_cpu.py and of its recorder (tools/record_repair_frame_pinned.py): `repair_frame(..,
want_details=True)` on frames of a few dozen rows, one case per path on which the host state of the run (the dictionary encoding, what the
cells held, the second pass) is shared between steps.  Each case is a function -> (engine, frame, keywords); `snapshot` turns the result
into plain JSON: the frame cell for cell, every details key except the timings, the models as digests of their saved blobs."""
import hashlib

import numpy as np
import pandas as pd

PARAMS = dict(n_estimators=3, learning_rate=0.3, min_data_in_leaf=2)
ZIP = {"Lyon": "69000", "Paris": "75000", "Nice": "06000", "Metz": "57000"}
REGION = {"Lyon": "ARA", "Paris": "IDF", "Nice": "PACA", "Metz": "GES"}


def people(n=40, seed=3, nulls=True):
    rng = np.random.default_rng(seed)
    city = rng.choice(sorted(ZIP), n)
    df = pd.DataFrame({"tid": np.arange(n) + 100, "city": city, "zip": np.array([ZIP[c] for c in city], object),
                       "region": np.array([REGION[c] for c in city], object),
                       "grade": np.where(np.isin(city, ["Lyon", "Paris"]), rng.choice([3, 4], n), rng.choice([1, 2], n))})
    if nulls:
        df.loc[rng.choice(n, 4, replace=False), "zip"] = None      # none in `region`: a NULL is a value of its own for IQ and flags its city
    return df


def _cells(pairs):
    return pd.DataFrame(list(pairs), columns=["tid", "attribute"])


def _metz(df, value, k=2):
    """k rows of Metz get the region `value`: city -> region then flags every Metz row."""
    at = np.flatnonzero((df["city"] == "Metz").to_numpy() & df["region"].notna().to_numpy())[:k]
    df.loc[at, "region"] = value
    return df


def given_cells_only():
    from tests.helpers import OracleEngine
    df = people()
    cells = _cells([(101, "zip"), (105, "zip"), (105, "region"), (117, "region"), (130, "zip")] +
                   [(int(t), "zip") for t in df["tid"][df["zip"].isna()]])
    return OracleEngine(), df, dict(targets=["zip", "region"], error_cells=cells, detect_nulls=False)


def detection_only():
    from tests.helpers import OracleEngine
    df = _metz(people(), "IDF")
    return OracleEngine(), df, dict(targets=["zip", "region"], constraints=[(["city"], "region")])


def detection_with_dead_classes():
    from tests.helpers import OracleEngine
    df = _metz(people(), "ZZZ")                    # `ZZZ` and `GES` are held by flagged cells only
    return OracleEngine(), df, dict(targets=["zip", "region"], constraints=[(["city"], "region")], only_noisy_targets=True)


def given_cells_and_dead_classes():
    from tests.helpers import OracleEngine
    df = _metz(people(), "ZZZ")
    lyon = df["tid"][(df["city"] == "Lyon") & df["zip"].notna()].tolist()
    cells = _cells([(int(lyon[0]), "zip"), (int(lyon[1]), "zip"), (int(lyon[1]), "region")])     # they hold values: kept from the first pass
    return OracleEngine(), df, dict(targets=["zip", "region"], error_cells=cells, constraints=[(["city"], "region")], only_noisy_targets=True)


def unknown_row_and_attribute():
    from tests.helpers import OracleEngine
    df = people()
    cells = _cells([(101, "zip"), (9999, "zip"), (105, "nope"), (105, "region"), (9998, "nope")])
    return OracleEngine(), df, dict(targets=["zip", "region"], error_cells=cells, detect_nulls=False)


def no_error_cells():
    from tests.helpers import OracleEngine
    return OracleEngine(), people(nulls=False), dict(targets=["zip", "region"])


# ---- regex-structure repair ------------------------------------------------------------------------------------------------------
PATTERN = "^[0-9]{1,3} patients$"


def samples(n=36, seed=11, dirty=()):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, n)
    df = pd.DataFrame({"tid": np.arange(n), "size": np.array([["s", "m", "l", "xl"][v] for v in g], object),
                       "ward": np.array(["w%d" % ((v + rng.integers(0, 2)) % 3) for v in g], object),
                       "sample": np.array([["10 patients", "20 patients", "32 patients", "619 patients"][v] for v in g], object)})
    for r, v in dirty:
        df.loc[r, "sample"] = v
    return df


def _strs(attr, raw):
    return [None if v is None else str(v) for v in raw]


def _regex_rules(*patterns):
    from repair.regex_structure import parse
    return dict(fd={}, nearest=None, regex=[dict(attr="sample", program=parse(p), current_str=_strs) for p in patterns])


def regex_repairs_every_cell():
    from tests.test_regex_structure_cpu import RegexOracleEngine
    df = samples(dirty=((5, "32 patixxts"), (17, "619 paxienxs")))
    return RegexOracleEngine(), df, dict(targets=["sample", "ward"], error_cells=_cells([(5, "sample"), (17, "sample"), (7, "ward")]),
                                         detect_nulls=False, rules=_regex_rules(PATTERN))


def regex_new_entry_and_a_model_cell():
    from tests.test_regex_structure_cpu import RegexOracleEngine
    df = samples(dirty=((5, "32 patixxts"), (17, "77 patixxts"), (30, "x2 patixxts"), (31, "77 patienxx"), (20, None), (8, "5 patienxx")))
    cells = _cells([(5, "sample"), (17, "sample"), (30, "sample"), (31, "sample"), (20, "sample"), (8, "sample"), (7, "ward")])
    return RegexOracleEngine(), df, dict(targets=["sample", "ward"], error_cells=cells, detect_nulls=False, rules=_regex_rules(PATTERN))


def regex_two_rules():
    from tests.test_regex_structure_cpu import RegexOracleEngine
    df = samples(dirty=((5, "32 patixxts"), (17, "619 paxienxs"), (30, "x2 patixxts")))
    cells = _cells([(5, "sample"), (17, "sample"), (30, "sample")])
    return RegexOracleEngine(), df, dict(targets=["sample", "ward"], error_cells=cells, detect_nulls=False,
                                         rules=_regex_rules("^[0-9]{3} patients$", "[0-9]{1,2} people"))


def regex_cells_from_device_detection():
    from tests.test_regex_structure_cpu import RegexOracleEngine
    df = samples(dirty=((5, "32 patixxts"), (17, "77 patixxts"), (30, "x2 patixxts"), (20, None)))
    return RegexOracleEngine(), df, dict(targets=["sample", "ward"], only_noisy_targets=True, rules=_regex_rules(PATTERN),
                                         value_detectors=dict(detectors=[dict(kind="regex", attr="sample", regex=PATTERN)]))


# ---- rule steps, merges, probability modes, analysis, training tables ------------------------------------------------------------
def fd_and_constant_steps():
    from tests.test_rule_resident_cpu import RuleOracleEngine
    df = people()
    df["country"] = "FR"
    cells = _cells([(101, "zip"), (105, "region"), (117, "region"), (117, "country"), (120, "country")] +
                   [(int(t), "region") for t in df["tid"][df["region"].isna()]])
    return RuleOracleEngine(), df, dict(targets=["zip", "region", "country"], error_cells=cells, detect_nulls=False,
                                        rules=dict(fd={"region": "city"}, nearest=None))


def nearest_merges_with_given_current():
    from tests.test_rule_resident_cpu import RuleOracleEngine
    df = people(nulls=False)
    typos = {103: "6900O", 110: "7500", 121: "99999", 127: "0600O"}
    for t, v in typos.items():
        df.loc[df["tid"] == t, "zip"] = v
    held = {int(t): v for t, v in zip(df["tid"], df["zip"])}
    rows_tid = df["tid"].to_numpy()
    cells = _cells([(t, "zip") for t in typos] + [(104, "region")])
    nearest = dict(targets=["zip"], threshold=2.0, cost=None, current_str=_strs, domain_str=_strs,
                   current=lambda attr, rows: [held[int(rows_tid[r])] for r in rows])
    return RuleOracleEngine(), df, dict(targets=["zip", "region"], error_cells=cells, detect_nulls=False, rules=dict(fd={}, nearest=nearest))


def continuous_target_with_pmf_costs():
    from tests.test_prob_modes_cpu import CostOracleEngine
    df = people(nulls=False)
    cells = _cells([(101, "grade"), (105, "grade"), (105, "zip"), (117, "zip"), (130, "grade")])

    def costs(attr, classes, rows):
        if attr == "grade":
            return None
        k, r = len(classes), len(rows)
        cost = (np.arange((r + 1) * k, dtype=np.float64).reshape(r + 1, k) % 3.0) / 2.0
        return dict(cost=cost, cost_row=np.arange(r, dtype=np.int32), cur_code=np.full(r, -1, np.int32), weight=0.5, renormalise=True)

    return CostOracleEngine(), df, dict(targets=["zip", "grade"], error_cells=cells, detect_nulls=False, continuous_columns=["grade"],
                                        want_pmf=True, top_k=3, pmf_costs=costs)


def domain_analysis_with_weak_cells():
    from repair.errors import ErrorModel
    from tests.test_domain_analysis import _DomainEngine, _fd_frame
    df, _ = _fd_frame(n_groups=10, per=6)
    opts = {"error.domain_analysis.enabled": "true", "error.max_attrs_to_compute_pairwise_stats": "2", "error.domain_threshold_beta": "0.5"}
    eopts = ErrorModel(row_id="tid", targets=["v"], discrete_thres=80, error_detectors=[], error_cells=None, opts=opts)._checked_options()
    return _DomainEngine(), df, dict(targets=["v"], constraints=[(["k"], "v")], only_noisy_targets=True,
                                     domain_analysis=dict(options=eopts, discrete_thres=80, continuous_columns=[]))


def distinct_training_rows():
    from tests.synth import make_table
    from tests.test_distinct_rows_cpu import DistinctOracleEngine
    dirty, _, _ = make_table(60, 5, seed=23, null_ratio=0.06, cards=[2, 3, 2, 2, 3])
    df = pd.DataFrame({"tid": np.arange(60)})
    for c in range(5):
        df["c%d" % c] = [None if v < 0 else "v%d" % v for v in dirty[c]]
    return DistinctOracleEngine(small=4), df, dict(targets=["c1", "c2", "c4"], distinct_training_rows=dict(max_ratio=1.0),
                                                   base_params=dict(PARAMS, max_depth=3))


def domain_analysis_then_dead_classes():
    engine, df, kw = domain_analysis_with_weak_cells()
    df.loc[3, "v"] = "v9"                          # a deviating cell with a value of its own: it stays an error cell, and its class dies
    return engine, df, kw


def rebalance():
    from tests import rebalance_cases as RC
    rng = np.random.default_rng(31)
    y = rng.choice(["a", "b", "c"], 60, p=[0.6, 0.28, 0.12])
    df = pd.DataFrame({"tid": np.arange(60), "f1": np.where(rng.random(60) < 0.7, np.char.add("x", y), "xa").astype(object),
                       "f2": rng.choice(["p", "q", "r"], 60).astype(object), "y": y.astype(object)})
    df.loc[rng.choice(60, 5, replace=False), "y"] = None
    df.loc[rng.choice(60, 3, replace=False), "f2"] = None
    return RC.oracle_engine(), df, dict(targets=["y"], rebalance=dict(k=3, random_state=42))


CASES = [given_cells_only, detection_only, detection_with_dead_classes, given_cells_and_dead_classes, unknown_row_and_attribute, no_error_cells,
         regex_repairs_every_cell, regex_new_entry_and_a_model_cell, regex_two_rules, regex_cells_from_device_detection, fd_and_constant_steps,
         nearest_merges_with_given_current, continuous_target_with_pmf_costs, domain_analysis_with_weak_cells,
         domain_analysis_then_dead_classes, distinct_training_rows, rebalance]


def run(case):
    from repair.pipeline import repair_frame
    engine, df, kw = case()
    kw = dict(dict(base_params=dict(PARAMS)), **kw)
    return repair_frame(engine, df, "tid", want_details=True, **kw)


# ---- the result as plain JSON ----------------------------------------------------------------------------------------------------
TIMINGS = ("_ms", "_sec", "seconds")


def plain(v):
    """Numbers, strings, None, lists and string-keyed dicts of them; floats through repr (exact), frames as their columns."""
    if isinstance(v, pd.DataFrame):
        return {"columns": [str(c) for c in v.columns], "rows": [plain(list(r)) for r in v.to_numpy(dtype=object).tolist()]}
    if isinstance(v, dict):
        return {str(k): plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple, np.ndarray)):
        return [plain(x) for x in (v.tolist() if isinstance(v, np.ndarray) else v)]
    if isinstance(v, (bytes, bytearray)):
        return "md5:" + hashlib.md5(bytes(v)).hexdigest()
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return "f:" + repr(float(v))
    raise TypeError("no plain form for %r" % type(v))


def snapshot(frame, details):
    """The comparable part of a `repair_frame(.., want_details=True)` result."""
    det = {k: v for k, v in details.items() if k != "times"}
    det["stats"] = [{k: v for k, v in st.items() if not k.endswith(TIMINGS)} for st in det.get("stats", [])]
    det["models"] = {str(t): bytes(b) for t, b in det.get("models", {}).items()}
    return dict(frame=plain(frame), details=plain(det))
