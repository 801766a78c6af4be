"""RepairModel -- the reference's fluent repair API (python/repair/model.py) on a Spark-free host,
with its hot path (`_build_repair_models` 955-1052, `_build_repair_stat_models_in_series` 768-815,
`_repair` 1062-1143) running on the MI355X engine through `repair.gbm` / librepairgbm.so.

Kept verbatim from the reference: setter names and validation messages, `option()` keys, `run()`
flags and their exclusivity rules, the output schemas
  (row_id, attribute, current_value, repaired[, prob | pmf | score]),
the estimator protocol of the per-attribute models (PoorModel / FunctionalDepModel / stat model),
"train on all rows with error cells NULLed, drop rows whose target is NULL", the fill-only-NULL
chain over target attributes, integral rounding, and "a failed build becomes PoorModel(None)".
Inputs are pandas DataFrames (or names registered with `repair.session.register_table`).
"""
import copy
import heapq
import json
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np
import pandas as pd

from repair import session
from repair.costs import UpdateCostFunction
from repair.detect_codes import LOF_MAX_RANGE
from repair.encode import is_integral_column, is_numeric_column
from repair.errors import (ConstraintErrorDetector, DomainValues, ErrorDetector, ErrorModel, GaussianOutlierErrorDetector, LOFOutlierErrorDetector,
                           NullErrorDetector, RegExErrorDetector, parse_constraint, load_constraints, parse_and_verify_constraints, _to_sql_string)
from repair.train import build_model, compute_class_nrow_stdv, rebalance_training_data, train_option_keys
from repair.train import _opt_gpu_device_id as _train_opt_gpu_device_id
from repair.utils import argtype_check, elapsed_time, get_option_value, job_group, setup_logger, to_list_str

_logger = setup_logger()

DataFrame = pd.DataFrame


class PoorModel():
    """Model to return the same value regardless of an input value (reference model.py:44-61)."""

    def __init__(self, v: Any) -> None:
        self.v = v

    @property
    def classes_(self) -> Any:
        return np.array([self.v])

    def predict(self, X: pd.DataFrame) -> Any:
        return [self.v] * len(X)

    def predict_proba(self, X: pd.DataFrame) -> Any:
        return [np.array([1.0])] * len(X)


class FunctionalDepModel():
    """sklearn-like model that follows a functional dependency x -> y (reference model.py:64-100)."""

    def __init__(self, x: str, fd_map: Dict[str, str]) -> None:
        self.fd_map = fd_map
        self.classes = sorted(set(fd_map.values()), key=str)   # deterministic (the reference's set order is hash-dependent)
        self.x = x
        self.fd_keypos_map = {c: i for i, c in enumerate(self.classes)}

    @property
    def classes_(self) -> Any:
        return np.array(self.classes)

    def predict(self, X: pd.DataFrame) -> Any:
        return [self.fd_map[x] if x in self.fd_map else None for x in X[self.x]]

    def predict_proba(self, X: pd.DataFrame) -> Any:
        pmf = []
        for x in X[self.x]:
            if x in self.fd_map:
                probs = np.zeros(len(self.classes))
                probs[self.fd_keypos_map[self.fd_map[x]]] = 1.0
                pmf.append(probs)
            else:
                _logger.warning('Unknown "%s" domain value found: %s' % (self.x, x))
                pmf.append(None)
        return pmf


class RepairModel():
    """Interface to detect error cells in given input data and build statistical models to repair them."""

    from collections import namedtuple
    _option = namedtuple("_option", "key default_value type_class validator err_msg")

    _opt_max_training_row_num = _option("model.max_training_row_num", 10000, int, lambda v: v >= 10, "`{}` should be greater than and equal to 10")
    _opt_max_training_column_num = _option("model.max_training_column_num", 65536, int, lambda v: v >= 2, "`{}` should be greater than 1")
    _opt_small_domain_threshold = _option("model.small_domain_threshold", 12, int, lambda v: v >= 3, "`{}` should be greater than 2")
    _opt_repair_by_regex_disabled = _option("model.rule.repair_by_regex.disabled", True, bool, None, None)
    _opt_repair_by_nearest_values_disabled = _option("model.rule.repair_by_nearest_values.disabled", True, bool, None, None)
    _opt_merge_threshold = _option("model.rule.merge_threshold", 2.0, float, None, None)
    _opt_repair_by_functional_deps_disabled = _option("model.rule.repair_by_functional_deps.disabled", False, bool, None, None)
    _opt_max_domain_size = _option("model.rule.max_domain_size", 1000, int, lambda v: v > 10, "`{}` should be greater than 10")
    _opt_cost_weight = _option("repair.pmf.cost_weight", 0.1, float, lambda v: v > 0.0, "`{}` should be positive")
    _opt_prob_threshold = _option("repair.pmf.prob_threshold", 0.0, float, None, None)
    _opt_prob_top_k = _option("repair.pmf.prob_top_k", 32, int, lambda v: v >= 3, "`{}` should be greater than 2")
    # new in this engine: the probability modes (pmf / prob / score / maximal likelihood) on the HBM-resident pipeline
    _opt_pmf_resident = _option("repair.pmf.resident", False, bool, None, None)
    # new in this engine: the rule-based repairs (`setRepairByRules`: FD rule models, constant models, nearest-value merges) on the
    # HBM-resident pipeline
    _opt_rule_resident = _option("model.rule.resident", False, bool, None, None)
    # regex-structure repair (`model.rule.repair_by_regex.disabled=""`) on the HBM-resident pipeline as well (needs `model.rule.resident` too):
    # the cells' strings through `engine.regex_structure` (rgbm_regex_structure), the repaired values into the encoding
    _opt_rule_regex_resident = _option("model.rule.regex.resident", False, bool, None, None)
    # `setTrainingDataRebalancingEnabled(True)` on the HBM-resident path: SMOTEN in code space on the device (repair.rebalance_codes)
    _opt_rebalance_resident = _option("model.rebalance.resident", False, bool, None, None)
    # new in this engine: the value detectors (RegExErrorDetector, DomainValues, GaussianOutlierErrorDetector) as code predicates on
    # the HBM-resident table (repair.detect_codes, `Table.detect_cells`)
    _opt_value_detectors_resident = _option("error.value_detectors.resident", False, bool, None, None)
    # new in this engine: LOFOutlierErrorDetector on the HBM-resident table, evaluated once per dictionary entry (repair.lof_codes,
    # rgbm_lof_1d); a column whose scikit-learn answer is not determined sends the run to the value-space path
    _opt_lof_resident = _option("error.lof.resident", False, bool, None, None)
    # new in this engine: every parsed denial constraint (single-tuple constants, several IQs, LT / GT) on the HBM-resident table
    # (repair.dc_codes, `Table.detect_dc` / `Table.detect_row_bits`); `X -> Y` constraints take `Table.detect_constraint` either way
    _opt_constraints_resident = _option("error.constraints.resident", False, bool, None, None)
    # ... and, with that option set, the ORDER constraints among them -- EQ predicates plus one or two LT / GT, no IQ
    # (`repair.dc_codes.scan_eligible`) -- by sort and scan (`Table.detect_dc_scan`) instead of pairs: O(n log n) whatever the groups are, so
    # a constraint without an EQ predicate is answered at any table size instead of refused above `max_pairs`.  Off by default.  Measured,
    # the scan route is the slower one only on small tables (20 000 rows in groups of 50: 0.170 ms against 0.156 ms for pairs)
    _opt_constraints_order_scan = _option("error.constraints.order_scan", False, bool, None, None)
    # new in this engine: `run(detect_errors_only=True)` on the HBM-resident table (`_device_detect_only_plan`, `pipeline.detect_frame`): the
    # detectors admitted by the options above run on the device, their cells are merged there (the table's cell set) and leave
    # it once, with the codes they hold.  None of the model conditions of the resident repair run applies.  Off by default.
    _opt_detect_only_resident = _option("error.detect_only.resident", False, bool, None, None)
    # new in this engine: a resident REPAIR run keeps its error cells in the table's cell set from detection through the null-out
    # (`pipeline._cells_on_set`): every detector's cells are merged on the device, the weak-labelled ones are pruned there, the
    # given cells go up once and the remaining ones come down once; the null-out and the dirty rows are read off the set.  The same cells,
    # frame and details; `_last_resident_info["cells_route"]` says 'set', or 'host' where the engine's table lacks the entries or the job
    # runs on several ranks.  Off by default.
    _opt_cells_resident = _option("error.cells.resident", False, bool, None, None)
    # new in this engine: on the HBM-resident pipeline, train every attribute's model on the DISTINCT rows of the table with their
    # multiplicities (found on the device, `Table.distinct_rows`): the same models, bytes included, at the cost of the distinct rows.  It
    # only matters for an attribute that `model.max_training_row_num` does not sample (a sampled attribute trains on its sample); the
    # whole table is used wherever the variant does not apply (repair.pipeline.distinct_training_tables; `_last_resident_info` says why)
    _opt_train_distinct_rows = _option("model.train.distinct_rows", False, bool, None, None)
    # ... unless the table holds more than this share of distinct rows (a policy default, not a measured break-even: DESIGN 5g)
    _opt_train_distinct_rows_max_ratio = _option("model.train.distinct_rows.max_ratio", 0.5, float, lambda v: 0.0 < v <= 1.0,
                                                 "`{}` should be in (0.0, 1.0]")
    # new in this engine: a resident repair run KEEPS its fit (`fittedModels()`: repair.fitted.FittedRepairModels -- the final dictionaries, the
    # chain, the model blobs), so that `setFittedModels` repairs later tables without training.  Off by default: nothing is kept.
    _opt_fitted_keep = _option("model.fitted.keep", False, bool, None, None)
    # new in this engine: which HIP device trains/predicts (read by repair.train.fixed_params)
    _opt_gpu_device_id = _train_opt_gpu_device_id

    option_keys = set([o.key for o in (
        _opt_max_training_row_num, _opt_max_training_column_num, _opt_small_domain_threshold, _opt_repair_by_regex_disabled,
        _opt_repair_by_nearest_values_disabled, _opt_merge_threshold, _opt_repair_by_functional_deps_disabled,
        _opt_max_domain_size, _opt_cost_weight, _opt_prob_threshold, _opt_prob_top_k, _opt_pmf_resident, _opt_rule_resident, _opt_rule_regex_resident, _opt_rebalance_resident,
        _opt_value_detectors_resident, _opt_lof_resident, _opt_constraints_resident, _opt_constraints_order_scan, _opt_detect_only_resident, _opt_cells_resident, _opt_train_distinct_rows, _opt_train_distinct_rows_max_ratio, _opt_fitted_keep, _opt_gpu_device_id)] +
        list(ErrorModel.option_keys) + list(train_option_keys))

    def __init__(self) -> None:
        self.db_name: str = ""
        self.input: Optional[Union[str, DataFrame]] = None
        self.row_id: Optional[str] = None
        self.targets: List[str] = []
        self.error_cells: Optional[Union[str, DataFrame]] = None
        self.error_detectors: List[ErrorDetector] = []
        self.discrete_thres: int = 80
        self.parallel_stat_training_enabled: bool = False
        self.training_data_rebalancing_enabled: bool = False
        self.repair_by_rules: bool = False
        self.repair_delta: Optional[int] = None
        self.repair_validation_enabled: bool = False
        self.cf: Optional[UpdateCostFunction] = None
        self.opts: Dict[str, str] = {}
        self._fitted: Any = None                      # `setFittedModels`: the fit that `run()` applies instead of training
        self._kept_fit: Any = None                    # `fittedModels()`: what the last run kept, or why it kept nothing
        self._kept_fit_why: str = "no run has kept a fit: set the option `model.fitted.keep` and run"

    # ------------------------------------------------------------------ fluent setters
    @argtype_check  # type: ignore
    def setDbName(self, db_name: str) -> "RepairModel":
        if isinstance(self.input, DataFrame):
            raise ValueError("Can not specify a database name when input is `DataFrame`")
        self.db_name = db_name
        return self

    @argtype_check  # type: ignore
    def setTableName(self, table_name: str) -> "RepairModel":
        if not table_name:
            raise ValueError("`table_name` should have at least character")
        self.input = table_name
        return self

    @argtype_check  # type: ignore
    def setInput(self, input: Union[str, DataFrame]) -> "RepairModel":
        if type(input) is str:
            self.setTableName(input)
        else:
            self.db_name = ""
            self.input = input
        return self

    @argtype_check  # type: ignore
    def setRowId(self, row_id: str) -> "RepairModel":
        if not row_id:
            raise ValueError("`row_id` should have at least character")
        self.row_id = row_id
        return self

    @argtype_check  # type: ignore
    def setTargets(self, attrs: List[str]) -> "RepairModel":
        if len(attrs) == 0:
            raise ValueError("`attrs` should have at least one attribute")
        self.targets = attrs
        return self

    @argtype_check  # type: ignore
    def setErrorCells(self, error_cells: Union[str, DataFrame]) -> "RepairModel":
        if type(error_cells) is str and not error_cells:
            raise ValueError("`error_cells` should have at least character")
        if self.row_id is None:
            raise ValueError("`setRowId` should be called before specifying error cells")
        df = session.resolve(error_cells)
        if not all(c in df.columns for c in [self._row_id, "attribute"]):
            raise ValueError("Error cells should have `%s` and `attribute` in columns" % self.row_id)
        self.error_cells = error_cells
        return self

    @argtype_check  # type: ignore
    def setErrorDetectors(self, detectors: List[ErrorDetector]) -> "RepairModel":
        self.error_detectors = detectors
        return self

    def setFittedModels(self, fitted_or_path: Any) -> "RepairModel":
        """`run()` and `run(repair_data=True)` train nothing: the error cells, detected as ever, are repaired by the chain of a kept fit
        (`fittedModels()` of an earlier run, or the path of its `save`).  None clears it."""
        from repair.fitted import FittedRepairModels
        if fitted_or_path is not None and not isinstance(fitted_or_path, FittedRepairModels):
            fitted_or_path = FittedRepairModels.load(str(fitted_or_path))
        self._fitted = fitted_or_path
        return self

    def fittedModels(self) -> Any:
        """The fit the last `run()` kept under `model.fitted.keep` (repair.fitted.FittedRepairModels).  ValueError, with the reason, when
        there is none: the option was off, the run used rule steps, was a multi-rank job or took the value-space path."""
        if self._kept_fit is None:
            raise ValueError("No fitted models: %s" % self._kept_fit_why)
        return self._kept_fit

    @argtype_check  # type: ignore
    def setDiscreteThreshold(self, thres: int) -> "RepairModel":
        if int(thres) < 2:
            raise ValueError("`thres` should be bigger than 1, got %s" % thres)
        self.discrete_thres = thres
        return self

    @argtype_check  # type: ignore
    def setParallelStatTrainingEnabled(self, enabled: bool) -> "RepairModel":
        self.parallel_stat_training_enabled = enabled
        return self

    @argtype_check  # type: ignore
    def setTrainingDataRebalancingEnabled(self, enabled: bool) -> "RepairModel":
        self.training_data_rebalancing_enabled = enabled
        return self

    @argtype_check  # type: ignore
    def setRepairByRules(self, enabled: bool) -> "RepairModel":
        self.repair_by_rules = enabled
        return self

    @argtype_check  # type: ignore
    def setRepairDelta(self, delta: int) -> "RepairModel":
        if delta <= 0:
            raise ValueError("Repair delta should be positive, got %s" % delta)
        self.repair_delta = int(delta)
        return self

    @argtype_check  # type: ignore
    def setUpdateCostFunction(self, cf: UpdateCostFunction) -> "RepairModel":
        self.cf = cf
        return self

    @argtype_check  # type: ignore
    def option(self, key: str, value: str) -> "RepairModel":
        if key not in self.option_keys:
            raise ValueError("Non-existent key specified: key=%s" % key)
        self.opts[key] = value
        return self

    def _get_option_value(self, *args) -> Any:  # type: ignore
        return get_option_value(self.opts, *args)

    @property
    def _row_id(self) -> str:
        return str(self.row_id)

    @property
    def _repair_by_nearest_values_enabled(self) -> bool:
        return not bool(self._get_option_value(*self._opt_repair_by_nearest_values_disabled)) and self.repair_by_rules and self.cf is not None

    @property
    def _repair_by_regex_enabled(self) -> bool:
        return not bool(self._get_option_value(*self._opt_repair_by_regex_disabled)) and self.repair_by_rules

    @property
    def _repair_by_functional_deps_enabled(self) -> bool:
        return not bool(self._get_option_value(*self._opt_repair_by_functional_deps_disabled)) and self.repair_by_rules

    # ------------------------------------------------------------------ input checks
    def _qualified_input_name(self) -> str:
        """`db.table` / `table` as the reference's messages print it; a DataFrame input has no name of its own."""
        if isinstance(self.input, str):
            return ("%s.%s" % (self.db_name, self.input)) if self.db_name else self.input
        return "input"

    def _check_input_table(self) -> Tuple[DataFrame, List[str]]:
        """RepairApi.checkInputTable (RepairApi.scala:34-67)."""
        df = session.resolve(self.input)
        rid = self._row_id
        name = self._qualified_input_name()
        if rid not in df.columns:
            raise ValueError("Column '%s' does not exist in '%s'." % (rid, name))
        unsupported = [t for t in (_sql_type_name(df[c]) for c in df.columns) if t not in _SUPPORTED_TYPES]
        if unsupported:
            raise ValueError("Supported types are %s, but unsupported ones found: %s" % (",".join(_SUPPORTED_TYPES), ",".join(unsupported)))
        if len(df.columns) < 3:
            raise ValueError("A least three columns (`%s` columns + two more ones) in table '%s'" % (rid, name))
        if not df[rid].is_unique:
            raise ValueError("Uniqueness does not hold in column '%s' of table '%s' (# of distinct '%s': %d, # of rows: %d)" % (
                rid, name, rid, df[rid].nunique(dropna=False), len(df)))
        continous = [c for c in df.columns if c != rid and is_numeric_column(df[c])]
        _logger.info("input_table: (%d rows x %d columns)" % (len(df), len(df.columns) - 1))
        # positional index without copying the table (a frame of 10^6 object cells takes > 1 s to copy + consolidate): nothing
        # downstream writes into `input_df`, every step that changes cells works on its own copy
        if isinstance(df.index, pd.RangeIndex) and df.index.start == 0 and df.index.step == 1:
            return df, continous
        return df.set_axis(pd.RangeIndex(len(df)), axis=0, copy=False), continous

    def _detect_errors(self, input_df: DataFrame, continous_columns: List[str]) -> Any:
        ec = None
        if self.error_cells is not None:
            ec = session.resolve(self.error_cells)[[self._row_id, "attribute"]]
        em = ErrorModel(row_id=self._row_id, targets=self.targets, discrete_thres=self.discrete_thres,
                        error_detectors=self.error_detectors, error_cells=ec, opts=self.opts)
        return em.detect(input_df, continous_columns)

    def _prepare_repair_base_cells(self, input_df: DataFrame, error_cells_df: DataFrame, target_columns: List[str]) -> DataFrame:
        """RepairApi.convertErrorCellsToNull (RepairApi.scala:171-211)."""
        base = input_df.copy()
        pos = pd.Series(np.arange(len(base)), index=base[self._row_id].to_numpy())
        for a, grp in error_cells_df.groupby("attribute"):
            if a in target_columns:
                rows = pos.reindex(grp[self._row_id].to_numpy()).dropna().to_numpy(np.int64)
                col = base[a].astype(object) if not is_numeric_column(base[a]) else base[a].astype("float64") if not is_integral_column(base[a]) else base[a].astype("Int64")
                col.iloc[rows] = None if not is_numeric_column(base[a]) else pd.NA if is_integral_column(base[a]) else np.nan
                base[a] = col
        return base

    # ------------------------------------------------------------------ rule models
    def _get_functional_deps(self, target_columns: List[str]) -> Optional[Dict[str, List[str]]]:
        dets = [d for d in self.error_detectors if isinstance(d, ConstraintErrorDetector)]
        if len(dets) != 1:
            if len(dets) > 1:
                _logger.warning("Multiple constraint classes not supported for detecting functional deps")
            return None
        ced = dets[0]
        tg = [c for c in target_columns if c in ced.targets] if ced.targets else target_columns
        deps: Dict[str, List[str]] = {}
        for stmt in load_constraints(ced.constraint_path, ced.constraints):
            try:
                ps = parse_constraint(stmt)
            except Exception:
                continue
            # X -> Y  ==  EQ(t1.X,t2.X) & IQ(t1.Y,t2.Y)
            if len(ps) == 2 and ps[0].op == "EQ" and ps[1].op == "IQ" and ps[0].constant is None and ps[1].constant is None \
                    and ps[0].left == ps[0].right and ps[1].left == ps[1].right and ps[1].left in tg:
                deps.setdefault(ps[1].left, []).append(ps[0].left)
        return deps or None

    def _fd_source(self, functional_deps: Optional[Dict[str, List[str]]], y: str, domain_stats: Dict[str, int]) -> Optional[str]:
        """The attribute whose functional dependency answers target `y`: the first listed source with a domain below
        `model.rule.max_domain_size`, or None.  Asked by `_build_repair_models` and by `_resident_rules`."""
        max_dom = int(self._get_option_value(*self._opt_max_domain_size))
        fx = [x for x in (functional_deps or {}).get(y, []) if x in domain_stats and int(domain_stats[x]) < max_dom]
        return fx[0] if fx else None

    def _build_rule_model(self, train_df: DataFrame, x: str, y: str) -> Any:
        sub = train_df[[x, y]].dropna()
        g = sub.groupby(x)[y].agg(lambda s: s.iloc[0] if s.nunique() == 1 else None).dropna()
        return FunctionalDepModel(x, {k: v for k, v in g.items()})

    # ------------------------------------------------------------------ hot path: training
    def _select_features(self, pairwise_attr_stats: Dict[str, Any], y: str, features: List[str]) -> List[str]:
        max_cols = int(self._get_option_value(*self._opt_max_training_column_num))
        if max_cols < len(features) and y in pairwise_attr_stats:
            heap: List[Tuple[float, str]] = []
            for f, corr in map(tuple, pairwise_attr_stats[y]):
                if f in features:
                    heapq.heappush(heap, (float(corr), f))
            top: List[Tuple[float, str]] = []
            for corr, f in [heapq.heappop(heap) for _ in range(len(heap))]:
                if len(top) <= 1 or (corr >= 0.0 and len(top) < max_cols):
                    top.append((corr, f))
            features = [f for _, f in top]
        return features

    def _sample_training_data_from(self, df: DataFrame) -> DataFrame:
        """model.py:755-766; the reference's Bernoulli sample is unseeded, this one is seeded (42)."""
        max_rows = int(self._get_option_value(*self._opt_max_training_row_num))
        if len(df) > max_rows:
            _logger.info("To reduce training data, extracts %s%% samples from %d rows" % (100.0 * max_rows / len(df), len(df)))
            return df.sample(n=max_rows, random_state=42)
        return df

    def _training_row_sampler(self) -> Any:
        """`_sample_training_data_from` as the `train_rows` of `repair.pipeline.repair_frame` take it: (attribute, positions of its
        non-NULL rows) -> the positions to train on, or None for all of them.  It must stay the same seeded sample as
        `DataFrame.sample(n, random_state=42)` above draws from the attribute's non-NULL rows."""
        max_rows = int(self._get_option_value(*self._opt_max_training_row_num))

        def sample(_attr: str, rows: np.ndarray) -> Optional[np.ndarray]:
            if len(rows) <= max_rows:
                return None
            _logger.info("To reduce training data, extracts %s%% samples from %d rows" % (100.0 * max_rows / len(rows), len(rows)))
            return rows[np.random.RandomState(42).choice(len(rows), max_rows, replace=False)]

        return sample

    def _build_repair_stat_models_in_series(self, models: Dict[str, Any], train_df: DataFrame, target_columns: List[str],
                                            continous_columns: List[str], num_class_map: Dict[str, int],
                                            feature_map: Dict[str, List[str]]) -> Dict[str, Any]:
        opts = dict(self.opts)
        for y in [c for c in target_columns if c not in models]:
            index = len(models) + 1
            df = train_df[train_df[y].notna()]
            if len(df) == 0:
                _logger.info("Skipping %d/%d model... type=classfier y=%s num_class=%s" % (index, len(target_columns), y, num_class_map[y]))
                models[y] = (PoorModel(None), feature_map[y], None)
                continue
            train_pdf = self._sample_training_data_from(df)
            is_discrete = y not in continous_columns
            X = train_pdf[feature_map[y]]
            X, y_ = rebalance_training_data(X, train_pdf[y], y) if is_discrete and self.training_data_rebalancing_enabled else (X, train_pdf[y])
            _logger.info("Building %d/%d model... type=%s y=%s features=%s #rows=%d%s" % (
                index, len(target_columns), "classfier" if is_discrete else "regressor", y, to_list_str(feature_map[y]), len(train_pdf),
                " #class=%d" % num_class_map[y] if num_class_map[y] > 0 else ""))
            (model, score), elapsed = build_model(X, y_, is_discrete, num_class_map[y], n_jobs=-1, opts=opts)
            if model is None:
                model = PoorModel(None)
            _logger.info("Finishes building '%s' model...  score=%s elapsed=%ss (class stdv=%s)" % (
                y, score, elapsed, compute_class_nrow_stdv(y_, is_discrete)))
            models[y] = (model, feature_map[y], None)
        return models

    def _resolve_prediction_order(self, models: Dict[str, Any], target_columns: List[str]) -> List[Any]:
        ordered, pending = [], list(target_columns)
        for y in target_columns:
            if not isinstance(models[y][0], FunctionalDepModel):
                ordered.append((y, models[y])); pending.remove(y)
        while pending:
            before = len(pending)
            for y in list(pending):
                if models[y][1][0] not in pending:
                    ordered.append((y, models[y])); pending.remove(y)
            assert len(pending) < before
        return ordered

    @job_group(name="repair model training")
    def _build_repair_models(self, train_df: DataFrame, target_columns: List[str], continous_columns: List[str],
                             domain_stats: Dict[str, int], pairwise_attr_stats: Dict[str, Any]) -> List[Any]:
        train_df = train_df.drop(columns=[self._row_id])
        functional_deps = self._get_functional_deps(target_columns) if self._repair_by_functional_deps_enabled else None
        _logger.info("[Repair Model Training Phase] Building %d models to repair the cells in %s" % (len(target_columns), to_list_str(target_columns)))
        models: Dict[str, Any] = {}
        num_class_map: Dict[str, int] = {}
        for y in target_columns:
            input_columns = [c for c in train_df.columns if c != y]
            is_discrete = y not in continous_columns
            num_class_map[y] = int(train_df[y].nunique(dropna=True)) if is_discrete else 0
            if is_discrete and num_class_map[y] <= 1:
                v = train_df[y].dropna().iloc[0] if num_class_map[y] == 1 else None
                models[y] = (PoorModel(v), input_columns, None)
            x = self._fd_source(functional_deps, y, domain_stats) if y not in models else None
            if x is not None:
                models[y] = (self._build_rule_model(train_df, x, y), [x], None)
        if len(models) != len(target_columns):
            feature_map = {y: self._select_features(pairwise_attr_stats, y, [c for c in train_df.columns if c != y])
                           for y in target_columns if y not in models}
            # one process drives one GPU: the reference's "parallel" mode (model.py:817-926) is a
            # scheduling choice with identical maths, so both settings train here in series.
            models = self._build_repair_stat_models_in_series(models, train_df, target_columns, continous_columns, num_class_map, feature_map)
        assert len(models) == len(target_columns)
        if any(isinstance(m, FunctionalDepModel) for m, _, _ in models.values()):
            return self._resolve_prediction_order(models, target_columns)
        return [(y, models[y]) for y in target_columns]

    # ------------------------------------------------------------------ hot path: inference
    @job_group(name="repairing")
    def _repair(self, models: List[Any], continous_columns: List[str], dirty_rows_df: DataFrame, error_cells_df: DataFrame,
                compute_repair_candidate_prob: bool, maximal_likelihood_repair: bool) -> Tuple[DataFrame, Dict[str, Any]]:
        """The body of the reference's grouped-map UDF `repair` (model.py:1095-1135) on the whole dirty frame."""
        _logger.info("[Repairing Phase] Computing %d repair updates in %d rows..." % (len(error_cells_df), len(dirty_rows_df)))
        pdf = dirty_rows_df.copy()
        need_pmf = compute_repair_candidate_prob or maximal_likelihood_repair
        pmfs: Dict[str, Any] = {}
        for y, (model, features, _) in models:
            X = pdf[features]
            isnull = pdf[y].isna().to_numpy()
            if need_pmf and y not in continous_columns:
                predicted = model.predict_proba(X)
                # the reference stores a JSON pmf in the cell; later models then see an unknown category,
                # i.e. the cell stays "missing" for them -- so the column is left NULL here
                pmfs[y] = (list(np.asarray(model.classes_).tolist()), predicted, isnull)
            else:
                predicted = np.asarray(model.predict(X), dtype=object if y not in continous_columns else None)
                if y in continous_columns and is_integral_column(dirty_rows_df[y]):
                    predicted = np.round(predicted.astype(np.float64))
                col = pdf[y].astype(object) if y not in continous_columns else pdf[y].astype("float64")
                col = col.where(~isnull, pd.Series(predicted, index=col.index))
                if y in continous_columns and is_integral_column(dirty_rows_df[y]):
                    col = col.astype("Int64")
                pdf[y] = col
        return pdf, pmfs

    # ------------------------------------------------------------------ result shaping
    def _flatten_join(self, repaired_rows_df: DataFrame, error_cells_df: DataFrame) -> DataFrame:
        rid = self._row_id
        pos = pd.Series(np.arange(len(repaired_rows_df)), index=repaired_rows_df[rid].to_numpy())
        rp = pos.reindex(error_cells_df[rid].to_numpy()).to_numpy(np.int64)
        vals = np.empty(len(error_cells_df), object)
        for a, idx in error_cells_df.groupby("attribute").indices.items():
            v = repaired_rows_df[a].to_numpy(dtype=object)[rp[idx]]
            vals[idx] = [None if pd.isna(x) else _to_str(x) for x in v]
        return error_cells_df.assign(repaired=vals)

    def _compute_repair_pmf(self, pmfs: Dict[str, Any], repaired_rows_df: DataFrame, dirty_rows_df: DataFrame,
                            error_cells_df: DataFrame, continous_columns: List[str]) -> DataFrame:
        rid = self._row_id
        thres = float(self._get_option_value(*self._opt_prob_threshold))
        top_k = int(self._get_option_value(*self._opt_prob_top_k))
        weight = float(self._get_option_value(*self._opt_cost_weight))
        pos = pd.Series(np.arange(len(dirty_rows_df)), index=dirty_rows_df[rid].to_numpy())
        rows = []
        for r in error_cells_df.itertuples(index=False):
            rowid, attr, cur = r[0], r[1], r[2]
            i = int(pos[rowid])
            if attr in continous_columns:
                v = repaired_rows_df[attr].iloc[i]
                rows.append((rowid, attr, {"value": cur, "prob": 0.0}, [{"class": None if pd.isna(v) else _to_str(v), "prob": 1.0}]))
                continue
            classes, predicted, _ = pmfs[attr]
            probs = predicted[i]
            if probs is None:
                cls, pr = [], []
            else:
                # a PoorModel(None) target (every label NULL) has the single class NULL, not the string 'None'
                cls = [None if c is None else _to_str(c) for c in classes]
                pr = [float(p) for p in np.asarray(probs)[:len(classes)]]
            if self.cf is not None and pr:
                # _compute_weighted_probs (model.py:1145-1165): costs weigh the probs of the cost function's targets only,
                # but the renormalisation runs for every attribute once a cost function is set
                if not self.cf.targets or attr in self.cf.targets:
                    costs = [self.cf.compute(cur, c) for c in cls] if cur else None
                    if costs is not None:
                        pr = [p * (1.0 / (1.0 + weight * c)) if c is not None else p for p, c in zip(pr, costs)]
                # the reference's `aggregate(probs, 0.0, (acc, x) -> acc + x)` (model.py:1158): a plain left-to-right double sum.
                # Not `sum()`: from Python 3.12 on it is a compensated sum and rounds differently.
                norm = 0.0
                for p in pr:
                    norm = norm + p
                pr = [p / norm for p in pr] if norm > 0 else pr
            cur_prob = pr[cls.index(cur)] if cur in cls else 0.0
            order = sorted(range(len(cls)), key=lambda j: -pr[j])   # stable: ties keep class order
            pmf = [{"class": cls[j], "prob": pr[j]} for j in order if pr[j] > thres][:top_k]
            rows.append((rowid, attr, {"value": cur, "prob": cur_prob}, pmf))
        return pd.DataFrame(rows, columns=[rid, "attribute", "current_value", "pmf"])

    def _compute_score(self, pmf_df: DataFrame) -> DataFrame:
        assert self.cf is not None
        out = []
        for r in pmf_df.itertuples(index=False):
            cur, pmf = r.current_value, r.pmf
            rep = pmf[0] if pmf else {"class": None, "prob": 0.0}
            base = cur["value"] if cur["value"] is not None else rep["class"]
            cost = self.cf.compute(base, rep["class"])
            p_cur = cur["prob"] if cur["prob"] > 0.0 else 1e-6
            score = float(np.log(rep["prob"] / p_cur)) * (1.0 / (1.0 + (cost if cost is not None else 256.0))) if rep["prob"] > 0 else float("-inf")
            out.append((r[0], r.attribute, cur["value"], rep["class"], score))
        return pd.DataFrame(out, columns=[self._row_id, "attribute", "current_value", "repaired", "score"])

    def _maximal_likelihood_repair(self, score_df: DataFrame, error_cells_df: DataFrame) -> DataFrame:
        assert self.repair_delta is not None
        n = len(error_cells_df)
        percent = min(1.0, 1.0 - self.repair_delta / n)
        thres = float(np.percentile(score_df["score"].to_numpy(np.float64), percent * 100.0)) if n else 0.0
        top = score_df[score_df["score"] >= thres].drop(columns=["score"])
        _logger.info("[Repairing Phase] %d repair updates (delta=%d) selected among %d candidates" % (len(top), self.repair_delta, n))
        return top

    def _repair_attrs(self, updates: DataFrame, base: DataFrame) -> DataFrame:
        """RepairMiscApi.repairAttrsFrom (RepairMiscApi.scala:184-247): apply (row_id, attribute, repaired) updates to a table.
        `repaired` arrives as strings; continuous attributes are cast back (`CAST(.. AS DOUBLE)` accepts Java's `3.1D`
        spelling), integral ones through `round` (half-up, as Spark rounds doubles) first (lines 224-229)."""
        out = base.copy()
        pos = pd.Series(np.arange(len(out)), index=out[self._row_id].to_numpy())
        for a, grp in updates.groupby("attribute"):
            if a not in out.columns:
                continue
            rows = pos.reindex(grp[self._row_id].to_numpy()).to_numpy(np.float64)
            keep = ~np.isnan(rows)                            # updates of unknown rows vanish in the LEFT OUTER JOIN
            rows = rows[keep].astype(np.int64)
            vals = grp["repaired"].to_numpy(dtype=object)[keep]
            if is_numeric_column(base[a]):
                num = np.array([_to_double(v) for v in vals], np.float64)
                if is_integral_column(base[a]):
                    num = np.where(np.isnan(num), np.nan, np.sign(num) * np.floor(np.abs(num) + 0.5))
                    col = out[a].astype("Int64")
                    col.iloc[rows] = pd.array([pd.NA if np.isnan(v) else int(v) for v in num], dtype="Int64")
                else:
                    col = out[a].astype("float64")
                    col.iloc[rows] = num
            else:
                col = out[a].astype(object)
                col.iloc[rows] = vals
            out[a] = col
        return out

    def _repair_by_nearest_values(self, repair_base_df: DataFrame, error_cells_df: DataFrame, target_columns: List[str]) -> Tuple[DataFrame, DataFrame]:
        assert self.cf is not None
        targets = [c for c in target_columns if c in self.cf.targets] if self.cf.targets else target_columns
        merge_thres = float(self._get_option_value(*self._opt_merge_threshold))
        rep = np.empty(len(error_cells_df), object)
        dom = {c: list(pd.unique(repair_base_df[c].dropna())) for c in targets}
        for i, r in enumerate(error_cells_df.itertuples(index=False)):
            rep[i] = None
            r = type('R', (), dict(attribute=r[1], current_value=r[2]))
            if r.attribute in dom and r.current_value:
                costs = sorted(((self.cf.compute(r.current_value, _to_str(v)), _to_str(v)) for v in dom[r.attribute]),
                               key=lambda t: (t[0] is None, t[0]))
                costs = [c for c in costs if c[0] is not None]
                if costs and costs[0][0] <= merge_thres and (len(costs) == 1 or costs[0][0] < costs[1][0]):
                    rep[i] = costs[0][1]
        done = pd.notna(pd.Series(rep)).to_numpy()
        repaired = error_cells_df[done].assign(repaired=rep[done])
        return error_cells_df[~done], repaired

    def _regex_programs(self) -> List[Tuple[str, Any]]:
        """(attribute, program) of every RegExErrorDetector, in list order, whose pattern gives a structure to repair with
        (`repair.regex_structure.parse`); a pattern that does not is logged with the reason and repairs nothing, as in
        `RepairApi.repairByRegularExpression` (RepairApi.scala:698-703).  (The reference's DomainValues is no RegExErrorDetector.)"""
        from repair.regex_structure import NotRepairable, parse
        out: List[Tuple[str, Any]] = []
        for d in self.error_detectors:
            if isinstance(d, RegExErrorDetector) and not isinstance(d, DomainValues):
                try:
                    out.append((d.attr, parse(d.regex)))
                except NotRepairable as e:
                    _logger.warning("Repairing using regex '%s' (attr='%s') failed because: %s" % (d.regex, d.attr, e))
        if len({a for a, _ in out}) < len(out):
            _logger.info("[Repairing Phase] several regexs on one attribute: the first that repairs a cell wins (the reference's union "
                         "would list the cell once per regex)")
        return out

    def _repair_by_regexs(self, input_df: DataFrame, error_cells_df: DataFrame) -> Tuple[DataFrame, DataFrame]:
        """Reference model.py:629-651 with `RegexStructureRepair` stated in `repair.regex_structure`: per RegExErrorDetector, in list
        order, the remaining error cells of its attribute whose current value (as a string, `_sql_strs`) fits the structure of the
        regex are rewritten from it; every distinct string is evaluated once.  They leave the error cells."""
        from repair.regex_structure import repair_cells
        programs = self._regex_programs()
        attrs = error_cells_df["attribute"].to_numpy(dtype=object)
        cur = error_cells_df["current_value"].to_numpy(dtype=object)
        rep = np.empty(len(error_cells_df), object)
        done = np.zeros(len(error_cells_df), bool)
        if programs:
            _logger.info("[Repairing Phase] Repairing data using the regexs of: %s" % to_list_str([a for a, _ in programs]))
        for attr, program in programs:
            idx = np.flatnonzero((attrs == attr) & ~done)
            if not len(idx) or attr not in input_df.columns:
                continue
            integral = is_numeric_column(input_df[attr]) and is_integral_column(input_df[attr])
            values, skipped = repair_cells(program, _sql_strs(cur[idx], integral))
            if skipped:
                _logger.info("[Repairing Phase] %d cells of `%s` hold a line terminator: left to the models" % (skipped, attr))
            for i, v in zip(idx, values):
                if v is not None:
                    rep[i], done[i] = v, True
        return error_cells_df[~done], error_cells_df[done].assign(repaired=rep[done])

    # ------------------------------------------------------------------ resident (device) path
    def _resident_engine(self) -> Any:
        """The engine of the HBM-resident path, or None: no HIP device, the estimator backend was swapped (CPU tests), or
        REPAIR_RESIDENT=0.  Tests inject one through `_engine_override`."""
        hook = getattr(self, "_engine_override", None)
        if hook is not None:
            return hook
        from repair import _native, gbm
        from repair.engine import resident_engine
        if gbm.get_backend() is not _native:
            return None
        return resident_engine(self._get_option_value(*self._opt_gpu_device_id))

    def _resident_plan(self, input_df: DataFrame, target_columns: List[str], continous_columns: List[str], domain_stats: Dict[str, int],
                       compute_repair_candidate_prob: bool, maximal_likelihood_repair: bool, prob_modes: bool = False) -> Optional[Dict[str, Any]]:
        """Decides whether this run can take the HBM-resident pipeline (repair.pipeline) and with which parameters.
        `prob_modes`: the caller shapes the probability modes itself (`_resident_result`), so they and a cost function qualify.

        It can when everything between error detection and the result frame is the per-attribute model loop itself:
        no rule-based repairs, no functional-dependency rule models, no rebalancing (unless `model.rebalance.resident` is set: the plan
        then carries `rebalance`), no cost function, plain repair output
        (cells or repaired data), no feature selection, and every discrete target has at least two classes.  The
        hyper-parameter search (`model.hp.max_evals` > 1) runs on the resident tables too (pipeline.search_on_table).
        Otherwise the value-space path (pandas + one estimator per attribute) below handles the run.

        With `model.rule.resident` set, `setRepairByRules(True)` qualifies as well (`_resident_rules`): the plan then carries `rules`."""
        rules = None
        if self.repair_by_rules:
            if not bool(self._get_option_value(*self._opt_rule_resident)):
                return None
            rules = self._resident_rules(input_df, target_columns, continous_columns, domain_stats,
                                         compute_repair_candidate_prob or maximal_likelihood_repair)
            if rules is None:
                return None
        elif not prob_modes and (compute_repair_candidate_prob or maximal_likelihood_repair or self.cf is not None):
            return None
        rebalance = None
        if self.training_data_rebalancing_enabled:
            if not bool(self._get_option_value(*self._opt_rebalance_resident)):
                return None
            from repair import dist
            if dist.world()[1] > 1:
                _logger.info("rebalancing stays on the value-space path: a multi-rank job does not rebalance its row shards")
                return None
            rebalance = dict(k=5, random_state=42)
        from repair.train import (_opt_learning_rate, _opt_max_bin, _opt_max_depth, _opt_max_evals, _opt_min_split_gain,
                                  _opt_n_estimators, _opt_reg_alpha, _opt_boosting_type, _opt_class_weight)
        g = lambda o: get_option_value(self.opts, *o)  # noqa: E731
        if g(_opt_boosting_type) != "gbdt" or g(_opt_class_weight) != "balanced":
            return None
        features = len(input_df.columns) - 2
        if int(self._get_option_value(*self._opt_max_training_column_num)) < features:
            return None
        if rules is None and self._repair_by_functional_deps_enabled and self._get_functional_deps(target_columns):
            return None
        for y in target_columns:
            if y not in continous_columns and int(domain_stats.get(y, 0)) < 2:
                return None
        max_depth = int(g(_opt_max_depth))
        if not 1 <= max_depth:
            return None
        engine = self._resident_engine()
        if engine is None:
            return None
        params = dict(n_estimators=int(g(_opt_n_estimators)), learning_rate=float(g(_opt_learning_rate)), max_depth=max_depth,
                      max_bin=int(g(_opt_max_bin)), lambda_l1=float(g(_opt_reg_alpha)), min_gain_to_split=float(g(_opt_min_split_gain)),
                      num_leaves=31, min_data_in_leaf=20, min_sum_hessian_in_leaf=1e-3, lambda_l2=0.0, bagging_fraction=1.0, bagging_freq=0,
                      feature_fraction=1.0, seed=42)
        distinct = None
        if bool(self._get_option_value(*self._opt_train_distinct_rows)):
            distinct = dict(max_ratio=float(self._get_option_value(*self._opt_train_distinct_rows_max_ratio)))
        return dict(engine=engine, params=params, search=int(g(_opt_max_evals)) > 1, rules=rules, distinct=distinct, rebalance=rebalance)

    def _resident_rules(self, input_df: DataFrame, target_columns: List[str], continous_columns: List[str], domain_stats: Dict[str, int],
                        prob_modes: bool) -> Optional[Dict[str, Any]]:
        """The rule-based repairs of this run as the `rules` of `repair.pipeline.repair_frame` take them, or None (with the reason in the
        log) where the resident pipeline does not restate them: the probability modes, regex-structure repair without
        `model.rule.regex.resident` (or together with nearest-value merges, or on a column that does not hold strings), an FD model for a
        continuous attribute or from a continuous target (its chain value is the raw prediction, not a dictionary entry), a cycle
        among the FD sources."""
        from repair.costs import Levenshtein

        def no(reason: str) -> None:
            _logger.info("rule-based repairs stay on the value-space path: %s" % reason)

        if prob_modes:
            return no("the probability modes are combined with rules")
        regex = None
        if self._repair_by_regex_enabled:
            if not bool(self._get_option_value(*self._opt_rule_regex_resident)):
                return no("regex-structure repair is enabled")
            if self._repair_by_nearest_values_enabled:
                # the merges read their domains from the table BEFORE the regex repairs are written (model.py `_run`); the resident table
                # is built with them
                return no("regex-structure repair together with nearest-value merges")
            regex = []
            for attr, program in self._regex_programs():
                if attr not in input_df.columns or attr not in target_columns:
                    continue
                if is_numeric_column(input_df[attr]) or pd.api.types.infer_dtype(input_df[attr], skipna=True) != "string":
                    return no("regex-structure repair of `%s`, which is not a column of strings" % attr)
                regex.append(dict(attr=attr, program=program, current_str=lambda a, values: _sql_strs(values, False)))
        fd: Dict[str, str] = {}
        deps = self._get_functional_deps(target_columns) if self._repair_by_functional_deps_enabled else None
        for y in target_columns:
            x = self._fd_source(deps, y, domain_stats)
            if x is None:
                continue
            if y in continous_columns:
                return no("an FD model for the continuous attribute `%s`" % y)
            if x in continous_columns and x in target_columns:
                return no("the FD source `%s` of `%s` is a continuous target" % (x, y))
            fd[y] = x
        for y in fd:
            seen, x = {y}, fd[y]
            while x in fd:
                if x in seen:
                    return no("a cycle among the FD sources of `%s`" % y)
                seen.add(x)
                x = fd[x]
        nearest = None
        if self._repair_by_nearest_values_enabled:
            cf = self.cf
            assert cf is not None
            integral = {c for c in input_df.columns if is_numeric_column(input_df[c]) and is_integral_column(input_df[c])}

            def current_str(attr: str, values: List[Any]) -> List[Any]:
                return _sql_strs(values, attr in integral)

            def domain_str(attr: str, values: List[Any]) -> List[Any]:
                # `_to_str` of the column's values as `_repair_by_nearest_values` reads them from the frame
                return [str(int(v)) if attr in integral else _to_str(float(v) if isinstance(v, (float, np.floating)) else v) for v in values]

            nearest = dict(targets=[c for c in target_columns if c in cf.targets] if cf.targets else list(target_columns),
                           threshold=float(self._get_option_value(*self._opt_merge_threshold)),
                           cost=None if type(cf) is Levenshtein else cf.compute, current_str=current_str, domain_str=domain_str)
        return dict(fd=fd, nearest=nearest, regex=regex or None)

    def _detector_conditions(self, input_df: DataFrame, continous_columns: List[str], detectors: List[ErrorDetector],
                             why: Optional[List[str]] = None) -> Optional[Dict[str, Any]]:
        """The DETECTOR conditions of a device-side detection, stated once for `_device_detection_plan` and `_device_detect_only_plan`:
        no `setErrorCells`, no detector with `targets` of its own, the detector types admitted under their options (docstring of
        `_device_detection_plan`), and every constraint that is not `X -> Y` passing `repair.dc_codes.check_constraint`.  Returns
        dict(cols, constraints, value_detectors (the outlier / LOF kinds still without their `attrs`), detect_nulls, domain_stats) or None;
        `why`, where given, then receives the reason."""
        def no(reason: str) -> None:
            if why is not None:
                why.append(reason)
            return None

        from repair.pipeline import constraint_to_columns
        value_resident = bool(self._get_option_value(*self._opt_value_detectors_resident))
        lof_resident = bool(self._get_option_value(*self._opt_lof_resident))
        constraints_resident = bool(self._get_option_value(*self._opt_constraints_resident))
        general: List[Any] = []      # the parsed predicates of the constraints that are not `X -> Y`
        vdets: List[Dict[str, Any]] = []
        if self.error_cells is not None:
            return no("the error cells are given (`setErrorCells`)")
        cols = [c for c in input_df.columns if c != self._row_id]
        cons: List[Any] = []          # ([x names], y name) of `X -> Y` constraints; the parsed predicates of any other one
        has_null = False
        for d in detectors:
            if getattr(d, "targets", None):
                return no("%s has targets of its own" % d)
            if type(d) is NullErrorDetector:
                has_null = True
            elif type(d) is ConstraintErrorDetector:
                stmts = load_constraints(d.constraint_path, d.constraints)
                try:
                    plist = parse_and_verify_constraints(stmts, list(input_df.columns)) if stmts else []
                except Exception:  # noqa: BLE001 - the pandas detector reports malformed constraints
                    return no("%s does not parse" % d)
                for preds in plist:
                    cc = constraint_to_columns(preds, cols)
                    if cc is not None:
                        cons.append(([cols[i] for i in cc[0]], cols[cc[1]]))
                    elif constraints_resident:
                        general.append(preds)
                        cons.append(preds)
                    else:
                        return no("constraint %s is not `X -> Y` and `%s` is not set" % (preds, self._opt_constraints_resident.key))
            elif value_resident and type(d) is RegExErrorDetector:
                vdets.append(dict(kind="regex", attr=d.attr, regex=d.regex))
            elif value_resident and type(d) is DomainValues:
                if d.attr not in continous_columns:          # `DomainValues._detect_impl`: nothing on a continuous attribute
                    vdets.append(dict(kind="domain", attr=d.attr, values=list(d.values), autofill=bool(d.autofill),
                                      min_count_thres=d.min_count_thres))
            elif value_resident and type(d) is GaussianOutlierErrorDetector:
                vdets.append(dict(kind="outlier", attrs=None))
            elif lof_resident and type(d) is LOFOutlierErrorDetector:
                # (`parallel_mode_threshold` / `num_parallelism` change nothing on the value-space path of this engine either)
                vdets.append(dict(kind="lof", attrs=None, k=int(d.error_detector_cls().n_neighbors)))
            else:
                return no("%s is not a detector the resident table restates under the options set" % d)
        from repair.utils import column_nunique
        domain_stats = {c: column_nunique(input_df, c) for c in cols}
        for preds in general:
            from repair.dc_codes import NotLowerable, check_constraint
            try:
                check_constraint(preds, cols, domain_stats)
            except NotLowerable as e:
                _logger.info("[Error Detection Phase] constraint %s stays with the value-space detector: %s" % (preds, e))
                return no("constraint %s does not lower: %s" % (preds, e))
        return dict(cols=cols, constraints=cons, value_detectors=vdets, detect_nulls=has_null, domain_stats=domain_stats)

    def _outlier_columns_ok(self, input_df: DataFrame, vdets: List[Dict[str, Any]], read: List[str]) -> bool:
        """The column checks of the outlier and LOF detectors on the continuous attributes `read` that detection looks at; fills their `attrs`."""
        if any(d["kind"] == "lof" and d["k"] >= len(input_df) // 2 for d in vdets):
            # scikit-learn searches so small a table by brute force, with inexact distances (`detect_codes.build_descriptors`)
            return False
        if any(d["kind"] in ("outlier", "lof") for d in vdets):
            # the columns the outlier and LOF detectors read: plain numpy numeric ones only (`pd.to_numeric(.., errors="coerce")` of anything else
            # and the masked comparison of a nullable column stay with the pandas detector), integers within float64's exact range (the
            # dictionaries are float64)
            for c in read:
                if not isinstance(input_df[c].dtype, np.dtype) or not is_numeric_column(input_df[c]):
                    return False
                if pd.api.types.is_integer_dtype(input_df[c]) and len(input_df) and input_df[c].notna().any() \
                        and float(input_df[c].abs().max()) >= 2.0 ** 53:
                    return False
                if any(d["kind"] == "lof" for d in vdets) and len(input_df) and input_df[c].notna().any():
                    # scikit-learn refuses an infinite value, and its squared distances overflow on a wider span: its errors to report
                    x = input_df[c].to_numpy(dtype=np.float64)
                    with np.errstate(over="ignore", invalid="ignore"):
                        if not float(np.nanmax(x) - np.nanmin(x)) <= LOF_MAX_RANGE:
                            return False
            for d in vdets:
                if d["kind"] in ("outlier", "lof"):
                    d["attrs"] = list(read)
        return True

    def _device_detection_plan(self, input_df: DataFrame, continous_columns: List[str], compute_repair_candidate_prob: bool,
                               maximal_likelihood_repair: bool) -> Optional[Dict[str, Any]]:
        """Can error DETECTION run on the resident table as well (reference python/repair/errors.py:545-582)?  Yes when the error
        cells come from NULL / denial-constraint detectors only (no own target lists; every constraint in the form the device
        detector handles, `pipeline.constraint_to_columns`) and the rest of the run qualifies for the resident pipeline: the
        frame is then encoded once and `pipeline.repair_frame` detects, NULLs, trains and repairs without an `error_cells_df` ever
        being built in pandas.

        With `error.value_detectors.resident` set, RegExErrorDetector, DomainValues and GaussianOutlierErrorDetector (exactly these
        types) qualify too: on the encoded table they are predicates on the dictionary codes (repair.detect_codes), found together
        with the NULL cells by one `Table.detect_cells` call.  The plan then carries `value_detectors`.

        With `error.lof.resident` set, LOFOutlierErrorDetector (exactly this type) qualifies too: its factor is a function of the
        dictionary entry (repair.lof_codes; `engine.lof_codes`, rgbm_lof_1d on the device), lowered to the same code predicates.  Not
        for a table of so few rows that scikit-learn searches it by brute force (n_neighbors >= rows // 2: inexact distances), nor for
        a column with an infinite value or a span beyond `detect_codes.LOF_MAX_RANGE` (scikit-learn raises there).

        With `error.constraints.resident` set, every other constraint `repair.dc_codes.check_constraint` accepts qualifies as well
        (single-tuple constants, several IQs, LT / GT): the plan carries its parsed predicates next to the `X -> Y` tuples and
        `pipeline.repair_frame` lowers them against the dictionaries.  A constraint that does not lower sends the run to the value-space
        path, as before, with the reason logged.  With `error.constraints.order_scan` set as well the plan carries `order_scan=True`:
        `pipeline.repair_frame` then sends the order constraints among them to `Table.detect_dc_scan`."""
        if not self.error_detectors:
            return None
        dets = self._detector_conditions(input_df, continous_columns, self.error_detectors)
        if dets is None:
            return None
        cols, cons, vdets, has_null, domain_stats = dets["cols"], dets["constraints"], dets["value_detectors"], dets["detect_nulls"], dets["domain_stats"]
        discretized = [c for c in cols if c in continous_columns or 1 < domain_stats[c] <= self.discrete_thres]
        cands = [c for c in (self.targets if self.targets else cols) if c in discretized]
        if not cands:
            return None
        # Error cells OUTSIDE the discretizable candidates must be seen by the pandas detectors: with noisy cells there and none in a
        # candidate the reference raises "At least one valid discretizable feature ..." (model.py `_run`), which the device path --
        # detecting in the candidates only -- would report as "already clean" (ADVICE r3).  Cheap host checks, before anything is uploaded.
        others = [c for c in (self.targets if self.targets else cols) if c in cols and c not in cands]
        if others and has_null and bool(input_df[others].isna().to_numpy().any()):
            return None
        if others and any(a in others for con in cons
                          for a in (list(con[0]) + [con[1]] if isinstance(con, tuple) else [r for p in con for r in p.references])):
            return None
        if others and any(d["kind"] not in ("outlier", "lof") and d["attr"] in others for d in vdets):
            return None
        if not self._outlier_columns_ok(input_df, vdets, [c for c in continous_columns if c in cands]):
            return None
        plan = self._resident_plan(input_df, cands, continous_columns, domain_stats, compute_repair_candidate_prob, maximal_likelihood_repair)
        if plan is None:
            return None
        plan.update(candidates=cands, constraints=cons, detect_nulls=has_null, value_detectors=vdets or None)
        if bool(self._get_option_value(*self._opt_constraints_resident)) and bool(self._get_option_value(*self._opt_constraints_order_scan)):
            plan.update(order_scan=True)
        eopts = ErrorModel(row_id=self._row_id, targets=self.targets, discrete_thres=self.discrete_thres, error_detectors=self.error_detectors,
                           error_cells=None, opts=self.opts)._checked_options()
        if eopts[ErrorModel._opt_domain_analysis_enabled.key]:
            # the reference's cell-domain analysis on the same resident table (repair.pipeline.analyse_cell_domains)
            plan.update(domain_analysis=dict(options=eopts, discrete_thres=self.discrete_thres, continuous_columns=list(continous_columns)))
        return plan

    def _device_detect_only_plan(self, input_df: DataFrame, continous_columns: List[str]) -> Optional[Dict[str, Any]]:
        """Can `run(detect_errors_only=True)` run on the resident table (option `error.detect_only.resident`)?  The DETECTOR conditions
        of `_device_detection_plan` (`_detector_conditions`, `_outlier_columns_ok`) and an engine; none of `_resident_plan`'s model
        conditions, and no "error cells outside the candidates" check: detection looks at ALL target attributes
        (`ErrorModel._target_attrs`) and every cell is returned, repairable or not.  An empty detector list means the reference's defaults
        (`ErrorModel._default_detectors`), which qualify when `error.value_detectors.resident` is set."""
        emodel = ErrorModel(row_id=self._row_id, targets=self.targets, discrete_thres=self.discrete_thres, error_detectors=self.error_detectors,
                            error_cells=None, opts=self.opts)
        def no(reason: str) -> None:
            _logger.info("[Error Detection Phase] device-side detection not taken: %s" % reason)
            return None

        why: List[str] = []
        dets = self._detector_conditions(input_df, continous_columns, self.error_detectors or emodel._default_detectors(input_df), why)
        if dets is None:
            return no(why[0])
        tattrs = emodel._target_attrs(list(input_df.columns))
        if not tattrs or len(input_df) == 0:
            return no("no target attribute, or no row")
        if not self._outlier_columns_ok(input_df, dets["value_detectors"], [c for c in continous_columns if c in tattrs]):
            return no("a continuous attribute that the outlier detectors of the resident table do not read as pandas does")
        engine = self._resident_engine()
        if engine is None:
            return no("no engine for the resident table")
        plan = dict(engine=engine, targets=tattrs, constraints=dets["constraints"], detect_nulls=dets["detect_nulls"],
                    value_detectors=dets["value_detectors"] or None,
                    order_scan=bool(self._get_option_value(*self._opt_constraints_resident))
                    and bool(self._get_option_value(*self._opt_constraints_order_scan)))
        eopts = emodel._checked_options()
        if eopts[ErrorModel._opt_domain_analysis_enabled.key]:
            plan.update(domain_analysis=dict(options=eopts, discrete_thres=self.discrete_thres, continuous_columns=list(continous_columns)))
        return plan

    def _detect_only_attempt(self, plan: Dict[str, Any], input_df: DataFrame, continous_columns: List[str]) -> Optional[DataFrame]:
        """`pipeline.detect_frame` with the plan, or None (with the reason in the log) when the run turns out not to qualify."""
        import time
        from repair.pipeline import NotResidentEligible, detect_frame
        vdets = None
        if plan.get("value_detectors"):
            from repair.detect_codes import build_descriptors

            def build(*a: Any, **kw: Any) -> Any:
                # whatever stops the restatement is the value-space detector's to report (as in `_resident_run`)
                try:
                    return build_descriptors(*a, **kw)
                except NotResidentEligible:
                    raise
                except Exception as e:  # noqa: BLE001
                    raise NotResidentEligible("value detectors: %s" % e)

            vdets = dict(detectors=plan["value_detectors"], build=build)
        _logger.info("[Error Detection Phase] on the HBM-resident table, target attributes %s" % to_list_str(plan["targets"]))
        t0 = time.perf_counter()
        try:
            frame, info = detect_frame(plan["engine"], input_df, self._row_id, targets=plan["targets"], constraints=plan["constraints"],
                                       detect_nulls=plan["detect_nulls"], value_detectors=vdets, domain_analysis=plan.get("domain_analysis"),
                                       order_scan=plan["order_scan"], continuous_columns=list(continous_columns), want_details=True)
        except NotResidentEligible as e:
            self._last_resident_info = None
            self._last_detection_on_device = False
            _logger.info("device-side detection not taken: %s" % e)
            return None
        info["times"]["pipeline_wall"] = time.perf_counter() - t0
        self._last_resident_info = info
        self._last_detection_on_device = True
        return frame

    def _cost_spec(self, engine: Any, attr: str, classes: Any, cur: List[Any], ml: bool) -> Dict[str, Any]:
        """The update costs of one target's cells as `repair.pipeline.repair_table(pmf_costs=...)` takes them, from the values
        `_compute_repair_pmf` / `_compute_score` see: the error cells' current values and `_to_str` of the classes.  One cost row per
        distinct current value plus the self row (each class against itself: the score's base when a cell has no current value);
        None costs are NaN.  Raises NotResidentEligible where the Python expressions would not be reproduced (a division by zero, a
        NaN cost, a matrix over 2^28 entries)."""
        from repair.costs import Levenshtein
        from repair.pipeline import NotResidentEligible
        cls = [_to_str(c) for c in classes]
        code = {c: i for i, c in enumerate(cls)}
        cur_code = np.array([code.get(v, -1) if v is not None else -1 for v in cur], np.int32)
        cf = self.cf
        if cf is None:
            return dict(cost=None, cur_code=cur_code, weight=0.0, renormalise=False)
        weight = float(self._get_option_value(*self._opt_cost_weight))
        if cf.targets and attr not in cf.targets:        # no re-weighting, but the renormalisation runs for every attribute
            return dict(cost=None, cur_code=cur_code, weight=weight, renormalise=True)
        vals = list(dict.fromkeys(v for v in cur if v is not None))
        K = len(cls)
        if (len(vals) + 1) * K > (1 << 28):
            raise NotResidentEligible("attribute `%s`: the cost matrix would hold %d x %d entries" % (attr, len(vals) + 1, K))
        cost = np.full((len(vals) + 1, K), np.nan, np.float64)
        if type(cf) is Levenshtein:
            # compute() is None for a falsy side: those rows / columns stay NaN
            rv = [i for i, v in enumerate(vals) if v]
            kc = [j for j, c in enumerate(cls) if c]
            if rv and kc:
                d = engine.edit_distance([str(vals[i]) for i in rv], [cls[j] for j in kc]).astype(np.float64)
                cost[np.ix_(rv, kc)] = d
            cost[len(vals), kc] = 0.0
        else:
            nan_seen = False
            for i, v in enumerate(list(vals) + [None]):
                for j, c in enumerate(cls):
                    x = cf.compute(v if v is not None else c, c)
                    if x is not None:
                        cost[i, j] = float(x)
                        nan_seen = nan_seen or np.isnan(cost[i, j])
            if nan_seen:
                raise NotResidentEligible("attribute `%s`: the cost function returned NaN" % attr)
        # a falsy current value is never weighed (`if cur`) but is the score's base: its costs must all be None, as compute() gives them
        if any(not v and not np.isnan(cost[i]).all() for i, v in enumerate(vals)):
            raise NotResidentEligible("attribute `%s`: the cost function has costs for an empty current value" % attr)
        body = cost[:len(vals)]
        with np.errstate(invalid="ignore"):
            if bool(((1.0 + weight * body) == 0.0).any()) or (ml and bool(((1.0 + cost) == 0.0).any())):
                raise NotResidentEligible("attribute `%s`: a cost makes a weight 1 / 0" % attr)
        row_of = {v: i for i, v in enumerate(vals)}
        cost_row = np.array([row_of[v] if v is not None else -1 for v in cur], np.int32)
        return dict(cost=cost, cost_row=cost_row, cur_code=cur_code, weight=weight, renormalise=True)

    def _current_values_by_position(self, input_df: DataFrame, error_cells_df: DataFrame) -> Any:
        """(attribute, ascending row positions) -> the current values of those error cells as `error_cells_df` holds them: what the cost
        functions see on the value-space path (`_repair_by_nearest_values`, `_compute_repair_pmf`)."""
        rid = self._row_id
        rpos = pd.Series(np.arange(len(input_df)), index=input_df[rid].to_numpy()).reindex(error_cells_df[rid].to_numpy()).to_numpy(np.int64)
        curv = error_cells_df["current_value"].to_numpy(dtype=object)
        by_attr = {}
        for a, idx in error_cells_df.groupby("attribute").indices.items():
            o = np.argsort(rpos[idx], kind="stable")
            by_attr[a] = (rpos[idx][o], curv[idx][o])
        return lambda a, rows: list(by_attr[a][1][np.searchsorted(by_attr[a][0], rows)])

    def _resident_run(self, plan: Dict[str, Any], input_df: DataFrame, target_columns: List[str], continous_columns: List[str],
                      error_cells_df: Optional[DataFrame], compute_repair_candidate_prob: bool, compute_repair_prob: bool,
                      compute_repair_score: bool, repair_data: bool, maximal_likelihood_repair: bool) -> DataFrame:
        """Steps 2 and 3 of `_run` on the device: the table is encoded once (dictionary indices -> codes, on the device), error
        cells are NULLed, the dirty rows split off, one model per target attribute trained and the chained repair run without
        the table leaving HBM (repair.pipeline.repair_frame); the host only shapes the (small) list of repaired cells.

        `error_cells_df` None: detection runs on the resident table as well (`_device_detection_plan`; `target_columns` are its
        candidates), so no `error_cells_df` is ever built in pandas.

        The probability modes (option `repair.pmf.resident`): the candidate distributions, the update-cost re-weighting and the score
        inputs come from the resident pipeline too (rgbm_table_repair_pmf_weighted, rgbm_edit_distance); the host shapes the frames of
        the value-space branch (`_compute_repair_pmf`, `_compute_score`, `_maximal_likelihood_repair`), the score's log vectorised."""
        import time
        from repair.pipeline import NotResidentEligible, repair_frame
        rid = self._row_id
        detect = error_cells_df is None
        prob = compute_repair_candidate_prob or maximal_likelihood_repair       # `_resident_plan` admits them with given cells only
        rules = plan.get("rules")
        if detect:
            if repair_data and not plan["detect_nulls"]:
                raise NotResidentEligible("repair_data without a NULL detector: NULL target cells of dirty rows would stay NULL")
            vdets = None
            if plan.get("value_detectors"):
                from repair.detect_codes import build_descriptors

                def build(*a: Any, **kw: Any) -> Any:
                    # whatever stops the restatement (a malformed pattern, a dictionary that does not cast back to the column's dtype)
                    # is the value-space detector's to report
                    try:
                        return build_descriptors(*a, **kw)
                    except NotResidentEligible:
                        raise
                    except Exception as e:  # noqa: BLE001
                        raise NotResidentEligible("value detectors: %s" % e)

                vdets = dict(detectors=plan["value_detectors"], build=build)
            cells = dict(constraints=plan["constraints"], detect_nulls=plan["detect_nulls"], only_noisy_targets=True,
                         domain_analysis=plan.get("domain_analysis"), value_detectors=vdets, order_scan=bool(plan.get("order_scan")))
            _logger.info("[Error Detection + Repair Model Training Phase] on the HBM-resident table, candidate attributes %s" % to_list_str(target_columns))
        else:
            if repair_data and not prob:
                # The repair UDF fills EVERY NULL target cell of a dirty row (model.py:1128,1133), the cell list below only the error
                # cells: with setErrorCells / non-NULL detectors a dirty row may hold further NULLs -- those runs keep the value-space path.
                dirty = input_df[rid].isin(set(error_cells_df[rid].tolist())).to_numpy()
                nulls_in_dirty = int(input_df.loc[dirty, target_columns].isna().to_numpy().sum())
                null_error_cells = int(error_cells_df["current_value"].isna().to_numpy().sum())
                if nulls_in_dirty > null_error_cells:
                    raise NotResidentEligible("%d NULL target cells of dirty rows are not error cells" % (nulls_in_dirty - null_error_cells))
            cells = dict(error_cells=error_cells_df[[rid, "attribute"]], detect_nulls=False)
            nearest = rules is not None and rules.get("nearest") is not None
            regex = rules is not None and rules.get("regex") is not None
            if prob or nearest or regex:
                # the cost functions and the regex structures see the error cells' current values as `error_cells_df` holds them
                current = self._current_values_by_position(input_df, error_cells_df)
            if regex:
                rules = dict(rules, regex=[dict(r, current=current) for r in rules["regex"]])
            if nearest:
                rules = dict(rules, nearest=dict(rules["nearest"], current=current))
            _logger.info("[Repair Model Training Phase] Building %d models on the HBM-resident table to %s %s" % (
                len(target_columns), "compute the repair distributions of" if prob else "repair the cells in", to_list_str(target_columns)))
        if prob:
            cells.update(want_pmf=True, top_k=int(self._get_option_value(*self._opt_prob_top_k)),
                         threshold=float(self._get_option_value(*self._opt_prob_threshold)),
                         pmf_costs=lambda attr, classes, rows: self._cost_spec(plan["engine"], attr, classes, current(attr, rows),
                                                                               maximal_likelihood_repair))
        keep = bool(self._get_option_value(*self._opt_fitted_keep)) and self._fitted is None
        if self._fitted is not None:
            cells.update(fitted=self._fitted)
        elif keep:                                         # (`repair_frame` sees either keyword only when it is used)
            cells.update(keep_fit=True)
        t0 = time.perf_counter()
        # (the probability modes train on the whole table: `model.train.distinct_rows` is not wired to them)
        frame, info = repair_frame(plan["engine"], input_df, rid, targets=target_columns, base_params=plan["params"],
                                   continuous_columns=[c for c in continous_columns if c in target_columns],
                                   train_rows=self._training_row_sampler(), want_details=True,
                                   search_opts=dict(self.opts) if plan.get("search") else None, rules=rules,
                                   distinct_training_rows=None if prob else plan.get("distinct"), rebalance=plan.get("rebalance"),
                                   cells_resident=bool(self._get_option_value(*self._opt_cells_resident)), **cells)
        info["times"]["pipeline_wall"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        self._last_resident_info = info
        self._last_detection_on_device = detect
        if self._fitted is not None and error_cells_df is not None:
            # the cells of an attribute without a kept model were counted and left as they are: they are not part of the result
            error_cells_df = error_cells_df[error_cells_df["attribute"].isin(self._fitted.chain)].reset_index(drop=True)
        if keep:
            from repair.fitted import FittedRepairModels
            pieces = info.get("fit")
            self._kept_fit = FittedRepairModels.from_pieces(pieces) if pieces is not None else None
            self._kept_fit_why = info.get("fit_refusal", "")
        try:
            by_rule = [f for f in (info.get("regex_cells"), info.get("merged_cells")) if f is not None and len(f)]
            return self._resident_result(input_df, frame, pd.concat(by_rule, ignore_index=True) if by_rule else None, error_cells_df,
                                         continous_columns, compute_repair_prob,
                                         compute_repair_score, repair_data, maximal_likelihood_repair, prob)
        finally:
            info["times"]["host_shape"] = time.perf_counter() - t0

    def _resident_result(self, input_df: DataFrame, frame: DataFrame, merged: Optional[DataFrame], error_cells_df: Optional[DataFrame],
                         continous_columns: List[str], compute_repair_prob: bool, compute_repair_score: bool, repair_data: bool,
                         maximal_likelihood_repair: bool, prob: bool) -> DataFrame:
        """The result of `_run` from what `repair_frame` returned: its frame (one row per repaired cell, raw values) and the
        nearest-value merges (`merged_cells`: repaired by rule, so they leave the error cells and are appended as `_run` appends
        `repaired_by_rules_df`)."""
        rid = self._row_id
        by_rules = None
        if error_cells_df is None:
            # the cells were detected on the table: the frame holds them, with their current values
            if merged is not None and len(merged):
                by_rules = merged
            if len(frame) == 0 and by_rules is None:
                _logger.info("Any error cell not found, so the input data is already clean")
                return input_df if repair_data else pd.DataFrame({rid: pd.Series([], dtype=input_df[rid].dtype), "attribute": pd.Series([], dtype=object),
                                                                  "current_value": pd.Series([], dtype=object), "repaired": pd.Series([], dtype=object)})
            attrs, raw = frame["attribute"].to_numpy(), frame["current_value"].to_numpy(dtype=object)
            cur = np.empty(len(frame), object)
            for a in set(attrs):
                cur[attrs == a] = _sql_strs(raw[attrs == a], is_integral_column(input_df[a]))
            cand = pd.DataFrame({rid: frame[rid].to_numpy(), "attribute": attrs, "current_value": cur,
                                 "repaired": np.asarray(_strs(frame["repaired"].tolist()), object)})
            return self._repair_result(input_df, cand, by_rules, repair_data)
        if merged is not None and len(merged):
            mrep = pd.Series(merged["repaired"].to_numpy(dtype=object),
                             index=pd.MultiIndex.from_arrays([merged[rid].to_numpy(), merged["attribute"].to_numpy()]))
            mkey = pd.MultiIndex.from_arrays([error_cells_df[rid].to_numpy(), error_cells_df["attribute"].to_numpy()])
            is_merged = mkey.isin(mrep.index)
            by_rules = error_cells_df[is_merged].assign(repaired=mrep.reindex(mkey[is_merged]).to_numpy(dtype=object))
            error_cells_df = error_cells_df[~is_merged].reset_index(drop=True)
        # the frame is ordered by (column, row): back onto the order of `error_cells_df`
        at = pd.MultiIndex.from_arrays([frame[rid].to_numpy(), frame["attribute"].to_numpy()]).get_indexer(
            pd.MultiIndex.from_arrays([error_cells_df[rid].to_numpy(), error_cells_df["attribute"].to_numpy()]))
        if not prob:
            values = pd.api.extensions.take(frame["repaired"].to_numpy(dtype=object), at, allow_fill=True, fill_value=None)
            return self._repair_result(input_df, error_cells_df.assign(repaired=_strs(values)), by_rules, repair_data)
        assert (at >= 0).all()
        pmf_l = frame["pmf"].to_numpy(dtype=object)[at]
        cp = frame["current_prob"].to_numpy(np.float64)[at]
        tc = frame["top1_cost"].to_numpy(np.float64)[at]
        pval = frame["pmf_value"].to_numpy(dtype=object)[at]
        cont = set(continous_columns)
        rows = []
        for i, r in enumerate(error_cells_df.itertuples(index=False)):
            rowid, attr, cur = r[0], r[1], r[2]
            if attr in cont:
                v = pval[i]
                rows.append((rowid, attr, {"value": cur, "prob": 0.0}, [{"class": None if v is None else _to_str(v), "prob": 1.0}]))
            else:
                rows.append((rowid, attr, {"value": cur, "prob": float(cp[i])}, [{"class": _to_str(d["class"]), "prob": d["prob"]} for d in pmf_l[i]]))

        def score_df() -> DataFrame:
            # _compute_score, vectorised: log(p_top1 / max(p_cur, 1e-6)) / (1 + cost(base, top-1)), None cost = 256
            top_p = np.array([p[0]["prob"] if p else 0.0 for p in pmf_l], np.float64)
            p_cur = np.where(cp > 0.0, cp, 1e-6)
            cost = np.where(np.isnan(tc), 256.0, tc)
            with np.errstate(divide="ignore", invalid="ignore"):
                score = np.where(top_p > 0, np.log(top_p / p_cur) * (1.0 / (1.0 + cost)), -np.inf)
            return pd.DataFrame([(r[0], r[1], r[2]["value"], r[3][0]["class"] if r[3] else None, float(sc))
                                 for r, sc in zip(rows, score)], columns=[rid, "attribute", "current_value", "repaired", "score"])

        return self._probability_result(input_df, error_cells_df, pd.DataFrame(rows, columns=[rid, "attribute", "current_value", "pmf"]), score_df,
                                        compute_repair_prob, compute_repair_score, repair_data, maximal_likelihood_repair)

    # ------------------------------------------------------------------ the result of a run, resident or value-space
    def _repaired_table(self, input_df: DataFrame, error_cells_df: DataFrame, updates: DataFrame, by_rules: Optional[DataFrame] = None) -> DataFrame:
        """`repair_data`: the input with the error cells (and the cells repaired by rule) NULLed, the rule repairs applied, and
        `updates` applied to the dirty rows, which follow the clean ones."""
        rid = self._row_id
        cells = error_cells_df if by_rules is None else pd.concat([error_cells_df, by_rules], ignore_index=True)
        base = self._prepare_repair_base_cells(input_df, cells, sorted(set(cells["attribute"])))
        if by_rules is not None:
            base = self._repair_attrs(by_rules, base)
        is_dirty = base[rid].isin(set(error_cells_df[rid].tolist())).to_numpy()
        dirty = self._repair_attrs(updates[[rid, "attribute", "repaired"]], base[is_dirty].reset_index(drop=True))
        return pd.concat([base[~is_dirty], dirty], ignore_index=True)

    def _repair_result(self, input_df: DataFrame, cand: DataFrame, by_rules: Optional[DataFrame], repair_data: bool) -> DataFrame:
        """The plain result: `cand` (row_id, attribute, current_value, repaired: one row per error cell a model repaired) and the
        cells repaired by rule, as the repaired table (`repair_data`) or as the list of cells whose value changes."""
        if repair_data:
            return self._repaired_table(input_df, cand, cand, by_rules)
        keep = cand["repaired"].isna() | ~((cand["current_value"] == cand["repaired"]) | (cand["current_value"].isna() & cand["repaired"].isna()))
        cand = cand[keep.to_numpy()].reset_index(drop=True)
        return cand if by_rules is None else pd.concat([cand, by_rules], ignore_index=True)

    def _probability_result(self, input_df: DataFrame, error_cells_df: DataFrame, pmf_df: DataFrame, score_df: Any, compute_repair_prob: bool,
                            compute_repair_score: bool, repair_data: bool, maximal_likelihood_repair: bool) -> DataFrame:
        """The probability modes' outputs from the candidate distributions `pmf_df` (`_compute_repair_pmf`'s frame): the pmf itself, its
        top-1 (`compute_repair_prob`), or -- maximal likelihood -- the scores (`score_df()`: how they are computed is the caller's),
        the `repair_delta` best of them, or those applied to the data."""
        rid = self._row_id
        if not maximal_likelihood_repair:
            pmf_df = pmf_df.assign(current_value=[c["value"] for c in pmf_df["current_value"]])
            if compute_repair_prob:
                return pd.DataFrame({rid: pmf_df[rid], "attribute": pmf_df["attribute"], "current_value": pmf_df["current_value"],
                                     "repaired": [p[0]["class"] if p else None for p in pmf_df["pmf"]],
                                     "prob": [p[0]["prob"] if p else None for p in pmf_df["pmf"]]})
            return pmf_df
        scores = score_df()
        if compute_repair_score:
            return scores
        top = self._maximal_likelihood_repair(scores, error_cells_df)
        return self._repaired_table(input_df, error_cells_df, top) if repair_data else top

    # ------------------------------------------------------------------ pipeline
    def _resident_attempt(self, what: str, plan: Dict[str, Any], *args: Any) -> Optional[DataFrame]:
        """`_resident_run`, or None (with `what` and the reason in the log) when the run turns out not to qualify."""
        from repair.pipeline import NotResidentEligible
        try:
            return self._resident_run(plan, *args)
        except NotResidentEligible as e:
            # only known once the table is built and the error cells are NULLed, e.g.: a target left with a single class / no value (the
            # reference's PoorModel short-cut, model.py:1008-1017), or NULL target cells in dirty rows that are not error cells under
            # repair_data.  (Unseen categories of a dirty row need no fallback: the table marks categorical columns, so a model treats
            # a category its training rows do not show as missing, like the reference's per-model encoders.)
            self._last_resident_info = None
            self._last_detection_on_device = False
            _logger.info("%s not taken: %s" % (what, e))
            return None

    def _fitted_plan(self) -> Dict[str, Any]:
        """The plan of a run that applies a kept fit: the checks that do not depend on the table (ValueError with the reason), the engine,
        and the one info line about the settings such a run does not read."""
        from repair import dist
        fitted = self._fitted
        if self.repair_by_rules:
            raise ValueError("Cannot apply fitted models with `setRepairByRules(True)`: a rule is a map of the fitted table, not a kept model")
        if dist.world()[1] > 1:
            raise ValueError("Cannot apply fitted models in a job on %d ranks" % dist.world()[1])
        if self.targets and set(self.targets) != set(fitted.chain):
            raise ValueError("Cannot apply fitted models: the targets of the run are the fitted targets %s, but `setTargets` gave %s"
                             % (to_list_str(fitted.chain), to_list_str(self.targets)))
        engine = self._resident_engine()
        if engine is None:
            raise ValueError("Cannot apply fitted models: no engine for the HBM-resident table (no HIP device, or REPAIR_RESIDENT=0)")
        ignored = sorted(k for k in self.opts if k.startswith(("model.lgb.", "model.hp.", "model.cv.")) or k in (
            self._opt_max_training_row_num.key, self._opt_train_distinct_rows.key, self._opt_train_distinct_rows_max_ratio.key))
        if self.training_data_rebalancing_enabled:
            ignored.append("setTrainingDataRebalancingEnabled")
        if ignored:
            _logger.info("[Repairing Phase] fitted models are applied, nothing is trained: %s not read" % to_list_str(ignored))
        return dict(engine=engine, params={}, search=False, rules=None, distinct=None, rebalance=None)

    def _run_fitted(self, input_df: DataFrame, continous_columns: List[str], flags: Any) -> DataFrame:
        """`_run` with `setFittedModels`: detection on whichever route the detectors take today -- the device detection plan, or the pandas
        detectors followed by given cells -- then ONE resident attempt that applies the fit (`pipeline.repair_frame(fitted=..)`); there is
        no value-space continuation: what would send a training run there is a ValueError here."""
        from repair.pipeline import NotResidentEligible
        fitted, repair_data = self._fitted, flags[3]
        plan = self._fitted_plan()
        missing = [c for c in fitted.columns if c not in input_df.columns]
        if missing:
            raise ValueError("Cannot apply fitted models: the fitted column `%s` is not in the input" % missing[0])
        try:
            dplan = self._device_detection_plan(input_df, continous_columns, False, False) if self.error_detectors else None
            if dplan is not None:
                dplan = dict(dplan, engine=plan["engine"], params={}, search=False, rules=None, distinct=None, rebalance=None)
                return self._resident_run(dplan, input_df, dplan["candidates"], continous_columns, None, *flags)
            _logger.info("[Error Detection Phase] Detecting errors in a table... ")
            error_cells_df, target_columns, _, _ = self._detect_errors(input_df, continous_columns)
            if len(error_cells_df) == 0:
                _logger.info("Any error cell not found, so the input data is already clean")
                return input_df if repair_data else error_cells_df.assign(repaired=pd.Series([], dtype=object))
            error_cells_df = error_cells_df[error_cells_df["attribute"].isin(target_columns)].reset_index(drop=True)
            return self._resident_run(plan, input_df, target_columns, continous_columns, error_cells_df, *flags)
        except NotResidentEligible as e:
            raise ValueError("Cannot apply fitted models: %s" % e)

    @elapsed_time  # type: ignore
    def _run(self, input_df: DataFrame, continous_columns: List[str], detect_errors_only: bool,
             compute_repair_candidate_prob: bool, compute_repair_prob: bool, compute_repair_score: bool,
             repair_data: bool, maximal_likelihood_repair: bool) -> DataFrame:
        rid = self._row_id
        flags = (compute_repair_candidate_prob, compute_repair_prob, compute_repair_score, repair_data, maximal_likelihood_repair)
        self._last_detection_on_device = False
        if self._fitted is not None and not detect_errors_only:
            return self._run_fitted(input_df, continous_columns, flags)
        if bool(self._get_option_value(*self._opt_fitted_keep)):
            self._kept_fit = None
            self._kept_fit_why = "the run took the value-space path: only a run on the HBM-resident table keeps its fit"
        # 0. Everything on the HBM-resident table, detection included, when the detectors and the run allow it
        dplan = None if detect_errors_only else self._device_detection_plan(input_df, continous_columns, compute_repair_candidate_prob,
                                                                            maximal_likelihood_repair)
        if detect_errors_only and bool(self._get_option_value(*self._opt_detect_only_resident)):
            oplan = self._device_detect_only_plan(input_df, continous_columns)
            if oplan is not None:
                out = self._detect_only_attempt(oplan, input_df, continous_columns)
                if out is not None:
                    return out
        if dplan is not None:
            out = self._resident_attempt("device-side detection", dplan, input_df, dplan["candidates"], continous_columns, None, *flags)
            if out is not None:
                return out
        # 1. Error Detection Phase
        _logger.info("[Error Detection Phase] Detecting errors in a table... ")
        error_cells_df, target_columns, pairwise_attr_stats, domain_stats = self._detect_errors(input_df, continous_columns)
        if detect_errors_only:
            return error_cells_df
        if len(error_cells_df) == 0:
            _logger.info("Any error cell not found, so the input data is already clean")
            return input_df if repair_data else error_cells_df.assign(repaired=pd.Series([], dtype=object))
        if len(target_columns) == 0:
            raise ValueError("At least one valid discretizable feature is needed to repair error cells, but no such feature found")
        error_cells_df = error_cells_df[error_cells_df["attribute"].isin(target_columns)].reset_index(drop=True)

        # 2. + 3. on the HBM-resident table when the run is the plain per-attribute model loop (the hot path of this engine), or one of
        # the probability modes with `repair.pmf.resident` set
        prob_modes = (compute_repair_candidate_prob or maximal_likelihood_repair) and bool(self._get_option_value(*self._opt_pmf_resident))
        plan = self._resident_plan(input_df, target_columns, continous_columns, domain_stats, compute_repair_candidate_prob,
                                   maximal_likelihood_repair, prob_modes=prob_modes)
        if plan is not None:
            out = self._resident_attempt("resident path", plan, input_df, target_columns, continous_columns, error_cells_df, *flags)
            if out is not None:
                return out

        # 2. Repair Model Training Phase
        repair_base_df = self._prepare_repair_base_cells(input_df, error_cells_df, target_columns)
        repaired_by_rules_df = None
        if self.repair_by_rules:
            repaired_by_rules_df = error_cells_df.iloc[0:0].assign(repaired=pd.Series([], dtype=object))
            if self._repair_by_regex_enabled:
                error_cells_df, by_regex = self._repair_by_regexs(input_df, error_cells_df)
                repaired_by_rules_df = pd.concat([repaired_by_rules_df, by_regex], ignore_index=True)
            if self._repair_by_nearest_values_enabled:
                error_cells_df, by_nv = self._repair_by_nearest_values(repair_base_df, error_cells_df, target_columns)
                repaired_by_rules_df = pd.concat([repaired_by_rules_df, by_nv], ignore_index=True)
            repair_base_df = self._repair_attrs(repaired_by_rules_df, repair_base_df)
        dirty_ids = set(error_cells_df[rid].tolist())
        is_dirty = repair_base_df[rid].isin(dirty_ids).to_numpy()
        clean_rows_df, dirty_rows_df = repair_base_df[~is_dirty], repair_base_df[is_dirty].reset_index(drop=True)
        models = self._build_repair_models(repair_base_df, target_columns, continous_columns, domain_stats, pairwise_attr_stats)

        # 3. Repair Phase
        repaired_rows_df, pmfs = self._repair(models, continous_columns, dirty_rows_df, error_cells_df,
                                              compute_repair_candidate_prob, maximal_likelihood_repair)
        if compute_repair_candidate_prob or maximal_likelihood_repair:
            if maximal_likelihood_repair:
                assert len(continous_columns) == 0
            else:
                assert not self._repair_by_nearest_values_enabled, "repairing data by nearest values not supported in this path"
            pmf_df = self._compute_repair_pmf(pmfs, repaired_rows_df, dirty_rows_df, error_cells_df, continous_columns)
            return self._probability_result(input_df, error_cells_df, pmf_df, lambda: self._compute_score(pmf_df), compute_repair_prob,
                                            compute_repair_score, repair_data, maximal_likelihood_repair)
        if repair_data:
            # every NULL target cell of a dirty row is filled (`_repair`), not the error cells alone: the rows are taken as they are
            clean_df = pd.concat([clean_rows_df, repaired_rows_df], ignore_index=True)
            assert len(clean_df) == len(input_df)
            return clean_df
        return self._repair_result(input_df, self._flatten_join(repaired_rows_df, error_cells_df), repaired_by_rules_df, False)

    def run(self, detect_errors_only: bool = False, compute_repair_candidate_prob: bool = False,
            compute_repair_prob: bool = False, compute_repair_score: bool = False, repair_data: bool = False,
            maximal_likelihood_repair: bool = False) -> DataFrame:
        """Starts processing to detect error cells in given input data and build a statistical model to
        repair them (reference model.py:1421-1537: same flags, same exclusivity rules, same messages)."""
        if self.input is None or self.row_id is None:
            raise ValueError("`setInput` and `setRowId` should be called before repairing")
        if maximal_likelihood_repair and self.repair_delta is None:
            raise ValueError("`setRepairDelta` should be called when enabling maximal likelihood repairing")
        if maximal_likelihood_repair and self.cf is None:
            raise ValueError("`setUpdateCostFunction` should be called when enabling maximal likelihood repairing")
        if maximal_likelihood_repair and len(self.cf.targets) > 0:  # type: ignore
            raise ValueError("`UpdateCostFunction.targets` cannot be used when enabling maximal likelihood repairing")
        flags = [("detect_errors_only", detect_errors_only), ("compute_repair_candidate_prob", compute_repair_candidate_prob),
                 ("compute_repair_prob", compute_repair_prob), ("compute_repair_score", compute_repair_score), ("repair_data", repair_data)]
        selected = [n for n, v in flags if v]
        if len(selected) > 1:
            raise ValueError("%s cannot be set to true simultaneously" % to_list_str(selected, sep="/", quote=True))
        if self._repair_by_nearest_values_enabled and (maximal_likelihood_repair or compute_repair_candidate_prob or compute_repair_prob or compute_repair_score):
            raise ValueError("Cannot repair data by nearest values when enabling `maximal_likelihood_repair`, "
                             "`compute_repair_candidate_prob`, `compute_repair_prob`, or `compute_repair_score`")
        if self._fitted is not None and (compute_repair_candidate_prob or compute_repair_prob or compute_repair_score or maximal_likelihood_repair):
            raise ValueError("Cannot apply fitted models in the probability modes (`compute_repair_candidate_prob`, `compute_repair_prob`, "
                             "`compute_repair_score`, `maximal_likelihood_repair`): they are answered by a run that trains")
        if compute_repair_prob or compute_repair_score:
            compute_repair_candidate_prob = True
        if compute_repair_score:
            maximal_likelihood_repair = True
        input_df, continous_columns = self._check_input_table()
        if maximal_likelihood_repair and len(continous_columns) != 0:
            raise ValueError("Cannot enable the maximal likelihood repair mode when continous attributes found")
        if self.targets and len(set(self.targets) & set(input_df.columns)) == 0:
            # the reference names the (qualified) input table here (model.py:1525-1526); a DataFrame input has no name
            raise ValueError("Target attributes not found in %s: %s" % (self._qualified_input_name(), to_list_str(self.targets)))
        self.opts.setdefault("model.gpu.device_id", self.opts.get("model.gpu.device_id", "0"))
        from repair.utils import column_code_cache
        with column_code_cache(input_df):     # NULL detection, domain statistics and the resident encoding share one hash pass per column
            df, elapsed = self._run(input_df, continous_columns, detect_errors_only, compute_repair_candidate_prob,
                                    compute_repair_prob, compute_repair_score, repair_data, maximal_likelihood_repair)
        _logger.info("!!!Total Processing time is %s(s)!!!" % elapsed)
        return df


# RepairBase.scala:41-47: the column types the reference accepts, in the order its message prints them
_SUPPORTED_TYPES = ["tinyint", "float", "smallint", "string", "double", "int", "bigint"]


def _sql_type_name(s: Any) -> str:
    """Spark SQL name of a pandas column's type (only what `checkInputTable` needs to tell apart)."""
    import datetime
    k = s.dtype.kind
    if k == "M":
        return "timestamp"
    if k == "m":
        return "interval"
    if k == "b" or str(s.dtype) == "boolean":
        return "boolean"
    if k in "iu" or str(s.dtype).startswith(("Int", "UInt")):
        bits = "".join(ch for ch in str(s.dtype) if ch.isdigit())
        return {"8": "tinyint", "16": "smallint", "32": "int"}.get(bits, "bigint")
    if k == "f" or str(s.dtype).startswith("Float"):
        return "float" if "32" in str(s.dtype) else "double"
    if isinstance(s.dtype, pd.CategoricalDtype):         # a dictionary-encoded column has the type of its dictionary
        return _sql_type_name(s.cat.categories.to_series())
    kind = pd.api.types.infer_dtype(s, skipna=True)      # one C pass; only the unusual answers need the element-wise look below
    if kind in ("string", "empty"):
        return "string"
    vals = s.dropna()
    if len(vals) and all(isinstance(v, datetime.datetime) for v in vals):
        return "timestamp"
    if len(vals) and all(isinstance(v, datetime.date) for v in vals):
        return "date"
    if len(vals) and all(isinstance(v, (bool, np.bool_)) for v in vals):
        return "boolean"
    return "string"


def _to_double(v: Any) -> float:
    """Spark's CAST(string AS DOUBLE): Java `Double.parseDouble` after trimming, which also takes a d/D/f/F suffix; anything
    else is NULL."""
    if v is None or (isinstance(v, float) and np.isnan(v)):
        return float("nan")
    if isinstance(v, (int, float, np.integer, np.floating)):
        return float(v)
    t = str(v).strip()
    if t[-1:] in "dDfF" and len(t) > 1:
        t = t[:-1]
    try:
        return float(t)
    except ValueError:
        return float("nan")


def _to_str(v: Any) -> str:
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    if isinstance(v, (np.integer,)):
        return str(int(v))
    return str(v)


def _is_null(v: Any) -> bool:
    return v is None or (isinstance(v, float) and np.isnan(v))


def _strs(values: Any) -> List[Optional[str]]:
    """`_to_str` of repaired values as the resident pipeline decodes them; None / NaN stays None."""
    return [None if _is_null(v) else _to_str(v) for v in values]


def _sql_strs(values: Any, integral: bool) -> List[Optional[str]]:
    """CAST(value AS STRING) of the error cells' current values (ErrorModel.detect); None / NaN stays None.  The resident pipeline
    decodes numeric dictionaries as float64, so the values of an integral attribute print as '2', never '2.0' (ErrorModel.detect
    keeps nullable ints integral)."""
    out = [None if _is_null(v) else _to_sql_string(v) for v in values]
    return [v if v is None else str(int(float(v))) for v in out] if integral else out
