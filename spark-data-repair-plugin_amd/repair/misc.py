"""`RepairMisc` (reference python/repair/misc.py:27-131,159-260): the helper API around the repair path, on pandas frames.

`repair` (apply predicted updates, RepairMiscApi.repairAttrsFrom), `flatten` (RepairMiscApi.flattenTable), `injectNull`
(RepairMiscApi.injectNullAt, the error injector the synthetic benchmark tables use), `splitInputTable` (k-means over q-gram
features, on the resident code table when a device is present: repair/qgram_kmeans.py), `toHistogram`,
`toErrorMap`, `describe` (the column statistics of Spark's ANALYZE, from per-code row counts: repair/table_stats.py) and
`generateDepGraph` (the Graphviz text of DepGraph.computeDepGraph from dense pair counts: repair/depgraph.py); the last two run on the
resident code table when a device is present and on their numpy statements otherwise, with the same result.
`discoverFunctionalDeps` has no counterpart in the reference: it finds the minimal (approximate) functional dependencies of a table and
returns them as constraint text for `ConstraintErrorDetector`, on the same two paths (repair/fd_discovery.py).
"""
import logging
from typing import Any, Dict, List

import numpy as np
import pandas as pd

from repair import session
from repair.utils import argtype_check

DataFrame = pd.DataFrame
_logger = logging.getLogger(__name__)


class RepairMisc():
    """Interface to provide helper functionalities."""

    def __init__(self) -> None:
        self.opts: Dict[str, str] = {}

    @argtype_check  # type: ignore
    def option(self, key: str, value: str) -> "RepairMisc":
        self.opts[str(key)] = str(value)
        return self

    @argtype_check  # type: ignore
    def options(self, options: Dict[str, str]) -> "RepairMisc":
        self.opts.update(options)
        return self

    @property
    def _db_name(self) -> str:
        return self.opts.get("db_name", "")

    @property
    def _target_attr_list(self) -> str:
        return self.opts.get("target_attr_list", "")

    def _check_required_options(self, required: List[str]) -> None:
        if not all(opt in self.opts.keys() for opt in required):
            raise ValueError("Required options not found: {}".format(", ".join(required)))

    def _qualified(self, name: str) -> str:
        return "%s.%s" % (self._db_name, name) if self._db_name else name

    def _input(self) -> DataFrame:
        return session.resolve(self.opts["table_name"])

    def _check_attrs(self, df: DataFrame, attrs: List[str]) -> None:
        missing = [a for a in attrs if a not in df.columns]
        if missing:
            raise ValueError("Columns '%s' do not exist in '%s'" % (", ".join(missing), self._qualified(self.opts["table_name"])))

    def repair(self) -> DataFrame:
        """Applies predicted repair updates into an input table (RepairMiscApi.scala:184-247)."""
        self._check_required_options(["repair_updates", "table_name", "row_id"])
        from repair.model import RepairModel
        updates = session.resolve(self.opts["repair_updates"])
        rid = self.opts["row_id"]
        if not {rid, "attribute", "repaired"} <= set(updates.columns):
            raise ValueError("Table '%s' must have '%s', 'attribute', and 'repaired' columns" % (self.opts["repair_updates"], rid))
        return RepairModel().setRowId(rid)._repair_attrs(updates[[rid, "attribute", "repaired"]], self._input())

    def flatten(self) -> DataFrame:
        """<row_id, attribute, value> with `CAST(value AS STRING)` (RepairMiscApi.scala:41-49); attribute-major like the
        reference's `INLINE(ARRAY(STRUCT..))` is row-major -- callers sort, so is the order here (row, then column)."""
        self._check_required_options(["table_name", "row_id"])
        from repair.errors import _to_sql_string
        df, rid = self._input(), self.opts["row_id"]
        cols = [c for c in df.columns if c != rid]
        ids = np.repeat(df[rid].to_numpy(), len(cols))
        attrs = np.tile(np.asarray(cols, object), len(df))
        vals = np.empty(len(df) * len(cols), object)
        for j, c in enumerate(cols):
            vals[j::len(cols)] = [None if pd.isna(v) else _to_sql_string(v) for v in df[c].to_numpy(dtype=object)]
        return pd.DataFrame({rid: ids, "attribute": attrs, "value": vals})

    def _resident_engine(self) -> Any:
        """A HIP engine when a device is present and REPAIR_RESIDENT is not 0, else None (as `RepairModel._resident_engine`); tests
        inject one through `_engine_override`."""
        hook = getattr(self, "_engine_override", None)
        if hook is not None:
            return hook
        from repair.engine import resident_engine
        return resident_engine(self.opts.get("gpu_device_id", "0"))

    def splitInputTable(self) -> DataFrame:
        """Splits an input table into `k` groups of similar rows: k-means over the bag-of-q-gram features of the target attributes
        (RepairMiscApi.scala:74-153) -> [row_id, "k"] in frame order.  Options: `target_attr_list` (default: every column but the row
        id), `q` (2), `clustering_alg` ("bisect-kmeans", "kmeans++" or "bisecting"), `seed` (0), `max_iter` (20), `tol` (1e-4).  The
        reference's two algorithm names run the ONE Lloyd loop of repair.qgram_kmeans (k-means++ seeding, iterations in code space), as
        before.  "bisecting" is the bisecting k-means of repair.qgram_bisect, modelled on MLlib's BisectingKMeans.run: a tree grown level by
        level, the largest divisible leaves split first, every row scored against the two children of its own node only, so `k` may be
        2 .. 1024 with it; it may return fewer than `k` groups (ids 0 .. k'-1) and does not read `tol`.  The seeding is not Spark's
        (`k-means||` is not restated), so the labels are not Spark's -- the reference's own test pins only the set of ids."""
        self._check_required_options(["table_name", "row_id", "k"])
        if not self.opts["k"].isdigit():
            raise ValueError("Option 'k' must be an integer, but '%s' found" % self.opts["k"])
        k = int(self.opts["k"])
        if k < 2:
            raise ValueError("Option 'k' must be 2 or more, but '%s' found" % self.opts["k"])
        alg = self.opts.get("clustering_alg", "bisect-kmeans")
        if alg not in ("bisect-kmeans", "kmeans++", "bisecting"):
            raise ValueError("Unknown clustering algorithm found: %s" % alg)
        if alg == "bisecting" and k > 1024:
            raise ValueError("Option 'k' must be 1024 or less with clustering_alg 'bisecting', but '%s' found" % self.opts["k"])
        try:
            q = int(self.opts.get("q", "2"))          # (the reference: `Try(optionMap("q").toInt).getOrElse(2)`)
        except ValueError:
            q = 2
        df, rid = self._input(), self.opts["row_id"]
        self._check_attrs(df, [rid])
        attrs = [a.strip() for a in self._target_attr_list.split(",") if a.strip()]
        if attrs:
            self._check_attrs(df, attrs)
        else:
            attrs = [c for c in df.columns if c != rid]
        from repair import qgram_kmeans
        return qgram_kmeans.split_rows(df, rid, attrs, k, q=q, seed=int(self.opts.get("seed", "0")), max_iter=int(self.opts.get("max_iter", "20")),
                                       tol=float(self.opts.get("tol", "1e-4")), engine=self._resident_engine(),
                                       alg="bisecting" if alg == "bisecting" else "kmeans")

    def injectNull(self) -> DataFrame:
        """Randomly injects NULL into the given attributes: `IF(rand() > ratio, col, NULL)` per cell
        (RepairMiscApi.scala:155-182).  The reference's `rand()` is unseeded; option `seed` (default 0) fixes it here."""
        self._check_required_options(["table_name", "target_attr_list"])
        if "null_ratio" in self.opts.keys():
            try:
                ratio = float(self.opts["null_ratio"])
                ok = True
            except ValueError:
                ok = False
            if not (ok and 0.0 < ratio <= 1.0):
                raise ValueError("Option 'null_ratio' must be a float in (0.0, 1.0], but '%s' found" % self.opts["null_ratio"])
        else:
            ratio = 0.01
        df = self._input().copy()
        attrs = [a.strip() for a in self._target_attr_list.split(",") if a.strip()]
        self._check_attrs(df, attrs)
        rng = np.random.Generator(np.random.PCG64(int(self.opts.get("seed", "0"))))
        for a in attrs:
            keep = rng.random(len(df)) > ratio
            col = df[a]
            if pd.api.types.is_integer_dtype(col) and not str(col.dtype).startswith(("Int", "UInt")):
                col = col.astype("Int64")
            df[a] = col.where(keep, other=pd.NA if str(col.dtype).startswith(("Int", "UInt")) else None)
        return df

    def describe(self) -> DataFrame:
        """Column statistics of an input table (RepairMiscApi.computeAndGetStats): [attrName, distinctCnt, min, max, nullCnt, avgLen,
        maxLen, hist], one row per column in frame order (the reference's order is a hash map's; callers sort).  Option `num_bins`
        (default 8, at most 254): the bins of the equi-height histogram of a numeric column.  The counts are exact where Spark's
        are HyperLogLog++ sketches, and the histogram edges are the exact ranks ceil(i * m / num_bins) where Spark's are approximate
        percentiles."""
        self._check_required_options(["table_name"])
        try:
            n_bins = int(self.opts.get("num_bins", "8"))
        except ValueError:
            raise ValueError("Option 'num_bins' must be an integer, but '%s' found" % self.opts["num_bins"]) from None
        from repair import table_stats
        return table_stats.describe_frame(self._input(), n_bins=n_bins, engine=self._resident_engine())

    def discoverFunctionalDeps(self) -> DataFrame:
        """The minimal (approximate) functional dependencies X -> Y of an input table, found level by level from integer measures of the
        code table (repair/fd_discovery.py; on the resident table when a device is present, on the numpy statement repair/fd_codes.py
        otherwise, with the same result: DESIGN.md 5o) -> [lhs, rhs, groups, removed_rows, violating_rows, error, constraint], ordered
        by the size of X, the columns' positions, then Y.  `constraint` is text that `ConstraintErrorDetector` takes unchanged, and
        `violating_rows` the rows it then flags.  Options: `row_id` (that column takes no part), `targets` (a comma list: the right-hand
        sides only), `max_lhs_size` ("2", 1 .. 4), `max_error` ("0.0": the share of the rows that may be removed for a dependency to hold,
        read exactly from its decimal text), `max_lhs_group_ratio` ("1.0": supersets of a left-hand side with more groups than this share
        of the rows are not looked at).  The reference cites constraint discovery and has no counterpart."""
        self._check_required_options(["table_name"])
        from fractions import Fraction
        from repair import fd_codes, fd_discovery
        from repair.errors import parse_constraint
        from repair.frame_encoding import FrameEncoding
        if not self.opts.get("max_lhs_size", "2").isdigit() or not 1 <= int(self.opts.get("max_lhs_size", "2")) <= fd_discovery.MAX_LHS_SIZE:
            raise ValueError("Option 'max_lhs_size' must be an integer in [1, %d], but '%s' found"
                             % (fd_discovery.MAX_LHS_SIZE, self.opts["max_lhs_size"]))
        for opt, default, hi in (("max_error", "0.0", 1), ("max_lhs_group_ratio", "1.0", None)):
            try:
                v = Fraction(self.opts.get(opt, default).strip())
                ok = v >= 0 and (hi is None or v < hi)
            except (ValueError, ZeroDivisionError):
                ok = False
            if not ok:
                raise ValueError("Option '%s' must be a decimal in [0.0, %s, but '%s' found" % (opt, "1.0)" if hi else "inf)", self.opts[opt]))
        df = self._input()
        rid = self.opts.get("row_id", "")
        if rid:
            self._check_attrs(df, [rid])
        cols = [c for c in df.columns if c != rid]
        targets = [a.strip() for a in self.opts.get("targets", "").split(",") if a.strip()]
        self._check_attrs(df, targets)
        if rid and rid in targets:
            raise ValueError("Option 'targets' must not hold the row id '%s'" % rid)
        names = ["lhs", "rhs", "groups", "removed_rows", "violating_rows", "error", "constraint"]
        n = len(df)
        records: List[Dict[str, Any]] = []
        if n > 0 and cols:
            enc = FrameEncoding.of_frame(df, cols)
            engine = self._resident_engine()
            if engine is not None:
                table = engine.upload_dictionaries(enc.indices, enc.remaps)
                measure = lambda lhs, rhs: engine.fd_measures(table, lhs, rhs)  # noqa: E731
            else:
                codes = np.stack([np.where(i >= 0, r[np.maximum(i, 0)] if len(r) else -1, -1).astype(np.int32)
                                  for i, r in zip(enc.indices, enc.remaps)])
                n_codes = [max(len(d), 1) for d in enc.dicts]
                measure = lambda lhs, rhs: fd_codes.fd_measures(codes, n_codes, lhs, rhs)  # noqa: E731
            log: List[str] = []
            records = fd_discovery.discover(measure, n, cols, targets or cols, max_lhs_size=int(self.opts.get("max_lhs_size", "2")),
                                            max_error=self.opts.get("max_error", "0.0"),
                                            max_lhs_group_ratio=self.opts.get("max_lhs_group_ratio", "1.0"), log=log)
            for line in log:
                _logger.info("discoverFunctionalDeps: %s" % line)
        rows = []
        for r in records:
            text = "t1&t2&%s&IQ(t1.%s,t2.%s)" % ("&".join("EQ(t1.%s,t2.%s)" % (a, a) for a in r["lhs"]), r["rhs"], r["rhs"])
            want = [("EQ", a, a, None) for a in r["lhs"]] + [("IQ", r["rhs"], r["rhs"], None)]
            try:
                got = [(p.op, p.left, p.right, p.constant) for p in parse_constraint(text)]
            except ValueError:
                got = []
            if got != want:
                _logger.warning("discoverFunctionalDeps: %s -> %s is left out, its constraint text does not parse back: %s"
                                % (",".join(r["lhs"]), r["rhs"], text))
                continue
            rows.append((",".join(r["lhs"]), r["rhs"], r["groups"], r["removed_rows"], r["violating_rows"], r["removed_rows"] / n, text))
        out = pd.DataFrame(rows, columns=names)
        for c in ("groups", "removed_rows", "violating_rows"):
            out[c] = out[c].astype(np.int64)
        out["error"] = out["error"].astype(np.float64)
        for c in ("lhs", "rhs", "constraint"):
            out[c] = out[c].astype(object)
        return out

    def toHistogram(self) -> DataFrame:
        """The value counts of the listed attributes (RepairMiscApi.convertToHistogram, :276-301): one row [attribute, histogram] per
        attribute of `targets` that exists and is not continuous (numeric), histogram = [{"value", "cnt"}] over its non-NULL values."""
        self._check_required_options(["table_name", "targets"])
        from repair.encode import is_numeric_column
        df = self._input()
        targets = {a.strip() for a in self.opts["targets"].split(",") if a.strip()}
        rows = []
        for c in df.columns:
            if c not in targets or is_numeric_column(df[c]):
                continue
            cnt = df[c].dropna().value_counts(sort=False)
            rows.append((c, [{"value": v, "cnt": int(n)} for v, n in cnt.items()]))
        return pd.DataFrame(rows, columns=["attribute", "histogram"])

    def toErrorMap(self) -> DataFrame:
        """[row_id, error_map]: one character per non-row-id column in frame order, `*` for a cell the error-cell table lists, `-`
        otherwise (RepairMiscApi.toErrorMap, :303-345)."""
        self._check_required_options(["table_name", "row_id", "error_cells"])
        rid = self.opts["row_id"]
        cells = session.resolve(self.opts["error_cells"])
        if not {rid, "attribute"} <= set(cells.columns):
            raise ValueError("Table '%s' must have '%s' and 'attribute' columns" % (self.opts["error_cells"], rid))
        df = self._input()
        self._check_attrs(df, [rid])
        cols = [c for c in df.columns if c != rid]
        marks = np.full((len(df), len(cols)), "-", dtype="<U1")
        row_of = pd.Series(np.arange(len(df)), index=pd.Index(df[rid].to_numpy()))
        row_of = row_of[~row_of.index.duplicated()]
        col_of = {c: j for j, c in enumerate(cols)}
        r = row_of.reindex(cells[rid].to_numpy()).to_numpy()
        c = cells["attribute"].map(col_of).to_numpy(dtype=np.float64, na_value=np.nan)
        ok = ~(np.isnan(r.astype(np.float64)) | np.isnan(c))
        marks[r[ok].astype(np.int64), c[ok].astype(np.int64)] = "*"
        return pd.DataFrame({rid: df[rid].to_numpy(), "error_map": ["".join(m) for m in marks]})

    def generateDepGraph(self) -> None:
        """Writes the dependency graph of an input table as `<path>/<filename_prefix>.dot` (DepGraph.generateDepGraph) and, when Graphviz's
        `dot` is installed, its SVG rendering next to it.  Options: `target_attr_list` (default: every column), `max_domain_size`
        (100), `max_attr_value_num` (30), `max_attr_value_length` (70), `pairwise_attr_stat_threshold` (1.0), `edge_label` and
        `overwrite` (non-empty = on), `filename_prefix` ("depgraph")."""
        self._check_required_options(["path", "table_name"])
        from repair import depgraph
        df = self._input()
        attrs = [a.strip() for a in self._target_attr_list.split(",") if a.strip()]
        self._check_attrs(df, attrs)
        text = depgraph.compute_dep_graph(
            df, attrs, max_domain_size=int(self.opts.get("max_domain_size", "100")), max_attr_value_num=int(self.opts.get("max_attr_value_num", "30")),
            max_attr_value_length=int(self.opts.get("max_attr_value_length", "70")),
            pairwise_attr_stat_threshold=float(self.opts.get("pairwise_attr_stat_threshold", "1.0")),
            edge_label=len(self.opts.get("edge_label", "")) > 0, engine=self._resident_engine())
        depgraph.write_dep_graph(text, self.opts["path"], "svg", self.opts.get("filename_prefix", "depgraph"), len(self.opts.get("overwrite", "")) > 0)
