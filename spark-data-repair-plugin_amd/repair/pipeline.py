"""`RepairModel.run()` on a label-encoded table that stays resident in HBM from detection to the repaired cells.

The reference walks  detect errors -> convertErrorCellsToNull -> clean/dirty split -> per-attribute models ->
chained repair -> flatten + join with the error cells  through Spark SQL and pandas (python/repair/model.py:1293-1419).
Here every step is a call on the engine's table object (csrc/rgbm_prep.hip and the rgbm_<step>.hip sources beside it for the relational steps,
csrc/rgbm.hip for the models); the host only merges the (small) cell lists.  The engine is an argument so the same
job logic runs on the CPU oracle engine in the tests.

Cells are (row position, column index); values are codes (-1 = NULL).  `repair.encode` / `Table.from_dictionaries`
map between values and codes.
"""
import os
import time

import numpy as np

from repair.engine import run_job
from repair.frame_encoding import FrameEncoding
from repair.utils import setup_logger

_logger = setup_logger()


def _merge_cells(n, parts):
    """Union of cell lists, ordered by (column, row), duplicates removed (detectors overlap: model.py `_detect_errors`
    + ErrorModel concatenates the detectors' frames and drops duplicates)."""
    if not parts:
        return np.zeros(0, np.int64), np.zeros(0, np.int32)
    key = np.concatenate([c.astype(np.int64) * n + r for r, c in parts])
    key = np.unique(key)
    return key % n, (key // n).astype(np.int32)


def detect_error_cells(table, targets, constraints=(), detect_nulls=True, error_cells=None, value_detectors=None, on_device=False,
                       keep_open=False):
    """Error cells of the target attributes: (rows, cols), ordered by (column, row), every cell once.

    on_device   : returns (rows, cols, codes), `codes` being what the cells hold now.  On a table with `cellset_open` the detectors'
                  results never leave the device one by one: a cell set over the targets is opened, every part below is detected with
                  ``fetch=False`` and followed by `Table.cellset_add`, and ONE `Table.cellset_emit` brings the union and its codes to the host
                  (csrc/rgbm_cellset.hip).  Given `error_cells` are host arrays: they join last, by the host merge, and the codes
                  are then read with `Table.read_cells`.  A table without the methods detects as with on_device=False and reads the codes.
    keep_open   : (with on_device, on a table that has `cellset_add_cells`, for at least one target) nothing is emitted: the given
                  `error_cells` join the set through `Table.cellset_add_cells`, the set STAYS OPEN for the caller -- who emits, prunes,
                  NULLs and closes it (`_cells_on_set`) -- and None is returned.  The set is closed here only when a detector raises.

    constraints : [(eq_cols, iq_col)] -- denial constraints  EQ(X1)..EQ(Xm) & IQ(Y)  (ErrorDetectorApi.scala:189-244); a
                  violating row contributes the constraint's attributes that are targets (`attrs`, line 211).  Next to them the
                  programs of `repair.dc_codes.lower_constraint`: dict(kind="dc", preds, refs[, max_pairs]) -> `Table.detect_dc`,
                  dict(kind="row_bits", cols, bits, refs) -> `Table.detect_row_bits`; a `max_pairs` refusal of the device
                  (RGBM_ERR_PARAM) raises NotResidentEligible.  dict(kind="dc_scan", preds, refs): a `dc` program that
                  `route_order_constraints` sent to `Table.detect_dc_scan`; its refusals (RGBM_ERR_PARAM) raise the same
    error_cells : (rows, cols) given by the caller (RepairModel.setErrorCells); non-target attributes are dropped
    value_detectors : per-column descriptors of the regex / value-domain / outlier detectors as code predicates
                  (`repair.detect_codes.build_descriptors`); one `Table.detect_cells` call answers them, and the NULL detector
                  rides in the same read of each column instead of `detect_nulls`.  Each descriptor gets its `cells` count.
    """
    tg = [int(t) for t in targets]
    parts = []
    dev = bool(on_device) and bool(tg) and hasattr(table, "cellset_open")
    given = None
    if error_cells is not None:
        r, c = np.asarray(error_cells[0], np.int64), np.asarray(error_cells[1], np.int32)
        keep = np.isin(c, tg) & (r >= 0) & (r < table.n)
        given = (r[keep], c[keep])
        if not dev:
            parts.append(given)

    def part(method, *a, **kw):
        """One detector call: its cells into `parts`, or (on the device) into the cell set; returns them or their count."""
        if dev:
            n = method(*a, fetch=False, **kw)
            table.cellset_add()
            return n
        parts.append(method(*a, **kw))
        return parts[-1]

    set_cols = sorted(set(tg))                         # the set emits by position in this list: column order, as `_merge_cells` orders
    if keep_open and not dev:
        raise ValueError("keep_open needs a table with a cell set and at least one target")
    if dev:
        table.cellset_open(set_cols)
    opened = dev
    try:
        if value_detectors:
            descs = {int(d["col"]): d for d in value_detectors if int(d["col"]) in tg}
            call = []
            for t in tg:                                   # position in the list = column order, as `_merge_cells` orders the result
                d = descs.get(t)
                null = bool(detect_nulls or (d is not None and d["null_is_error"]))
                lo, hi, bits = (d["keep_lo"], d["keep_hi"], d["flag_bits"]) if d is not None else (0, -1, None)
                if null or lo <= hi or bits is not None:
                    call.append((t, null, lo, hi, bits))
            if call:
                res = part(table.detect_cells, [x[0] for x in call], [x[1] for x in call], [x[2] for x in call], [x[3] for x in call],
                           [x[4] for x in call])
                if dev:
                    # the call's own count per column: it is the first part, so the set holds nothing else yet and a count-only emit gives it
                    found = np.zeros(table.c, np.int64)
                    if descs:
                        found[set_cols] = table.cellset_emit(fetch=False)
                else:
                    found = np.bincount(res[1], minlength=table.c) if len(res[1]) else np.zeros(table.c, np.int64)
                for d in descs.values():
                    d["cells"] = int(found[int(d["col"])])
        elif detect_nulls and tg:
            part(table.detect_nulls, tg)
        for con in constraints:
            if isinstance(con, dict):
                attrs = [int(a) for a in con["refs"] if a in tg]
                if not attrs:
                    continue
                try:
                    if con["kind"] == "dc":
                        part(table.detect_dc, con["preds"], cell_cols=attrs, max_pairs=int(con.get("max_pairs", 0)))
                    elif con["kind"] == "dc_scan":         # an order constraint by sort and scan (`route_order_constraints`)
                        part(table.detect_dc_scan, con["preds"], cell_cols=attrs)
                    else:
                        part(table.detect_row_bits, con["cols"], con["bits"], cell_cols=attrs)
                except Exception as e:  # noqa: BLE001
                    if getattr(e, "code", None) == -2:     # RGBM_ERR_PARAM: more pairs than max_pairs, a key span beyond 2^63
                        raise NotResidentEligible("denial constraint: %s" % e)
                    raise
                continue
            eq, iq = con
            attrs = []
            for a in list(eq) + [iq]:
                if a in tg and a not in attrs:
                    attrs.append(a)
            if attrs:
                part(table.detect_constraint, list(eq), int(iq), cell_cols=attrs)
        if keep_open:
            if given is not None and len(given[0]):
                table.cellset_add_cells(*given)
            opened = False                                 # the caller's from here on
            return None
        if dev:
            rows, cols, codes, _ = table.cellset_emit()
    finally:
        if opened:
            table.cellset_close()
    if dev and given is None:
        return rows, cols, codes
    if dev:
        parts = [(rows, cols), given]
    rows, cols = _merge_cells(table.n, parts)
    return (rows, cols, table.read_cells(rows, cols)) if on_device else (rows, cols)


# searched parameter (sklearn alias, train.py:148-156) -> LightGBM core name of rgbm_params
_POINT_TO_CORE = dict(num_leaves="num_leaves", subsample="bagging_fraction", subsample_freq="bagging_freq", colsample_bytree="feature_fraction",
                      min_child_samples="min_data_in_leaf", min_child_weight="min_sum_hessian_in_leaf", reg_lambda="lambda_l2")


def search_on_table(engine, table, t, n_codes, base_params, opts, y_value=None, rows=None):
    """The hyper-parameter search of one target (train.py:133-209) on RESIDENT tables: every CV fold is a pair of device row gathers
    of the training table (no pandas slicing, no re-encoding, no upload per fit -- the value-space search pays all three for each
    of its >= 150 fits), trained and scored through the table API; the folds of `model.hp.batch_size` evaluations are in flight
    together, one HIP stream per fit.  Same points (RandomState(42)), same folds (StratifiedKFold / KFold shuffled with the
    evaluation index) and same stopping rule as repair.train.run_search -- it IS that loop.  Returns core parameters of the best point."""
    from sklearn.metrics import f1_score, mean_squared_error
    from sklearn.model_selection import KFold, StratifiedKFold
    from repair.engine import balanced_class_weight, model_params
    from repair.train import _opt_n_splits, run_search
    from repair.utils import get_option_value
    col = table.read_column(t)
    rows = np.flatnonzero(col >= 0) if rows is None else np.asarray(rows, np.int64)
    y = col[rows]
    feats = [c for c in range(table.c) if c != t]
    discrete = y_value is None
    n_splits = int(get_option_value(opts, *_opt_n_splits))

    def folds(seed):
        cv = StratifiedKFold(n_splits=n_splits, shuffle=True, random_state=seed) if discrete else KFold(n_splits=n_splits, shuffle=True, random_state=seed)
        return list(cv.split(np.zeros(len(rows)), y))

    def core(point):
        p = dict(base_params)
        for k, v in point.items():
            p[_POINT_TO_CORE[k]] = int(v) if k in ("num_leaves", "subsample_freq", "min_child_samples") else float(v)
        return p

    def fold_score(point, fold):
        tr, va = fold
        ttab, vtab = table.gather_rows(np.sort(rows[tr])), table.gather_rows(np.sort(rows[va]))
        cnt = ttab.count_codes(t)[0]
        m = engine.train(ttab, t, feats, balanced_class_weight(cnt), model_params(int(n_codes[t]), core(point), continuous=not discrete), y_value=y_value)
        lab, pr = engine.repair_chain(vtab, [m], [t], [feats], 0, vtab.n)
        truth = vtab.read_column(t)
        if discrete:
            return float(f1_score(truth, lab[0], average="macro"))
        return -float(mean_squared_error(np.asarray(y_value, np.float64)[truth], pr[0]))

    def score(m, vtab):
        lab, pr = engine.repair_chain(vtab, [m], [t], [feats], 0, vtab.n)
        truth = vtab.read_column(t)
        if discrete:
            return float(f1_score(truth, lab[0], average="macro"))
        return -float(mean_squared_error(np.asarray(y_value, np.float64)[truth], pr[0]))

    def batch_scores(jobs):
        """All fold fits of a batch of evaluations through ONE batched training call (engine.train_many ->
        rgbm_table_train_batch); a fit that fails yields its exception, like the fold_score future would."""
        fits, truths = [], []
        for point, (tr, va) in jobs:
            rtr, rva = np.sort(rows[tr]), np.sort(rows[va])
            ttab, vtab = table.gather_rows(rtr), table.gather_rows(rva)
            cnt = np.bincount(col[rtr], minlength=int(n_codes[t]))        # the fold's label counts (the host holds the column already)
            fits.append((ttab, t, feats, balanced_class_weight(cnt), dict(model_params(int(n_codes[t]), core(point), continuous=not discrete), want_model=False), y_value, vtab))
            truths.append(col[rva])
        out = []
        for res, truth in zip(engine.train_many(fits), truths):     # the validation rows were scored while the fits trained
            try:
                if isinstance(res, Exception):
                    out.append(res)
                elif discrete:
                    out.append(float(f1_score(truth, res[1], average="macro")))
                else:
                    out.append(-float(mean_squared_error(np.asarray(y_value, np.float64)[truth], res[2])))
            except Exception as e:   # noqa: BLE001
                out.append(e)
        return out

    use_batch = hasattr(engine, "train_many") and table.n <= engine.small_rows()
    point, _, _ = run_search(opts, folds, fold_score, batch_scores=batch_scores if use_batch else None)
    return {_POINT_TO_CORE[k]: (int(v) if k in ("num_leaves", "subsample_freq", "min_child_samples") else float(v)) for k, v in point.items()}


def distinct_rows(codes, n_codes, max_mult=255):
    """The DISTINCT rows of a label-encoded table and how often each occurs: codes [C][N] int32 (-1 = NULL) ->
    (distinct [C][M] int32, mult [M] uint8, inverse [N] int64: the distinct row every original row maps to).
    A row that occurs more than `max_mult` times is kept as several rows whose multiplicities add up (the trainer carries a multiplicity in one byte).
    What it is for: `_native.Table(distinct, n_codes).set_row_multiplicity(mult)` trains byte for byte the models of the whole table
    (identical rows take identical paths and gradients in every tree; all sums are exact integers) at the cost of its distinct rows -- a quarter
    of the rows on the categorical tables this plugin repairs (the synthetic 10M x 16 benchmark table holds 2.48M distinct rows).  A VARIANT of
    the workload: bench.py --dedup reports it apart from the row-for-row line.  The reference's frames hold every row (model.py:768-815)."""
    codes = np.ascontiguousarray(codes, np.int32)
    C, N = codes.shape
    # mixed-radix keys over (code + 1) in [0, n_codes]: as few uint64 words per row as the radices need
    words, cur, room = [], np.zeros(N, np.uint64), 1
    for c in range(C):
        radix = int(n_codes[c]) + 1
        if room * radix >= (1 << 63):
            words.append(cur); cur, room = np.zeros(N, np.uint64), 1
        cur = cur * np.uint64(radix) + (codes[c] + 1).astype(np.uint64)
        room *= radix
    words.append(cur)
    if len(words) == 1:
        _, first, inverse, counts = np.unique(words[0], return_index=True, return_inverse=True, return_counts=True)
    else:
        key = np.ascontiguousarray(np.stack(words, axis=1)).view([("w%d" % i, np.uint64) for i in range(len(words))]).reshape(N)
        _, first, inverse, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    reps = (counts + max_mult - 1) // max_mult                      # distinct rows kept more than once
    rows = np.repeat(first, reps)
    mult = np.full(len(rows), max_mult, np.int64)
    last = np.cumsum(reps) - 1
    mult[last] = counts - (reps - 1) * max_mult
    start = np.concatenate([[0], np.cumsum(reps)[:-1]])
    return np.ascontiguousarray(codes[:, rows]), mult.astype(np.uint8), start[inverse].astype(np.int64)


def distinct_training_tables(engine, table, targets, base_params, spec, train_tables, search_opts=None, continuous=(), rebalanced=()):
    """The opt-in hook `repair_table(distinct_training_rows=dict(max_ratio=..))`: enters ONE distinct-row table of `table`
    (`Table.distinct_rows()`: rgbm_table_distinct_rows, multiplicities attached) into `train_tables` for every target in `targets` that
    qualifies.  A target keeps the whole table, with the reason logged and returned, when
      - `train_rows` picked a sample for it (`train_tables` holds it already), or it trains on a rebalanced table (`rebalanced`);
      - a hyper-parameter search runs (`search_opts`): it gathers folds, and gathers drop multiplicities;
      - the parameters are not what the multiplicity trainer honours (include/rgbm.h rgbm_table_set_row_multiplicity: the level grower,
        1 <= max_depth <= 7, no bagging, at most 32 features with a free byte in the last 16-feature record), or the target is
        continuous (the variant is pinned for classifiers);
      - the table, or its distinct table, has at most `engine.small_rows()` rows: `run_job` sends such tables to the batched trainer, which
        does not carry multiplicities;
      - the table holds more than max_ratio * N distinct rows (M rows cost more each than N: DESIGN 5g);
      - the engine's table has no `distinct_rows`.
    The parameter checks restate what the trainer would refuse, to spare the `distinct_rows()` call; they are not the guard.  What only the
    trainer can know -- a table of 17 to 31 features whose bins do not fit the one-pass forms that carry the multiplicity, a run-time switch
    -- it refuses with RGBM_ERR_PARAM, and `run_job(fallback_tables=..)` then trains that target on the whole table (`repair_table` moves it to
    `skipped` with the trainer's message).
    Returns (the distinct table or None, dict(rows=N, distinct=M or None when it was not computed, used_for=[targets], skipped={target: reason})).
    The table is freed at once when no target qualifies; the caller frees it otherwise."""
    N = int(table.n)
    max_ratio = float(spec.get("max_ratio", 0.5))
    small = int(engine.small_rows()) if hasattr(engine, "small_rows") else 0
    info = dict(rows=N, distinct=None, used_for=[], skipped={})
    F = int(table.c) - 1
    depth = int(base_params.get("max_depth", -1))
    bagging = int(base_params.get("bagging_freq", 0)) > 0 and float(base_params.get("bagging_fraction", 1.0)) < 1.0
    for_all = None
    if not hasattr(table, "distinct_rows"):
        for_all = "the engine's table has no distinct_rows"
    elif search_opts is not None:
        for_all = "a hyper-parameter search gathers folds, and gathers drop multiplicities"
    elif not 1 <= depth <= 7 or os.environ.get("RGBM_GROWER") == "leafwise":
        for_all = "max_depth %d: rows with multiplicities train with the level grower (1 <= max_depth <= 7)" % depth
    elif bagging:
        for_all = "bagging draws per original row"
    elif F > 32 or F % 16 == 0:
        for_all = "%d features: rows with multiplicities take at most 32 with a free byte in the last 16-feature record" % F
    elif N <= small:
        for_all = "%d rows: tables of up to %d rows go to the batched trainer, which carries no multiplicities" % (N, small)
    cand = []
    for t in targets:
        if for_all is not None:
            info["skipped"][t] = for_all
        elif t in rebalanced:
            info["skipped"][t] = "trained on a rebalanced table (rebalance)"
        elif t in train_tables:
            info["skipped"][t] = "trained on a row sample (train_rows)"
        elif t in continuous:
            info["skipped"][t] = "continuous target: rows with multiplicities are pinned for classifiers"
        else:
            cand.append(t)
    dtab = None
    if cand:
        dtab = table.distinct_rows()
        M = info["distinct"] = int(dtab.n)
        why = None
        if M <= small:
            why = "%d distinct rows: tables of up to %d rows go to the batched trainer, which carries no multiplicities" % (M, small)
        elif M > max_ratio * N:
            why = "%d distinct rows of %d: more than max_ratio = %g of them" % (M, N, max_ratio)
        if why is not None:
            info["skipped"].update({t: why for t in cand})
            if hasattr(dtab, "close"):
                dtab.close()
            dtab = None
        else:
            info["used_for"] = list(cand)
            train_tables.update({t: dtab for t in cand})
    for t, why in info["skipped"].items():
        _logger.info("[Repair Model Training Phase] target column %d trains on the whole table, not on its distinct rows: %s" % (t, why))
    if info["used_for"]:
        _logger.info("[Repair Model Training Phase] target columns %s train on the %d distinct rows of %d" % (info["used_for"], info["distinct"], N))
    return dtab, info


def rebalanced_training_table(table, t, rows=None, k=5, random_state=42, name=None, class_names=None):
    """The training table of discrete target column t after `rebalance_training_data` (train.py:242-293), built on the device: the NULL
    pattern of the needed columns is read, `repair.rebalance_codes.rebalance_plan` makes every draw on the host, `Table.smoten` grows the
    synthetic rows, and `gather_rows` + `concat` + one final `gather_rows` put the frame [rows without NULLs, synthetic rows class by class,
    rows with NULLs] into the plan's order.  `rows`: the training rows in the value-space frame's order (the sampler's; default: the rows whose
    target is not NULL, ascending).  Returns (table, plan)."""
    from repair.rebalance_codes import rebalance_plan
    rows = np.flatnonzero(table.read_column(t) >= 0) if rows is None else np.asarray(rows, np.int64)
    sub = table.gather_rows(rows)                      # the training rows in frame order: everything below counts positions in it
    feats = [c for c in range(int(table.c)) if c != t]
    has_null = np.zeros(len(rows), bool)
    for f in feats:
        has_null |= sub.read_column(f) < 0
    plan = rebalance_plan(sub.read_column(t), has_null, target=str(t) if name is None else name, class_names=class_names, k=k,
                          random_state=random_state)
    parts = []
    if len(plan["fit"]):
        parts.append(sub.gather_rows(plan["fit"]))
    if len(plan["classes"]):
        parts.append(sub.smoten(t, feats, plan["fit"], plan["classes"], plan["pick_off"], plan["picks"], k=k))
    if len(plan["with_null"]):
        parts.append(sub.gather_rows(plan["with_null"]))
    frame = type(table).concat(parts)
    out = frame.gather_rows(plan["order"])
    for p in parts + [frame, sub]:
        if hasattr(p, "close"):
            p.close()
    return out, plan


class NotResidentEligible(ValueError):
    """The run is not the plain per-attribute model loop after all (only known once the error cells are NULLed): a discrete target
    is left with fewer than two classes, a continuous one with no value.  The reference short-cuts those with `PoorModel`
    (model.py:1008-1017, 779-783); `RepairModel._run` catches this and takes the value-space path, which has that short-cut."""


def _detector_report(value_detectors):
    if not value_detectors:
        return None
    return [dict(col=int(d["col"]), kinds=list(d.get("kinds", ())), codes_flagged=int(d.get("codes_flagged", 0)),
                 cells=int(d.get("cells", 0))) for d in value_detectors]


class DeadClasses(NotResidentEligible):
    """Detection ran on the device and found error cells that hold the ONLY occurrences of some values of a target attribute: the
    dictionaries were built before the cells were known, so those values would stay behind as classes without rows.  Carries the
    detected cells (row positions, column indices): `repair_frame` NULLs them in the dictionary indices, drops the dead values,
    uploads again and goes on WITHOUT detecting a second time (and without leaving the resident path).  What the first pass found out and
    the second does not compute again rides along: `domain_info` (the cell-domain summary; the cells carried are the pruned ones) and
    `value_detectors` (the detector report)."""

    def __init__(self, msg, rows, cols, domain_info=None, value_detectors=None):
        super().__init__(msg)
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int32)
        self.domain_info, self.value_detectors = domain_info, value_detectors


class UnseenCategories(NotResidentEligible):
    """A dirty row holds a categorical feature value that none of the target's training rows has (see `unseen_categories`)."""


def unseen_categories(table, dirty_tab, targets, ordered_cols=(), train_tables=None):
    """[(target, feature, codes)]: categorical feature codes that occur in the rows a target model has to repair but in none of the
    rows it trains on.  The value-space path gives such a value the code -1 (the model's own dictionary does not hold it: it is
    MISSING for that model); the resident table codes it like any other value and the trees would bin it next to its dictionary
    neighbours.  Callers that promise the value-space result (RepairModel.run) check this and fall back."""
    C = table.c
    d = np.stack([dirty_tab.read_column(c) for c in range(C)])
    total = [table.count_codes(c)[0] for c in range(C)]
    out = []
    for t in targets:
        need = d[t] < 0                                   # the rows this model's prediction is used for; all of them are dirty rows
        if not need.any():
            continue
        for f in range(C):
            if f == t or f in ordered_cols:
                continue
            v = d[f][need]
            v = v[v >= 0]
            if len(v) == 0:
                continue
            held = np.bincount(v, minlength=len(total[f]))   # rows with this code whose target cell is NULL: not training rows
            if train_tables and t in train_tables:            # the model trains on a row sample (its target cells are all non-NULL)
                seen = train_tables[t].count_codes(f)[0]
            else:
                seen = total[f] - held
            gone = np.flatnonzero((held > 0) & (seen <= 0))
            if len(gone):
                out.append((t, f, gone))
    return out


class TableBackend:
    """`repair.domain` backend on a resident table: `Table.pair_counts` / `Table.cell_domains` (csrc/rgbm_domain.hip).  Dense tables
    beyond the library's cap (RGBM_ERR_PARAM) or more correlated attributes than the kernel takes leave the resident path."""
    MAX_CORR = 8

    def __init__(self, table, view):
        self.table, self.view = table, view

    def pair_counts(self, pairs):
        from repair.domain import Joint
        try:
            dense = self.table.pair_counts(pairs, luts=self.view.luts, n_bins=self.view.n_bins)
        except Exception as e:  # noqa: BLE001
            if getattr(e, "code", None) == -2:
                raise NotResidentEligible("cell-domain analysis: %s" % e)
            raise
        return [Joint.from_dense(d) for d in dense]

    def cell_domains(self, target, rows, corr, ptable, min_cnt, single_ok, beta, row_count, want_probs=False):
        if len(corr) > self.MAX_CORR:
            raise NotResidentEligible("cell-domain analysis: %d correlated attributes (the device entry takes %d)" % (len(corr), self.MAX_CORR))
        pidx = [ptable.index[frozenset((int(c), int(target)))] for c in corr]
        return self.table.cell_domains(target, rows, pidx, min_cnt, single_ok, beta, row_count, want_probs=want_probs)

    def drop_weak(self, target, corr, ptable, min_cnt, single_ok, beta, row_count):
        """(cells examined, cells cleared) of the target's column of the table's open cell set (`Table.cellset_drop_weak`)."""
        if len(corr) > self.MAX_CORR:
            raise NotResidentEligible("cell-domain analysis: %d correlated attributes (the device entry takes %d)" % (len(corr), self.MAX_CORR))
        pidx = [ptable.index[frozenset((int(c), int(target)))] for c in corr]
        return self.table.cellset_drop_weak(target, pidx, min_cnt, single_ok, beta, row_count)


def analyse_cell_domains(table, targets, rows, cols, spec, cell_counts=None):
    """The second half of ErrorModel.detect (errors.py:553-578) on the resident table, BEFORE any cell is NULLed: pair counts on the
    device, entropies and attribute selection on the host from the integer counts, cell domains on the device.
    spec: dict(options={error.*: value}, discrete_thres, domain_stats [C], continuous={column: ascending distinct values},
    keep_weak=False).  Returns repair.domain.analyse's dict.  `cell_counts` {column: cells}: the cells lie in the table's open cell set
    (rows and cols are None) and the weak-labelled ones are cleared there; the dict then holds `weak_counts` (repair.domain.analyse)."""
    from repair import domain
    view = domain.discretised_view(table.n_codes, spec["domain_stats"], spec.get("continuous") or {}, int(spec["discrete_thres"]))
    return domain.analyse(TableBackend(table, view), int(table.n), view, targets, spec["domain_stats"], rows, cols, spec.get("options") or {},
                          want_weak=not spec.get("keep_weak", False), cell_counts=cell_counts)


def nearest_value_merges(engine, table, targets, rows, cols, current, spec):
    """`_repair_by_nearest_values` (python/repair/model.py; reference model.py:1279-1291) on the NULLed table: per error cell the code of
    the value it is merged to, or -1.  A cell of one of spec["targets"] with a truthy current value is merged to the closest live value
    of its column (`count_codes` > 0 after the NULL-out) when that cost is <= spec["threshold"] and strictly below the second closest;
    pairs whose cost is None do not take part.  The distinct current values and the live values go to the engine as two string pools
    (`engine.nearest_values`: Levenshtein distances and the row reduction on the device; any other cost function fills the matrix on the
    host, NaN for None, for the same reduction)."""
    out = np.full(len(rows), -1, np.int32)
    cost_fn = spec.get("cost")
    for t in [int(t) for t in spec["targets"] if int(t) in targets]:
        sel = np.flatnonzero(cols == t)
        if len(sel) == 0:
            continue
        live = np.flatnonzero(table.count_codes(t)[0] > 0)
        dom = list(spec["domain"](t, live))
        cur = list(spec["current"](t, rows[sel], current[sel]))
        b_at = [j for j, v in enumerate(dom) if v]               # compute() is None for a falsy side
        vals = list(dict.fromkeys(v for v in cur if v))
        if not vals or not b_at:
            continue
        if len(vals) * len(b_at) > (1 << 28):
            raise NotResidentEligible("target column %d: the nearest-value cost matrix would hold %d x %d entries" % (t, len(vals), len(b_at)))
        pool_b = [dom[j] for j in b_at]
        if cost_fn is None:
            near = engine.nearest_values(vals, pool_b, float(spec["threshold"]))
        else:
            cost = np.full((len(vals), len(pool_b)), np.nan, np.float64)
            for i, v in enumerate(vals):
                for j, d in enumerate(pool_b):
                    x = cost_fn(v, d)
                    if x is not None:
                        cost[i, j] = float(x)
                        if np.isnan(cost[i, j]):
                            raise NotResidentEligible("target column %d: the cost function returned NaN" % t)
            near = engine.nearest_values(vals, pool_b, float(spec["threshold"]), cost=cost)
        near = np.asarray(near, np.int64)
        code_of = np.where(near >= 0, live[np.asarray(b_at, np.int64)[np.maximum(near, 0)]], -1).astype(np.int32)
        row_of = {v: i for i, v in enumerate(vals)}
        at = np.array([row_of[v] if v else -1 for v in cur], np.int64)
        out[sel] = np.where(at >= 0, code_of[np.maximum(at, 0)], -1)
    return out


def rule_step_summary(table, t, step, cell_rows, dirty_rows, dirty_tab, labels):
    """What a rule step did to the error cells of its target, for `_last_resident_info`: dict(target, kind, x, cells, mapped[, conflict,
    unseen, null_source]).  FD steps: `mapped` cells took the source's single value; `conflict`: the source value occurs with several
    target values; `unseen`: it occurs in no row whose target cell is non-NULL; `null_source`: the source cell itself is NULL."""
    info = dict(target=int(t), kind=step["kind"], x=int(step["x"]), cells=int(len(cell_rows)), mapped=int((labels >= 0).sum()))
    if step["kind"] != "fd" or len(cell_rows) == 0:
        return info
    x = int(step["x"])
    xv = dirty_tab.read_column(x)[np.searchsorted(dirty_rows, cell_rows)]      # the source as the step saw it (after the chain before it)
    total = table.count_codes(x)[0]
    nrows, _ = table.detect_nulls([t])
    held = table.gather_rows(nrows).count_codes(x)[0] if len(nrows) else np.zeros_like(total)
    seen = (total - held) > 0                                                  # the value occurs next to a non-NULL target cell
    miss = (labels < 0) & (xv >= 0)
    info.update(conflict=int((miss & seen[np.maximum(xv, 0)]).sum()), unseen=int((miss & ~seen[np.maximum(xv, 0)]).sum()),
                null_source=int((xv < 0).sum()))
    return info


def cell_pmfs(engine, table, pmf_tab, targets, models, rows, cols, current, dirty_rows, continuous, y_values, integral, top_k, threshold,
              pmf_costs):
    """The candidate distributions of the error cells (rows, cols, current) for `repair_table(want_pmf=True)`, whose arguments these
    are: `pmf_tab` holds the dirty rows un-repaired, `models` the trained models by target.  Returns dict(pmf_class, pmf_prob,
    current_prob[, top1_cost, pmf_value])."""
    pc = np.full((len(rows), top_k), -1, np.int32)
    pp = np.zeros((len(rows), top_k), np.float64)
    cp = np.zeros(len(rows), np.float64)
    tc = np.full(len(rows), np.nan, np.float64)
    pv = np.full(len(rows), np.nan, np.float64)
    for t in targets:
        sel = np.flatnonzero(cols == t)
        feats = [c for c in range(table.c) if c != t]
        if t in continuous:       # continuous attributes have no pmf (model.py:1215-1222: the value with prob 1.0)
            if pmf_costs is not None and t in models:
                from repair.engine import chained_repair
                _, _, v = chained_repair(engine, pmf_tab, [engine.load_model(models[t])], [t], [feats], 0, pmf_tab.n, y_values, integral)
                pv[sel] = v[0][np.searchsorted(dirty_rows, rows[sel])]
            continue
        if len(sel) == 0:
            continue
        model = engine.load_model(models[t])
        # NULL cells of t in the dirty frame: a superset of this target's error cells when NULL detection is off
        drows, _ = pmf_tab.detect_nulls([t])
        j = np.searchsorted(dirty_rows[drows], rows[sel])
        cur_for = np.full(len(drows), -1, np.int32)
        cur_for[j] = current[sel]                          # the value the cell held (model.py:1196-1199: its probability)
        spec = pmf_costs(t, rows[sel]) if pmf_costs is not None else None
        if pmf_costs is None:
            _, dcls, dpr, dcp = pmf_tab.repair_pmf(model, t, feats, top_k=top_k, threshold=threshold, cur_codes=cur_for)
        else:
            spec = dict(spec or {})
            if spec.get("cur_code") is not None:
                cur_for[j] = spec["cur_code"]
            crow = None
            if spec.get("cost") is not None:
                crow = np.full(len(drows), -1, np.int32)
                if spec.get("cost_row") is not None:
                    crow[j] = spec["cost_row"]
            _, dcls, dpr, dcp, dtc = pmf_tab.repair_pmf_weighted(model, t, feats, top_k=top_k, threshold=threshold, cur_codes=cur_for,
                                                                 cost_rows=crow, cost=spec.get("cost"), weight=float(spec.get("weight", 0.0)),
                                                                 renormalise=bool(spec.get("renormalise", False)))
            tc[sel] = dtc[j]
        pc[sel], pp[sel], cp[sel] = dcls[j], dpr[j], dcp[j]
    out = dict(pmf_class=pc, pmf_prob=pp, current_prob=cp)
    if pmf_costs is not None:
        out.update(top1_cost=tc, pmf_value=pv)
    return out


def _detect_and_prune(table, targets, constraints, detect_nulls, error_cells, only_noisy_targets, domain_analysis, value_detectors, regex_cols):
    """Phase 1 of `repair_table`: the error cells, before anything is NULLed.  Returns (rows, cols, the targets to repair, domain summary or
    None, the value detectors' descriptors, seconds).

    only_noisy_targets: train models for the target attributes that hold at least one error cell only (the reference's `target_columns` are
                 the noisy columns, errors.py:472-477); `_target_plan` then insists that every label of such a target keeps a training row.
    domain_analysis: the checked `error.*` options and the view's inputs (`analyse_cell_domains`): the reference's cell-domain analysis
                 runs on the detected cells of the noisy targets before anything is NULLed, and the weak-labelled cells (the current
                 value is the most probable one) leave the error cells (errors.py:507-530).  None = every detected cell is repaired.
    value_detectors: per-column code predicates of the regex / value-domain / outlier detectors (`detect_error_cells`), or a callable
                 (table) -> such a list, called on the table before any cell is NULLed (autofill and quartiles need its rows per code).
    regex_cols : columns with a regex-structure repair (`repair_frame`: rules['regex']).  When the cells are detected here and one lies in such
                 a column, nothing is NULLed: DeadClasses hands the (pruned) cells to the caller, who evaluates them and comes back with the
                 remaining ones as `error_cells`."""
    t0 = time.perf_counter()
    if callable(value_detectors):
        value_detectors = value_detectors(table)
    found_rows, found_cols = detect_error_cells(table, targets, constraints, detect_nulls, error_cells, value_detectors=value_detectors)
    noisy = set(int(c) for c in np.unique(found_cols))
    kept = [t for t in targets if t in noisy] if only_noisy_targets else targets
    rows, cols, domain_info = found_rows, found_cols, None
    if domain_analysis is not None and len(found_rows):
        da = analyse_cell_domains(table, [t for t in kept if t in noisy], found_rows, found_cols, domain_analysis)
        domain_info = dict(pairwise=da["pairwise"], noisy_cells=int(len(found_rows)), weak_cells=int(da["weak"].sum()))
        _logger.info("[Error Detection Phase] %d noisy cells fixed and %d error cells remaining..." % (domain_info["weak_cells"],
                                                                                                   len(found_rows) - domain_info["weak_cells"]))
        rows, cols = found_rows[~da["weak"]], found_cols[~da["weak"]]
    seconds = time.perf_counter() - t0
    if regex_cols and error_cells is None and len(rows):
        in_regex = np.isin(cols, list(regex_cols))
        if in_regex.any():
            # regex-structure repair rewrites cells from their STRINGS, and a repaired string may be new to its column: the caller evaluates
            # the cells, patches the encoding and comes back with the remaining cells as given (the route of DeadClasses)
            raise DeadClasses("%d detected cells lie in attributes with a regex-structure repair" % int(in_regex.sum()), rows, cols,
                              domain_info=domain_info, value_detectors=_detector_report(value_detectors))
    return rows, cols, kept, domain_info, value_detectors, seconds


SET_ROUTE_METHODS = ("cellset_open", "cellset_add", "cellset_emit", "cellset_close", "cellset_add_cells", "cellset_drop_weak", "cellset_null",
                     "cellset_rows")


def set_route_refusal(table, targets):
    """Why phases 1 and 2 cannot run on the table's cell set (`_cells_on_set`), or None."""
    missing = [m for m in SET_ROUTE_METHODS if not hasattr(table, m)]
    if missing:
        return "the engine's table has no %s" % ", ".join(missing)
    if not targets:
        return "no target attribute"
    from repair import dist
    if dist.world()[1] > 1:
        return "a job on %d ranks merges its cells on the host" % dist.world()[1]
    return None


def _cells_on_set(engine, table, targets, constraints, detect_nulls, error_cells, only_noisy_targets, domain_analysis, value_detectors, regex_cols,
                  nearest):
    """Phases 1 and 2 of `repair_table` on the table's CELL SET: what `_detect_and_prune` and `_null_and_merge` give, cell for
    cell, without the error cells travelling in between.  Every detector's cells join the set on the device and the given `error_cells` go
    up once (`detect_error_cells(keep_open=True)`); a count-only emit names the noisy columns; the cell-domain analysis clears the
    weak-labelled cells in the set (`Table.cellset_drop_weak`, one call per target); ONE fetching emit brings the remaining cells down with
    the codes they hold; `Table.cellset_null` NULLs them from the matrix and `Table.cellset_rows` gives the dirty rows.  With
    nearest-value merges the merged cells are written back and the dirty rows of the others come from `Table.rows_of_cells`.
    Returns (the pruned cells as detected: rows, cols; the targets to repair; domain summary or None; the detectors' descriptors; seconds
    of phase 1; then `_null_and_merge`'s tuple)."""
    t0 = time.perf_counter()
    if callable(value_detectors):
        value_detectors = value_detectors(table)
    set_cols = sorted(set(targets))
    detect_error_cells(table, targets, constraints, detect_nulls, error_cells, value_detectors=value_detectors, on_device=True, keep_open=True)
    try:
        counts = np.asarray(table.cellset_emit(fetch=False), np.int64)
        noisy = set(c for c, k in zip(set_cols, counts) if k > 0)
        noisy_cells = int(counts.sum())
        kept = [t for t in targets if t in noisy] if only_noisy_targets else targets
        domain_info = None
        if domain_analysis is not None and noisy_cells:
            da = analyse_cell_domains(table, [t for t in kept if t in noisy], None, None, domain_analysis,
                                      cell_counts={c: int(k) for c, k in zip(set_cols, counts)})
            domain_info = dict(pairwise=da["pairwise"], noisy_cells=noisy_cells, weak_cells=int(sum(da["weak_counts"].values())))
            _logger.info("[Error Detection Phase] %d noisy cells fixed and %d error cells remaining..." % (domain_info["weak_cells"],
                                                                                                       noisy_cells - domain_info["weak_cells"]))
        rows, cols, current, _ = table.cellset_emit()
        seconds = time.perf_counter() - t0
        if regex_cols and error_cells is None and len(rows):
            in_regex = np.isin(cols, list(regex_cols))
            if in_regex.any():                             # as in `_detect_and_prune`: nothing is NULLed, the caller comes back with the cells
                raise DeadClasses("%d detected cells lie in attributes with a regex-structure repair" % int(in_regex.sum()), rows, cols,
                                  domain_info=domain_info, value_detectors=_detector_report(value_detectors))
        table.cellset_null()
        if nearest is None or not len(rows):
            tail = (rows, cols, current, None, table.cellset_rows())
        else:
            near = nearest_value_merges(engine, table, kept, rows, cols, current, nearest)
            done = near >= 0
            merged = dict(rows=rows[done], cols=cols[done], current=current[done], repaired=near[done])
            table.write_cells(merged["rows"], merged["cols"], merged["repaired"])
            tail = (rows[~done], cols[~done], current[~done], merged, table.rows_of_cells(rows[~done]))
    finally:
        table.cellset_close()
    return (rows, cols, kept, domain_info, value_detectors, seconds) + tail


def _null_and_merge(engine, table, targets, rows, cols, nearest):
    """Phase 2: convertErrorCellsToNull (RepairApi.scala:171-211), then the nearest-value merges (`nearest`: rules['nearest'] of
    `repair_table`, or None) written back -- model.py `_repair_attrs(repaired_by_rules_df, ..)`.  Returns (rows, cols, current of the
    cells that stay error cells, the merged cells as dict(rows, cols, current, repaired) or None, the dirty rows: model.py:549-553)."""
    current = table.read_cells(rows, cols)
    table.null_cells(rows, cols, targets)
    if nearest is None or not len(rows):
        return rows, cols, current, None, table.rows_of_cells(rows)
    near = nearest_value_merges(engine, table, targets, rows, cols, current, nearest)
    done = near >= 0
    merged = dict(rows=rows[done], cols=cols[done], current=current[done], repaired=near[done])
    table.write_cells(merged["rows"], merged["cols"], merged["repaired"])
    return rows[~done], cols[~done], current[~done], merged, table.rows_of_cells(rows[~done])


def _target_plan(table, targets, continuous, rules, only_noisy_targets, second_pass):
    """Phase 3: what answers each target on the NULLed table.  Returns (label counts {model target: rows per class}, rule steps {target:
    dict(x, lut, kind='fd' | 'constant')}, the chain: the targets in prediction order).

    rules      : None, or dict(fd={target: source column}): the target is answered by the functional dependency source -> target
                 (`Table.fd_map` on the whole NULLed table) unless it is left with fewer than two classes; such a discrete target gets a
                 constant step (its one live class, or NULL) instead of NotResidentEligible.  Rule targets are not trained, and the chain runs
                 the other targets in target order, then each FD target once its source is no longer pending (`_resolve_prediction_order`).
    only_noisy_targets: every label of a discrete model target must still have a training row -- `RepairModel.run()` with detection on the
                 device: the cells are not known when the dictionaries are built, so a value that only error cells held would stay behind
                 as a class without rows (num_class enters the softmax hessian factor); DeadClasses then carries `second_pass`: every detected
                 cell (the pruned ones), the domain summary and the detector report, so that the second pass does not analyse again.
    A continuous target needs one non-NULL row, a discrete one two classes (the reference's `PoorModel`, model.py:1008-1017, is the
    constant step of `rules`); NotResidentEligible otherwise."""
    label_counts, rule_steps = {}, {}
    fd = dict(rules.get("fd") or {}) if rules is not None else {}
    for t in targets:
        cnt, _ = table.count_codes(t)
        live = np.flatnonzero(cnt > 0)
        if t in continuous:
            if len(live) < 1:
                raise NotResidentEligible("continuous target column %d has no non-NULL row to learn from" % t)
        elif t in fd and len(live) >= 2:
            # FunctionalDepModel (model.py `_build_rule_model`): the map of the whole NULLed table; no model, so no label-count checks
            rule_steps[t] = dict(x=int(fd[t]), lut=np.asarray(table.fd_map(int(fd[t]), t), np.int32), kind="fd")
            continue
        elif only_noisy_targets and len(live) < len(cnt):
            raise DeadClasses("target column %d: %d of its %d values are held by error cells only" % (t, len(cnt) - len(live), len(cnt)), **second_pass)
        elif len(live) < 2 and rules is not None:
            # PoorModel (model.py:1008-1017): the one live class, or NULL when the column has no value left
            rule_steps[t] = dict(x=-1, lut=np.array([live[0] if len(live) else -1], np.int32), kind="constant")
            continue
        elif len(live) < 2:
            raise NotResidentEligible("target column %d has fewer than two classes among its non-NULL rows; the reference short-cuts such "
                             "attributes with a constant model (model.py:1008-1017) -- drop it from `targets`" % t)
        label_counts[t] = cnt
    pending = [t for t in targets if rule_steps.get(t, {}).get("kind") == "fd"]
    chain = [t for t in targets if t not in pending]
    while pending:
        ready = [t for t in pending if rule_steps[t]["x"] not in pending]
        if not ready:
            raise NotResidentEligible("the functional dependencies of target columns %s form a cycle" % pending)
        chain += ready
        pending = [t for t in pending if t not in ready]
    return label_counts, rule_steps, chain


def _training_tables(engine, table, dirty_tab, model_targets, continuous, label_counts, base_params, train_rows, rebalance, check_unseen,
                     distinct_training_rows, search_opts):
    """Phase 4: the table each of `model_targets` trains on where that is not the whole NULLed table.  Returns ({target: table}, the label
    counts with those of such tables, `rebalanced` {target: dict(median, rows, synthetic, classes)} or None, the distinct-row table or
    None (the caller closes it), its report or None).

    train_rows : {target: row positions} or a callable (target, positions of its non-NULL rows) -> positions -- train that
                 target's model on these rows only (model.max_training_row_num sampling, model.py:755-766); default: every row
                 whose target cell is not NULL.
    rebalance  : None (off) or dict(k=5, random_state=42[, names, class_names: callables for the log]) -- `setTrainingDataRebalancingEnabled`:
                 every discrete target that is trained trains on its rebalanced table (`rebalanced_training_table`: SMOTEN on the device, the
                 draws on the host), made from its `train_rows` in the order given (the sampler's) or from all its non-NULL rows.  The class
                 weights, the unseen-category check and the hyper-parameter search see that table.
    check_unseen: False, True or the ordered columns: raise UnseenCategories when a dirty row holds a category no training row of the
                 target has (`unseen_categories`).
    distinct_training_rows: None (off) or dict(max_ratio=float) -- train the targets that qualify on the DISTINCT rows of the NULLed table with
                 their multiplicities (`distinct_training_tables`: one `Table.distinct_rows()` call on the device); same models, bytes
                 included.  Taken after the error cells are NULLed, the merges written back, the label counts taken from the whole table and
                 the unseen-category check made on it: the distinct table holds rows whose target cell is NULL too (the trainer skips them,
                 as on the whole table)."""
    train_tables, counts = {}, dict(label_counts)
    if callable(train_rows):
        picked = {t: train_rows(t, np.flatnonzero(table.read_column(t) >= 0)) for t in model_targets}
        sampled = {t: r for t, r in picked.items() if r is not None}
    else:
        sampled = dict(train_rows or {})
    rebalanced = None
    if rebalance is not None:
        if not hasattr(table, "smoten"):
            raise NotResidentEligible("rebalancing: the engine's table has no smoten")
        from repair import dist
        if dist.world()[1] > 1:
            raise NotResidentEligible("rebalancing: a multi-rank job does not rebalance its row shards")
        spec = dict(rebalance)
        names, class_names = spec.pop("names", None), spec.pop("class_names", None)
        rebalanced = {}
        for t in [t for t in model_targets if t not in continuous]:
            train_tables[t], plan = rebalanced_training_table(table, t, rows=sampled.get(t), name=names(t) if names else None,
                                                              class_names=class_names(t) if class_names else None, **spec)
            counts[t] = train_tables[t].count_codes(t)[0]
            rebalanced[t] = dict(median=plan["median"], rows=int(train_tables[t].n), synthetic=int(len(plan["picks"])),
                                 classes=[int(c) for c in plan["classes"]])
    for t, r in sampled.items():
        if t not in (rebalanced or {}):
            train_tables[t] = table.gather_rows(np.sort(np.asarray(r, np.int64)))
            counts[t] = train_tables[t].count_codes(t)[0]
    if check_unseen:
        ordered = set(continuous) | set(check_unseen if not isinstance(check_unseen, bool) else ())
        gone = unseen_categories(table, dirty_tab, model_targets, train_tables=train_tables, ordered_cols=ordered)
        if gone:
            raise UnseenCategories("%d (target, feature) pairs hold categories no training row has, e.g. target column %d / feature column %d"
                                   % (len(gone), gone[0][0], gone[0][1]))
    distinct_tab, distinct_info = None, None
    if distinct_training_rows is not None:
        distinct_tab, distinct_info = distinct_training_tables(engine, table, model_targets, base_params, distinct_training_rows, train_tables,
                                                               search_opts, continuous, rebalanced=rebalanced or {})
    return train_tables, counts, rebalanced, distinct_tab, distinct_info


def _train_and_repair(engine, table, dirty_tab, chain, label_counts, base_params, want_stats, y_values, integral, train_tables, search_opts,
                      rule_steps, distinct_tab, distinct_info):
    """Phase 5: `run_job`.  A fit the trainer refuses on the distinct table trains on the whole one (`fallback_tables`) and moves to
    `skipped` of `distinct_info` with the trainer's message; the distinct table is closed either way.

    search_opts: reference option dict (model.hp.*, model.cv.n_splits): run the hyper-parameter search of every target on the
                 resident tables before its final fit (`search_on_table`); None = the fixed parameters."""
    n_codes = np.asarray(table.n_codes, np.int32)
    search = None
    if search_opts is not None:
        def search(t, tab):
            return search_on_table(engine, tab, t, n_codes, base_params, search_opts, y_value=y_values.get(t))
        # fold fits a search keeps in flight per target (run_search: model.hp.batch_size evaluations x model.cv.n_splits folds): run_job
        # budgets device memory with it
        from repair.train import search_fits_in_flight
        search.fits_in_flight = search_fits_in_flight(search_opts)
    try:
        res = run_job(engine, table, dirty_tab, n_codes, chain, label_counts, base_params, want_stats=want_stats,
                      y_values=y_values, integral=integral, train_tables=train_tables, param_search=search, rule_steps=rule_steps,
                      fallback_tables={t: table for t in distinct_info["used_for"]} if distinct_tab is not None else None)
    finally:
        if distinct_tab is not None and hasattr(distinct_tab, "close"):
            distinct_tab.close()
    for t, why in (res.get("fell_back") or {}).items():          # the trainer refused the distinct table for this fit: it trained on the whole one
        distinct_info["used_for"] = [u for u in distinct_info["used_for"] if u != t]
        distinct_info["skipped"][t] = "the trainer refused the distinct table: %s" % why
        _logger.info("[Repair Model Training Phase] target column %d trained on the whole table after all: %s" % (t, why))
    return res


def _apply_fitted(engine, dirty_tab, fitted):
    """The phase that stands for `_target_plan`, `_training_tables` and `_train_and_repair` when a kept fit is applied (`repair_table(fitted=..)`,
    DESIGN 5q): nothing is trained.  The dirty rows are translated into the code space of the fit on the device (`engine.recode`:
    rgbm_table_recode), the table gets the fitted column kinds and values, every blob is loaded (`engine.load_model`) and `chained_repair` runs the
    fitted chain on it.  Labels are FITTED codes.  Returns (the model-space table, a result shaped like `run_job`'s, dict(unmapped {column:
    cells that held a value the fitted dictionaries cannot express}, recode_seconds)).

    fitted : dict(chain=[target columns in prediction order], feats={target: feature columns in the fit's order}, blobs={target: bytes},
             y_values={continuous target: the fitted values}, integral={targets}, luts=[per column int32 LUT or None], n_codes_out=[per column],
             categorical=[columns], values={numeric column: the fitted values})."""
    from repair.engine import chained_repair
    t0 = time.perf_counter()
    model_tab, unmapped = engine.recode(dirty_tab, fitted["luts"], fitted["n_codes_out"])
    for j in fitted.get("categorical", ()):
        model_tab.set_column_kind(int(j), True)
    for j, v in (fitted.get("values") or {}).items():
        if len(v):
            model_tab.set_column_values(int(j), v)
    t_recode = time.perf_counter() - t0
    chain = [int(t) for t in fitted["chain"]]
    t0 = time.perf_counter()
    models = [engine.load_model(fitted["blobs"][t]) for t in chain]
    t_load = time.perf_counter() - t0
    t0 = time.perf_counter()
    y_values = {int(t): np.asarray(v, np.float64) for t, v in (fitted.get("y_values") or {}).items()}
    labels, probs, values = chained_repair(engine, model_tab, models, chain, [list(fitted["feats"][t]) for t in chain], 0, model_tab.n, y_values,
                                           set(int(t) for t in fitted.get("integral", ())))
    res = dict(labels=labels, probs=probs, values=values if y_values else None, models={}, stats=[],
               times=dict(train=0.0, exchange=t_load, infer=time.perf_counter() - t0, gather=0.0, recode=t_recode))
    info = dict(unmapped={j: int(k) for j, k in enumerate(np.asarray(unmapped, np.int64)) if fitted["luts"][j] is not None},
                recode_seconds=t_recode)
    return model_tab, res, info


def _shape(engine, table, dirty_tab, pmf_tab, res, chain, rows, cols, current, dirty_rows, rule_steps, want_rule_steps, continuous, y_values,
           integral, want_pmf, top_k, threshold, pmf_costs):
    """Phase 6: flatten + join with the error cells (RepairMiscApi.scala:41-49, model.py:1398-1401).  Returns the per-cell entries of the
    result: repaired, repaired_value, prob, models, stats[, rule_steps][, the entries of `cell_pmfs`].

    pmf_costs  : (want_pmf) the probability modes of RepairModel.run(): a callable (target, ascending row positions of its error cells)
                 -> dict(cost [R + 1][K] float64 or None, cost_row [cells] int32 (-1 = no cost), cur_code [cells] int32 (the current
                 value's class, -1 = none), weight, renormalise) or None, handed to `Table.repair_pmf_weighted`; adds `top1_cost` and
                 `pmf_value`.  With it the pmf table is chained as the value-space `_repair` chains it (model.py): in target order, a
                 continuous target's prediction fills its NULL cells before the later targets are scored (`pmf_value` holds it),
                 discrete targets stay NULL."""
    tpos = np.full(table.c, -1, np.int64)
    tpos[chain] = np.arange(len(chain))
    pos = np.searchsorted(dirty_rows, rows)
    repaired = res["labels"][tpos[cols], pos].astype(np.int32)
    prob = res["probs"][tpos[cols], pos] if res["probs"] is not None else None
    repaired_value = res["values"][tpos[cols], pos] if res.get("values") is not None else np.full(len(rows), np.nan)
    out = dict(repaired=repaired, repaired_value=repaired_value, prob=prob, models=res["models"], stats=res["stats"])
    if want_rule_steps:
        out["rule_steps"] = [rule_step_summary(table, t, rule_steps[t], rows[cols == t], dirty_rows, dirty_tab, repaired[cols == t])
                             for t in chain if t in rule_steps]
    if want_pmf:
        out.update(cell_pmfs(engine, table, pmf_tab, chain, res["models"], rows, cols, current, dirty_rows, continuous, y_values, integral,
                             top_k, threshold, pmf_costs))
    return out


def repair_table(engine, table, targets, base_params, constraints=(), detect_nulls=True, error_cells=None,
                 want_pmf=False, top_k=32, threshold=0.0, want_stats=False, continuous=None, train_rows=None,
                 check_unseen=False, search_opts=None, only_noisy_targets=False, pmf_costs=None, domain_analysis=None, rules=None,
                 value_detectors=None, distinct_training_rows=None, rebalance=None, regex_cols=None, cells_resident=False, keep_fit=False,
                 fitted=None):
    """Detect, NULL out, split, train, repair, shape.  ``table`` is modified in place (error cells become NULL).  The phases, and where each
    parameter is described: `_detect_and_prune` (constraints, detect_nulls and error_cells as `detect_error_cells` takes them,
    only_noisy_targets, domain_analysis, value_detectors, regex_cols), `_null_and_merge` (rules['nearest']: `nearest_value_merges`),
    `_target_plan` (rules['fd'], only_noisy_targets), `_training_tables` (train_rows, rebalance, check_unseen, distinct_training_rows),
    `_train_and_repair` (search_opts), `_shape` (want_pmf, top_k, threshold, pmf_costs).

    cells_resident : phases 1 and 2 on the table's cell set (`_cells_on_set`): the same cells, codes and dirty rows, the error cells going up
                 at most once (the given ones) and coming down once.  A table without the set's methods, or a job on several ranks, takes
                 the host route and the log says why.  The result then holds `cells_route`: 'set' or 'host'.

    keep_fit   : the result also holds `fit`: dict(chain, y_values, integral) -- with `models`, what an apply run needs of this one.
    fitted     : apply a kept fit (`_apply_fitted` describes the dict) instead of training: phases 1 and 2 are unchanged but look at the fitted
                 targets only; the error cells of the other targets are counted (`fitted`: dict(unmapped, unfitted_cells, recode_seconds) of
                 the result), not NULLed and not repaired.  The chain is the fitted one, whatever targets hold error cells.

    continuous : {column: (ascending distinct values, is_integral)} -- CONTINUOUS target attributes (byte/short/int/long/float/
                 double in the reference, RepairBase.scala:41-44): repaired by an L2 regressor on the values behind their codes
                 (train.py:97-100), integral ones rounded (model.py:1130-1132); `repaired_value` carries the prediction.
    rules      : the rule-based repairs of `RepairModel.setRepairByRules`, None = none of them: dict(fd={target: source column},
                 nearest=None or the dict of `nearest_value_merges`).  Merged cells leave the error cells (`merged` holds them).
    want_stats : with `distinct_training_rows`, the stats of a target trained on the distinct table describe that fit (its M rows).
    Returns dict(rows, cols, current, repaired, repaired_value, prob[, pmf_class, pmf_prob, current_prob[, top1_cost, pmf_value]],
    dirty_rows, models, times, stats[, domain][, rule_steps, merged][, value_detectors][, distinct_rows][, rebalanced]): one entry per error cell,
    ordered by (column, row).
    """
    continuous = dict(continuous or {})
    tg = [int(t) for t in targets]
    nearest = rules.get("nearest") if rules is not None else None
    unfitted = {}
    if fitted is not None:
        if rules is not None or want_pmf:
            raise ValueError("a kept fit is applied without rule steps and without the probability modes")
        in_fit = set(int(t) for t in fitted["chain"])
        others = [t for t in tg if t not in in_fit]
        tg = [t for t in tg if t in in_fit]
        if callable(value_detectors):
            value_detectors = value_detectors(table)
        if others:                                         # counted before anything is NULLed; they stay as they are
            _, ocols = detect_error_cells(table, others, constraints, detect_nulls, error_cells, value_detectors=value_detectors)
            unfitted = {int(c): int(k) for c, k in zip(*np.unique(ocols, return_counts=True))}
        only_noisy_targets = False                         # (no class of a kept model is counted on this table)
    route = None
    if cells_resident:
        why = set_route_refusal(table, tg)
        route = "host" if why else "set"
        if why:
            _logger.info("[Error Detection Phase] the cell set's route is not taken (%s): the cells are merged on the host" % why)
    if route == "set":
        t_null = time.perf_counter()
        det_rows, det_cols, run_targets, domain_info, detectors, t_detect, rows, cols, current, merged, dirty_rows = _cells_on_set(
            engine, table, tg, constraints, detect_nulls, error_cells, only_noisy_targets, domain_analysis, value_detectors, regex_cols, nearest)
        t_null += t_detect                                 # `prepare` starts where detection ends, as on the host route
    else:
        det_rows, det_cols, run_targets, domain_info, detectors, t_detect = _detect_and_prune(
            table, tg, constraints, detect_nulls, error_cells, only_noisy_targets, domain_analysis, value_detectors, regex_cols)
        t_null = time.perf_counter()
        rows, cols, current, merged, dirty_rows = _null_and_merge(engine, table, run_targets, det_rows, det_cols, nearest)
    out = dict(rows=rows, cols=cols, current=current, dirty_rows=dirty_rows, models={}, stats=[])
    if route is not None:
        out["cells_route"] = route
    if rules is not None:
        out.update(rule_steps=[], merged=merged)
    if domain_info is not None:
        out["domain"] = domain_info
    if detectors:
        out["value_detectors"] = _detector_report(detectors)
    if fitted is not None:
        out["fitted"] = dict(unmapped={}, unfitted_cells=unfitted, recode_seconds=0.0)
    if len(rows) == 0:
        out.update(repaired=np.zeros(0, np.int32), repaired_value=np.zeros(0, np.float64), prob=np.zeros(0, np.float64),
                   times=dict(detect=t_detect, prepare=time.perf_counter() - t_null))
        return out
    dirty_tab = table.gather_rows(dirty_rows)
    if fitted is not None:
        t_prep = time.perf_counter() - t_null
        model_tab, res, finfo = _apply_fitted(engine, dirty_tab, fitted)
        out["fitted"].update(finfo)
        chain = [int(t) for t in fitted["chain"]]
        t_shape = time.perf_counter()
        out.update(_shape(engine, table, model_tab, None, res, chain, rows, cols, current, dirty_rows, {}, False, continuous,
                          fitted.get("y_values") or {}, fitted.get("integral", ()), False, top_k, threshold, None))
        out["times"] = dict(res["times"], detect=t_detect, prepare=t_prep, shape=time.perf_counter() - t_shape)
        return out
    pmf_tab = table.gather_rows(dirty_rows) if want_pmf else None      # stays un-repaired: pmf mode does not chain
    label_counts, rule_steps, chain = _target_plan(table, run_targets, continuous, rules, only_noisy_targets,
                                                   dict(rows=det_rows, cols=det_cols, domain_info=domain_info, value_detectors=out.get("value_detectors")))
    t_prep = time.perf_counter() - t_null
    y_values = {t: np.asarray(continuous[t][0], np.float64) for t in chain if t in continuous}
    integral = {t for t in chain if t in continuous and continuous[t][1]}
    train_tables, train_counts, rebalanced, distinct_tab, distinct_info = _training_tables(
        engine, table, dirty_tab, [t for t in chain if t not in rule_steps], continuous, label_counts, base_params, train_rows, rebalance,
        check_unseen, distinct_training_rows, search_opts)
    if rebalanced is not None:
        out["rebalanced"] = rebalanced
    if distinct_info is not None:
        out["distinct_rows"] = distinct_info
    res = _train_and_repair(engine, table, dirty_tab, chain, train_counts, base_params, want_stats, y_values, integral, train_tables,
                            search_opts, rule_steps, distinct_tab, distinct_info)
    t_shape = time.perf_counter()
    out.update(_shape(engine, table, dirty_tab, pmf_tab, res, chain, rows, cols, current, dirty_rows, rule_steps, rules is not None,
                      continuous, y_values, integral, want_pmf, top_k, threshold, pmf_costs))
    out["times"] = dict(res["times"], detect=t_detect, prepare=t_prep, shape=time.perf_counter() - t_shape)
    if keep_fit:
        out["fit"] = dict(chain=list(chain), y_values=y_values, integral=sorted(integral), rule_targets=sorted(rule_steps))
    return out


def encode_frame(df, columns):
    """Dictionary encoding of the listed columns: (indices [C][n] int32 with -1 = NULL, remaps, dictionaries).

    `remaps[c][i]` is the code of dictionary entry i: its rank among the column's distinct values in ascending order
    (strings by code point, numbers numerically) -- the contract of repair.encode, so codes mean the same on both paths;
    `repair.frame_encoding.FrameEncoding` states it and holds the three while `repair_frame` edits them."""
    enc = FrameEncoding.of_frame(df, columns)
    return enc.indices, enc.remaps, enc.dicts


def _cell_positions(enc, df, row_id, error_cells):
    """An error-cell frame (`row_id`, `attribute`) -> (row positions, column positions); cells of unknown rows / attributes drop out
    (join semantics)."""
    import pandas as pd
    if row_id not in error_cells.columns or "attribute" not in error_cells.columns:
        raise ValueError("Error cells should have `%s` and `attribute` in columns" % row_id)
    rpos = pd.Series(np.arange(len(df)), index=df[row_id].to_numpy()).reindex(error_cells[row_id].to_numpy()).to_numpy(np.float64)
    cpos = np.array([enc.pos.get(a, -1) for a in error_cells["attribute"]], np.int64)
    ok = ~np.isnan(rpos) & (cpos >= 0)
    return rpos[ok].astype(np.int64), cpos[ok].astype(np.int32)


def _known_cells(engine, enc, target_cols, kr, kc, regex_rules):
    """The error cells (kr, kc) are known before the table is (re)built: regex-structure repair of those it applies to (the DISTINCT
    current-value strings of each rule's cells go through `engine.regex_structure`; the first rule that repairs a cell wins), every cell of
    a target column NULLed in the encoding and the classes only they held dropped (the reference NULLs every error cell and then writes the
    rule repairs, model.py `_repair_attrs`), the repaired values written back.  Returns (the repaired cells: dict(rows, cols, current,
    repaired: strings), the remaining cells (rows, cols))."""
    from repair.regex_structure import repair_cells
    done = np.zeros(len(kr), bool)
    cur_s, rep_s = np.empty(len(kr), object), np.empty(len(kr), object)
    for r in regex_rules:
        j = enc.pos.get(r["attr"])
        sel = np.flatnonzero((kc == j) & ~done) if j is not None and j in target_cols else np.zeros(0, np.int64)
        if not len(sel):
            continue
        raw = list(r["current"](enc.columns[j], kr[sel])) if r.get("current") is not None else list(enc.values(kr[sel], j))
        strs = r["current_str"](enc.columns[j], raw)
        values, skipped = repair_cells(r["program"], strs, engine.regex_structure)
        if skipped:
            _logger.info("[Repairing Phase] %d cells of `%s` hold a line terminator: left to the models" % (skipped, enc.columns[j]))
        for i, sv, v in zip(sel, strs, values):
            if v is not None:
                done[i], cur_s[i], rep_s[i] = True, sv, v
    in_targets = np.isin(kc, target_cols)
    enc.null_cells(kr[in_targets], kc[in_targets], prune=target_cols)
    for j in np.unique(kc[done]):
        at = np.flatnonzero(done & (kc == j))
        enc.write(j, kr[at], rep_s[at])
    return dict(rows=kr[done], cols=kc[done], current=cur_s[done], repaired=rep_s[done]), (kr[~done], kc[~done])


def _nearest_current(enc, nv, t, rows, codes):
    """The current-value strings of cells of column t for the nearest-value rule `nv`: the caller's where it holds them already."""
    if nv.get("current") is not None:
        return nv["current"](enc.columns[t], rows)
    return nv["current_str"](enc.columns[t], list(enc.current_values(rows, np.full(len(rows), t, np.int32), codes)))


def _column_space(engine, enc, df, targets, constraints, detect_nulls, analyse, keep_weak, continuous_columns=(), train_rows=None,
                  check_unseen=False, pmf_costs=None, domain_analysis=None, rules=None, value_detectors=None, rebalance=None):
    """The arguments of `repair_frame` that speak of attributes by NAME as `repair_table` takes them, by column position and code, against the
    dictionaries the table was just built from: constraints, continuous, train_rows, check_unseen, pmf_costs, domain_analysis, rules,
    value_detectors (`analyse`: not on a second pass, which detects nothing) and rebalance.  Returns them as keywords."""
    import pandas as pd
    cols, pos, dicts = enc.columns, enc.pos, enc.dicts
    dtypes = {c: df[c].dtype for c in cols}
    da_spec = None
    if domain_analysis is not None and analyse:
        ccols = domain_analysis.get("continuous_columns")
        if ccols is None:
            ccols = [c for j, c in enumerate(cols) if dicts[j].dtype != object]
        da_spec = dict(options=domain_analysis.get("options") or {}, discrete_thres=domain_analysis["discrete_thres"],
                       domain_stats=[len(d) for d in dicts], keep_weak=keep_weak,
                       continuous={pos[c]: np.asarray(dicts[pos[c]], np.float64) for c in ccols if c in pos and dicts[pos[c]].dtype != object})
    cons = []
    for con in constraints:
        if isinstance(con, tuple):
            cons.append(([pos[x] for x in con[0]], pos[con[1]]))
        else:                                  # a parsed constraint: lowered against the dictionaries the table is built from
            from repair.dc_codes import NotLowerable, lower_constraint
            try:
                cons.append(lower_constraint(con, cols, dicts, dtypes))
            except NotLowerable as e:
                raise NotResidentEligible("denial constraint %s: %s" % (con, e))
    cont = {pos[c]: (np.asarray(dicts[pos[c]], np.float64), pd.api.types.is_integer_dtype(df[c])) for c in continuous_columns
            if c in pos and c in targets}
    table_rules = None
    if rules is not None:
        table_rules = dict(fd={pos[y]: pos[x] for y, x in dict(rules.get("fd") or {}).items()}, nearest=None)
        nv = rules.get("nearest")
        if nv is not None:
            table_rules["nearest"] = dict(targets=[pos[a] for a in nv["targets"] if a in pos], threshold=nv["threshold"], cost=nv.get("cost"),
                                          current=lambda t, rows, codes: _nearest_current(enc, nv, t, rows, codes),
                                          domain=lambda t, live: nv["domain_str"](cols[t], list(dicts[t][live])))
    detectors = None
    if analyse and value_detectors and value_detectors.get("detectors"):
        build = value_detectors.get("build")
        if build is None:
            from repair.detect_codes import build_descriptors as build
        dets = list(value_detectors["detectors"])
        # the LOF kind evaluates the filled column: it needs the NULL count (rows minus the counted ones) and the engine's `lof_codes`
        extra = dict(lof=getattr(engine, "lof_codes", None), n_rows=len(df)) if any(d["kind"] == "lof" for d in dets) else {}

        def detectors(table):
            return build(dets, cols, dicts, dtypes, lambda j: table.count_codes(j)[0], list(targets), null_all=bool(detect_nulls), **extra)
    numeric = [pos[c] for c in cols if pd.api.types.is_numeric_dtype(df[c]) and not pd.api.types.is_bool_dtype(df[c])]
    return dict(constraints=cons, detect_nulls=detect_nulls, continuous=cont, domain_analysis=da_spec, rules=table_rules, value_detectors=detectors,
                pmf_costs=(lambda t, r: pmf_costs(cols[t], dicts[t], r)) if pmf_costs is not None else None,
                rebalance=dict(rebalance, names=lambda t: cols[t], class_names=lambda t: dicts[t]) if rebalance is not None else None,
                check_unseen=(numeric or True) if check_unseen else False,
                train_rows=(lambda t, r: train_rows(cols[t], r)) if callable(train_rows) else train_rows)


def _upload(engine, enc):
    """The table of the encoding, with the column kinds and values the trainer bins by."""
    table = engine.upload_dictionaries(enc.indices, enc.remaps)
    for j, d in enumerate(enc.dicts):              # numeric columns: bin bounds at the midpoints of the values, like LightGBM on raw numbers
        if d.dtype != object and len(d) > 0:
            table.set_column_values(j, d)
        elif d.dtype == object:
            table.set_column_kind(j, True)         # categories a model's training rows do not show are missing for that model
    return table


def route_order_constraints(constraints, table):
    """The lowered constraints with every `kind="dc"` program that is an order constraint (`repair.dc_codes.scan_eligible`) marked
    `kind="dc_scan"`: `detect_error_cells` sends those to `Table.detect_dc_scan`.  A table without that method keeps the pairs route."""
    from repair.dc_codes import scan_eligible
    if not hasattr(table, "detect_dc_scan"):
        return list(constraints)
    return [dict(con, kind="dc_scan") if isinstance(con, dict) and con["kind"] == "dc" and scan_eligible(con["preds"]) else con
            for con in constraints]


def constraint_routes(constraints):
    """Per lowered constraint the entry that answers it: 'fd' (`Table.detect_constraint`), 'dc' (pairs), 'dc_scan' or 'row_bits'."""
    return [con["kind"] if isinstance(con, dict) else "fd" for con in constraints]


def _fitted_column_space(fitted, enc):
    """A kept fit (`repair.fitted.FittedRepairModels`) against the encoding of a later frame, as `repair_table(fitted=..)` takes it: the
    LUTs of `repair.fitted.fitted_luts`, and the chain, features, dictionaries, kinds and values by the FRAME's column positions."""
    from repair.fitted import fitted_luts
    luts = fitted_luts(fitted, enc)
    pos = enc.pos
    fdict = {c: fitted.dicts[j] for j, c in enumerate(fitted.columns)}
    n_codes_out = [max(len(enc.dicts[j]), 1) if luts[j] is None else max(len(fdict[c]), 1) for j, c in enumerate(enc.columns)]
    tg = fitted.targets
    return dict(chain=[pos[t] for t in fitted.chain], feats={pos[t]: [pos[f] for f in tg[t]["features"]] for t in fitted.chain},
                blobs={pos[t]: tg[t]["blob"] for t in fitted.chain},
                y_values={pos[t]: np.asarray(tg[t]["y_values"], np.float64) for t in fitted.chain if tg[t]["continuous"]},
                integral={pos[t] for t in fitted.chain if tg[t]["continuous"] and tg[t]["integral"]},
                luts=luts, n_codes_out=n_codes_out,
                categorical=[pos[c] for j, c in enumerate(fitted.columns) if fitted.categorical[j]],
                values={pos[c]: np.asarray(fitted.dicts[j], np.float64) for j, c in enumerate(fitted.columns) if not fitted.categorical[j]})


def _upload_and_run(engine, enc, df, targets, cells, regex_rules, by_name, through, analyse=True, order_scan=False, fitted=None):
    """One pass: upload the encoding, `repair_table` on it.  `cells`: the known error cells or None; `by_name` / `through`: the keywords of
    `_column_space` / those `repair_table` takes as they are; `order_scan`: `route_order_constraints` on the lowered constraints.
    Returns (the continuous targets {column: (values, is_integral)}, result); the result (or the DeadClasses raised) holds
    `constraint_routes`."""
    table = _upload(engine, enc)
    kw = _column_space(engine, enc, df, targets, analyse=analyse, **by_name)
    if order_scan:
        kw["constraints"] = route_order_constraints(kw["constraints"], table)
    routes = constraint_routes(kw["constraints"])
    regex_cols = [enc.pos[r["attr"]] for r in regex_rules if r["attr"] in enc.pos] if cells is None else None
    if fitted is not None:                                 # (the keyword reaches `repair_table` only when a fit is applied)
        through = dict(through, fitted=_fitted_column_space(fitted, enc))
    try:
        res = repair_table(engine, table, [enc.pos[t] for t in targets], error_cells=cells, regex_cols=regex_cols, **through, **kw)
    except DeadClasses as e:
        e.constraint_routes = routes
        raise
    res["constraint_routes"] = routes
    return kw["continuous"], res


def _result_frame(enc, df, row_id, res, cont, want_pmf, with_costs, label_dicts=None):
    """(row_id, attribute, current_value, repaired[, prob][, pmf, current_prob[, top1_cost, pmf_value]]) of the repaired cells.
    `label_dicts`: the dictionaries behind the labels where they are not the encoding's (an applied fit: the FITTED ones, by column)."""
    import pandas as pd
    rows, ccols = res["rows"], res["cols"]
    repaired = (enc if label_dicts is None else FrameEncoding(enc.columns, enc.indices, enc.remaps, label_dicts)).decode(res["repaired"], ccols)
    for j, (_, is_int) in cont.items():                       # continuous attributes: the regressor's value, not a dictionary entry
        sel = ccols == j
        v = res["repaired_value"][sel]
        repaired[sel] = [int(x) for x in v] if is_int else [float(x) for x in v]
    frame = pd.DataFrame({row_id: df[row_id].to_numpy()[rows], "attribute": np.asarray(enc.columns, object)[ccols],
                          "current_value": enc.current_values(rows, ccols, res["current"]), "repaired": repaired})
    if res.get("prob") is not None:
        frame["prob"] = res["prob"]
    if want_pmf and len(rows):
        pc, pp = res["pmf_class"], res["pmf_prob"]
        frame["pmf"] = [[{"class": enc.dicts[ccols[i]][k], "prob": float(p)} for k, p in zip(pc[i], pp[i]) if k >= 0] for i in range(len(rows))]
        frame["current_prob"] = res["current_prob"]
        if with_costs:
            frame["top1_cost"] = res["top1_cost"]
            pval = np.empty(len(rows), object)
            pval[:] = None
            for j, (_, is_int) in cont.items():
                sel = np.flatnonzero(ccols == j)
                v = res["pmf_value"][sel]
                pval[sel] = [None if np.isnan(x) else (int(x) if is_int else float(x)) for x in v]
            frame["pmf_value"] = pval
    return frame


def _cell_frame(enc, df, row_id, rows, cols, current, repaired):
    import pandas as pd
    return pd.DataFrame({row_id: df[row_id].to_numpy()[rows], "attribute": np.asarray(enc.columns, object)[cols],
                         "current_value": np.asarray(current, object), "repaired": np.asarray(repaired, object)})


def _details(enc, df, row_id, res, rules, regex_done):
    """`repair_table`'s report with attribute names for column positions; `regex_done`: the cells of `_known_cells`, or None."""
    cols = enc.columns
    details = dict(times=res.get("times", {}), stats=res.get("stats", []), models=res.get("models", {}), columns=cols)
    if any(r != "fd" for r in res.get("constraint_routes") or ()):      # (runs with `X -> Y` constraints alone report what they always did)
        details["constraint_routes"] = list(res["constraint_routes"])
    if res.get("domain") is not None:
        d = res["domain"]
        details.update(pairwise_attr_stats={cols[t]: [(cols[y], h) for y, h in lst] for t, lst in d["pairwise"].items()},
                       noisy_cells=d["noisy_cells"], weak_cells=d["weak_cells"])
    if res.get("cells_route") is not None:
        details["cells_route"] = res["cells_route"]
    if res.get("value_detectors"):
        details["value_detectors"] = [dict(attribute=cols[d["col"]], kinds=d["kinds"], codes_flagged=d["codes_flagged"], cells=d["cells"])
                                      for d in res["value_detectors"]]
    if res.get("rebalanced") is not None:
        details["rebalanced"] = {cols[t]: d for t, d in res["rebalanced"].items()}
    if res.get("distinct_rows") is not None:
        d = res["distinct_rows"]
        details["distinct_rows"] = dict(rows=d["rows"], distinct=d["distinct"], used_for=[cols[t] for t in d["used_for"]],
                                        skipped={cols[t]: why for t, why in d["skipped"].items()})
    if rules is not None:
        details["rule_steps"] = [dict(st, target=cols[st["target"]], x=cols[st["x"]] if st["x"] >= 0 else None) for st in res.get("rule_steps", [])]
        mg = res.get("merged")
        mcur, mrep, mrows, mcols = [], [], np.zeros(0, np.int64), np.zeros(0, np.int32)
        if mg is not None and len(mg["rows"]):
            nv = rules["nearest"]
            mrows, mcols = mg["rows"], mg["cols"]
            raw_rep = enc.decode(mg["repaired"], mcols)
            mcur, mrep = np.empty(len(mrows), object), np.empty(len(mrows), object)
            for j in np.unique(mcols):
                sel = np.flatnonzero(mcols == j)
                mcur[sel] = _nearest_current(enc, nv, j, mrows[sel], mg["current"][sel])
                mrep[sel] = nv["domain_str"](cols[j], list(raw_rep[sel]))
        details["merged_cells"] = _cell_frame(enc, df, row_id, mrows, mcols, mcur, mrep)
        details["nearest_values"] = {cols[j]: int((mcols == j).sum()) for j in np.unique(mcols)}
        if regex_done is not None:
            details["regex_cells"] = _cell_frame(enc, df, row_id, regex_done["rows"], regex_done["cols"], regex_done["current"], regex_done["repaired"])
            details["regex_repairs"] = {cols[j]: int((regex_done["cols"] == j).sum()) for j in np.unique(regex_done["cols"])}
    return details


def _fit_pieces(enc, res, cont):
    """What `repair_frame(keep_fit=True)` adds to its details: `fit` (the pieces of `repair.fitted.FittedRepairModels.from_pieces`, from the
    encoding of the FINAL pass and that pass's result) or `fit_refusal` (why there is none)."""
    from repair import dist
    fit = res.get("fit")
    if fit is None:
        return dict(fit_refusal="the run trained nothing (it found no error cell)")
    if fit["rule_targets"]:
        return dict(fit_refusal="the run used rule steps (%s): a rule is a map of the fitted table, not a model"
                    % ", ".join("`%s`" % enc.columns[t] for t in fit["rule_targets"]))
    if dist.world()[1] > 1:
        return dict(fit_refusal="the run was a job on %d ranks" % dist.world()[1])
    cols = enc.columns
    targets = {}
    for t in fit["chain"]:
        targets[cols[t]] = dict(blob=bytes(res["models"][t]), features=[cols[c] for c in range(len(cols)) if c != t], continuous=t in cont,
                                integral=bool(t in cont and cont[t][1]),
                                y_values=np.asarray(fit["y_values"][t], np.float64) if t in fit["y_values"] else None)
    return dict(fit=dict(columns=list(cols), dicts=[np.array(d, copy=True) for d in enc.dicts], categorical=[d.dtype == object for d in enc.dicts],
                         chain=[cols[t] for t in fit["chain"]], targets=targets))


def repair_frame(engine, df, row_id, targets=None, constraints=(), base_params=None, want_pmf=False, top_k=32, threshold=0.0,
                 error_cells=None, detect_nulls=True, continuous_columns=(), train_rows=None, want_details=False,
                 check_unseen=False, search_opts=None, only_noisy_targets=False, pmf_costs=None, domain_analysis=None, rules=None,
                 value_detectors=None, distinct_training_rows=None, rebalance=None, order_scan=False, cells_resident=False, keep_fit=False,
                 fitted=None):
    """DataFrame in, the reference's result frame out: (row_id, attribute, current_value, repaired, prob[, pmf]) -- the
    shape of `RepairModel.run()` / `run(compute_repair_candidate_prob=True)` (python/repair/model.py:1398-1419).

    Columns are discrete (one class per distinct value) unless named in `continuous_columns` (numeric columns; those targets
    get regressors and `repaired` is the predicted number, rounded for integer columns); `constraints` are `X1,..,Xm -> Y`
    dependencies given as the tuple ([x names], y name), or any other parsed constraint as its list of `repair.errors.Predicate`
    (`repair.dc_codes.lower_constraint` turns it into a program on the codes; `order_scan`: the order constraints among those programs
    -- `repair.dc_codes.scan_eligible` -- go to `Table.detect_dc_scan` where the engine's table has it; whenever one of the constraints is such
    a program the details name each constraint's entry as `constraint_routes`: 'fd', 'dc', 'dc_scan' or 'row_bits', in the order given); `error_cells` is a frame with `row_id` and `attribute` columns
    (RepairModel.setErrorCells).  Regex / value-domain / outlier / LOF detectors come as `value_detectors`; any other scikit-learn
    backed detector stays with `repair.model.RepairModel` (the value-space API).

    value_detectors: dict(detectors=[dict(kind='regex', attr, regex) | dict(kind='domain', attr, values, autofill, min_count_thres) |
    dict(kind='outlier', attrs) | dict(kind='lof', attrs, k)][, build=callable(detectors, columns, dicts, dtypes, counts, targets, null_all[, lof,
    n_rows: with a 'lof' kind]) -> descriptors]) -- the
    detectors by attribute name and what turns them into per-column code predicates (default `repair.detect_codes.build_descriptors`).
    The descriptors are built after the upload, so `counts(j)` (rows per code of column j: autofill, quartiles) comes from the table;
    one `Table.detect_cells` call then finds their cells and the NULL cells.  The details hold `value_detectors`: per descriptor the
    attribute, the kinds merged, the codes flagged and the cells found.

    pmf_costs (with want_pmf): the update costs of RepairModel.run()'s probability modes, a callable (attribute, its classes (the
    target's dictionary, ascending), ascending row positions of its error cells) -> the dict `repair_table` describes, or None.  The
    frame then also holds `top1_cost` (cost of the top-1 class against the current value) and `pmf_value` (continuous targets: the
    prediction of the un-repaired pmf chain).

    domain_analysis: dict(options={error.*: checked value}, discrete_thres[, continuous_columns]) -- the cell-domain analysis and the
    weak-label pruning of the detected cells (`repair_table`); the details then hold `pairwise_attr_stats` {attribute: [(attribute, H)]},
    `noisy_cells` and `weak_cells`.

    rules: the rule-based repairs by attribute NAME (`repair_table` has the column form): dict(fd={target: source},
    nearest=None or dict(targets=[attributes], threshold, cost=None (Levenshtein) or callable, current_str=callable(attribute, raw
    values) -> strings, domain_str=callable(attribute, dictionary values) -> strings[, current=callable(attribute, row positions) ->
    strings: the error cells' current values where the caller holds them already])).  The frame then lacks the merged cells; the details
    hold them as `merged_cells` (row_id, attribute, current_value, repaired: strings), their number per attribute as `nearest_values`,
    and `rule_steps` (`rule_step_summary` with attribute names).
    rules['regex']: None or [dict(attr, program (`repair.regex_structure.parse`), current_str=callable(attribute, raw values) -> strings[,
    current=callable(attribute, row positions) -> the cells' current values where the caller holds them])] in detector order -- regex-structure
    repair (`_repair_by_regexs`).  Once the error cells are known (given, or detected on the device and handed back: the route of
    DeadClasses), the DISTINCT current-value strings of each attribute's cells go through `engine.regex_structure`; a repaired cell gets
    its new value in the dictionary indices (a string the column did not hold becomes a dictionary entry, the codes stay the ascending
    ranks), the others are NULLed as given cells, and the table is built once.  The frame lacks the repaired cells; the details hold them
    as `regex_cells` (a frame like `merged_cells`) and their number per attribute as `regex_repairs`.

    distinct_training_rows: None or dict(max_ratio=float), as `repair_table` takes it; the details then hold `distinct_rows` with attribute
    names: dict(rows, distinct, used_for=[attributes], skipped={attribute: reason}).

    cells_resident: as `repair_table` takes it, in both passes; the details then hold `cells_route` ('set' or 'host'; the second pass's when
    there is one: its cells are the given ones).

    keep_fit: the details hold `fit`, the pieces of `repair.fitted.FittedRepairModels.from_pieces` -- the column names, the dictionaries the
    FINAL pass uploaded (after the pruning of known cells and after a DeadClasses second pass), the kinds as `_upload` decides them, the chain
    and per chain target its blob, features, continuous / integral flags and y_values -- or `fit_refusal`, the reason there is none (rule
    steps, a multi-rank job, nothing trained).
    fitted: a `repair.fitted.FittedRepairModels`: nothing is trained.  Detection, the NULL-out, the cell-set route, the dirty rows
    and the frame's shape are as ever; between them `_apply_fitted` translates the dirty rows into the fit's code space on the device and
    runs the kept chain.  `repaired` is decoded with the FITTED dictionaries.  Error cells of a target without a kept model stay as they are
    and are counted: the details hold `fitted`: dict(unmapped {attribute: cells}, unfitted_cells {attribute: cells}, recode_seconds), and
    one warning names them.  Rules, the probability modes, a hyper-parameter search and the training options do not apply (ValueError for
    the first two; `base_params`, `train_rows`, `rebalance`, `distinct_training_rows` are not read).

    rebalance: None or dict(k=5, random_state=42), as `repair_table` takes it.  A column whose dictionary is not in the order of its sorted
    values (mixed types) raises NotResidentEligible; the details hold `rebalanced` {attribute: dict(median, rows, synthetic, classes)}."""
    cols = [c for c in df.columns if c != row_id]
    targets = list(targets) if targets is not None else list(cols)
    unknown = [t for t in targets if t not in cols]
    if unknown:
        raise ValueError("Target attributes not found in the input: %s" % ",".join(unknown))
    if fitted is not None:
        if rules is not None or want_pmf:
            raise ValueError("a kept fit is applied without rule steps and without the probability modes")
        missing = [c for c in fitted.columns if c not in cols]
        if missing:
            raise ValueError("the fitted column `%s` is not in the frame" % missing[0])
        train_rows = rebalance = distinct_training_rows = search_opts = None
        check_unseen = keep_fit = False
    enc = FrameEncoding.of_frame(df, cols)
    if rebalance is not None:
        from repair.rebalance_codes import check_dictionary_order
        for j, c in enumerate(cols):
            check_dictionary_order(enc.dicts[j], "`%s`" % c)
    target_cols = sorted(enc.pos[t] for t in targets if fitted is None or t in fitted.targets)     # (applying a fit: the cells of the others stay)
    regex_rules = list((rules or {}).get("regex") or [])
    by_name = dict(continuous_columns=continuous_columns, train_rows=train_rows, check_unseen=check_unseen, pmf_costs=pmf_costs,
                   domain_analysis=domain_analysis, rules=rules, value_detectors=value_detectors, rebalance=rebalance,
                   keep_weak=error_cells is not None)
    through = dict(base_params=dict(base_params or {}), want_pmf=want_pmf, top_k=top_k, threshold=threshold, search_opts=search_opts,
                   only_noisy_targets=only_noisy_targets, distinct_training_rows=distinct_training_rows)
    if cells_resident:                                     # (`repair_table` sees the keyword only when it is set)
        through["cells_resident"] = True
    if keep_fit:
        through["keep_fit"] = True
    cells = None
    regex_done = [dict(rows=np.zeros(0, np.int64), cols=np.zeros(0, np.int32), current=np.zeros(0, object), repaired=np.zeros(0, object))]
    if error_cells is not None:
        done, cells = _known_cells(engine, enc, target_cols, *_cell_positions(enc, df, row_id, error_cells), regex_rules)
        regex_done.append(done)
    if error_cells is not None and not detect_nulls and not constraints and rules is None and fitted is None:
        # every error cell is known and NULLed: the class counts the models will see are final.  Say so BEFORE anything is uploaded
        # (a constraint / regex / user-given cell may hold the only occurrence of a class; an all-NULL numeric column has no value)
        for t in targets:
            live = enc.live_classes(enc.pos[t])
            if live < (1 if t in continuous_columns else 2):
                raise NotResidentEligible("target `%s` is left with %d distinct value(s) once the error cells are removed" % (t, live))
    try:
        cont, res = _upload_and_run(engine, enc, df, targets, cells, regex_rules, dict(by_name, constraints=constraints, detect_nulls=detect_nulls),
                                    through, order_scan=order_scan, fitted=fitted)
    except DeadClasses as e:
        # Detection ran on the device; some values of a target were held by error cells only (a typo occurs once).  The cells are
        # known now: NULL them on the host side of the encoding, drop the dead values, upload the (cached) encoding again and go on
        # with the cells as GIVEN -- no second detection, no pandas detectors, no value-space fallback.  Cells of a user-given
        # error_cells frame were NULLed before the first attempt: what they held is what the encoding recorded then.
        _logger.info("%s: re-encoding the target dictionaries without them" % e)
        done, second = _known_cells(engine, enc, target_cols, e.rows, e.cols, regex_rules)
        regex_done.append(done)
        cont, res = _upload_and_run(engine, enc, df, targets, second, regex_rules, dict(by_name, constraints=(), detect_nulls=False), through,
                                    analyse=False)
        if e.domain_info is not None:
            res["domain"] = e.domain_info
        if e.value_detectors:
            res["value_detectors"] = e.value_detectors
        res["constraint_routes"] = e.constraint_routes
    label_dicts = None
    if fitted is not None:
        fdict = {c: fitted.dicts[j] for j, c in enumerate(fitted.columns)}
        label_dicts = [fdict.get(c, enc.dicts[j]) for j, c in enumerate(enc.columns)]
        cont = {enc.pos[t]: (np.asarray(fitted.targets[t]["y_values"], np.float64), bool(fitted.targets[t]["integral"]))
                for t in fitted.chain if fitted.targets[t]["continuous"]}
        left = {enc.columns[j]: k for j, k in sorted(res["fitted"]["unfitted_cells"].items())}
        if left:
            _logger.warning("[Repairing Phase] error cells in attributes without a kept model are left as they are: %s"
                            % ", ".join("`%s`: %d" % (a, k) for a, k in left.items()))
    frame = _result_frame(enc, df, row_id, res, cont, want_pmf, pmf_costs is not None, label_dicts=label_dicts)
    if not want_details:
        return frame
    regex_cells = {k: np.concatenate([d[k] for d in regex_done]) for k in regex_done[0]}
    details = _details(enc, df, row_id, res, rules, regex_cells if regex_rules else None)
    if fitted is not None:
        f = res["fitted"]
        details["fitted"] = dict(unmapped={enc.columns[j]: k for j, k in sorted(f["unmapped"].items())}, unfitted_cells=left,
                                 recode_seconds=f["recode_seconds"])
    if keep_fit:
        details.update(_fit_pieces(enc, res, cont))
    return frame, details


def _detect_only_frame(df, row_id, enc, rows, cols, codes):
    """[row_id, "attribute", "current_value"] of the cells, `current_value` = CAST(value AS STRING) decoded once per dictionary entry: the
    codes of a column that occur among its cells are formatted (`repair.errors._to_sql_string`; the float64 dictionary of an integral
    column prints integral) and gathered; NULL stays None."""
    import pandas as pd
    from repair.encode import is_integral_column
    from repair.errors import _to_sql_string
    cur = np.empty(len(rows), object)
    cur[:] = None
    for j in np.unique(cols):
        sel = np.flatnonzero((cols == j) & (codes >= 0))
        if not len(sel):
            continue
        used, inverse = np.unique(codes[sel], return_inverse=True)
        strs = np.empty(len(used), object)
        strs[:] = [_to_sql_string(v) for v in enc.dicts[j][used]]
        if is_integral_column(df[enc.columns[j]]):
            strs[:] = [str(int(float(v))) for v in strs]
        cur[sel] = strs[inverse]
    return pd.DataFrame({row_id: pd.Series(df[row_id].to_numpy()[rows], dtype=df[row_id].dtype),
                         "attribute": pd.Series(np.asarray(enc.columns, object)[cols], dtype=object),
                         "current_value": pd.Series(cur, dtype=object)})


def detect_frame(engine, df, row_id, targets=None, constraints=(), detect_nulls=True, value_detectors=None, domain_analysis=None,
                 order_scan=False, continuous_columns=(), want_details=False):
    """`RepairModel.run(detect_errors_only=True)` on the resident table: the frame [row_id, "attribute", "current_value"] of the error cells
    of ALL target attributes (ErrorModel.detect returns every cell, repairable or not), detected, merged and read on the device.

    The frame is encoded and uploaded once; `constraints`, `value_detectors` and `domain_analysis` are `repair_frame`'s, lowered against
    the dictionaries (`_column_space`; `order_scan`: `route_order_constraints`); `detect_error_cells(on_device=True)` leaves the union of
    the detectors' cells and the codes they hold in one emit of the table's cell set.  With `domain_analysis` the cell-domain analysis
    runs on those cells for the noisy discretizable targets (continuous, or 1 < |domain| <= discrete_thres; `continuous_columns` where
    the dict names none) and the weak-labelled cells are dropped on the host, as `repair_table`'s phase 1 does.

    Row order: attribute in frame column order, then row position.  (The value-space frame has the detectors' concatenation order; a
    caller that compares the two sorts both.)  No cell: the empty frame with the same columns and dtypes.  `want_details`: (frame,
    details) with `constraint_routes`, `value_detectors`, `pairwise_attr_stats` / `noisy_cells` / `weak_cells` as `repair_frame` gives
    them, and `times` (seconds: encode, upload, detect, domain, shape)."""
    cols = [c for c in df.columns if c != row_id]
    targets = list(targets) if targets is not None else list(cols)
    unknown = [t for t in targets if t not in cols]
    if unknown:
        raise ValueError("Target attributes not found in the input: %s" % ",".join(unknown))
    times = {}
    t0 = time.perf_counter()
    enc = FrameEncoding.of_frame(df, cols)
    times["encode"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    table = _upload(engine, enc)
    times["upload"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    if domain_analysis is not None and domain_analysis.get("continuous_columns") is None:
        domain_analysis = dict(domain_analysis, continuous_columns=list(continuous_columns))
    kw = _column_space(engine, enc, df, targets, constraints, detect_nulls, True, False, domain_analysis=domain_analysis,
                       value_detectors=value_detectors)
    cons = route_order_constraints(kw["constraints"], table) if order_scan else kw["constraints"]
    vdets = kw["value_detectors"](table) if callable(kw["value_detectors"]) else None
    target_cols = sorted(enc.pos[t] for t in targets)
    rows, ccols, codes = detect_error_cells(table, target_cols, cons, detect_nulls, None, value_detectors=vdets, on_device=True)
    times["detect"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    res = dict(constraint_routes=constraint_routes(cons), value_detectors=_detector_report(vdets))
    spec = kw["domain_analysis"]
    if spec is not None and len(rows):
        stats, cont = spec["domain_stats"], spec.get("continuous") or {}
        discretized = [j for j in range(len(cols)) if j in cont or 1 < stats[j] <= int(spec["discrete_thres"])]
        noisy = set(int(c) for c in np.unique(ccols))
        repairable = [j for j in discretized if j in noisy]
        if repairable and len(discretized) > 1:
            da = analyse_cell_domains(table, repairable, rows, ccols, spec)
            res["domain"] = dict(pairwise=da["pairwise"], noisy_cells=int(len(rows)), weak_cells=int(da["weak"].sum()))
            _logger.info("[Error Detection Phase] %d noisy cells fixed and %d error cells remaining..." % (res["domain"]["weak_cells"],
                                                                                                       len(rows) - res["domain"]["weak_cells"]))
            rows, ccols, codes = rows[~da["weak"]], ccols[~da["weak"]], codes[~da["weak"]]
    times["domain"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    frame = _detect_only_frame(df, row_id, enc, rows, ccols, codes)
    times["shape"] = time.perf_counter() - t0
    if not want_details:
        return frame
    res["times"] = times
    return frame, _details(enc, df, row_id, res, None, None)


def constraint_to_columns(preds, columns):
    """Parsed denial constraint (repair.errors.parse_constraint) -> (eq column indices, iq column index) when it has the form
    the device detector handles -- two tuples, same attribute on both sides, EQ predicates plus exactly one IQ -- else None
    (single-tuple constant predicates, LT/GT, several IQs stay with the pandas detector)."""
    pos = {c: i for i, c in enumerate(columns)}
    eq, iq = [], []
    for p in preds:
        if p.constant is not None or p.right is None or p.left != p.right or p.left not in pos:
            return None
        if p.op == "EQ":
            eq.append(pos[p.left])
        elif p.op == "IQ":
            iq.append(pos[p.left])
        else:
            return None
    if len(iq) != 1 or len(eq) > 12:
        return None
    return eq, iq[0]
