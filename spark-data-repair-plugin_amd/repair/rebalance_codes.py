"""Training-data rebalancing in code space: `repair.train.rebalance_training_data` -- SMOTEN for the classes below the
median class size, RandomUnderSampler for those above it -- restated on the int32 dictionary codes of the resident table.

SMOTEN treats every column as nominal, so it is a function of the codes alone: the Value Difference Metric between two rows is a sum
over the features of a quantity that depends only on the pair of codes.  `smoten_codes` is the numpy statement the device entry
(`Table.smoten`, csrc/rgbm_smoten.hip) is held to, integer for integer; `rebalance_plan` is the host part of the recipe: histogram,
median, targets, every random draw and the final row order.  The draws define the result and are O(n): they stay in numpy."""
import logging

import numpy as np

_logger = logging.getLogger(__name__)

K_NEIGHBORS = 5        # reference train.py:271-274


def check_dictionary_order(values, what="column"):
    """The codes of a column are the ranks of its values in the dictionary; `repair.train._ordinal_codes` ranks them with np.unique.  Both
    agree unless np.unique cannot compare the values (mixed types: it then orders them by their string form) -- the mode's tie rule
    (the smallest code) and the class order would differ.  A check on the dictionary, not on the rows."""
    from repair.pipeline import NotResidentEligible
    vals = values if isinstance(values, np.ndarray) else np.asarray(values, dtype=object)
    try:
        u = np.unique(vals)
    except TypeError:
        raise NotResidentEligible("rebalancing: the values of %s have mixed types; their order is the value-space path's to define" % what)
    if len(u) != len(vals) or any(a != b for a, b in zip(u.tolist(), np.asarray(vals).tolist())):
        raise NotResidentEligible("rebalancing: the dictionary of %s is not in the order of its sorted values" % what)


def vdm_tables(codes, n_codes, target_col, feat_cols, fit_rows):
    """P_f [V_f][K] = share of class c among the fit rows with code v in feature f (count / row sum, one float64 division); rows of
    codes that no fit row holds are 0.0 and never read."""
    codes = np.asarray(codes)
    fit_rows = np.asarray(fit_rows, np.int64)
    K = int(n_codes[target_col])
    y = codes[target_col, fit_rows].astype(np.int64)
    out = []
    for f in feat_cols:
        cnt = np.zeros((int(n_codes[f]), K), np.float64)
        np.add.at(cnt, (codes[f, fit_rows].astype(np.int64), y), 1.0)
        s = cnt.sum(axis=1, keepdims=True)
        out.append(np.divide(cnt, s, out=np.zeros_like(cnt), where=s > 0))
    return out


def pair_table(p, present=None):
    """D [u][u] over the codes `present` (default all) of one feature: (sum over the classes, ascending from 0.0, of |P[a][c] - P[b][c]|)
    squared by a plain product."""
    q = p if present is None else p[present]
    d = np.zeros((len(q), len(q)), np.float64)
    for c in range(q.shape[1]):
        d += np.abs(q[:, c][:, None] - q[:, c][None, :])
    return d * d


def smoten_codes(codes, n_codes, target_col, feat_cols, fit_rows, targets, k=K_NEIGHBORS, random_state=42, picks=None):
    """SMOTEN (`repair.train.smoten_resample`, operation for operation) on the code matrix `codes` [c][n] (int32, -1 = NULL).

    fit_rows : row positions in frame order; none holds a NULL in the target or a feature.  The metric is fitted on all of them.
    targets  : {class code: wanted row count}.
    Returns a list, classes ascending, of dict(klass, rows (positions within fit_rows of the class's rows), nn [m][k] (positions within
    the class's rows, ordered by (distance, position), the row itself excluded), picks [n_new], synth [n_new][c] (target = class,
    features = the mode of the drawn row's neighbours, ties to the smallest code, every other column -1)).  Classes with m <= k or
    n_new <= 0 are skipped.  The sum over the classes runs over all n_codes[target] of them: absent ones add +0.0 and keep the bits.
    picks    : {class: draws} to use instead of the seeded ones (tests)."""
    codes = np.asarray(codes)
    fit_rows = np.asarray(fit_rows, np.int64)
    feat_cols = [int(f) for f in feat_cols]
    c = codes.shape[0]
    y = codes[target_col, fit_rows]
    proba = vdm_tables(codes, n_codes, target_col, feat_cols, fit_rows)
    out = []
    for klass, n_target in sorted(targets.items(), key=lambda kv: kv[0]):
        rows = np.flatnonzero(y == klass)
        m = len(rows)
        n_new = int(n_target) - m
        if n_new <= 0 or m <= k:
            continue
        xc = codes[:, fit_rows[rows]][feat_cols].astype(np.int64)         # [F][m]
        dist = np.zeros((m, m), np.float64)
        for j in range(len(feat_cols)):
            present, inv = np.unique(xc[j], return_inverse=True)
            d = pair_table(proba[j], present)
            dist += d[inv[:, None], inv[None, :]]
        np.fill_diagonal(dist, -1.0)                                      # the row itself comes first and is dropped
        nn = np.argsort(dist, axis=1, kind="stable")[:, 1:k + 1]
        draws = np.random.RandomState(random_state).choice(np.arange(m), size=n_new, replace=True)
        if picks is not None and klass in picks:
            draws = np.asarray(picks[klass], np.int64)
        neigh = xc[:, nn[draws]]                                          # [F][n_new][k]
        synth = np.full((n_new, c), -1, np.int32)
        synth[:, target_col] = klass
        for j, f in enumerate(feat_cols):
            counts = np.zeros((n_new, int(n_codes[f])), np.int64)
            np.add.at(counts, (np.repeat(np.arange(n_new), k), neigh[j].ravel()), 1)
            synth[:, f] = counts.argmax(axis=1)                           # first maximum = smallest code
        out.append(dict(klass=int(klass), rows=rows, nn=nn.astype(np.int64), picks=draws.astype(np.int64), synth=synth))
    return out


def rebalance_plan(y, has_null, target="", class_names=None, k=K_NEIGHBORS, random_state=42):
    """`repair.train.rebalance_training_data` as a recipe.  `y` [n]: the target codes of one target's training rows in the order the
    value-space frame holds them (the sampler's order when `model.max_training_row_num` bites, ascending positions otherwise);
    `has_null` [n]: the row holds a NULL feature.

    Returns dict(median, fit (positions within the training rows of the rows without NULLs: SMOTEN's fit rows, frame order),
    with_null (those with one), classes (ascending codes SMOTEN grows), targets {class: rows wanted among the fit rows},
    pick_off [len(classes) + 1], picks (the draws, class by class, positions within the class's fit rows), synth_class [n_synth],
    order (the final frame as positions into [fit rows, synthetic rows class by class, rows with NULLs]), y_out (its target codes))."""
    y = np.asarray(y, np.int64)
    has_null = np.asarray(has_null, bool)
    cls, cnt = np.unique(y, return_counts=True)
    median = int(np.median(cnt))
    fit, with_null = np.flatnonzero(~has_null), np.flatnonzero(has_null)
    y_fit, y_na = y[fit], y[with_null]
    targets = {}
    for key, count in zip(cls.tolist(), cnt.tolist()):
        if count < median:
            nna = int((y_na == key).sum())
            if count - nna > k:
                targets[key] = median - nna
            else:
                _logger.warning("Over-sampling of '%s' in y='%s' failed because the number of the clean rows is too small: %d" % (
                    class_names[key] if class_names is not None else key, target, count - nna))
    classes, picks, pick_off = [], [], [0]
    for key in sorted(targets):
        m = int((y_fit == key).sum())
        n_new = targets[key] - m
        if n_new <= 0 or m <= k:           # (neither happens: count - nna = m > k and median > count)
            continue
        classes.append(key)
        picks.append(np.random.RandomState(random_state).choice(np.arange(m), size=n_new, replace=True).astype(np.int64))
        pick_off.append(pick_off[-1] + n_new)
    synth_class = np.concatenate([np.full(len(p), c, np.int64) for c, p in zip(classes, picks)]) if classes else np.zeros(0, np.int64)
    y_frame = np.concatenate([y_fit, synth_class, y_na])
    order = np.arange(len(y_frame), dtype=np.int64)
    rus = {key: median for key, count in zip(cls.tolist(), cnt.tolist()) if count > median}
    if rus:
        rs = np.random.RandomState(42)
        keep = []
        for key in np.unique(y_frame).tolist():
            rows = np.flatnonzero(y_frame == key)
            if key in rus:
                rows = rows[rs.choice(np.arange(len(rows)), size=int(rus[key]), replace=False)]
            keep.append(rows)
        order = np.concatenate(keep)
    return dict(median=median, fit=fit, with_null=with_null, classes=np.asarray(classes, np.int32), targets=targets,
                pick_off=np.asarray(pick_off, np.int64), picks=np.concatenate(picks) if picks else np.zeros(0, np.int64),
                synth_class=synth_class, order=order, y_out=y_frame[order])


def rebalanced_codes(codes, n_codes, target_col, feat_cols, train_rows, plan, k=K_NEIGHBORS, random_state=42):
    """The rebalanced training table [c][rows] of a plan on the host: what the pipeline assembles on the device with `Table.smoten`,
    `gather_rows` and `concat`."""
    codes = np.asarray(codes)
    train_rows = np.asarray(train_rows, np.int64)
    fit_rows = train_rows[plan["fit"]]
    parts = [codes[:, fit_rows]]
    if len(plan["classes"]):
        res = smoten_codes(codes, n_codes, target_col, feat_cols, fit_rows, plan["targets"], k=k, random_state=random_state)
        assert [r["klass"] for r in res] == list(plan["classes"])
        parts += [r["synth"].T for r in res]
    parts.append(codes[:, train_rows[plan["with_null"]]])
    return np.concatenate(parts, axis=1)[:, plan["order"]]
