"""Parsed denial constraints (`repair.errors.parse_constraint`) as programs on a table's DICTIONARY CODES -- what
`Table.detect_constraint` / `Table.detect_dc` / `Table.detect_row_bits` (csrc/rgbm_prep.hip the first, csrc/rgbm_dc.hip the other two) take.
`scan_eligible` says which `dc` programs `Table.detect_dc_scan` (csrc/rgbm_dc.hip too) takes as well: the order constraints.

A column of the label-encoded table holds codes 0..D-1 into its dictionary (`pipeline.encode_frame`: the distinct non-NULL values,
ascending; -1 = NULL).  `lower_constraint` gives one of three programs, each with exactly the rows `errors._violating_rows` gives on
the frame:

  (eq, iq)                                   X1..Xm -> Y: EQ predicates plus exactly one IQ, `pipeline.constraint_to_columns` as before
  dict(kind="dc", preds, refs)               any other two-tuple constraint: preds = [(op, left column, right column, left rank, right
                                             rank)].  Equality of values is equality of codes; an order predicate compares
                                             `pd.to_numeric(.., errors="coerce")` of the values, so it compares RANKS of the dictionary
                                             entries' numbers (dense: equal numbers share a rank; NaN -> -1 = "no number"; two attributes
                                             are ranked in one merged order).  None = the codes are the ranks already.
  dict(kind="row_bits", cols, bits, refs)    single-tuple constraint (constants): a predicate is a function of the value alone, so it is
                                             evaluated once per DISTINCT value plus once for NULL -- with the very expression of
                                             `_violating_rows`, on the dictionary cast to the column's dtype -- into one bit per code
                                             (the last bit = NULL); predicates on one column are ANDed.

`refs`: the column indices the predicates reference, in order of first reference (the attributes a violating row contributes,
errors.py `ConstraintErrorDetector._detect_impl`).  What does not lower raises `NotLowerable` with the reason; the value-space detector
then evaluates (and reports) the constraint.  Plain numpy / pandas: both engines (and the tests) use it.
"""
import numpy as np
import pandas as pd

from repair.detect_codes import dictionary_series, pack_bits
from repair.errors import _constant_predicate_holds

MAX_PREDS = 16          # rgbm_table_detect_dc
MAX_EQ = 12             # KeySpec of csrc/rgbm_prep.h


class NotLowerable(ValueError):
    """The constraint stays with the value-space detector; the message says why."""


def dense_ranks(*numbers):
    """float64 arrays -> int32 arrays of their dense ranks in ONE merged ascending order (equal numbers share a rank), NaN -> -1."""
    arrs = [np.asarray(a, np.float64) for a in numbers]
    allv = np.concatenate(arrs) if arrs else np.zeros(0)
    uniq = np.unique(allv[~np.isnan(allv)])
    out = []
    for a in arrs:
        r = np.searchsorted(uniq, a).astype(np.int32)
        r[np.isnan(a)] = -1
        out.append(r)
    return out


def _numbers(values, dtype):
    """`pd.to_numeric(column, errors="coerce")` of the dictionary entries, as `_violating_rows` takes it of the column (a column without
    any value still has a one-code domain on the table: that code has no number)."""
    if len(values) == 0:
        return np.full(1, np.nan)
    return pd.to_numeric(dictionary_series(values, dtype), errors="coerce").to_numpy(dtype=np.float64, na_value=np.nan)


def _refs(preds, pos):
    out = []
    for p in preds:
        for a in p.references:
            if pos[a] not in out:
                out.append(pos[a])
    return out


def _row_bits(preds, pos, dicts, dtypes):
    per_col = {}
    for p in preds:
        j = pos[p.left]
        vals = dictionary_series(dicts[j], dtypes[p.left])
        # (a column without any value still has a one-code domain on the table: `Engine.upload_dictionaries`)
        holds = np.concatenate([_constant_predicate_holds(vals, p) if len(vals) else np.zeros(1, bool),
                                _constant_predicate_holds(pd.Series([None], dtype=object), p)])            # the last entry: NULL
        per_col[j] = holds if j not in per_col else (per_col[j] & holds)
    cols = list(per_col)
    return dict(kind="row_bits", cols=cols, bits=[pack_bits(per_col[j]) for j in cols], refs=_refs(preds, pos))


def _unquoted(constant):
    c = constant.strip()
    return c[1:-1] if len(c) >= 2 and c[0] == c[-1] and c[0] in "\"'" else c


def check_constraint(preds, columns, n_values):
    """Which program a parsed constraint lowers to -- 'fd' (the old (eq, iq) tuple), 'dc' or 'row_bits' -- from its shape and the number
    of distinct values per attribute (`n_values`: {attribute: count}) alone; raises `NotLowerable` otherwise."""
    from repair.pipeline import constraint_to_columns
    for p in preds:
        for a in p.references:
            if a not in columns:
                raise NotLowerable("%r references `%s`, which is not a column of the table" % (p, a))
    if constraint_to_columns(preds, columns) is not None:
        return "fd"
    if all(p.constant is not None for p in preds):
        for p in preds:
            if p.op in ("LT", "GT"):
                try:
                    float(_unquoted(p.constant))
                except ValueError:
                    raise NotLowerable("%r: the constant is not a number (the value-space detector reports it)" % (p,))
        return "row_bits"
    if any(p.constant is not None or p.right is None for p in preds):
        raise NotLowerable("%s mixes constant and two-tuple predicates" % (preds,))
    if len(preds) > MAX_PREDS:
        raise NotLowerable("%d predicates (the device entry takes %d)" % (len(preds), MAX_PREDS))
    if len(preds) < 2:
        raise NotLowerable("fewer than two predicates")
    keyed, ordered = set(), set()
    for p in preds:
        if p.op in ("EQ", "IQ"):
            if p.left != p.right:
                raise NotLowerable("%r compares two attributes for (in)equality" % (p,))
            keyed.add(p.left)
        else:
            ordered.update(p.references)
    both = sorted(keyed & ordered)
    if both:
        raise NotLowerable("attribute `%s` is used under an EQ / IQ and under an LT / GT predicate" % both[0])
    eq = list(dict.fromkeys(p.left for p in preds if p.op == "EQ"))
    if len(eq) > MAX_EQ:
        raise NotLowerable("%d EQ attributes (the device entry takes %d)" % (len(eq), MAX_EQ))
    span = 1
    for a in eq:
        span *= int(n_values[a]) + 1
        if span >= 1 << 63:
            raise NotLowerable("the EQ attributes span more than 2^63 value combinations")
    return "dc"


def scan_eligible(preds):
    """Whether the lowered predicates of a `kind="dc"` program -- [(op, left column, right column, left rank, right rank)] -- are an ORDER
    constraint, which `Table.detect_dc_scan` (rgbm_table_detect_dc_scan) answers by sort and scan instead of pairs: at most MAX_PREDS
    predicates, at most MAX_EQ distinct EQ attributes, no IQ, and exactly one or two LT / GT (within one attribute or across two, ranked
    or not).  Any IQ and three or more order predicates take the pairs of `Table.detect_dc`."""
    preds = list(preds)
    ops = [p[0] for p in preds]
    if not 1 <= len(preds) <= MAX_PREDS or any(op not in ("EQ", "LT", "GT") for op in ops):
        return False
    if len({p[1] for p in preds if p[0] == "EQ"}) > MAX_EQ or any(p[0] == "EQ" and p[1] != p[2] for p in preds):
        return False
    return 1 <= sum(op in ("LT", "GT") for op in ops) <= 2


def lower_constraint(preds, columns, dicts, dtypes):
    """One parsed constraint -> its program (module docstring).  columns: the table's attribute names; dicts[j]: dictionary of column j;
    dtypes: {attribute: dtype of the frame's column}."""
    from repair.pipeline import constraint_to_columns
    pos = {c: j for j, c in enumerate(columns)}
    kind = check_constraint(preds, columns, {c: len(dicts[j]) for c, j in pos.items()})
    if kind == "fd":
        return constraint_to_columns(preds, columns)
    if kind == "row_bits":
        return _row_bits(preds, pos, dicts, dtypes)
    out = []
    for p in preds:
        l, r = pos[p.left], pos[p.right]
        if p.op in ("EQ", "IQ"):
            out.append((p.op, l, r, None, None))
            continue
        nl = _numbers(dicts[l], dtypes[p.left])
        if l == r:
            # a numeric dictionary is ascending and holds every number once: its codes are the ranks
            identity = np.asarray(dicts[l]).dtype != object and len(dicts[l]) > 0 and not np.isnan(nl).any() and bool(np.all(np.diff(nl) > 0))
            rank = None if identity else dense_ranks(nl)[0]
            out.append((p.op, l, r, rank, rank))
        else:
            rl, rr = dense_ranks(nl, _numbers(dicts[r], dtypes[p.right]))
            out.append((p.op, l, r, rl, rr))
    return dict(kind="dc", preds=out, refs=_refs(preds, pos))
