"""The value detectors of `repair.errors` (RegExErrorDetector, DomainValues, GaussianOutlierErrorDetector, and LOFOutlierErrorDetector through
repair.lof_codes) as predicates on a column's
DICTIONARY CODES -- what `Table.detect_cells` (rgbm_table_detect_cells, csrc/rgbm_prep.hip) takes.

A column of the label-encoded table holds codes 0..D-1 into its dictionary (`pipeline.encode_frame`: the distinct non-NULL values,
ascending; -1 = NULL).  A regex or a value domain is a function of the value alone, so it is evaluated once per DISTINCT value (D
evaluations, not N) into one bit per code; a numeric dictionary is ascending, so Tukey fences keep a contiguous code range, and the
quartiles follow exactly from the rows per code.  Every function here must give exactly the cells the value-space detector gives on
the frame.  Plain numpy / pandas: both engines (and the tests) use it.

A descriptor is  dict(col, attribute, kinds, null_is_error, keep_lo, keep_hi, flag_bits, codes_flagged):  `keep_lo > keep_hi` = no
range test, `flag_bits` None = no bitset, else uint64 [ceil(D / 64)] with bit c set = code c is an error.
"""
import re

import numpy as np
import pandas as pd

NO_RANGE = (0, -1)
LOF_MAX_RANGE = 1e150      # the LOF kind: beyond it the square of a difference leaves float64 (1.3e154) or comes close


def pack_bits(flags):
    """bool [D] -> uint64 [ceil(D / 64)], bit c % 64 of word c // 64 = flags[c]."""
    flags = np.asarray(flags, bool)
    words = np.zeros((len(flags) + 63) // 64 * 64, np.uint8)
    words[:len(flags)] = flags
    return np.packbits(words.reshape(-1, 8), axis=1, bitorder="little").reshape(-1).view("<u8").astype(np.uint64)


def unpack_bits(words, n):
    """The inverse of `pack_bits`: bool [n]."""
    b = np.unpackbits(np.ascontiguousarray(words, "<u8").view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def dictionary_series(values, dtype):
    """The dictionary values as a Series of the COLUMN's dtype: numeric dictionaries are float64 (`encode_frame`), and
    `df[attr].astype(str)` prints an int64 column as '2' and a float column as '2.0'."""
    if np.asarray(values).dtype == object:
        return pd.Series(np.asarray(values, object), dtype=object).astype(dtype)
    return pd.Series(np.asarray(values, np.float64)).astype(dtype)


def regex_flags(series, regex):
    """bool [D]: the values `RegExErrorDetector._detect_regex` flags -- `re.search` finds nothing in `astype(str)` of the value."""
    pat = re.compile(regex)
    return np.array([pat.search(v) is None for v in series.astype(str).tolist()], bool)


def domain_regex(series, counts, values, autofill, min_count_thres):
    """The pattern `DomainValues._detect_impl` hands to the regex detector: the un-escaped, un-anchored alternation of its values; with
    `autofill` of the values seen MORE than `min_count_thres` times (the given values when none is), '$^' without any value."""
    values = list(values)
    if autofill:
        freq = [str(v) for v in series[np.asarray(counts) > min_count_thres].tolist()]
        if freq:
            values = freq
    return "(%s)" % "|".join(values) if values else "$^"


def order_statistics(counts, ks):
    """Codes of the order statistics `ks` (0-based positions in the sorted multiset) of a column with `counts` rows per code."""
    cum = np.cumsum(np.asarray(counts, np.int64))
    return np.searchsorted(cum, np.asarray(ks, np.int64), side="right")


def percentiles_from_counts(values, counts, q=(25, 75)):
    """`np.percentile(expanded, q)` (method 'linear') of the multiset that holds values[c] counts[c] times, bit for bit: numpy's own
    virtual index (n - 1) * q / 100, its two bracketing order statistics and its two-sided interpolation (`_lerp`: a + (b - a) * t,
    replaced by b - (b - a) * (1 - t) where t >= 0.5), in numpy's operations and order."""
    values = np.asarray(values, np.float64)
    n = int(np.sum(np.asarray(counts, np.int64)))
    if n < 1:
        raise ValueError("no value")
    quantiles = np.true_divide(np.asarray(q, np.float64), 100)
    virtual = (n - 1) * quantiles
    prev = np.floor(virtual)
    nxt = prev + 1
    above = virtual >= n - 1                                   # at or beyond the last position: the maximum on both sides
    prev[above], nxt[above] = -1, -1
    prev, nxt = prev.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(virtual - prev, dtype=virtual.dtype)
    a = values[order_statistics(counts, np.where(prev < 0, n + prev, prev))]
    b = values[order_statistics(counts, np.where(nxt < 0, n + nxt, nxt))]
    diff = np.subtract(b, a)
    out = np.asanyarray(np.add(a, diff * gamma))
    np.subtract(b, diff * (1 - gamma), out=out, where=gamma >= 0.5)
    return out


def tukey_fences(values, counts):
    """(lo, hi) of GaussianOutlierErrorDetector: q1 - 1.5 (q3 - q1), q3 + 1.5 (q3 - q1)."""
    q1, q3 = percentiles_from_counts(values, counts, (25, 75))
    return q1 - 1.5 * (q3 - q1), q3 + 1.5 * (q3 - q1)


def kept_code_range(values, lo, hi):
    """Codes [keep_lo, keep_hi] of an ascending dictionary that are NOT outliers, i.e. not (v < lo) | (v > hi)."""
    values = np.asarray(values, np.float64)
    return int(np.searchsorted(values, lo, side="left")), int(np.searchsorted(values, hi, side="right")) - 1


def build_descriptors(detectors, columns, dicts, dtypes, counts, targets, null_all=False, lof=None, n_rows=None):
    """Per-column descriptors of `Table.detect_cells` for the detectors  dict(kind='regex', attr, regex) /
    dict(kind='domain', attr, values, autofill, min_count_thres) / dict(kind='outlier', attrs=[continuous target attributes]) /
    dict(kind='lof', attrs=[continuous target attributes], k=20).

    kind 'lof' (LOFOutlierErrorDetector; repair.lof_codes): `lof` is the callable (values, counts, k) -> (scores, flags, n_ties, n_near)
    that evaluates the filled column's multiset -- the engine's `lof_codes` where it has one, `repair.lof_codes.lof_codes` when None --
    and `n_rows` the rows of the table (rows minus the counted ones = the NULL cells, which the detector fills with the median).  A
    column whose answer is not determined (a neighbour tie, a score within rounding of the threshold), that holds fewer than two rows,
    that scikit-learn searches by brute force (k >= rows // 2: its x^2 + y^2 - 2xy distances are not the exact differences) or whose
    values span more than LOF_MAX_RANGE (scikit-learn's squared distances overflow) raises `pipeline.NotResidentEligible`.

    columns: the table's attribute names; dicts[j]: dictionary of column j; dtypes: {attribute: dtype of the frame's column};
    counts: callable(j) -> rows per code of column j on the un-NULLed table (read only where a detector needs it); targets: the
    attributes detection looks at (a detector on another attribute contributes nothing); null_all: NullErrorDetector is present --
    NULL cells of every target are errors.  Detectors on one column merge: OR of the bitsets, intersection of the kept ranges, OR of the
    NULL flags.  Returns the descriptors in column order, one per column with any predicate."""
    pos = {c: j for j, c in enumerate(columns)}
    tset = set(targets)
    merged = {}

    def slot(attr):
        j = pos[attr]
        if j not in merged:
            merged[j] = dict(col=j, attribute=attr, kinds=[], null=False, flags=None, lo=None, hi=None)
        return merged[j]

    if null_all:
        for t in targets:
            if t in pos:
                s = slot(t)
                s["null"] = True
                s["kinds"].append("null")
    for d in detectors:
        kind = d["kind"]
        if kind in ("regex", "domain"):
            attr = d["attr"]
            if attr not in tset or attr not in pos:
                continue
            j = pos[attr]
            series = dictionary_series(dicts[j], dtypes[attr])
            if kind == "regex":
                regex = d["regex"]
                if not regex or not regex.strip():
                    continue
            else:
                cnt = counts(j) if d.get("autofill") else None
                regex = domain_regex(series, cnt, d.get("values") or [], bool(d.get("autofill")), d.get("min_count_thres", 12))
            f = regex_flags(series, regex)
            s = slot(attr)
            s["kinds"].append(kind)
            s["null"] = True                                   # `s.isna() | ~match`
            s["flags"] = f if s["flags"] is None else (s["flags"] | f)
        elif kind == "outlier":
            for attr in d["attrs"]:
                if attr not in tset or attr not in pos:
                    continue
                j = pos[attr]
                vals = np.asarray(dicts[j], np.float64)
                cnt = np.asarray(counts(j), np.int64)
                if len(vals) == 0 or int(cnt.sum()) == 0:      # no non-NULL value: the detector skips the column
                    continue
                lo, hi = tukey_fences(vals, cnt)
                klo, khi = kept_code_range(vals, lo, hi)
                s = slot(attr)
                s["kinds"].append(kind)
                bad = (vals < lo) | (vals > hi)
                if klo > khi and bad.any():                    # (not reachable with finite fences: the quartiles lie between them)
                    s["flags"] = bad if s["flags"] is None else (s["flags"] | bad)
                elif klo <= khi:
                    s["lo"] = klo if s["lo"] is None else max(s["lo"], klo)
                    s["hi"] = khi if s["hi"] is None else min(s["hi"], khi)
        elif kind == "lof":
            from repair.lof_codes import filled_multiset, lof_codes
            from repair.pipeline import NotResidentEligible
            if n_rows is None:
                raise ValueError("the LOF detector needs the table's row count")
            for attr in d["attrs"]:
                if attr not in tset or attr not in pos:
                    continue
                j = pos[attr]
                vals = np.asarray(dicts[j], np.float64)
                cnt = np.asarray(counts(j), np.int64)
                n_null = int(n_rows) - int(cnt.sum())
                fvals, fcnt, med_at, code_at = filled_multiset(vals, cnt, n_null)
                n, k = int(fcnt.sum()), int(d.get("k", 20))
                if n < 2:
                    raise NotResidentEligible("LOF detector on `%s`: %d row(s), scikit-learn needs two" % (attr, n))
                if k >= n // 2:
                    # scikit-learn's algorithm='auto' then searches by brute force, with distances from x^2 + y^2 - 2xy: values that are
                    # large next to their spread lose their differences there, and its answer is not |v_c - v_j|'s
                    raise NotResidentEligible("LOF detector on `%s`: %d rows with %d neighbours, scikit-learn searches such a column by "
                                              "brute force (k >= n // 2) and its distances are not exact" % (attr, n, k))
                if not float(fvals[-1] - fvals[0]) <= LOF_MAX_RANGE:
                    raise NotResidentEligible("LOF detector on `%s`: the values span more than %g, scikit-learn's squared distances "
                                              "overflow" % (attr, LOF_MAX_RANGE))
                _, bad, n_ties, n_near = (lof or lof_codes)(fvals, fcnt, k)
                if n_ties + n_near > 0:
                    raise NotResidentEligible("LOF detector on `%s`: %d value(s) whose neighbours are tied or whose score is within rounding of the "
                                              "threshold (%d + %d)" % (attr, n_ties + n_near, n_ties, n_near))
                bad = np.asarray(bad, bool)
                f = np.zeros(len(vals), bool)
                live = code_at >= 0
                f[live] = bad[code_at[live]]
                s = slot(attr)
                s["kinds"].append(kind)
                s["flags"] = f if s["flags"] is None else (s["flags"] | f)
                if n_null > 0 and bad[med_at]:                 # the NULL cells hold the median
                    s["null"] = True
        else:
            raise ValueError("unknown detector kind %r" % (kind,))
    out = []
    for j in sorted(merged):
        s = merged[j]
        D = len(dicts[j])
        flags = np.zeros(D, bool) if s["flags"] is None else s["flags"].copy()
        lo, hi = NO_RANGE
        if s["lo"] is not None:
            lo, hi = s["lo"], s["hi"]
            if lo > hi:                                        # two kept ranges that do not meet: every code is outside one of them
                flags[:] = True
                lo, hi = NO_RANGE
        flagged = flags.copy()
        if lo <= hi:
            flagged[:lo] = True
            flagged[hi + 1:] = True
        has_bits = bool(flags.any())
        if lo <= hi and lo == 0 and hi >= D - 1:
            lo, hi = NO_RANGE                                  # nothing outside the fences
        out.append(dict(col=j, attribute=s["attribute"], kinds=s["kinds"], null_is_error=bool(s["null"]), keep_lo=int(lo), keep_hi=int(hi),
                        flag_bits=pack_bits(flags) if has_bits else None, codes_flagged=int(flagged.sum())))
    return out
