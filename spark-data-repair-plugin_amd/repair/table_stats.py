"""Column statistics in code space: the numpy statement of `rgbm_table_column_stats` (csrc/rgbm_colstats.hip) and what `RepairMisc.describe`
makes of its integers (RepairMiscApi.computeAndGetStats, RepairMiscApi.scala).

A label-encoded column is a dictionary (its distinct values in ascending order) and one int32 code per row.  Every figure of Spark's
`ANALYZE TABLE .. COMPUTE STATISTICS FOR ALL COLUMNS` is then a function of the rows per code and of the dictionary: distinct = the codes
that occur, min / max = the lowest / highest of them, the value lengths = sums over `count x len(dictionary entry)`, and the edges of an
equi-height histogram = rank selection in the cumulative counts.  `column_stats` DEFINES those integers; the device entry returns the same
ones, with no tolerance anywhere.
"""
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import pandas as pd

FIELDS = ("nulls", "distinct", "min_code", "max_code", "len_sum", "len_max")      # stats_out [.][6] of rgbm_table_column_stats, in this order
MAX_BINS = 254
DEFAULT_STRING_SIZE = 20          # Spark's defaultSize of a string column: what ANALYZE reports for a column without any value


def column_stats(codes: Any, n_codes: Sequence[int], cols: Sequence[int], len_luts: Optional[Sequence[Any]] = None,
                 n_bins: int = 0) -> Dict[str, Any]:
    """Statistics of the listed columns of an int32 code table [c][n] (-1 or any code outside [0, n_codes[col]) is NULL, as
    `rgbm_table_count_codes` treats it).  With m = the column's non-NULL rows, per listed column (a column may be listed twice):

      nulls                 rows that are NULL
      distinct              codes held by at least one row
      min_code, max_code    the lowest / highest such code, -1 when there is none
      len_sum, len_max      sum(count[c] * len_lut[c]) as int64 and the largest len_lut[c] (entries are >= 0) of an occurring code; both 0
                            when `len_luts[j]` is None
      edges[0 .. n_bins]    (n_bins > 0) edges[0] = min_code; edges[i] = the smallest code whose cumulative non-NULL count is
                            >= ceil(i * m / n_bins), in integers (i * m + n_bins - 1) // n_bins; all -1 when m = 0

    Returns {field: int64 [len(cols)]} for FIELDS plus "edges": int32 [len(cols)][n_bins + 1], or None when n_bins == 0."""
    codes = np.asarray(codes, np.int32)
    cols = [int(c) for c in cols]
    if len(cols) < 1:
        raise ValueError("at least one column")
    if any(c < 0 or c >= codes.shape[0] for c in cols):
        raise ValueError("column index out of range")
    if not (n_bins == 0 or 1 <= n_bins <= MAX_BINS):
        raise ValueError("n_bins must be 0 or 1..%d" % MAX_BINS)
    luts = [None] * len(cols) if len_luts is None else list(len_luts)
    if len(luts) != len(cols):
        raise ValueError("one length LUT (or None) per listed column expected")
    out = {f: np.zeros(len(cols), np.int64) for f in FIELDS}
    edges = np.full((len(cols), n_bins + 1), -1, np.int32) if n_bins > 0 else None
    for j, c in enumerate(cols):
        nc = int(n_codes[c])
        v = codes[c]
        ok = (v >= 0) & (v < nc)
        count = np.bincount(v[ok], minlength=nc).astype(np.int64)
        held = np.flatnonzero(count)
        m = int(ok.sum())
        out["nulls"][j] = len(v) - m
        out["distinct"][j] = len(held)
        out["min_code"][j] = held[0] if len(held) else -1
        out["max_code"][j] = held[-1] if len(held) else -1
        if luts[j] is not None:
            lut = np.asarray(luts[j], np.int64)
            if len(lut) != nc:
                raise ValueError("the length LUT of column %d must hold one entry per code (%d)" % (c, nc))
            out["len_sum"][j] = int((count * lut).sum())
            out["len_max"][j] = max(0, int(lut[held].max())) if len(held) else 0
        if edges is not None and m > 0:
            cum = np.cumsum(count)
            ranks = np.asarray([(i * m + n_bins - 1) // n_bins for i in range(1, n_bins + 1)], np.int64)
            edges[j, 0] = held[0]
            edges[j, 1:] = np.searchsorted(cum, ranks, side="left")
    out["edges"] = edges
    return out


def dict_strings(s: pd.Series, values: Any) -> List[str]:
    """`CAST(value AS STRING)` of the dictionary entries of column `s` (`pipeline.encode_frame` keeps the dictionary of a numeric column as
    float64: an integral column prints as integers, `8`, any other number as a double, `16.0`)."""
    from repair.encode import is_integral_column, is_numeric_column
    from repair.errors import _to_sql_string
    if is_numeric_column(s):
        if is_integral_column(s):
            return [str(int(v)) for v in values]
        return [_to_sql_string(float(v)) for v in values]
    return [_to_sql_string(v) for v in values]


def describe_frame(df: pd.DataFrame, n_bins: int = 8, engine: Any = None) -> pd.DataFrame:
    """[attrName, distinctCnt, min, max, nullCnt, avgLen, maxLen, hist], one row per column in frame order.  The frame is encoded once; the
    integers come from `engine.column_stats` on the uploaded table when an engine is given and from `column_stats` otherwise."""
    from repair.encode import is_numeric_column
    from repair.pipeline import encode_frame
    names = ["attrName", "distinctCnt", "min", "max", "nullCnt", "avgLen", "maxLen", "hist"]
    if not 1 <= n_bins <= MAX_BINS:
        raise ValueError("Option 'num_bins' must be an integer in [1, %d], but '%s' found" % (MAX_BINS, n_bins))
    cols = list(df.columns)
    if not cols:
        return pd.DataFrame([], columns=names)
    idx, remaps, dicts = encode_frame(df, cols)
    numeric = [is_numeric_column(df[c]) for c in cols]
    strings = [None if num else dict_strings(df[c], d) for c, num, d in zip(cols, numeric, dicts)]
    # the length LUT of a discrete column counts characters; one entry per code (an all-NULL column is a one-code domain without a row)
    luts = [None if s is None else np.asarray([len(x) for x in s] or [0], np.int32) for s in strings]
    listed = list(range(len(cols)))
    if engine is not None and len(df) > 0:
        st = engine.column_stats(engine.upload_dictionaries(idx, remaps), listed, len_luts=luts, n_bins=n_bins)
    else:
        codes = np.stack([np.where(i >= 0, r[np.maximum(i, 0)] if len(r) else -1, -1).astype(np.int32) for i, r in zip(idx, remaps)])
        st = column_stats(codes, [max(len(d), 1) for d in dicts], listed, len_luts=luts, n_bins=n_bins)
    rows = []
    for j, c in enumerate(cols):
        m = len(df) - int(st["nulls"][j])
        lo = hi = hist = None
        if numeric[j]:
            avg_len = max_len = int(getattr(df[c].dtype, "itemsize", 8))
            if m > 0:
                s = dict_strings(df[c], [dicts[j][int(st["min_code"][j])], dicts[j][int(st["max_code"][j])]])
                lo, hi = s[0], s[1]
                v = np.asarray(dicts[j], np.float64)[st["edges"][j]]
                if v[-1] > v[0]:                      # (max = min: the reference divides 0 by 0; its tests do not say what comes of it)
                    hist = [float((v[i + 1] - v[i]) / (v[-1] - v[0])) for i in range(n_bins)]
        elif m > 0:
            avg_len, max_len = -(-int(st["len_sum"][j]) // m), int(st["len_max"][j])
        else:
            avg_len = max_len = DEFAULT_STRING_SIZE
        rows.append((c, int(st["distinct"][j]), lo, hi, int(st["nulls"][j]), avg_len, max_len, hist))
    out = pd.DataFrame(rows, columns=names)
    for c in ("min", "max", "hist"):
        out[c] = out[c].astype(object)
    return out
