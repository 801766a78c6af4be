"""An independent, dense statement of one k-means assignment step over bag-of-q-gram features (reference RepairMiscApi.scala:52-153):
the explicit N x V bag matrix built from the ROW STRINGS (not from per-value bags), scores h - 2 X C^T, arg-min, counts through
np.add.at.  tests/test_split_input_table_cpu.py holds repair.qgram_kmeans (code space) against it."""
import numpy as np
import pandas as pd


def row_grams(values, q):
    """The q-grams of one row (`computeQgram` over `array(attrs)` cast to string): NULLs skipped, a string no longer than q is its own q-gram."""
    out = []
    for s in values:
        if s is None:
            continue
        if len(s) <= q:
            out.append(s)
        else:
            out.extend(s[i:i + q] for i in range(len(s) - q + 1))
    return out


def row_strings(df, attrs):
    """Per row the attributes as strings (None = NULL); floats that hold whole numbers print as Spark's CAST does (`1.0`)."""
    cols = []
    for a in attrs:
        col = []
        for v in df[a].to_numpy(dtype=object):
            if v is None or (not isinstance(v, str) and pd.isna(v)):
                col.append(None)
            elif isinstance(v, (float, np.floating)):
                col.append(repr(float(v)))
            else:
                col.append(str(v))
        cols.append(col)
    return list(zip(*cols)) if cols else [()] * len(df)


def bag_matrix(df, attrs, q):
    """(X float64 [N][V], vocabulary in order of first appearance over the rows)."""
    rows = row_strings(df, attrs)
    vocab = {}
    grams = [[vocab.setdefault(g, len(vocab)) for g in row_grams(r, q)] for r in rows]
    x = np.zeros((len(rows), max(len(vocab), 1)), np.float64)
    for i, g in enumerate(grams):
        np.add.at(x[i], g, 1.0)
    return x, list(vocab)


def assign(x, centres):
    """(labels, margin): arg-min of h - 2 X C^T (first minimum), second-best minus best score, |best|."""
    h = (centres * centres).sum(axis=1)
    s = h[None, :] - 2.0 * (x @ centres.T)
    lab = np.argmin(s, axis=1)
    srt = np.sort(s, axis=1)
    return lab.astype(np.int32), srt[:, 1] - srt[:, 0], np.abs(srt[:, 0])


def counts_of(labels, codes, n_codes, off, d_tot, k):
    """counts[k][d_tot] and sizes[k] of the given labels over a code table [c][N] (-1 / out of range = NULL)."""
    counts = np.zeros((k, d_tot), np.int64)
    for j in range(codes.shape[0]):
        ok = (codes[j] >= 0) & (codes[j] < n_codes[j])
        np.add.at(counts, (labels[ok], off[j] + codes[j][ok]), 1)
    sizes = np.zeros(k, np.int64)
    np.add.at(sizes, labels, 1)
    return counts, sizes


RANDOM_FRAME_SEED = 14       # chosen so that the dense restatement alone leaves fewer than 1 % of the rows without a clear margin (the initial
                             # centres are rows, so every score of the first iteration is an integer and exact ties are common)


def random_frame(n, seed=RANDOM_FRAME_SEED):
    """tid + six string attributes built from one pool of syllables (so the attributes share q-grams), with strings no longer than
    q = 2 among them, 5 % NULLs and one attribute that is NULL in every row."""
    rng = np.random.default_rng(seed)
    syll = ["ab", "bc", "ca", "xy", "yz", "zx", "mn", "no", "om", "q"]
    words = ["".join(rng.choice(syll, int(rng.integers(2, 7)))) for _ in range(120)]
    words += ["a", "b", "xy", ""]
    words = np.asarray(sorted(set(words)), dtype=object)
    data = {"tid": np.arange(n)}
    group = rng.integers(0, 4, n)                                  # four kinds of rows, so that there is something to find
    for j in range(5):
        pick = (group * 29 + rng.integers(0, 23, n) + 3 * j) % len(words)
        col = words[pick].copy()
        col[rng.random(n) < 0.05] = None
        data["a%d" % j] = col
    data["a5"] = np.full(n, None, dtype=object)
    return pd.DataFrame(data)
