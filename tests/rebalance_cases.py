"""Frames and code tables for the rebalancing tests (tests/test_rebalance_codes_cpu.py, tests/test_gpu_rebalance.py): the value frames
`rebalance_training_data` is compared on, an encoder / decoder between them and the code space, and the generators of the tables on which
the device entry is held to `repair.rebalance_codes.smoten_codes`."""
import os
import sys

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "spark-data-repair-plugin_amd"))


# ---- value frames (X, y) ------------------------------------------------------------------------------------------------------------
def four_class_frame(seed=0, n=400):
    """The four-class frame of tests/test_rebalance.py, with NULL features."""
    rng = np.random.default_rng(seed)
    y = pd.Series(rng.choice(["a", "b", "c", "d"], n, p=[0.55, 0.25, 0.15, 0.05]), name="t")
    X = pd.DataFrame({"f1": rng.choice(["x", "y", "z"], n), "f2": rng.integers(0, 5, n).astype(object), "f3": rng.choice(["p", "q"], n)})
    X.loc[rng.choice(n, 20, replace=False), "f2"] = None
    return X, y


def too_few_clean_rows_frame():
    rng = np.random.default_rng(5)
    y = pd.Series(["a"] * 60 + ["b"] * 30 + ["c"] * 4 + ["d"] * 9, name="t")
    X = pd.DataFrame({"f1": rng.choice(["x", "y"], 103), "f2": rng.choice(["u", "v", "w"], 103).astype(object)})
    X.loc[[95, 96, 97, 98], "f2"] = None            # class d: 9 rows, 5 clean ones -- not more than k
    return X, y


def numeric_features_frame(seed=2, n=300):
    rng = np.random.default_rng(seed)
    y = pd.Series(rng.choice(["r", "s", "t"], n, p=[0.6, 0.3, 0.1]), name="t")
    X = pd.DataFrame({"i": rng.integers(0, 7, n), "x": rng.choice([0.5, 1.25, -3.0, 10.0], n), "s": rng.choice(["k", "l"], n)})
    X.loc[rng.choice(n, 15, replace=False), "x"] = np.nan
    return X, y


def balanced_frame():
    """No class below the median, none above it."""
    rng = np.random.default_rng(7)
    y = pd.Series(["a", "b", "c"] * 30, name="t")
    return pd.DataFrame({"f1": rng.choice(["x", "y"], 90), "f2": rng.choice(["u", "v", "w"], 90)}), y


def none_below_frame():
    """Median = the smallest class size: under-sampling only."""
    rng = np.random.default_rng(8)
    y = pd.Series(["a"] * 50 + ["b"] * 20 + ["c"] * 20, name="t")
    return pd.DataFrame({"f1": rng.choice(["x", "y"], 90), "f2": rng.choice(["u", "v", "w"], 90)}), y


def none_above_frame():
    """Median = the largest class size: over-sampling only."""
    rng = np.random.default_rng(9)
    y = pd.Series(["a"] * 40 + ["b"] * 40 + ["c"] * 12, name="t")
    return pd.DataFrame({"f1": rng.choice(["x", "y"], 92), "f2": rng.choice(["u", "v", "w"], 92)}), y


VALUE_FRAMES = dict(four_class=four_class_frame, too_few_clean=too_few_clean_rows_frame, numeric=numeric_features_frame,
                    balanced=balanced_frame, none_below=none_below_frame, none_above=none_above_frame)


def encode(X, y):
    """(codes [c][n] int32 with -1 = NULL, n_codes, dictionaries, column names): the target is the last column; the encoding is the
    resident path's (`repair.pipeline.encode_frame`)."""
    from repair.pipeline import encode_frame
    df = pd.concat([X.reset_index(drop=True), y.reset_index(drop=True)], axis=1)
    cols = list(df.columns)
    idx, remaps, dicts = encode_frame(df, cols)
    codes = np.full(idx.shape, -1, np.int32)
    for j in range(len(cols)):
        ok = idx[j] >= 0
        codes[j, ok] = remaps[j][idx[j, ok]]
    return codes, np.asarray([max(len(d), 1) for d in dicts], np.int32), dicts, cols


def decode(codes, dicts):
    """[rows][c] object values of a code table [c][rows], None for NULL."""
    out = np.empty((codes.shape[1], codes.shape[0]), object)
    for j, d in enumerate(dicts):
        ok = codes[j] >= 0
        out[ok, j] = np.asarray(d, object)[codes[j, ok]]
        out[~ok, j] = None
    return out


def frame_values(X, y):
    """The value-space result in the same form: None for every kind of NULL, numbers as floats where the dictionary holds floats."""
    df = pd.concat([X.reset_index(drop=True), y.reset_index(drop=True)], axis=1)
    out = np.empty(df.shape, object)
    for j, c in enumerate(df.columns):
        v = df[c].to_numpy(dtype=object)
        isna = pd.isna(df[c]).to_numpy()
        numeric = pd.api.types.is_numeric_dtype(df[c]) and not pd.api.types.is_bool_dtype(df[c])
        out[:, j] = [None if na else (float(x) if numeric else x) for x, na in zip(v, isna)]
    return out


# ---- code tables for the device entry ------------------------------------------------------------------------------------------------
def random_table(seed, n, n_codes, K, class_p=None, target_last=True):
    """codes [F + 1][n] (the target last) of a random table without NULLs: features of n_codes[j] codes each, correlated with the class so
    that the metric separates the rows."""
    rng = np.random.default_rng(seed)
    y = rng.choice(K, n, p=class_p)
    cols = []
    for V in n_codes:
        shift = rng.integers(0, max(V, 1), K)
        noise = rng.integers(0, max(V, 1), n)
        cols.append(np.where(rng.random(n) < 0.5, (shift[y] + noise % 2) % max(V, 1), noise))
    codes = np.asarray(cols + [y], np.int32)
    return codes, np.asarray(list(n_codes) + [K], np.int32)


def tie_table():
    """F = 3, V = 3, about 80 rows of the grown class: few distinct rows, so the k-th and the (k + 1)-th neighbour of most rows are equally far."""
    codes, n_codes = random_table(11, 240, [3, 3, 3], 3, class_p=[0.34, 0.33, 0.33])
    return codes, n_codes


def identical_table(m=40, others=30):
    """Every row of class 0 is the same row: every distance inside the class is 0."""
    rng = np.random.default_rng(12)
    feats = np.concatenate([np.tile([[1], [2], [0]], (1, m)), rng.integers(0, 3, (3, others))], axis=1)
    y = np.concatenate([np.zeros(m, np.int64), 1 + rng.integers(0, 2, others)])
    return np.asarray(np.vstack([feats, y[None, :]]), np.int32), np.asarray([3, 3, 3, 3], np.int32)


def large_v_table(table_codes, n=700):
    """One feature above the pair-table limit, one at it, one below, one of a single code."""
    return random_table(13, n, [table_codes + 1, table_codes, 2, 1, 300], 3, class_p=[0.2, 0.5, 0.3])


def tie_share(codes, n_codes, klass, k):
    """Share of the class's rows whose k-th and (k + 1)-th neighbours (the row itself excluded) are equally far."""
    from repair.rebalance_codes import pair_table, vdm_tables
    F = codes.shape[0] - 1
    fit = np.arange(codes.shape[1])
    P = vdm_tables(codes, n_codes, F, list(range(F)), fit)
    rows = np.flatnonzero(codes[F] == klass)
    dist = np.zeros((len(rows), len(rows)))
    for j in range(F):
        dist += pair_table(P[j])[codes[j, rows][:, None], codes[j, rows][None, :]]
    np.fill_diagonal(dist, -1.0)
    d = np.sort(dist, axis=1)
    return float(np.mean(d[:, k] == d[:, k + 1]))


def picks_for(codes, target_col, classes, n_new, k=5, random_state=42):
    """(pick_off, picks, targets): the statement's draws for n_new[i] new rows of classes[i]."""
    off, picks, targets = [0], [], {}
    for c, nn in zip(classes, n_new):
        m = int((codes[target_col] == c).sum())
        picks.append(np.random.RandomState(random_state).choice(np.arange(m), size=nn, replace=True))
        off.append(off[-1] + nn)
        targets[int(c)] = m + nn
    return np.asarray(off, np.int64), np.concatenate(picks).astype(np.int64), targets


# ---- the oracle engine with the two table entries the rebalancing needs, on the numpy statement ---------------------------------------
def oracle_engine():
    """tests.helpers.OracleEngine whose tables have `smoten` (the statement `smoten_codes`) and `concat`: the pipeline and `RepairModel.run()`
    on the CPU."""
    from repair.rebalance_codes import smoten_codes
    from tests.helpers import OracleEngine

    class Table(OracleEngine._Table):
        def gather_rows(self, rows):
            return Table(self.codes[:, np.asarray(rows, np.int64)], self.n_codes, self.values, self.kinds)

        def smoten(self, target_col, feat_cols, fit_rows, classes, pick_off, picks, k=5, want_nn=False):
            y = self.codes[target_col, np.asarray(fit_rows, np.int64)]
            targets = {int(c): int((y == c).sum()) + int(pick_off[i + 1] - pick_off[i]) for i, c in enumerate(classes)}
            res = smoten_codes(self.codes, self.n_codes, target_col, list(feat_cols), fit_rows, targets, k=k)
            assert np.array_equal(np.concatenate([r["picks"] for r in res]), np.asarray(picks))
            return Table(np.concatenate([r["synth"] for r in res]).T, self.n_codes, self.values, self.kinds)

        @staticmethod
        def concat(parts):
            return Table(np.concatenate([p.codes for p in parts], axis=1), parts[0].n_codes, parts[0].values, parts[0].kinds)

    class Engine(OracleEngine):
        def upload(self, codes, n_codes):
            return Table(codes, n_codes)

        def upload_dictionaries(self, indices, remaps):
            t = OracleEngine.upload_dictionaries(self, indices, remaps)
            return Table(t.codes, t.n_codes)

    return Engine()


def skewed_run_frame(n=600, seed=31):
    """A frame for `RepairModel.run()`: a skewed four-class attribute, NULL cells in it and in two of its features."""
    rng = np.random.default_rng(seed)
    y = rng.choice(["a", "b", "c", "d"], n, p=[0.55, 0.25, 0.14, 0.06])
    f1 = np.where(rng.random(n) < 0.7, np.char.add("x", y), rng.choice(["xa", "xb", "xc", "xd"], n)).astype(object)
    f2 = rng.choice(["p", "q", "r"], n).astype(object)
    f3 = rng.integers(0, 4, n).astype(object)
    df = pd.DataFrame({"tid": np.arange(n), "f1": f1, "f2": f2, "f3": f3, "y": y.astype(object)})
    df.loc[rng.choice(n, 40, replace=False), "y"] = None
    df.loc[rng.choice(n, 15, replace=False), "f2"] = None
    df.loc[rng.choice(n, 10, replace=False), "f1"] = None
    return df
