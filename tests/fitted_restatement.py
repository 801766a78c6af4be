"""Plain-loop restatements for the kept-fit tests (tests/test_fitted_cpu.py, tests/test_fitted_gpu.py): the recode of a code table, the
LUTs from a later frame's dictionaries to the fitted ones, and the apply run -- per chain target, predict on the recoded features and fill
the NULLs.  Written from the contract (include/rgbm.h rgbm_table_recode; the issue's rules for `fitted_luts`), cell by cell, sharing no
code with repair/recode_codes.py, repair/fitted.py or repair/pipeline.py."""
import numpy as np
import pandas as pd


def recode_loops(codes, n_codes, luts, n_codes_out):
    C, n = len(codes), len(codes[0]) if len(codes) else 0
    out = [[-1] * n for _ in range(C)]
    unmapped = [0] * C
    for j in range(C):
        for i in range(n):
            v = int(codes[j][i])
            if v < 0 or v >= int(n_codes[j]):
                continue
            if luts[j] is None:
                out[j][i] = v
            else:
                out[j][i] = int(luts[j][v])
                if out[j][i] < 0:
                    unmapped[j] += 1
    return np.asarray(out, np.int32).reshape(C, n), np.asarray(unmapped, np.int64)


def nearest_fitted_code(fitted_values, v):
    """The code of the fitted value nearest to v; ties to the lower value (below the minimum the first, above the maximum the last)."""
    best, best_d = -1, None
    for k, f in enumerate(fitted_values):
        d = abs(float(v) - float(f))
        if best_d is None or d < best_d:          # strict: the first (lower) of two equally near values stays
            best, best_d = k, d
    return best


def lut_loops(fitted_dict, fitted_categorical, new_dict, new_is_object):
    """The LUT of one column: new code -> fitted code."""
    lut = [-1] * max(len(new_dict), 1)
    if len(fitted_dict) == 0 or len(new_dict) == 0:
        return np.asarray(lut, np.int32)
    if bool(new_is_object) != bool(fitted_categorical):
        raise ValueError("kinds differ")
    for k, v in enumerate(new_dict):
        if new_is_object:
            for q, f in enumerate(fitted_dict):
                if f == v:
                    lut[k] = q
        else:
            lut[k] = nearest_fitted_code(fitted_dict, v)
    return np.asarray(lut, np.int32)


def apply_loops(fitted, df, row_id, cells, load_model):
    """The apply run on frame `df` with the error cells `cells` [(row id, attribute)]: {(row id, attribute): repaired value} for the error
    cells of the fitted targets.  Values are mapped to fitted codes one by one (an error cell of a fitted target is NULL), then per chain
    target the model scores the dirty rows from its feature columns, the arg-max class (first maximum) or the regressor's value (rounded
    half to even for an integral target) fills the NULL cells of the target column, and the later models see it."""
    ids = list(df[row_id])
    at = {r: i for i, r in enumerate(ids)}
    in_fit = set(fitted.chain)
    err = set((r, a) for r, a in cells if a in in_fit and r in at)
    dirty = sorted(set(at[r] for r, _ in err))
    col_of = {c: j for j, c in enumerate(fitted.columns)}
    codes = {}
    for c in fitted.columns:
        j = col_of[c]
        d, cat = fitted.dicts[j], fitted.categorical[j]
        out = []
        for i in dirty:
            v = df[c].iloc[i]
            if (ids[i], c) in err or pd.isna(v):
                out.append(-1)
            elif cat:
                hit = [q for q, f in enumerate(d) if f == v]
                out.append(hit[0] if hit else -1)
            else:
                out.append(nearest_fitted_code(d, v) if len(d) else -1)
        codes[c] = np.asarray(out, np.int32)
    result = {}
    for t in fitted.chain:
        spec = fitted.targets[t]
        X = np.ascontiguousarray(np.stack([codes[f] for f in spec["features"]]))
        pred = load_model(spec["blob"]).predict(X)
        for k, i in enumerate(dirty):
            if spec["continuous"]:
                v = float(pred[k][0])
                if spec["integral"]:
                    v = float(np.round(v))
                fill, value = nearest_fitted_code(spec["y_values"], v), (int(v) if spec["integral"] else v)
            else:
                fill = int(np.argmax(pred[k]))
                value = fitted.dicts[col_of[t]][fill]
            if codes[t][k] < 0:
                codes[t][k] = fill
            if (ids[i], t) in err:
                result[(ids[i], t)] = value
    return result
