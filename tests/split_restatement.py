"""One tree of LightGBM 3.3.1's serial learner on binned data, restated in plain Python for tests/split_cases.py: the split search of a leaf
(FeatureHistogram::FindBestThresholdSequentially, both directions), the choice among features and among leaves, the gates in front of a
search and Tree::Split's numbering.  Written as loops in LightGBM's visiting order -- the tie rules are what the loops do with a strict
`>`, nowhere a comparator -- and not derived from oracle/rgbm_oracle_train.inc, which tests/test_split_cases_cpu.py holds against it.

Sums of (g, h) are exact (fractions.Fraction, supplied per row by the case); every gain, output and count estimate is LightGBM's double
expression in LightGBM's order of operations on the correctly rounded sums.

grow(bins, feats, g, h, ...) -> (tree, trace)
  bins    [F][n] bin of every row; the NaN bin of a feature is its V
  feats   [(V, has_nan)] per feature
  g, h    per-row Fractions
  tree    dict(feat, theta, dleft, left, right, gain, leaf_value (un-shrunk outputs), leaf_count); child >= 0: node, < 0: ~leaf
  trace   dict(leaves = {leaf index at search time: dict(n, searched, gain, best = [(feature, theta, direction)] -- every candidate that
          holds the leaf's best gain, direction 'r' reverse (NaN left) or 'f' forward --, halves = [(feature, bin, direction)] -- bins whose
          count estimate h * cnt_factor fell exactly on k + 1/2)} in search order as a list `searches`, and `picks` = [(leaf taken,
          [leaves that held the same gain])] per split.
"""
import math
from fractions import Fraction

import numpy as np

K_EPSILON = float(np.float32(1e-15))            # kEpsilon is a float literal
NEG_INF = float("-inf")


def _threshold_l1(s, l1):
    reg = abs(s) - l1
    if reg < 0.0:
        reg = 0.0
    return (1.0 if s > 0.0 else (-1.0 if s < 0.0 else 0.0)) * reg


def _leaf_gain(G, H, l1, l2):
    sg = _threshold_l1(G, l1) if l1 > 0.0 else G
    return (sg * sg) / (H + l2)


def _leaf_output(G, H, l1, l2):
    sg = _threshold_l1(G, l1) if l1 > 0.0 else G
    return -sg / (H + l2)


def _round_int(x):
    return int(x + 0.5)                          # (long long)(x + 0.5): truncation of a non-negative double


def _search_leaf(rows, bins, feats, used, g, h, p):
    """the best split of one leaf: dict(gain, feature, theta, dleft, lg, lh (exact left sums), lout, rout, best, halves) or gain -inf"""
    l1, l2 = p["lambda_l1"], p["lambda_l2"]
    mdl, msh, mgs = p["min_data_in_leaf"], p["min_sum_hessian_in_leaf"], p["min_gain_to_split"]
    num_data = len(rows)
    G = sum((g[r] for r in rows), Fraction(0))
    H = sum((h[r] for r in rows), Fraction(0))
    sum_gradient = float(G)
    sum_hessian = float(H) + 2 * K_EPSILON
    gain_shift = _leaf_gain(sum_gradient, sum_hessian, l1, l2)
    min_gain_shift = gain_shift + mgs
    cnt_factor = num_data / sum_hessian
    leaf = dict(gain=NEG_INF, feature=-1)
    cands, halves = [], []                       # every kept candidate (relative gain, feature, theta, direction)

    for f in range(len(feats)):
        if not used[f]:
            continue
        V, has_nan = feats[f]
        if V == 0 or V + has_nan <= 1:
            continue
        hg = [Fraction(0)] * (V + has_nan)
        hh = [Fraction(0)] * (V + has_nan)
        for r in rows:
            b = bins[f][r]
            hg[b] += g[r]
            hh[b] += h[r]
        out = dict(gain=NEG_INF, feature=f)
        splittable = False

        def estimate(b, direction):
            x = float(hh[b]) * cnt_factor
            if x - math.floor(x) == 0.5:
                halves.append((f, b, direction))
            return _round_int(x)

        # reverse: from the top value bin down, the NaN rows stay left; the first candidate visited keeps a tie
        best_gain, best = NEG_INF, None
        rg, rh, right_count = Fraction(0), Fraction(0), 0
        for b in range(V - 1, -1, -1):
            rg += hg[b]
            rh += hh[b]
            right_count += estimate(b, "r")
            sum_right_hessian = float(rh) + K_EPSILON
            if right_count < mdl or sum_right_hessian < msh:
                continue
            left_count = num_data - right_count
            if left_count < mdl:
                break
            lg, lh = G - rg, H - rh
            sum_left_hessian = float(lh) + K_EPSILON
            if sum_left_hessian < msh:
                break
            cur = _leaf_gain(float(lg), sum_left_hessian, l1, l2) + _leaf_gain(float(rg), sum_right_hessian, l1, l2)
            if cur <= min_gain_shift:
                continue
            splittable = True
            cands.append((cur - min_gain_shift, f, b - 1, "r"))
            if cur > best_gain:
                best_gain, best = cur, (b - 1, lg, lh, left_count)
        if splittable and best_gain > out["gain"] + min_gain_shift:
            out.update(gain=best_gain - min_gain_shift, theta=best[0], dleft=1, lg=best[1], lh=best[2])

        # forward: only with a NaN bin, the NaN rows go right; the first candidate visited keeps a tie; replaces reverse only when greater
        if has_nan and V >= 1:
            best_gain, best = NEG_INF, None
            lg, lh, left_count = Fraction(0), Fraction(0), 0
            for b in range(0, V):
                lg += hg[b]
                lh += hh[b]
                left_count += estimate(b, "f")
                sum_left_hessian = float(lh) + K_EPSILON
                if left_count < mdl or sum_left_hessian < msh:
                    continue
                right_count = num_data - left_count
                if right_count < mdl:
                    break
                rg, rh = G - lg, H - lh
                sum_right_hessian = float(rh) + K_EPSILON
                if sum_right_hessian < msh:
                    break
                cur = _leaf_gain(float(lg), sum_left_hessian, l1, l2) + _leaf_gain(float(rg), sum_right_hessian, l1, l2)
                if cur <= min_gain_shift:
                    continue
                splittable = True
                cands.append((cur - min_gain_shift, f, b, "f"))
                if cur > best_gain:
                    best_gain, best = cur, (b, lg, lh, left_count)
            if splittable and best_gain > out["gain"] + min_gain_shift:
                out.update(gain=best_gain - min_gain_shift, theta=best[0], dleft=0, lg=best[1], lh=best[2])

        # across features in ascending order: only a strictly greater gain replaces, so the smaller index keeps a tie
        if out["gain"] > leaf["gain"]:
            leaf = out

    if leaf["feature"] >= 0:
        lH = float(leaf["lh"]) + K_EPSILON
        rH = float(H - leaf["lh"]) + K_EPSILON
        leaf["lout"] = _leaf_output(float(leaf["lg"]), lH, l1, l2)
        leaf["rout"] = _leaf_output(float(G - leaf["lg"]), rH, l1, l2)
    leaf["best"] = [(f, t, d) for (gn, f, t, d) in cands if gn == leaf["gain"]]
    leaf["halves"] = halves
    return leaf


def grow(bins, feats, g, h, used=None, num_leaves=31, max_depth=7, min_data_in_leaf=20, min_sum_hessian_in_leaf=1e-3,
         min_gain_to_split=0.0, lambda_l1=0.0, lambda_l2=0.0):
    p = dict(min_data_in_leaf=min_data_in_leaf, min_sum_hessian_in_leaf=min_sum_hessian_in_leaf, min_gain_to_split=min_gain_to_split,
             lambda_l1=lambda_l1, lambda_l2=lambda_l2)
    F, n = len(feats), len(g)
    used = [True] * F if used is None else list(used)
    none = dict(gain=NEG_INF, feature=-1)
    rows = {0: list(range(n))}
    depth = {0: 0}
    best = {0: none}
    parent_of = {0: (-1, False)}                  # leaf -> (node that points to it, through its left link)
    tree = dict(feat=[], theta=[], dleft=[], left=[], right=[], gain=[], leaf_value=[0.0], leaf_count=[n])
    searches, picks = [], []

    def search(leaf):
        ok = len(rows[leaf]) >= 2 * min_data_in_leaf and not (max_depth > 0 and depth[leaf] >= max_depth)
        res = _search_leaf(rows[leaf], bins, feats, used, g, h, p) if ok else dict(none, best=[], halves=[])
        best[leaf] = res
        searches.append(dict(leaf=leaf, n=len(rows[leaf]), searched=ok, gain=res["gain"], best=res["best"], halves=res["halves"]))

    search(0)
    L = 1
    while L < num_leaves:
        # among leaves in ascending order: a greater gain replaces; at the same gain the smaller feature does; else the earlier leaf stays
        bl = 0
        for l in range(1, L):
            a, b = best[l], best[bl]
            if a["gain"] > b["gain"]:
                bl = l
            elif a["gain"] == b["gain"] and a["feature"] >= 0 and a["feature"] < b["feature"]:
                bl = l
        sp = best[bl]
        if not sp["gain"] > 0.0:
            break
        picks.append((bl, [l for l in range(L) if best[l]["gain"] == sp["gain"]]))
        node, right_leaf = L - 1, L
        f, theta, dleft = sp["feature"], sp["theta"], sp["dleft"]
        tree["feat"].append(f); tree["theta"].append(theta); tree["dleft"].append(dleft); tree["gain"].append(sp["gain"])
        tree["left"].append(~bl); tree["right"].append(~right_leaf)
        pn, through_left = parent_of[bl]
        if pn >= 0:
            tree["left" if through_left else "right"][pn] = node
        parent_of[bl], parent_of[right_leaf] = (node, True), (node, False)
        V, has_nan = feats[f]
        go_left = [r for r in rows[bl] if (dleft if (has_nan and bins[f][r] == V) else bins[f][r] <= theta)]
        go_right = [r for r in rows[bl] if not (dleft if (has_nan and bins[f][r] == V) else bins[f][r] <= theta)]
        rows[bl], rows[right_leaf] = go_left, go_right
        tree["leaf_value"][bl] = sp["lout"]
        tree["leaf_value"].append(sp["rout"])
        tree["leaf_count"][bl] = len(go_left)
        tree["leaf_count"].append(len(go_right))
        depth[bl] = depth[right_leaf] = depth[bl] + 1
        best[bl], best[right_leaf] = none, none
        L += 1
        if L >= num_leaves:
            break
        search(bl)
        search(right_leaf)
    return tree, dict(searches=searches, picks=picks)
