"""Value-space restatements for `RepairMisc.describe` / `generateDepGraph`: the column statistics of repair/table_stats.py said again with
pandas on the VALUES (`nunique`, `isna().sum()`, ranks among the sorted values) instead of on per-code counts, random code tables and
frames for both, and a regular-expression reader of the written DOT text.  tests/test_describe_cpu.py, tests/test_depgraph_cpu.py and
tests/test_gpu_column_stats.py share them."""
import json
import os
import re

import numpy as np
import pandas as pd

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "misc_describe_depgraph.json")


def golden():
    with open(GOLDEN, encoding="utf-8") as f:
        return json.load(f)


def random_dictionary(rng, d):
    """d distinct strings of 0..12 characters in ascending order (code order = value order)."""
    out = set()
    while len(out) < d:
        out.add("".join(rng.choice(list("abcxyz-0"), int(rng.integers(0, 13)))) + "%d" % len(out))
    return sorted(out)


def value_space_stats(values, dictionary, n_bins):
    """The statement of `table_stats.column_stats` for one column given as VALUES (None = NULL) and its ascending dictionary (which may hold
    entries no row holds): a dict of the six numbers and the edges as codes."""
    s = pd.Series(values, dtype=object)
    code_of = {v: i for i, v in enumerate(dictionary)}
    have = sorted(s.dropna().tolist())
    m = len(have)
    out = dict(nulls=int(s.isna().sum()), distinct=int(s.nunique()), min_code=code_of[have[0]] if m else -1, max_code=code_of[have[-1]] if m else -1,
               len_sum=int(sum(len(v) for v in have)), len_max=max([len(v) for v in have] or [0]))
    if n_bins > 0:
        # the smallest value with at least `rank` values at or below it is the rank-th smallest value
        out["edges"] = [out["min_code"]] + [code_of[have[-(-(i * m) // n_bins) - 1]] if m else -1 for i in range(1, n_bins + 1)]
    return out


def random_codes(rng, n, n_codes, null=0.05, held=None):
    """One int32 column of n rows over `n_codes` codes of which only the codes in `held` (default: a random two thirds) occur."""
    if held is None:
        held = np.flatnonzero(rng.random(n_codes) < 0.67)
        if len(held) == 0:
            held = np.asarray([int(rng.integers(0, n_codes))])
    col = np.asarray(held, np.int64)[rng.integers(0, len(held), n)].astype(np.int32)
    col[rng.random(n) < null] = -1
    return col


def misc_frame(n, seed=7):
    """tid + two low-domain string attributes that depend on each other, one with characters that HTML escapes, an int and a float
    column, an int32 column, a constant number, a wide string attribute, 5 % NULLs in most of them and one attribute that is NULL in every row."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 12, n)
    b = (a // 3 + (rng.random(n) < 0.1)) % 5
    data = {"tid": np.arange(n)}
    data["city"] = np.asarray(["city-%02d" % v for v in a], dtype=object)
    data["state"] = np.asarray(["s<%d>&" % v for v in b], dtype=object)
    data["level"] = (a % 4).astype(np.int64)
    data["score"] = np.round(rng.normal(size=n), 1) + (b == 2) * 1.5
    data["small"] = rng.integers(-3, 40, n).astype(np.int32)
    data["const"] = np.full(n, 2.5)
    data["text"] = np.asarray(["".join(rng.choice(list("abcdefgh"), int(rng.integers(1, 30)))) for _ in range(n)], dtype=object)
    data["none"] = np.full(n, None, dtype=object)
    df = pd.DataFrame(data)
    for c in ("city", "state", "text"):
        df.loc[rng.random(n) < 0.05, c] = None
    df.loc[rng.random(n) < 0.05, "score"] = np.nan
    return df


NODE = re.compile(r'^"([^"]+)" \[color="black" label=<\n(.*?)</table>>\];', re.S | re.M)
PORT = re.compile(r'<tr><td port="(-?\d+)">(.*?)</td></tr>')
HUB_NODE = re.compile(r'^"([^"]+)" \[ shape="box" \];$', re.M)
HUB_EDGE = re.compile(r'^\s*"([^"]+)" -> "([^"]+)":nodeName \[ arrowhead="diamond" penwidth="1.0" \];$', re.M)
EDGE = re.compile(r'^\s*"([^"]+)":(-?\d+) -> "([^"]+)":(-?\d+) \[ color="(gray\d+)" penwidth="([^"]+)" (label="[^"]*")? ?\];$', re.M)


def parse_dot(text):
    """The DOT text of `compute_dep_graph` as the structure of the golden fixture: nodes {id: values in port order (escaped as written; the
    "..." entry of a truncated node last, port -1)}, hubs [[attr, node id]], hub_boxes [attr], edges [[from attr, from value, to attr, to
    value, colour, penwidth, label or None]] in the order written."""
    nodes, port_of = {}, {}
    for name, body in NODE.findall(text):
        entries = [(int(p), v) for p, v in PORT.findall(body)]
        nodes[name] = [v for _, v in entries]
        port_of[name] = {p: v for p, v in entries}
    edges = []
    for a, pa, b, pb, colour, w, label in EDGE.findall(text):
        edges.append([a.rsplit("_", 1)[0], port_of[a][int(pa)], b.rsplit("_", 1)[0], port_of[b][int(pb)], colour, float(w), label or None])
    return dict(nodes=nodes, hubs=[[h, n] for h, n in HUB_EDGE.findall(text)], hub_boxes=HUB_NODE.findall(text), edges=edges)
