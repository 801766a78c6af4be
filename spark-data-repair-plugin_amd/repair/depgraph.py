"""The dependency graph of `RepairMisc.generateDepGraph` (DepGraph.computeDepGraph, DepGraph.scala:88-197) in code space: DESIGN.md 5k.

Three things the repair path has already make it up: the dense joint counts of attribute pairs (`Table.pair_counts` on the resident table,
a numpy count of the same layout without a device), the conditional entropies H(x|y) read from them (`domain.pairwise_stats`), and a
per-pair listing `x value -> {y value: count}` read off the same tables.  All counts are integers, so both paths print the same floats.
What is left is the Graphviz text, laid out as the reference lays it out so that its users' `dot` draws the same picture.
"""
import html
import itertools
import logging
import math
import os
import shutil
import subprocess
from typing import Any, Dict, List, Sequence, Tuple

import numpy as np
import pandas as pd

_logger = logging.getLogger(__name__)

TRUNCATED = ("...", -1)           # the entry a truncated pair appends to both of its nodes


def dense_pair_counts(codes: np.ndarray, n_codes: Sequence[int], pairs: Sequence[Tuple[int, int]]) -> List[np.ndarray]:
    """The layout of `Table.pair_counts` counted with numpy: per pair an int64 [(n_codes[x] + 1)][(n_codes[y] + 1)] array, NULL in the last
    slot of each side."""
    out = []
    for x, y in pairs:
        dx, dy = int(n_codes[x]), int(n_codes[y])
        kx = np.where((codes[x] < 0) | (codes[x] >= dx), dx, codes[x]).astype(np.int64)
        ky = np.where((codes[y] < 0) | (codes[y] >= dy), dy, codes[y]).astype(np.int64)
        out.append(np.bincount(kx * (dy + 1) + ky, minlength=(dx + 1) * (dy + 1)).astype(np.int64).reshape(dx + 1, dy + 1))
    return out


def _joint_counts(codes: np.ndarray, n_codes: Sequence[int], remaps: Any, idx: np.ndarray, pairs: Sequence[Tuple[int, int]],
                  engine: Any) -> List[np.ndarray]:
    if engine is not None and codes.shape[1] > 0:
        try:
            return [np.asarray(d, np.int64) for d in engine.upload_dictionaries(idx, remaps).pair_counts(pairs)]
        except Exception as ex:  # noqa: BLE001
            if getattr(ex, "code", None) != -2:             # -2 = RGBM_ERR_PARAM: a pair beyond the dense tables of the entry
                raise
            _logger.info("the joint counts of the dependency graph are counted on the host: %s" % ex)
    return dense_pair_counts(codes, n_codes, pairs)


def _trim(s: str, max_length: int) -> str:
    return s[:max_length] + "..." if len(s) > max_length else s


def _node_text(name: str, entries: Sequence[Tuple[str, int]], max_length: int) -> str:
    cells = "\n".join('<tr><td port="%d">%s</td></tr>' % (i, html.escape(_trim(v, max_length), quote=False)) for v, i in entries)
    return ('\n"%s" [color="black" label=<\n  <table>\n    <tr><td bgcolor="black" port="nodeName"><i><font color="white">%s</font></i></td></tr>\n'
            '    %s\n  </table>>];\n' % (name, name, cells))


def compute_dep_graph(df: pd.DataFrame, target_attrs: Sequence[str], max_domain_size: int = 100, max_attr_value_num: int = 30,
                      max_attr_value_length: int = 70, pairwise_attr_stat_threshold: float = 1.0, edge_label: bool = False,
                      engine: Any = None) -> str:
    """The DOT text of the dependency graph of `df` over `target_attrs` (empty = every column).

    Candidates are the target attributes, in frame column order, with at most `max_domain_size` distinct non-NULL values; every pair of
    them is oriented so that x has the larger or equal domain; the pairs with max(H(x|y), 0) <= the threshold are drawn: the first
    `max_attr_value_num` x values (ascending) that meet a non-NULL y, the y values they meet, and one edge per (x value, y value) whose
    colour and width follow the share and the count of the pair.  Node ids count from 0 in every call."""
    from repair import domain
    from repair.pipeline import encode_frame
    from repair.table_stats import dict_strings
    wanted = set(target_attrs) if target_attrs else set(df.columns)
    attrs = [c for c in df.columns if c in wanted]
    idx, remaps, dicts = encode_frame(df, attrs)
    dom = [len(d) for d in dicts]                               # exact non-NULL distinct counts (every dictionary entry occurs)
    cand = [j for j in range(len(attrs)) if dom[j] <= max_domain_size]
    if len(cand) < 2:
        raise ValueError("At least two candidate attributes needed to build a dependency graph")
    pairs = [(y, x) if dom[x] < dom[y] else (x, y) for x, y in itertools.combinations(cand, 2)]
    # the candidates alone go to the device, as columns 0 .. len(cand) - 1
    pos = {j: i for i, j in enumerate(cand)}
    c_idx = np.ascontiguousarray(idx[cand])
    c_remaps = [remaps[j] for j in cand]
    c_n_codes = [max(dom[j], 1) for j in cand]
    codes = np.stack([np.where(i >= 0, r[np.maximum(i, 0)] if len(r) else -1, -1).astype(np.int32) for i, r in zip(c_idx, c_remaps)])
    dense = _joint_counts(codes, c_n_codes, c_remaps, c_idx, [(pos[x], pos[y]) for x, y in pairs], engine)
    rows = len(df)
    # H(x|y) = H(x, y) - H(y) over every group, NULL groups included, no frequency filter (the correction term never fires)
    joint = {frozenset(p): d.reshape(-1)[d.reshape(-1) > 0] for p, d in zip(pairs, dense)}
    single: Dict[int, Any] = {}
    for (x, y), d in zip(pairs, dense):
        for a, marg in ((x, d.sum(axis=1)), (y, d.sum(axis=0))):
            single.setdefault(a, marg[marg > 0])
    stats = domain.pairwise_stats(rows, pairs, joint, single, {j: dom[j] for j in cand})
    kept = [(p, d) for p, d in zip(pairs, dense) if any(a == p[1] and max(h, 0.0) <= pairwise_attr_stat_threshold for a, h in stats[p[0]])]
    if not kept:
        raise ValueError("No highly-correlated attribute pair (threshold: %s) found" % repr(float(pairwise_attr_stat_threshold)))

    hubs, nodes, edges = [], [], []
    next_id = 0
    for (x, y), d in kept:
        body = d[:-1, :-1]                                      # both sides non-NULL
        xs = np.flatnonzero(body.sum(axis=1) > 0)
        truncate = max_attr_value_num < len(xs)
        xs = xs[:max_attr_value_num]
        if len(xs) == 0:
            continue
        ys: List[int] = []                                      # in order of first appearance, x ascending then y ascending
        seen = set()
        for xc in xs:
            for yc in np.flatnonzero(body[xc] > 0):
                if int(yc) not in seen:
                    seen.add(int(yc))
                    ys.append(int(yc))
        sx, sy = dict_strings(df[attrs[x]], dicts[x]), dict_strings(df[attrs[y]], dicts[y])
        names, ports = [], []
        for attr, values, strs in ((attrs[x], [int(v) for v in xs], sx), (attrs[y], ys, sy)):
            name = "%s_%d" % (attr, next_id)
            next_id += 1
            entries = [(strs[v], i) for i, v in enumerate(values)] + ([TRUNCATED] if truncate else [])
            hubs.append((name, attr))
            nodes.append(_node_text(name, entries, max_attr_value_length))
            names.append(name)
            ports.append({v: i for i, v in enumerate(values)})
        size_x = len(xs) + (1 if truncate else 0)               # (the reference's map holds the "..." entry too)
        for xc in xs:
            total = int(body[xc].sum())
            for yc in np.flatnonzero(body[xc] > 0):
                cnt = int(body[xc, yc])
                p = (cnt + 0.0) / total
                w = 0.1 + math.log(cnt) / (0.1 + math.log((rows + 0.0) / size_x))
                label = 'label="%d/%d"' % (cnt, total) if edge_label else ""
                edges.append('"%s":%d -> "%s":%d [ color="gray%d" penwidth="%s" %s ];'
                             % (names[0], ports[0][int(xc)], names[1], ports[1][int(yc)], int(100.0 * (1.0 - p)), repr(w), label))
    for name, attr in hubs:
        nodes.append('"%s" [ shape="box" ];' % attr)
        edges.append('"%s" -> "%s":nodeName [ arrowhead="diamond" penwidth="1.0" ];' % (attr, name))
    if not nodes:
        raise ValueError("Failed to a generate dependency graph because no correlated attribute found")
    return ('\ndigraph {\n  graph [pad="0.5" nodesep="1.0" ranksep="4" fontname="Helvetica" rankdir=LR];\n  node [shape=plaintext]\n\n  %s\n  %s\n}\n'
            % ("\n".join(sorted(nodes)), "\n".join(sorted(edges))))


IMAGE_FORMATS = ("png", "svg")


def write_dep_graph(text: str, path: str, fmt: str, prefix: str, overwrite: bool) -> None:
    """The files of DepGraph.generateDepGraph (DepGraph.scala:222-255): a fresh directory `path` (removed first when `overwrite`), the DOT
    text as `<prefix>.dot` in it and, when Graphviz's `dot` is installed, `<prefix>.<fmt>` rendered by a child process whose failure is
    ignored (the reference logs it and goes on)."""
    if fmt.lower() not in IMAGE_FORMATS:
        raise ValueError("Invalid image format: %s" % fmt)
    if overwrite:
        shutil.rmtree(path, ignore_errors=True)
    try:
        os.mkdir(path)
    except OSError:
        raise ValueError("`overwrite` is set to true, but could not remove output dir path '%s'" % path if overwrite
                         else "output dir path '%s' already exists" % path) from None
    src = os.path.join(path, prefix + ".dot")
    with open(src, "w", encoding="utf-8") as f:
        f.write(text)
    dot = shutil.which("dot")
    if dot:
        try:
            with open(os.path.join(path, "%s.%s" % (prefix, fmt)), "wb") as out:
                subprocess.run([dot, "-T" + fmt, src], stdout=out, stderr=subprocess.DEVNULL, check=False)
        except OSError:
            pass
