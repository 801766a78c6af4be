"""CPU: `RepairMisc.generateDepGraph` / `repair.depgraph` on the case of the reference's DepGraphSuite: its nine input
rows, its options and its expected graph are tests/golden/misc_describe_depgraph.json, as values.  The written `.dot` is read back with
regular expressions (tests/misc_restatement.py parse_dot).  Node ids are exact; the values of a node are compared as a set (the reference's
order is Spark's `collect()`, ours is ascending); colours are exact and pen widths agree to 1e-12 relative, the bound tests/test_domain_analysis.py
uses for a literal-formula comparison (Java's and C's `log` may differ in the last bit).

The fixture records 18 value edges: every `"node":port -> "node":port` line of the reference's expected text (5 for x -> z, 6 for
y -> x, 7 for y -> z)."""
import math
import os
import re

import pandas as pd
import pytest

from tests import misc_restatement as R

G = R.golden()["depgraph"]


def _frame():
    return pd.DataFrame(G["rows"], columns=G["columns"])


def _run(df, name, path, **opts):
    from repair.api import Delphi
    from repair.misc import RepairMisc
    Delphi.register_table(name, df)
    o = dict(G["options"], table_name=name, path=str(path))
    o.update(opts)
    assert RepairMisc().options(o).generateDepGraph() is None
    with open(os.path.join(str(path), o["filename_prefix"] + ".dot"), encoding="utf-8") as f:
        return f.read()


def test_the_graph_of_the_reference_suite(tmp_path):
    text = _run(_frame(), "dep_ref", tmp_path / "d")
    got = R.parse_dot(text)
    assert sorted(got["nodes"]) == sorted(G["nodes"]) == ["x_1", "x_2", "y_0", "y_4", "z_3", "z_5"]
    for name, values in G["nodes"].items():
        assert set(got["nodes"][name]) == set(values) and len(got["nodes"][name]) == len(values), name
    assert sorted(got["hubs"]) == sorted(G["hubs"])
    assert sorted(got["hub_boxes"]) == sorted(h for h, _ in G["hubs"])
    assert not any(n.startswith("tid") for n in got["nodes"])            # 9 values > max_domain_size 8: not a candidate
    assert len(G["edges"]) == 18 and len(got["edges"]) == len(G["edges"])
    want = {tuple(e[:4]): e[4:] for e in G["edges"]}
    assert len(want) == len(G["edges"])
    for e in got["edges"]:
        colour, width = want[tuple(e[:4])]
        assert e[4] == colour, e
        assert abs(e[5] - width) <= 1e-12 * abs(width), (e, width)
        assert e[6] is None                                              # no edge_label
    # the header and the order of the reference: node tables, hub boxes, then the edge lines, each group sorted as strings
    assert text.startswith('\ndigraph {\n  graph [pad="0.5" nodesep="1.0" ranksep="4" fontname="Helvetica" rankdir=LR];\n  node [shape=plaintext]\n')
    assert text.rstrip().endswith("}")
    edge_lines = [ln.strip() for ln in text.splitlines() if " -> " in ln]
    assert edge_lines == sorted(edge_lines) and len(edge_lines) == 18 + 6


def test_threshold_zero_finds_no_pair(tmp_path):
    with pytest.raises(ValueError) as ei:
        _run(_frame(), "dep_ref0", tmp_path / "d", pairwise_attr_stat_threshold=G["no_pair_threshold"])
    assert G["no_pair_message"] in str(ei.value)
    assert not os.path.exists(str(tmp_path / "d"))                       # the graph is computed before any file is touched


def test_fewer_than_two_candidates(tmp_path):
    with pytest.raises(ValueError, match="At least two candidate attributes needed to build a dependency graph"):
        _run(_frame(), "dep_few", tmp_path / "d", target_attr_list="tid,x")
    with pytest.raises(ValueError, match="At least two candidate"):
        _run(_frame(), "dep_few", tmp_path / "d", max_domain_size="2")   # x and z have 3 values, y has 4
    assert sorted(R.parse_dot(_run(_frame(), "dep_few", tmp_path / "d", max_domain_size="3"))["nodes"]) == ["x_0", "z_1"]
    with pytest.raises(ValueError, match="do not exist"):
        _run(_frame(), "dep_few", tmp_path / "d", target_attr_list="x,nope")


def test_default_targets_are_every_column_and_node_ids_restart(tmp_path):
    o = {k: v for k, v in G["options"].items() if k != "target_attr_list"}
    from repair.api import Delphi
    from repair.misc import RepairMisc
    Delphi.register_table("dep_all", _frame())
    for d in ("a", "b"):                                                 # the counter starts at 0 in every call
        RepairMisc().options(dict(o, table_name="dep_all", path=str(tmp_path / d))).generateDepGraph()
        got = R.parse_dot(open(str(tmp_path / d / "g.dot"), encoding="utf-8").read())
        assert sorted(got["nodes"]) == ["x_1", "x_2", "y_0", "y_4", "z_3", "z_5"]


def test_truncation_adds_the_dots_entry_and_changes_size_x(tmp_path):
    got = R.parse_dot(_run(_frame(), "dep_trunc", tmp_path / "d", max_attr_value_num="2"))
    # y (4 values) and x / z (3 values) all exceed 2 shown x values: every node ends with the "..." entry on port -1
    for name, values in got["nodes"].items():
        assert values[-1] == "..." and "..." not in values[:-1], name
    assert got["nodes"]["y_0"] == ["test-1", "test-2", "..."] and got["nodes"]["x_1"] == ["1", "2", "3", "..."]
    assert got["nodes"]["x_2"] == ["1", "2", "..."] and got["nodes"]["z_3"] == ["1.0", "2.0", "..."]
    by = {tuple(e[:4]): e for e in got["edges"]}
    assert len(by) == len(got["edges"]) == 4 + 3 + 4
    e = by[("y", "test-1", "x", "2")]                                    # 2 of the 4 rows of test-1; size_x = 2 shown values + the "..." entry
    assert e[4] == "gray50" and abs(e[5] - (0.1 + math.log(2) / (0.1 + math.log(9.0 / 3)))) <= 1e-12 * e[5]
    e = by[("x", "2", "z", "1.0")]                                       # 3 of the 5 rows of x = 2
    assert e[4] == "gray40" and abs(e[5] - (0.1 + math.log(3) / (0.1 + math.log(9.0 / 3)))) <= 1e-12 * e[5]


def test_html_escaping_trimming_and_edge_labels(tmp_path):
    df = pd.DataFrame({"a": ["p<q&r>s-long", "p<q&r>s-long", "k", "k"], "b": ["<&>", "<&>", "plain", None]})
    text = _run(df, "dep_html", tmp_path / "d", target_attr_list="a,b", max_attr_value_length="8", edge_label="1")
    got = R.parse_dot(text)
    assert got["nodes"] == {"a_0": ["k", "p&lt;q&amp;r&gt;s-..."], "b_1": ["plain", "&lt;&amp;&gt;"]}     # cut to 8 characters, then escaped
    assert sorted(e[:4] + [e[6]] for e in got["edges"]) == [["a", "k", "b", "plain", 'label="1/1"'], ["a", "p&lt;q&amp;r&gt;s-...", "b", "&lt;&amp;&gt;", 'label="2/2"']]
    assert all(e[4] == "gray0" for e in got["edges"])
    assert 'label="' not in _run(df, "dep_html", tmp_path / "e", target_attr_list="a,b", edge_label="")


def test_nulls_count_in_the_entropy_and_are_absent_from_the_edges(tmp_path):
    """x determines y on the rows where both are given, so H(x|y) would be 0 there; the two rows with a NULL y are a group of their own in
    which x is a or b, and the row with a NULL x is the group (NULL, p): H(x|y) = H(x, y) - H(y) with NULL as a value is 0.68 bit."""
    df = pd.DataFrame({"x": ["a", "a", "b", "b", "a", "b", None], "y": ["p", "p", "q", "q", None, None, "p"]})

    def h(counts):
        return -sum(c / 7.0 * math.log(c / 7.0) / math.log(2.0) for c in counts)
    h_x_given_y = h([2, 1, 2, 1, 1]) - h([3, 2, 2])
    assert abs(h_x_given_y - (3 / 7.0 * 0.9182958340544896 + 2 / 7.0)) < 1e-12
    with pytest.raises(ValueError, match="No highly-correlated attribute pair \\(threshold: 0.67\\) found"):
        _run(df, "dep_null", tmp_path / "d", target_attr_list="x,y", pairwise_attr_stat_threshold="0.67")
    got = R.parse_dot(_run(df, "dep_null", tmp_path / "d", target_attr_list="x,y", pairwise_attr_stat_threshold="0.69", edge_label="y"))
    assert got["nodes"] == {"x_0": ["a", "b"], "y_1": ["p", "q"]}
    assert sorted(e[:5] + [e[6]] for e in got["edges"]) == [["x", "a", "y", "p", "gray0", 'label="2/2"'], ["x", "b", "y", "q", "gray0", 'label="2/2"']]
    w = 0.1 + math.log(2) / (0.1 + math.log(7.0 / 2))                    # rows = all seven
    assert all(abs(e[5] - w) <= 1e-12 * w for e in got["edges"])


def test_overwrite_and_the_existing_directory(tmp_path):
    out = tmp_path / "d"
    _run(_frame(), "dep_ow", out, filename_prefix="depgraph", pairwise_attr_stat_threshold="1.0")
    assert os.path.exists(str(out / "depgraph.dot"))
    with pytest.raises(ValueError, match=re.escape("output dir path '%s' already exists" % str(out))):
        _run(_frame(), "dep_ow", out, filename_prefix="depgraph", pairwise_attr_stat_threshold="1.0")
    _run(_frame(), "dep_ow", out, filename_prefix="g", pairwise_attr_stat_threshold="1.0", overwrite="true")
    assert os.path.exists(str(out / "g.dot")) and not os.path.exists(str(out / "depgraph.dot"))
    missing = tmp_path / "no" / "such" / "d"
    with pytest.raises(ValueError, match=re.escape("`overwrite` is set to true, but could not remove output dir path '%s'" % str(missing))):
        _run(_frame(), "dep_ow", missing, overwrite="true")
    from repair.misc import RepairMisc
    with pytest.raises(ValueError, match="Required options not found: path, table_name"):
        RepairMisc().option("table_name", "dep_ow").generateDepGraph()


def test_an_unknown_image_format_is_refused(tmp_path):
    from repair import depgraph
    with pytest.raises(ValueError, match="Invalid image format: jpg"):
        depgraph.write_dep_graph("digraph {}", str(tmp_path / "d"), "jpg", "g", False)
    assert not os.path.exists(str(tmp_path / "d"))


def test_numpy_pair_counts_have_the_layout_of_the_device_entry():
    import numpy as np
    from repair import depgraph, domain
    rng = np.random.default_rng(3)
    codes = np.stack([rng.integers(-1, 4, 200), rng.integers(-1, 6, 200)]).astype(np.int32)
    codes[1, :5] = 9                                                    # beyond the dictionary: NULL
    got = depgraph.dense_pair_counts(codes, [4, 6], [(0, 1), (1, 0)])
    for (x, y), d in zip([(0, 1), (1, 0)], got):
        dx, dy = [4, 6][x], [4, 6][y]
        assert d.dtype == np.int64 and d.shape == (dx + 1, dy + 1) and d.sum() == 200
        np.testing.assert_array_equal(d, domain.Joint.from_bins(codes[x], codes[y], dx, dy).dense())
