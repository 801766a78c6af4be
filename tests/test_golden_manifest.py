"""CPU suite: the committed oracle digests of the benchmarked shapes (tests/golden/bench_*_digests.json) hold what the -m gpu tests of
tests/test_gpu_bench_shapes.py say they pin.  Those tests need an MI355X; a regeneration that drops a target, truncates a digest list or
leaves a file on an older numerics version must fail HERE, on any machine (tests/bench_golden_expect.py holds the one table of both)."""
import glob
import importlib.util
import os
import re

import numpy as np
import pytest

from tests import bench_golden_expect as E
from tests.synth import make_table


def _generator():
    spec = importlib.util.spec_from_file_location("make_bench_job_golden", os.path.join(E.GOLDEN_DIR, "make_bench_job_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_digest_file_is_expected_and_every_expected_file_exists():
    have = {os.path.basename(p) for p in glob.glob(os.path.join(E.GOLDEN_DIR, "bench_*_digests.json"))}
    assert have == set(E.EXPECTED), "tests/golden holds %s, tests/bench_golden_expect.py expects %s" % (sorted(have), sorted(E.EXPECTED))


@pytest.mark.parametrize("name", sorted(E.EXPECTED))
def test_digest_file_holds_the_expected_targets_and_counts(name):
    gold = E.load(name)
    counts = E.check(name, gold, _generator().NUMERICS_VERSION)
    assert counts
    for key, g in gold["targets"].items():
        assert all(isinstance(d, str) and re.fullmatch(r"[0-9a-f]{32}", d) for d in g["digests"]), "%s %s: a digest is not 32 hex characters" % (name, key)
        assert g["oracle_seconds"] > 0 and g["threads"] >= 1, "%s %s: no record of the oracle run" % (name, key)
        assert 0 < g["train_rows"] <= gold["table"]["rows"]
        # NULL injection is i.i.d. with the table's null_ratio: the training rows are the rest, to 6 standard deviations (cheap; the drawn check below is exact)
        n, q = gold["table"]["rows"], gold["table"]["null_ratio"]
        assert abs(g["train_rows"] - n * (1.0 - q)) <= 6.0 * (n * q * (1.0 - q)) ** 0.5, "%s %s: train_rows %d is not %d rows less %g NULLs" % (name, key, g["train_rows"], n, q)


@pytest.mark.parametrize("name", sorted(n for n, e in E.EXPECTED.items() if e["draw_rows"]))
def test_train_rows_and_k_are_those_of_the_drawn_table(name):
    """Only where the table is cheap to draw (10M x 16, 12.5M x 32: seconds, 3 GB).  The 35M- and 100M-row tables are not drawn here; the
    -m gpu tests, which draw them anyway, make the same check."""
    gold = E.load(name)
    tb = gold["table"]
    dirty, clean, cards = make_table(tb["rows"], tb["cols"], seed=tb["seed"], null_ratio=tb["null_ratio"])
    del clean
    assert set(gold["targets"]) == set(E.EXPECTED[name]["targets"])
    for key, g in gold["targets"].items():
        t = int(key[1:])
        assert g["K"] == int(cards[t]), "%s %s: K = %d, the table's column has %d codes" % (name, key, g["K"], int(cards[t]))
        assert g["train_rows"] == int(np.count_nonzero(dirty[t] >= 0)), "%s %s: train_rows is not the non-NULL count of the column" % (name, key)
