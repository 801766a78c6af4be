"""What every tests/golden/bench_*_digests.json MUST hold -- one table for tests/test_gpu_bench_shapes.py (-m gpu: asserted before any
training starts) and tests/test_golden_manifest.py (CPU suite: a shrunken or stale file fails on a machine without a GPU).

The digest tests used to iterate whatever keys a file held, so a regeneration that dropped the K = 24 target of the 12.5M x 32 shard
left its test green on the binary target alone.  A target listed here and absent from the file is a FAILURE -- never a skip, never
fewer cases.  Every file is written by tests/golden/make_bench_job_golden.py from the CPU oracle, never from the HIP library."""
import json
import os

from repair.synth import CARDS

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENERATOR = "tests/golden/make_bench_job_golden.py"


def _t(K, digests, exact=True):
    return {"K": K, "digests": digests, "exact": exact}


# file -> the table it was drawn from (the file's "table" entry, verbatim), its "iters", and per target: K, the digest count, and whether
# that count is exact or a lower bound.  draw_rows: the table is cheap enough to draw in the CPU suite (train_rows and K checked against it).
EXPECTED = {
    # BASELINE configs[2], the benchmarked job: all 16 targets, >= 60 iterations each, the four cheap ones for all 300 of the reference's job
    "bench_job_digests.json": {
        "table": {"rows": 10_000_000, "cols": 16, "seed": 42, "null_ratio": 0.01}, "iters": 60, "draw_rows": True,
        "targets": {"c%d" % c: (_t(CARDS[c % len(CARDS)], 300) if c in (0, 11, 1, 12) else _t(CARDS[c % len(CARDS)], 60, exact=False)) for c in range(16)},
    },
    # one GPU's row shard of BASELINE configs[3]: two 16-feature chunks, the binary and the K = 24 target, 30 iterations
    "bench_shard_digests.json": {
        "table": {"rows": 12_500_000, "cols": 32, "seed": 43, "null_ratio": 0.01}, "iters": 30, "draw_rows": True,
        "targets": {"c0": _t(2, 30), "c7": _t(24, 30)},
    },
    # the WHOLE table of BASELINE configs[3] (bench.py --config 100m32), two chunks: the binary and the K = 3 target, 5 iterations
    "bench_whole_digests.json": {
        "table": {"rows": 100_000_000, "cols": 32, "seed": 43, "null_ratio": 0.01, "generator": "make_table_parallel"}, "iters": 5, "draw_rows": False,
        "targets": {"c0": _t(2, 5), "c1": _t(3, 5)},
    },
    # K x n_train above 2^31 on a two-chunk table: 35M x 32, the K = 64 target, 2 iterations (the second one's gradients come from updated scores)
    "bench_big_index_digests.json": {
        "table": {"rows": 35_000_000, "cols": 32, "seed": 43, "null_ratio": 0.01}, "iters": 2, "draw_rows": False,
        "targets": {"c10": _t(64, 2)}, "min_elements": 2 ** 31,          # K * train_rows must EXCEED this
    },
}


def load(name):
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        return json.load(f)


def check(name, gold, numerics_version):
    """Asserts that `gold` (the parsed file `name`) holds exactly the expected table, targets, K values and digest counts, for the numerics
    version given.  Returns {target column: number of digests} in the file's order."""
    exp = EXPECTED[name]
    assert gold.get("generator") == GENERATOR, "%s: written by %r, not by %s" % (name, gold.get("generator"), GENERATOR)
    assert gold.get("numerics_version") == numerics_version, \
        "%s: numerics version %r, the library / generator is at %r: regenerate it (%s)" % (name, gold.get("numerics_version"), numerics_version, GENERATOR)
    assert gold.get("table") == exp["table"], "%s: table %r, expected %r" % (name, gold.get("table"), exp["table"])
    assert gold.get("iters") == exp["iters"], "%s: iters %r, expected %r" % (name, gold.get("iters"), exp["iters"])
    assert set(gold["targets"]) == set(exp["targets"]), "%s: holds targets %s, expected exactly %s (missing: %s)" % (
        name, sorted(gold["targets"]), sorted(exp["targets"]), sorted(set(exp["targets"]) - set(gold["targets"])))
    counts = {}
    for key, e in exp["targets"].items():
        g = gold["targets"][key]
        assert g["K"] == e["K"], "%s %s: K = %r, expected %d" % (name, key, g["K"], e["K"])
        n = len(g["digests"])
        assert (n == e["digests"]) if e["exact"] else (n >= e["digests"]), \
            "%s %s: %d digests, expected %s%d" % (name, key, n, "" if e["exact"] else "at least ", e["digests"])
        assert n >= exp["iters"], "%s %s: %d digests for a file of %d iterations" % (name, key, n, exp["iters"])
        if "min_elements" in exp:
            assert g["K"] * g["train_rows"] > exp["min_elements"], "%s %s: K x train_rows = %d does not exceed %d" % (name, key, g["K"] * g["train_rows"], exp["min_elements"])
        counts[int(key[1:])] = n
    return counts
