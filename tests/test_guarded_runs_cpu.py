"""tests/guarded_runs.py against the suite as it is: every listed node id is a test that exists (a renamed test or parameter must not
quietly shrink a family), every GPU test file and test function is in a family or excluded for one of the agreed reasons, and the two
readers of a child's output read the library's lines as it prints them."""
import glob
import os
import re
import subprocess
import sys

import pytest

from tests import guarded_runs as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAY_BE_EXCLUDED = {"test_gpu_bench_shapes.py", "test_gpu_rowshard.py", "test_gpu_shard_job.py", "test_gpu_fusion.py"}
GUARDED = "test_gpu_guarded.py"       # the runs themselves


def _collect(args):
    python = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])     # the child sees the packages this process sees
    out = subprocess.run([*python, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", *args], cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT).stdout.decode("utf-8", "replace")
    return [line.strip() for line in out.splitlines() if line.startswith("tests/") and "::" in line], out


def _gpu_files():
    return sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")) if os.path.basename(p) != GUARDED)


def _file_of(node_id):
    return node_id.split("::")[0].split("/")[-1]


@pytest.fixture(scope="module")
def functions_of_included_files():
    """file -> the test functions pytest collects from it"""
    files = [f for f in _gpu_files() if f not in G.EXCLUDED_FILES]
    ids, out = _collect(["tests/" + f for f in files])
    assert ids, out
    fns = {f: set() for f in files}
    for i in ids:
        fns[_file_of(i)].add(i.split("[")[0])
    return fns


def test_every_listed_node_id_is_collected_and_nothing_else():
    listed = [i for ids, _ in G.FAMILIES.values() for i in ids]
    assert len(listed) == len(set(listed)), "a node id is listed twice"
    got, out = _collect(listed)
    assert sorted(got) == sorted(listed), "not collected: %r\nnot listed: %r\n%s" % (
        sorted(set(listed) - set(got))[:10], sorted(set(got) - set(listed))[:10], out[-2000:])


def test_every_listed_file_is_gpu_marked():
    for f in sorted({_file_of(i) for ids, _ in G.FAMILIES.values() for i in ids}):
        src = open(os.path.join(ROOT, "tests", f)).read()
        assert re.search(r"^pytestmark = pytest\.mark\.gpu\b", src, re.M), f


def test_limits_are_whole_tens_of_seconds():
    for family, (ids, limit_s) in G.FAMILIES.items():
        assert ids and isinstance(limit_s, int) and limit_s >= 10 and limit_s % 10 == 0, family


def test_every_gpu_file_is_in_a_family_or_one_of_the_four():
    assert set(G.EXCLUDED_FILES) <= MAY_BE_EXCLUDED and all(G.EXCLUDED_FILES.values())
    in_families = {_file_of(i) for ids, _ in G.FAMILIES.values() for i in ids}
    assert not in_families & set(G.EXCLUDED_FILES)
    for f in _gpu_files():
        assert (f in in_families) != (f in G.EXCLUDED_FILES), "%s is in no family and not among the excluded files" % f
    for f in G.EXCLUDED_FILES:
        assert f in _gpu_files(), "%s no longer exists" % f


def test_functions_are_left_out_by_name_for_an_agreed_reason_and_fewer_than_one_in_five(functions_of_included_files):
    in_families = {i.split("[")[0] for ids, _ in G.FAMILIES.values() for i in ids}
    assert set(G.EXCLUDED_TESTS.values()) <= set(G.EXCLUSION_REASONS)
    assert not in_families & set(G.EXCLUDED_TESTS), "a test is both run and excluded"
    every = set().union(*functions_of_included_files.values())
    assert set(G.EXCLUDED_TESTS) <= every, "an excluded test does not exist: %r" % sorted(set(G.EXCLUDED_TESTS) - every)
    for f, fns in functions_of_included_files.items():
        left_out = fns - in_families
        assert left_out <= set(G.EXCLUDED_TESTS), "%s: in no family and not excluded: %r" % (f, sorted(left_out - set(G.EXCLUDED_TESTS)))
        assert 5 * len(left_out) < len(fns), "%s: %d of %d test functions left out" % (f, len(left_out), len(fns))


# the library's lines as csrc/rgbm_runtime.hip prints them
REPORT = ("[rgbm guard] buffer of 520 bytes (block 6291456): 8 byte(s) of the slack + back guard were overwritten, "
          "first at offset 0 from the buffer's end")
FRONT = "[rgbm guard] buffer of 4096 bytes (block 6291456): 4 byte(s) of the front guard were overwritten, first at offset -4 from the buffer's start"
GUARD_ON = "[rgbm guard] on, self-check ok"
POISON_ON = "[rgbm poison] on"
SUMMARY = "36 passed in 4.21s"


def test_guard_reports_reads_the_report_lines():
    clean = "\n".join([GUARD_ON, POISON_ON, "....", SUMMARY])
    assert G.guard_reports(clean) == []
    assert G.guard_reports("") == []
    dirty = "\n".join([GUARD_ON, POISON_ON, ".." + REPORT, FRONT, "..", SUMMARY])      # -s: a report may follow pytest's dots on one line
    assert G.guard_reports(dirty) == [".." + REPORT, FRONT]


def test_banners_needs_both_lines_and_the_self_check():
    assert G.banners("\n".join([POISON_ON, GUARD_ON, SUMMARY]))
    assert G.banners("\n".join(["collected", ".." + GUARD_ON, ".." + POISON_ON]))        # -s: after pytest's dots
    assert not G.banners("")
    assert not G.banners(SUMMARY)
    assert not G.banners(GUARD_ON)
    assert not G.banners(POISON_ON)
    assert not G.banners("\n".join(["[rgbm guard] on", POISON_ON]))                       # on, but the check never checked itself
    assert not G.banners("\n".join(["[rgbm guard] on, self-check failed", POISON_ON]))
    assert not G.banners("\n".join([REPORT, POISON_ON]))                                  # a report is no banner


def test_passed_count_reads_the_summary_line():
    assert G.passed_count("...\n" + SUMMARY + "\n") == 36
    assert G.passed_count("1 failed, 35 passed in 4.21s") == 35
    assert G.passed_count("35 passed, 2 warnings in 14.21s (0:00:14)") == 35
    assert G.passed_count("1 failed in 0.21s") == -1
    assert G.passed_count("") == -1
