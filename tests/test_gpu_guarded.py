"""-m gpu: every kernel family's smallest edge cases once more, in a fresh child process with guard zones around every device buffer
(RGBM_GUARD=1) on poisoned memory (RGBM_POISON=1) -- tests/guarded_runs.py says which tests and why in a child.  A family passes when its
child passes every test, said that both switches were on (the guard after checking itself) and the guard reported no buffer."""
import os
import subprocess
import sys
import time

import pytest

from tests import guarded_runs as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# set when a child timed out, died of a signal or aborted, or reported a HIP fault as an error and went on to exit 1: nothing more goes onto
# the device after a fault or a hang
_a_child_died = []
# the HIP runtime's error texts for a fault of the device (hipGetErrorString), as the library's checks put them into an exception
HIP_FAULTS = ("an illegal memory access was encountered", "unspecified launch failure", "the launch timed out and was terminated",
              "misaligned address", "hardware exception", "device-side assert", "HSA_STATUS_ERROR", "Memory access fault")


@pytest.mark.parametrize("family", list(G.FAMILIES))
def test_family_under_guard_zones_and_poison(family):
    if _a_child_died:
        pytest.fail("not run: an earlier guarded child died (%s)" % _a_child_died[0])
    node_ids, limit_s = G.FAMILIES[family]
    env = dict(os.environ, RGBM_GUARD="1", RGBM_POISON="1", PYTHONUNBUFFERED="1")
    t0 = time.perf_counter()
    try:
        child = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", *node_ids], cwd=ROOT, env=env,
                               timeout=limit_s, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired as e:
        _a_child_died.append("%s: no end after %d s" % (family, limit_s))
        pytest.fail("the guarded child of %r did not end within %d s; its output so far:\n%s" % (family, limit_s, (e.output or b"").decode("utf-8", "replace")))
    wall = time.perf_counter() - t0
    out = child.stdout.decode("utf-8", "replace")
    print("guarded family %s: %d nodes, child wall time %.1f s, exit %d" % (family, len(node_ids), wall, child.returncode))
    if child.returncode < 0 or child.returncode in (134, 139):
        _a_child_died.append("%s: exit %d" % (family, child.returncode))
    elif any(text in out for text in HIP_FAULTS):
        _a_child_died.append("%s: a HIP fault in its output, exit %d" % (family, child.returncode))
    reports = G.guard_reports(out)
    assert child.returncode == 0 and G.banners(out) and not reports and G.passed_count(out) == len(node_ids), (
        "guarded child of %r: exit %d, both banners with self-check ok: %s, %d guard report(s), %d of %d tests passed\n%s\n---- the child's output\n%s"
        % (family, child.returncode, G.banners(out), len(reports), G.passed_count(out), len(node_ids), "\n".join(reports), out))
