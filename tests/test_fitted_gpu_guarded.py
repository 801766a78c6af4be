"""-m gpu: the smallest cases of tests/test_fitted_gpu.py (its GUARDED list: the row edges of `Table.recode` up to 257 on every route, the
refusals) once more, in one fresh child process with guard zones around every device buffer (RGBM_GUARD=1) on poisoned memory
(RGBM_POISON=1), by the rule of tests/test_gpu_guarded.py: the child passes every test, says that both switches were on (the guard after
checking itself) and the guard reports no buffer; after a child that died or reported a HIP fault nothing further is started.  No fault is
provoked: these are passing cases, run again under the library's own guard."""
import os
import subprocess
import sys
import time

import pytest

from tests.guarded_runs import banners, guard_reports, passed_count
from tests.test_fitted_gpu import GUARDED
from tests.test_gpu_guarded import HIP_FAULTS, _a_child_died

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 20          # the child took 3.0 s on the MI355X (42 nodes); five times that, rounded up to whole tens


def test_recode_under_guard_zones_and_poison():
    if _a_child_died:
        pytest.fail("not run: an earlier guarded child died (%s)" % _a_child_died[0])
    env = dict(os.environ, RGBM_GUARD="1", RGBM_POISON="1", PYTHONUNBUFFERED="1")
    t0 = time.perf_counter()
    try:
        child = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", "-p", "no:cacheprovider", *GUARDED], cwd=ROOT, env=env,
                               timeout=LIMIT_S, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    except subprocess.TimeoutExpired as e:
        _a_child_died.append("recode: no end after %d s" % LIMIT_S)
        pytest.fail("the guarded child did not end within %d s; its output so far:\n%s" % (LIMIT_S, (e.output or b"").decode("utf-8", "replace")))
    out = child.stdout.decode("utf-8", "replace")
    print("guarded recode: %d nodes, child wall time %.1f s, exit %d" % (len(GUARDED), time.perf_counter() - t0, child.returncode))
    if child.returncode < 0 or child.returncode in (134, 139):
        _a_child_died.append("recode: exit %d" % child.returncode)
    elif any(text in out for text in HIP_FAULTS):
        _a_child_died.append("recode: a HIP fault in its output, exit %d" % child.returncode)
    reports = guard_reports(out)
    assert child.returncode == 0 and banners(out) and not reports and passed_count(out) == len(GUARDED), (
        "guarded child: exit %d, both banners with self-check ok: %s, %d guard report(s), %d of %d tests passed\n%s\n---- the child's output\n%s"
        % (child.returncode, banners(out), len(reports), passed_count(out), len(GUARDED), "\n".join(reports), out))
