"""Record tests/golden/repair_frame_pinned.json: what `repair_frame(.., want_details=True)` returns for the cases of
tests/repair_frame_pinned_cases.py on the CPU engines of the test suite.

    python tools/record_repair_frame_pinned.py [--out tests/golden/repair_frame_pinned.json]

Run it on the commit whose behaviour is to be pinned (the parent of a host-side refactor), never on the code under test."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "spark-data-repair-plugin_amd"))
os.environ.setdefault("REPAIR_TESTING", "1")
from tests import repair_frame_pinned_cases as C

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "repair_frame_pinned.json"))
a = ap.parse_args()
try:
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
except Exception:  # noqa: BLE001
    commit = None
out = dict(recorded_at_commit=commit, cases={})
for case in C.CASES:
    frame, details = C.run(case)
    out["cases"][case.__name__] = C.snapshot(frame, details)
    print("%-40s %3d cells, details %s" % (case.__name__, len(frame), sorted(k for k in details if k not in ("times", "stats", "models", "columns"))))
with open(a.out, "w", encoding="utf-8") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))
