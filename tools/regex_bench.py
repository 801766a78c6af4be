"""Regex-structure repair of a pool of distinct strings: `HipEngine.regex_structure` (rgbm_regex_structure, csrc/rgbm_regex.hip) -- wall
clock with packing the strings into code points, the copies and the decoding of the repaired strings included, and the library call alone
on the packed pool -- against the statement `repair.regex_structure.repair_values` in Python, which is what a CPU engine runs.  Pools of
10^5 and 10^6 distinct strings of 8..40 code points for `^[0-9]{1,3} patients$`: a third fits the structure, a third fails at `^`, a third
at `$`.  The two results are compared for equality before any time is reported.

    python tools/regex_bench.py [--sizes 100000,1000000] [--reps 3] [--out profiles/regex_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N                                                   # noqa: E402
from repair.engine import HipEngine                                               # noqa: E402
from repair.regex_structure import parse, program_arrays, repair_values           # noqa: E402

PATTERN = "^[0-9]{1,3} patients$"


def pool(n):
    out = []
    for i in range(n):
        tag = np.base_repr(i, 36).lower()
        if i % 3 == 0:
            out.append("%d %s" % (i % 1000, tag.rjust(7, "_")))                   # 1..3 digits, a blank and 7 code points: fits
        elif i % 3 == 1:
            out.append("x%d patients %s" % (i % 1000, tag))                       # no digit at the start
        else:
            out.append("%d patients of ward %s" % (i % 1000, tag))                # more than nine code points after the digits
    assert len(set(out)) == n and 8 <= min(map(len, out)) and max(map(len, out)) <= 40
    return out


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = HipEngine(0)
    program = parse(PATTERN)
    arrays = program_arrays(program)
    res = dict(pattern=PATTERN, pools=[])
    for n in (int(x) for x in a.sizes.split(",")):
        strings = pool(n)
        t = time.perf_counter()
        want = repair_values(program, strings)
        statement = time.perf_counter() - t
        best, med, got = timed(lambda: eng.regex_structure(program, strings), a.reps)
        assert got == want, "the device result differs from the statement"
        cp, off = N.pack_code_points(strings)
        call_best, call_med, raw = timed(lambda: N.regex_structure_raw(arrays["segs"], arrays["anchors"], arrays["const_cp"], cp, off), a.reps)
        row = dict(strings=n, code_points=int(off[-1]), repaired=int(raw[3][3]), routes=raw[3][:3].tolist(),
                   statement_ms=statement * 1e3, statement_runs=1, engine_ms_best=best * 1e3, engine_ms_median=med * 1e3,
                   library_call_ms_best=call_best * 1e3, library_call_ms_median=call_med * 1e3, speedup_engine_vs_statement=statement / best)
        res["pools"].append(row)
        print(json.dumps(row), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
