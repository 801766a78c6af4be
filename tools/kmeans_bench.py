"""One Lloyd assignment step of the q-gram k-means (`Table.kmeans_assign`, rgbm_table_kmeans_assign, csrc/rgbm_kmeans.hip) on the bench
table shape (synthetic 10M rows x 16 columns, 1 % NULLs), all columns, k = 2, 8, 32, with random P and h of the table's dictionaries --

  * ms per call, best of `--reps` after a warm-up call, and the median: wall clock, the upload of P / h and the copy of counts / sizes
    included (`first` = 0 after the warm-up, so the previous labels are read as in every step but the first);
  * the numpy step (repair.qgram_kmeans.assign_step) on the same arrays (unless --no-host; `--host-rows` of them, scaled to all rows);
  * the stream floor  N * (4 n_cols + 8) B  over the 6.29 TB/s copy ceiling DESIGN.md uses;
  * the share of the call that the copy of `counts` takes: a device-to-host copy of k * d_tot * 8 B timed on its own (hipMemcpy).

The device step is compared with the numpy step on the first `--check-rows` rows (a table of its own) before any time is reported.

    python tools/kmeans_bench.py [--rows 10000000] [--cols 16] [--reps 5] [--out profiles/kmeans_bench.json]

`--bisect`: one pass of a level of the bisecting k-means instead (`Table.kmeans_bisect`, rgbm_table_kmeans_bisect) at m = 1, 4, 32, 512 slots
(`--ms`).  The labels are grown as the loop grows them: a complete binary tree in level order, level l splitting all 2^l nodes of the level
above with random P and h, so at m slots every row belongs to one of the m nodes being split and is scored.  The timed call repeats the
level's pass (the rows carry their children's ids, nothing changes), best of `--reps` after a warm-up call and the median, beside the same
stream floor.  Every pass of the tower is compared with the numpy pass (repair.qgram_bisect.bisect_step) on the first `--check-rows` rows
before any time is reported.  `counter_sweeps`: 1 = the counters of all slots in LDS, n = the pass swept in n windows of slots, 0 = global
counters.  For the k-means step of another build on the same machine:  RGBM_LIB_PATH=<its library> ... --ks 2,8,64 --no-host.

    python tools/kmeans_bench.py --bisect [--ms 1,4,32,512] [--out profiles/kmeans_bisect_bench.json]
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
from repair import qgram_kmeans as Q                                              # noqa: E402
from tests.helpers import csrc_constant                                           # noqa: E402
from tests.synth import make_table                                                # noqa: E402

COPY_CEILING = 6.29e12                       # B/s, DESIGN.md


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return min(ts), float(np.median(ts)), out


def copy_ms(nbytes, reps):
    """A device-to-host copy of nbytes into pageable memory, on its own (hipMemcpy of the runtime the library runs on)."""
    import ctypes as C
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    d, host = C.c_void_p(), np.zeros(max(nbytes // 8, 1), np.int64)
    assert hip.hipMalloc(C.byref(d), C.c_size_t(host.nbytes)) == 0
    try:
        assert hip.hipMemset(d, 0, C.c_size_t(host.nbytes)) == 0 and hip.hipDeviceSynchronize() == 0

        def copy():
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), d, C.c_size_t(host.nbytes), 2) == 0      # 2 = hipMemcpyDeviceToHost
        best, _, _ = timed(copy, reps)
    finally:
        hip.hipFree(d)
    return best * 1e3


def level(m):
    """Level m of a complete binary tree in level order: (slot_of [4m - 1], child [2m]); nodes m-1 .. 2m-2 split into 2m-1 .. 4m-2."""
    child = np.arange(2 * m - 1, 4 * m - 1, dtype=np.int32)
    slot_of = np.full(4 * m - 1, -1, np.int32)
    slot_of[m - 1:2 * m - 1] = np.arange(m)
    slot_of[child] = np.repeat(np.arange(m), 2)
    return slot_of, child


def bisect(a, codes, n_codes, cols, off, d_tot, res):
    from repair import qgram_bisect as QB
    n = codes.shape[1]
    ms = sorted(int(x) for x in a.ms.split(","))
    assert all(m >= 1 and m & (m - 1) == 0 for m in ms), "--ms: powers of two (the levels of a complete tree)"
    bound = {name: csrc_constant(name) for name in ("KB_LDS_P_DOUBLES", "KB_LDS_COUNTERS", "KB_MAX_SWEEPS")}
    res.update(lds_bounds=bound, passes={})
    tab = N.Table(codes, n_codes)
    cm = min(a.check_rows, n)
    sub = np.ascontiguousarray(codes[:, :cm])
    small, ref = N.Table(sub, n_codes), None
    rng = np.random.default_rng(5)
    m = 1
    while m <= ms[-1]:
        slot_of, child = level(m)
        p, h = rng.normal(size=(d_tot, 2 * m)) * 3.0, rng.random(2 * m) * 2.0
        cnt, sz, nch = small.kmeans_bisect(cols, off, slot_of, child, p, h, m == 1)
        ref, c_r, s_r, n_r = QB.bisect_step(sub, n_codes, off, p, h, slot_of, child, ref)
        assert np.array_equal(small.kmeans_read(), ref) and np.array_equal(cnt, c_r) and np.array_equal(sz, s_r) and nch == n_r == cm, m
        cnt, sz, nch = tab.kmeans_bisect(cols, off, slot_of, child, p, h, m == 1)
        assert nch == n and int(sz.sum()) == n, m
        if m in ms:
            best, med, out = timed(lambda: tab.kmeans_bisect(cols, off, slot_of, child, p, h, False), a.reps)
            assert out[2] == 0 and np.array_equal(out[1], sz) and np.array_equal(out[0], cnt)
            cp = copy_ms(2 * m * d_tot * 8, a.reps)
            win = min(m, bound["KB_LDS_COUNTERS"] // (2 * d_tot))            # the library's rule: slots whose counters fit the LDS together
            sweeps = -(-m // win) if win >= 1 else 0
            res["passes"]["m=%d" % m] = dict(ms_best=best * 1e3, ms_median=med * 1e3, ratio_to_stream_floor=best / (res["stream_floor_ms"] * 1e-3),
                                             p_in_lds=(d_tot + 1) * (2 * m | 1) <= bound["KB_LDS_P_DOUBLES"],
                                             counter_sweeps=sweeps if sweeps <= bound["KB_MAX_SWEEPS"] else 0, counts_copy_ms=cp,
                                             counts_copy_share=cp / (best * 1e3), smallest_child=int(sz.min()), largest_child=int(sz.max()))
        m *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bisect", action="store_true")
    ap.add_argument("--ms", default="1,4,32,512")
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ks", default="2,8,32")
    ap.add_argument("--check-rows", type=int, default=200_000)
    ap.add_argument("--host-rows", type=int, default=1_000_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, c = a.rows, a.cols
    codes, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    n_codes = np.asarray(cards, np.int32)
    cols = np.arange(c, dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(n_codes[:-1], dtype=np.int64)]).astype(np.int64)
    d_tot = int(n_codes.sum())
    floor = n * (4 * c + 8) / COPY_CEILING
    res = dict(rows=n, cols=c, d_tot=d_tot, stream_floor_ms=floor * 1e3, library="RGBM_LIB_PATH" if os.environ.get("RGBM_LIB_PATH") else "this build")
    if a.bisect:
        bisect(a, codes, n_codes, cols, off, d_tot, res)
        return report(res, a.out)
    bound = {name: csrc_constant(name) for name in ("KM_LDS_P_DOUBLES", "KM_LDS_COUNTERS")}
    res.update(lds_bounds=bound, steps={})
    tab = N.Table(codes, n_codes)
    m = min(a.check_rows, n)
    small = N.Table(np.ascontiguousarray(codes[:, :m]), n_codes)
    rng = np.random.default_rng(5)
    for k in [int(x) for x in a.ks.split(",")]:
        p, h = rng.normal(size=(d_tot, k)) * 3.0, rng.random(k) * 2.0
        cnt, sz, nch = small.kmeans_assign(cols, off, p, h, True)
        a_r, c_r, s_r, n_r = Q.assign_step(np.ascontiguousarray(codes[:, :m]), n_codes, off, p, h, None)
        assert np.array_equal(small.kmeans_read(), a_r) and np.array_equal(cnt, c_r) and np.array_equal(sz, s_r) and nch == n_r, k
        tab.kmeans_assign(cols, off, p, h, True)
        best, med, out = timed(lambda: tab.kmeans_assign(cols, off, p, h, False), a.reps)
        assert out[2] == 0 and int(out[1].sum()) == n
        cp = copy_ms(k * d_tot * 8, a.reps)
        step = dict(ms_best=best * 1e3, ms_median=med * 1e3, ratio_to_stream_floor=best / floor,
                    p_in_lds=(d_tot + 1) * (k | 1) <= bound["KM_LDS_P_DOUBLES"], counters_in_lds=k * d_tot <= bound["KM_LDS_COUNTERS"],
                    counts_copy_ms=cp, counts_copy_share=cp / (best * 1e3))
        if not a.no_host:
            hm = min(a.host_rows, n)
            sub = np.ascontiguousarray(codes[:, :hm])
            hb, _, _ = timed(lambda: Q.assign_step(sub, n_codes, off, p, h, None), 1)
            step.update(numpy_ms=hb * 1e3 * n / hm, numpy_rows_measured=hm, speedup_vs_numpy=hb * n / hm / best)
        res["steps"]["k=%d" % k] = step
    report(res, a.out)


def report(res, out):
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
