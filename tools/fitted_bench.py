"""Fit once, repair later tables, measured: nothing here is gated.

  * a FIT run (`model.fitted.keep`) and an APPLY run (`setFittedModels`) of one synthetic frame (default 1M rows x 16 string columns, 1 %
    NULLs, NULL detector) through `RepairModel.run()`: wall clock of each, the pipeline's own phase times, and that both frames are equal;
  * `Table.recode` (rgbm_table_recode) on the bench table shape (default 10M x 16 int32 codes) with every LUT staged in LDS, and with the
    first column's LUT (a dictionary declared 100 003 codes wide) gathered from global memory: wall clock per call -- LUT upload, the
    allocation of the result from the library's pool, the kernel, the copy of the counts and the synchronise included --, warm, median /
    min / max of `--reps` calls after one warm-up call; every result is compared with the numpy statement first;
  * the yardstick of a streaming pass: a device-to-device copy of the same bytes (`hipMemcpy` between two resident buffers,
    synchronised), timed the same way in the same process.  recode / copy is the ratio reported.

    python tools/fitted_bench.py [--rows 10000000] [--cols 16] [--fit-rows 1000000] [--estimators 30] [--reps 9] [--no-run] [--out profiles/FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "spark-data-repair-plugin_amd")]

from repair import _native as N          # noqa: E402
from repair import recode_codes          # noqa: E402
from repair.synth import make_table      # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); out = fn(); ts.append(time.perf_counter() - t)
    return dict(ms_median=float(np.median(ts)) * 1e3, ms_min=min(ts) * 1e3, ms_max=max(ts) * 1e3, reps=reps), out


def recode_part(n, c, reps):
    codes, _, cards = make_table(n, c, seed=7, null_ratio=0.01)
    rng = np.random.default_rng(11)
    res = dict(rows=n, cols=c, n_codes=[int(v) for v in cards], limits=N.recode_limits(), bytes_read=4 * n * c, bytes_written=4 * n * c)
    try:                                             # (the runtime librepairgbm.so is linked against: the same device, the same process)
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")

    def chk(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d)" % (what, rc))
    nbytes = C.c_size_t(4 * n * c)
    src, dst = C.c_void_p(), C.c_void_p()
    chk(hip.hipMalloc(C.byref(src), nbytes), "hipMalloc"); chk(hip.hipMalloc(C.byref(dst), nbytes), "hipMalloc")
    chk(hip.hipMemcpy(src, codes.ctypes.data_as(C.c_void_p), nbytes, C.c_int(1)), "hipMemcpy host to device")

    def copy():
        chk(hip.hipMemcpy(dst, src, nbytes, C.c_int(3)), "hipMemcpy device to device"); chk(hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    res["copy"], _ = timed(copy, reps)
    res["copy"]["GBps_read_plus_write"] = 8.0 * n * c / res["copy"]["ms_median"] / 1e6
    back = np.empty_like(codes)
    chk(hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), dst, nbytes, C.c_int(2)), "hipMemcpy device to host")
    assert np.array_equal(back, codes)
    del back
    chk(hip.hipFree(src), "hipFree"); chk(hip.hipFree(dst), "hipFree")
    print(json.dumps({"copy": res["copy"]}), flush=True)
    for name, wide0 in (("lds_luts", None), ("one_global_lut", 100003)):
        n_codes = cards.copy()
        if wide0:
            n_codes[0] = wide0
            codes = codes.copy()
            codes[0] = rng.integers(-1, wide0, n).astype(np.int32)      # the gather spans the whole LUT
        luts = [rng.integers(-1, int(k), int(k)).astype(np.int32) for k in n_codes]
        tab = N.Table(codes, n_codes)

        def call():
            out, un = tab.recode(luts, n_codes)
            out.close()
            return un
        out, un = tab.recode(luts, n_codes)
        want, want_un = recode_codes.recode(codes, n_codes, luts, n_codes)
        assert np.array_equal(un, want_un) and all(np.array_equal(out.read_column(j), want[j]) for j in range(c)), name
        out.close()
        tm, _ = timed(call, reps)
        tm.update(routes=tab.recode_report()["routes"], GBps_read_plus_write=8.0 * n * c / tm["ms_median"] / 1e6,
                  ratio_to_copy=tm["ms_median"] / res["copy"]["ms_median"], unmapped_cells=int(un.sum()))
        res[name] = tm
        tab.close()
        print(json.dumps({name: tm}), flush=True)
    return res


def run_part(n, c, estimators):
    import pandas as pd
    from repair.errors import NullErrorDetector
    from repair.model import RepairModel
    dirty, _, cards = make_table(n, c, seed=13, null_ratio=0.01)
    df = pd.DataFrame({"tid": np.arange(n)})
    for j in range(c):
        v = np.array(["c%d_v%02d" % (j, k) for k in range(int(cards[j]))], object)[np.maximum(dirty[j], 0)]
        v[dirty[j] < 0] = None
        df["c%d" % j] = v

    def model():
        m = RepairModel().setInput(df).setRowId("tid").setErrorDetectors([NullErrorDetector()])
        for k, v in {"model.hp.max_evals": "1", "model.lgb.n_estimators": str(estimators), "model.max_training_row_num": str(n)}.items():
            m = m.option(k, v)
        return m
    m = model().option("model.fitted.keep", "true")
    t = time.perf_counter(); out = m.run(); fit_s = time.perf_counter() - t
    fit = m.fittedModels()
    fit_times = dict(m._last_resident_info["times"])
    m2 = model().setFittedModels(fit)
    t = time.perf_counter(); again = m2.run(); apply_s = time.perf_counter() - t
    key = ["tid", "attribute"]
    same = out.sort_values(key).reset_index(drop=True).equals(again.sort_values(key).reset_index(drop=True))
    return dict(rows=n, cols=c, n_estimators=estimators, repaired_cells=int(len(out)), fit_run_s=fit_s, apply_run_s=apply_s, frames_equal=bool(same),
                fit_times=fit_times, apply_times=dict(m2._last_resident_info["times"]),
                apply_fitted=dict(recode_seconds=m2._last_resident_info["fitted"]["recode_seconds"],
                                  unmapped=int(sum(m2._last_resident_info["fitted"]["unmapped"].values()))),
                blob_bytes=int(sum(len(fit.targets[t]["blob"]) for t in fit.chain)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--cols", type=int, default=16)
    ap.add_argument("--fit-rows", type=int, default=1_000_000)
    ap.add_argument("--estimators", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-run", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if N.device_count() < 1:
        raise SystemExit("fitted_bench.py measures on a HIP device; none found")
    res = dict(recode=recode_part(a.rows, a.cols, a.reps))
    if not a.no_run:
        res["run"] = run_part(a.fit_rows, a.cols, a.estimators)
        print(json.dumps(res["run"]), flush=True)
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    else:
        print(txt)


if __name__ == "__main__":
    main()
