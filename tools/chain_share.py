"""How much of a concurrent run the level grower's chain of small kernels can gate, from a rocprofv3 kernel trace.
    python tools/chain_share.py KERNEL_TRACE.csv [--skip-first FRACTION]
The trace is `rocprofv3 --kernel-trace --output-format csv` of `bench.py --steps N` (six target models in flight, one stream each).
Per stream that ran level passes (one target model's fit, in start order): when it starts and ends, its kernel launches, and the share of its
own time (first kernel start .. last kernel end) spent in pass kernels (k_level_mt, k_level_root, k_level_final, k_grad*), in chain kernels
(every other kernel) and in gaps (no kernel of the stream running).  Over the timed region (from --skip-first of the way through the trace,
default 0.25, so that set-up and warm-up are left out, to the last kernel) it reports the share of wall time in which no pass kernel of ANY
stream is running: the part of the run the chain gates outright.  The chain time that runs beside another target's pass is hidden."""
import csv, sys
from collections import defaultdict

PASS = ("k_level_mt", "k_level_root", "k_level_final", "k_grad")


def main():
    args = sys.argv[1:]
    skip = 0.25
    if "--skip-first" in args:
        i = args.index("--skip-first"); skip = float(args[i + 1]); del args[i:i + 2]
    streams = defaultdict(list)
    with open(args[0]) as f:
        for r in csv.DictReader(f):
            key = r.get("Stream_Id") or r.get("Queue_Id")
            streams[key].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), any(p in r["Kernel_Name"] for p in PASS), r["Kernel_Name"]))
    fits = {k: sorted(v) for k, v in streams.items() if any("k_level_mt" in x[3] or "k_level_root" in x[3] for x in v)}
    if not fits:
        print("no level-grower stream in the trace"); return
    t0 = min(v[0][0] for v in fits.values())
    t1 = max(max(x[1] for x in v) for v in fits.values())
    print("%-8s %10s %10s %8s %7s %7s %7s" % ("stream", "start ms", "end ms", "launches", "pass %", "chain %", "gap %"))
    tot = [0.0, 0.0, 0.0]
    for k, v in sorted(fits.items(), key=lambda kv: kv[1][0][0]):
        a, b = v[0][0], max(x[1] for x in v)
        tp = sum(e - s for s, e, p, _ in v if p); tc = sum(e - s for s, e, p, _ in v if not p)
        busy, end = 0, a
        for s, e, _, _ in v:          # union of the stream's kernels (they do not overlap inside one stream; kept general)
            if e > end:
                busy += e - max(s, end); end = e
        span = max(b - a, 1)
        print("%-8s %10.2f %10.2f %8d %7.1f %7.1f %7.1f" % (k, (a - t0) * 1e-6, (b - t0) * 1e-6, len(v), 100.0 * tp / span, 100.0 * tc / span, 100.0 * (span - busy) / span))
        tot[0] += tp; tot[1] += tc; tot[2] += span - busy
    s_all = sum(tot)
    print("all streams: pass %.1f %%, chain %.1f %%, gaps %.1f %% of the summed stream time (%.1f ms)" % (100 * tot[0] / s_all, 100 * tot[1] / s_all, 100 * tot[2] / s_all, s_all * 1e-6))
    # wall time of the timed region with no pass kernel of any stream running
    w0 = t0 + int((t1 - t0) * skip)
    iv = sorted((max(s, w0), e) for v in fits.values() for s, e, p, _ in v if p and e > w0)
    covered, end = 0, w0
    for s, e in iv:
        if e > end:
            covered += e - max(s, end); end = e
    wall = t1 - w0
    print("timed region %.1f ms: no pass kernel of any stream running in %.1f %% of it (%.1f ms)" % (wall * 1e-6, 100.0 * (wall - covered) / wall, (wall - covered) * 1e-6))


if __name__ == "__main__":
    main()
