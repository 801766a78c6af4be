"""Per-launch fixed cost of the level grower's passes from two kernel traces of the same fits at two row counts.
    python tools/level_setup_intercept.py SMALL_kernel_trace.csv SMALL.log BIG_kernel_trace.csv BIG.log ROWS_SMALL ROWS_BIG [--launches]
The traces are `rocprofv3 --kernel-trace` runs of tools/probe.py (one target at a time, RGBM_TIMING=1, RGBM_DISTINCT=0) with the row blocks pinned to
one value (RGBM_MT_BLOCKS / RGBM_LV_BLOCKS), so that the i-th k_level_mt / k_level_root launch of both runs has the same grid and the same class trees
per workgroup and differs in the rows per workgroup only.  With t = a + b * rows the intercept a = (r * t_small - t_big) / (r - 1), r = rows_big /
rows_small, is what a launch costs before its first row and after its last one.  Launches are labelled with the plan lines of the log
("[rgbm] level L launch: ... T t G g gx x ... rot r") and grouped by (kernel, form, class trees per workgroup, routing / later window, level, workgroups).  --launches: instead of the table, one line per group with the
time of every launch in it (us, in launch order): the raw record in a form small enough to keep."""
import csv, re, sys, statistics
from collections import defaultdict


def launches(trace):
    rows = []
    with open(trace) as f:
        for r in csv.DictReader(f):
            n = r["Kernel_Name"]
            if "k_level_mt" in n or "k_level_root" in n:
                rows.append((int(r["Start_Timestamp"]), "root" if "k_level_root" in n else "mt", (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3,
                             int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])))
    rows.sort()
    return rows


def plans(log):
    """[fit] -> list of (level, route, T, G, gx, rot) in launch order"""
    fits, cur = [], None
    for line in open(log, errors="replace"):
        if line.startswith("[rgbm] root:"):
            cur = []; fits.append(cur)
        m = re.match(r"\[rgbm\] level (\d+) launch: chunk \d+ slots (\d+)\.\.(\d+) route (\d) T (\d+) G (\d+) gx (\d+) acc2 (\d) rot (\d)", line)
        if m and cur is not None:
            cur.append(tuple(int(x) for x in m.groups()))
    return fits


def labelled(trace, log):
    ls, fits = launches(trace), plans(log)
    out, i = [], 0
    iters = sum(1 for x in ls if x[1] == "root") // len(fits)       # (the probe runs every fit with the same iteration count)
    for fit in fits:                      # every fit: iterations of (root, the plan's launches)
        n0 = len(out)
        while i < len(ls) and ls[i][1] == "root":
            out.append((("root", 0, 0, 0), ls[i][2], ls[i][3])); i += 1
            for (level, s0, s1, route, T, G, gx, acc2, rot) in fit:
                assert ls[i][1] == "mt" and ls[i][3] == G * gx, (ls[i], G, gx)
                out.append((("mt rot" if rot else "mt rep", T, route, level), ls[i][2], ls[i][3])); i += 1
            if len(out) - n0 == iters * (1 + len(fit)):
                break
    return out


def main():
    ts, ls_, tb, lb, rs, rb = sys.argv[1:7]
    a, b = labelled(ts, ls_), labelled(tb, lb)
    assert len(a) == len(b), (len(a), len(b))
    r = float(rb) / float(rs)
    groups = defaultdict(list)
    for (ka, ta, ga), (kb, tb_, gb) in zip(a, b):
        assert ka == kb and ga == gb
        groups[ka + (ga,)].append((ta, tb_, (r * ta - tb_) / (r - 1.0), ga))
    if "--launches" in sys.argv:
        for k in sorted(groups):
            print("%s T %d route %d level %d workgroups %d | %s rows: %s | %s rows: %s" % (k[0], k[1], k[2], k[3], k[4], rs, " ".join("%.1f" % x[0] for x in groups[k]),
                                                                                           rb, " ".join("%.1f" % x[1] for x in groups[k])))
        return
    print("| kernel | T | route | level | launches | workgroups | t(%s rows) us | t(%s rows) us | intercept us (median) | intercept min..max | share of t small |" % (rs, rb))
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for k in sorted(groups):
        v = groups[k]
        med = statistics.median(x[2] for x in v)
        ms, mb = statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)
        print("| %s | %d | %d | %d | %d | %d | %.1f | %.1f | %.1f | %.1f..%.1f | %.0f %% |" % (k[0], k[1], k[2], k[3], len(v), v[0][3], ms, mb, med, min(x[2] for x in v), max(x[2] for x in v), 100.0 * med / ms))


if __name__ == "__main__":
    main()
