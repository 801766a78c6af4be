"""Code size / register / scratch / LDS / occupancy table of the library's device functions, one line each
(hipcc -Rpass-analysis=kernel-resource-usage on the device code object of a source, sizes from its FUNC symbols).
    python tools/kernel_resources.py [--src rgbm_prep.hip]... [--csrc DIR] [--sorted] [name filter [hipcc flags]]
Cross-compiles for gfx950 with the Makefile's code-generation flags; no GPU needed.  Every csrc/*.hip unless --src names some; --csrc: another
checkout's csrc directory; --sorted: one list sorted by name without the per-file headings (two checkouts' lists then diff line by line -- a kernel
of a shared header shows once per file that launches it)."""
import glob, re, subprocess, sys, os, tempfile
argv = sys.argv[1:]
sources = []
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(ROOT, "spark-data-repair-plugin_amd", "csrc")
while "--src" in argv:
    i = argv.index("--src"); sources.append(argv[i + 1]); del argv[i:i + 2]
if "--csrc" in argv:
    i = argv.index("--csrc"); csrc = os.path.abspath(argv[i + 1]); del argv[i:i + 2]
one_list = "--sorted" in argv
if one_list:
    argv.remove("--sorted")
flt = argv[0] if argv else ""
if not sources:
    sources = sorted(os.path.basename(p) for p in glob.glob(os.path.join(csrc, "*.hip")))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "")) for n in out]


def table(source):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "device.co")
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden", "--offload-arch=gfx950",
               "--cuda-device-only", "--no-gpu-bundle-output", "-c", source, "-o", obj, "-Rpass-analysis=kernel-resource-usage"] + argv[1:]
        out = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True).stderr
        if not os.path.exists(obj):
            sys.exit(out)
        syms = subprocess.run(["/opt/rocm/llvm/bin/llvm-readelf", "-sW", obj], capture_output=True, text=True).stdout
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    cur = None; rows = []
    for line in out.splitlines():
        m = re.search(r"remark: +Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1), "code": size.get(m.group(1), -1)}; rows.append(cur); continue
        m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    for r, name in zip(rows, demangle([r["mangled"] for r in rows])):
        r["name"] = name
    return [r for r in rows if flt in r["name"]]


def fmt(r):
    return "%-70s %7d %5d %5d %7d %7d %7d %6d %4d" % (r["name"][:70], r["code"], r.get("VGPRs", -1), r.get("TotalSGPRs", -1), r.get("VGPRs Spill", -1),
                                                     r.get("SGPRs Spill", -1), r.get("ScratchSize", -1), r.get("LDS Size", -1), r.get("Occupancy", -1))


print("%-70s %7s %5s %5s %7s %7s %7s %6s %4s" % ("kernel", "code B", "VGPR", "SGPR", "vspill", "sspill", "scratch", "LDS", "occ"))
lines = []
for source in sources:
    rows = table(source)
    if one_list:
        lines += [fmt(r) for r in rows]
    elif rows:
        print("# %s: %d device functions" % (source, len(rows)))
        print("\n".join(fmt(r) for r in rows))
if one_list:
    print("\n".join(sorted(lines)))
