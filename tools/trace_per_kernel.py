"""kernel trace CSV -> per kernel (template arguments dropped): launches, average us, total ms; level-grower kernels first"""
import csv, re, sys
from collections import defaultdict
d = defaultdict(lambda: [0, 0])
for r in csv.DictReader(open(sys.argv[1])):
    n = re.sub(r"\(.*", "", r["Kernel_Name"]); n = re.sub(r"^void ", "", n); n = re.sub(r"<(true|false)>", lambda m: m.group(0), re.sub(r"<[^<>]{12,}>", "<...>", n))
    d[n][0] += 1; d[n][1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
tot = sum(v[1] for v in d.values())
print("%-60s %8s %9s %9s" % ("kernel", "launches", "us each", "total ms"))
for n, (c, t) in sorted(d.items(), key=lambda kv: -kv[1][1]):
    print("%-60s %8d %9.1f %9.2f" % (n[:60], c, t * 1e-3 / c, t * 1e-6))
print("all kernels: %.1f ms" % (tot * 1e-6))
