#!/usr/bin/env python3
"""Summary of an A/B written by tools/gpu_ab_plain.sh: per workload and arm the rounds, median and max - min of kernel_ms_per_rank
and of value, the median gain of `new` over `parent`, and whether it exceeds three times the larger spread.
Usage: tools/ab_summary.py <ab.txt> [base arm] [new arm]"""
import statistics
import sys

base = sys.argv[2] if len(sys.argv) > 2 else "parent"
new = sys.argv[3] if len(sys.argv) > 3 else "new"
runs = {}
for line in open(sys.argv[1]):
    f = line.split()
    if len(f) >= 10 and f[2] == "round" and f[4] == "kernel_ms_per_rank":
        runs.setdefault(f[1], {}).setdefault(f[0], []).append((float(f[5]), float(f[7]), f[9]))
for wl, arms in runs.items():
    print(wl)
    stat = {}
    for arm, r in sorted(arms.items()):
        k, v = [x[0] for x in r], [x[1] for x in r]
        stat[arm] = (statistics.median(k), max(k) - min(k), statistics.median(v), max(v) - min(v))
        print("  %-8s kernel ms %s  median %.4f  max - min %.4f | value MB/s %s  median %.1f  max - min %.1f | bit_exact %s"
              % (arm, " ".join("%.4f" % x for x in k), stat[arm][0], stat[arm][1], " ".join("%.1f" % x for x in v), stat[arm][2], stat[arm][3],
                 all(x[2] == "True" for x in r)))
    if base in stat and new in stat:
        gk = stat[base][0] - stat[new][0]
        sk = max(stat[base][1], stat[new][1])
        gv = stat[new][2] - stat[base][2]
        sv = max(stat[base][3], stat[new][3])
        print("  gain: kernel %.4f ms (%.2f %%), 3 x spread %.4f -> %s | value %+.1f MB/s (%.2f %%), 3 x spread %.1f -> %s"
              % (gk, 100 * gk / stat[base][0], 3 * sk, "a gain" if gk > 3 * sk else "slower" if -gk > sk else "inside the spread",
                 gv, 100 * gv / stat[base][2], 3 * sv, "a gain" if gv > 3 * sv else "slower" if -gv > sv else "inside the spread"))
