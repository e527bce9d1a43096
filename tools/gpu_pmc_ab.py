#!/usr/bin/env python3
"""SQ counters of the headline launch for every brotli-rs_amd/_ab/libbrx_<name>.so (tools/ab_build.sh), each in a rocprofv3 run of
its own: `rocprofv3 --kernel-trace --pmc <counters> -- python bench.py --workload W --steps 2 --warmup 1 --verify 0`, nothing else
traced, under `timeout -k 10` (which ends rocprofv3 AND the bench.py under it when the limit passes).
Prints per arm the mean per dispatch of brx_decode_kernel, and the differences between the arms `parent` and `new`.
Run on the GPU box:  python tools/gpu_pmc_ab.py [workload] [counter ...]"""
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "brotli-rs_amd", "libbrx.so")
workload = sys.argv[1] if len(sys.argv) > 1 else "alice29x4096"
counters = sys.argv[2:] or ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_INSTS_SALU", "SQ_BUSY_CYCLES"]
exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
keep = tempfile.mkdtemp(prefix="brx_keep_", dir="/tmp")
shutil.copy2(LIB, os.path.join(keep, "libbrx.so"))
res = {}
try:
    for so in sorted(glob.glob(os.path.join(ROOT, "brotli-rs_amd", "_ab", "libbrx_*.so"))):
        arm = os.path.basename(so)[len("libbrx_"):-3]
        shutil.copy(so, LIB)
        d = tempfile.mkdtemp(prefix="brx_pmc_", dir="/tmp")
        cmd = ["timeout", "-k", "10", "300", exe, "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
               os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", "2", "--warmup", "1", "--verify", "0"]
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        if r.returncode != 0:  # a fault or an abort: nothing more is started on the GPU
            sys.stderr.write(r.stderr.decode(errors="replace")[-2000:])
            sys.exit("rocprofv3 run of arm %s ended with status %d" % (arm, r.returncode))
        tot, launches = dict.fromkeys(counters, 0.0), set()
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                if row["Kernel_Name"].startswith("brx_decode_kernel(") and row["Counter_Name"] in tot:
                    tot[row["Counter_Name"]] += float(row["Counter_Value"])
                    launches.add(row["Dispatch_Id"])
        shutil.rmtree(d, ignore_errors=True)
        if not launches:
            sys.exit("arm %s: no counter rows" % arm)
        res[arm] = {c: tot[c] / len(launches) for c in counters}
        print("%s: %s, %d dispatches of brx_decode_kernel" % (arm, workload, len(launches)))
        for c in counters:
            print("  %-22s %14.0f per dispatch" % (c, res[arm][c]))
        if "SQ_ACTIVE_INST_VALU" in res[arm] and "SQ_INSTS_VALU" in res[arm]:
            print("  %-22s %14.0f" % ("ACTIVE_INST - INSTS", res[arm]["SQ_ACTIVE_INST_VALU"] - res[arm]["SQ_INSTS_VALU"]))
finally:
    shutil.copy2(os.path.join(keep, "libbrx.so"), LIB)
    shutil.rmtree(keep, ignore_errors=True)
if "parent" in res and "new" in res:
    print("new - parent:")
    for c in counters:
        print("  %-22s %+14.0f (%+.2f %%)" % (c, res["new"][c] - res["parent"][c], 100 * (res["new"][c] / res["parent"][c] - 1)))
