#!/bin/bash
# A/B of plain bench.py runs on one GPU box: every brotli-rs_amd/_ab/libbrx_<name>.so (tools/ab_build.sh) in turn, ROUNDS times,
# interleaved; one line per run: arm, workload, round, kernel_ms_per_rank, value, bit_exact.  Every run has its own time limit and
# the first fault, abort or time-out ends the job.  Summary (median, max - min per arm): tools/ab_summary.py.
# Usage: ROUNDS=3 STEPS=20 WLS="alice29x4096 ..." tools/gpu_ab_plain.sh <out.txt>
set -u
export HSA_ENABLE_IPC_MODE_LEGACY=0
OUT=${1:?output file}
cp brotli-rs_amd/libbrx.so /tmp/libbrx_keep.so || exit 1
trap 'cp /tmp/libbrx_keep.so brotli-rs_amd/libbrx.so' EXIT
for r in $(seq ${ROUNDS:-3}); do
  for so in brotli-rs_amd/_ab/libbrx_*.so; do
    name=${so##*libbrx_}; name=${name%.so}
    cp $so brotli-rs_amd/libbrx.so || exit 1
    for wl in ${WLS:-alice29x4096}; do
      timeout -k 10 ${LIMIT:-240} python bench.py --workload $wl --steps ${STEPS:-20} --warmup ${WARMUP:-3} > /tmp/ab_line.txt 2> /tmp/ab_err.txt
      rc=$?
      if [ $rc -ne 0 ]; then echo "$name $wl round $r: exit status $rc" | tee -a $OUT; tail -5 /tmp/ab_err.txt; exit $rc; fi
      python - $name $wl $r <<'PY' | tee -a $OUT
import json, sys
d = json.loads(open('/tmp/ab_line.txt').read().strip().splitlines()[-1])
print(sys.argv[1], sys.argv[2], "round", sys.argv[3], "kernel_ms_per_rank", d["kernel_ms_per_rank"][0], "value", d["value"], "bit_exact", d["bit_exact"])
PY
    done
  done
done
