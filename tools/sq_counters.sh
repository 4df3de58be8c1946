#!/bin/bash
# SQ counters of the vertex kernel for one workload (one counter per rocprofv3 pass; run on the GPU box from the repo root):
#   bash tools/sq_counters.sh <workload> [steps]   ->  gpurun_out/sq_<workload>.json
set -o pipefail
wl=${1:?workload}; steps=${2:-5}
O=gpurun_out/sq_$wl; mkdir -p $O
cd /tmp 2>/dev/null; export TMPDIR=/tmp; cd - >/dev/null
args=""
for c in SQ_WAVES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_INST_CYCLES_VMEM SQ_LDS_BANK_CONFLICT; do
  rocprofv3 --pmc $c --output-format csv -d $O/$c -- python3 bench.py --full --loop-only --workload $wl --steps $steps --warmup 2 > $O/$c.log 2>&1 || echo "$c failed"
  args="$args $c=$O/$c"
done
python3 tools/pmc_summary.py gpurun_out/sq_$wl.json $args
find $O -name "*.db" -delete
