#!/bin/bash
# SQ counters of the vertex kernel for one workload (one counter per rocprofv3 pass; run on the GPU box from the repo root):
#   bash tools/sq_counters.sh <workload> [steps]   ->  gpurun_out/sq_<workload>.json
# Each pass has a time limit of its own and the script ends at the first pass that fails or runs into it: nothing is started on a card
# after a pass went wrong on it.  The limit: a --loop-only bench.py run of a few steps (no CPU reference) takes well under a minute, the
# 100k lattice included; rocprofv3's start-up and output come on top.  600 s is a ceiling for a loaded host, not an expectation.
set -eo pipefail
wl=${1:?workload}; steps=${2:-5}
O=gpurun_out/sq_$wl; mkdir -p $O
cd /tmp 2>/dev/null; export TMPDIR=/tmp; cd - >/dev/null
args=""
for c in SQ_WAVES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_WAVE_CYCLES SQ_INST_CYCLES_VMEM SQ_LDS_BANK_CONFLICT; do
  timeout -k 10 600 rocprofv3 --pmc $c --output-format csv -d $O/$c -- python3 bench.py --full --loop-only --workload $wl --steps $steps --warmup 2 > $O/$c.log 2>&1
  args="$args $c=$O/$c"
done
python3 tools/pmc_summary.py gpurun_out/sq_$wl.json $args
find $O -name "*.db" -delete
