#!/bin/bash
# Tiled PPPM kernels against the kernels without LDS (scema_md_pppm_tiling mode 1 / 0 alternating in one process) on charge-scaled PE-10k:
# 24 x 24 x 20 (interpolation tiled), 30 x 30 x 30 (both kernels tiled) and the unchanged 12 x 12 x 12 as a control, at 72 and 576 replicas,
# then the per-kernel table of the 72-replica runs per mode (a profiled run of its own).  usage, on the GPU box from the repo root:
#   tools/pppm_tiled_ab.sh [tag]      logs -> $TOOLS_OUT/<tag>_*   (copy what is kept to profiles/)
TOOLS_OUT=${TOOLS_OUT:-tools_out}
TAG=${1:-pppm_tiled}
SIZES=${SIZES:-72 576}
set -o pipefail
mkdir -p $TOOLS_OUT
run() {   # name, charge scale, accuracy
  for N in $SIZES; do
    timeout -k 10 400 python tools/pppm_tiled_ab.py --sims $N --charge-scale $2 --accuracy $3 > $TOOLS_OUT/${TAG}_$1_${N}sims.json.log 2> $TOOLS_OUT/${TAG}_$1_${N}sims.err || { tail -5 $TOOLS_OUT/${TAG}_$1_${N}sims.err; return 1; }
    python -c "
import json; d = json.loads(open('$TOOLS_OUT/${TAG}_$1_${N}sims.json.log').read().splitlines()[-1])
print('$1', d['sims'], 'replicas, mesh', d['grid'], 'ms per update mode 0 / 1:', round(d['mode0_ms']['mean'], 1), '/', round(d['mode1_ms']['mean'], 1), 'gain %.1f %%' % (100 * d['tiled_gain']), 'mode-0 spread %.1f %%' % (100 * d['mode0_spread_between_runs']), 'paths', d['runs'][1]['paths']['spread'], d['runs'][1]['paths']['force'])"
  done
}
run 24x24x20 4 1e-4 && run 30x30x30 3 1e-5 && run 12x12x12 1 1e-4 || exit 1
for W in "24x24x20 4 1e-4" "30x30x30 3 1e-5"; do
  set -- $W
  for MODE in 1 0; do
    timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/${TAG}_prof -- python tools/pppm_tiled_ab.py --sims 72 --charge-scale $2 --accuracy $3 --only $MODE --updates 1 > $TOOLS_OUT/${TAG}_prof.log 2>&1 || { tail -5 $TOOLS_OUT/${TAG}_prof.log; exit 1; }
    python tools/kernel_table.py $TOOLS_OUT/${TAG}_prof > $TOOLS_OUT/${TAG}_kernel_table_$1_72sims_mode$MODE.txt
    rm -rf $TOOLS_OUT/${TAG}_prof
    grep -i "pppm\|k_pair" $TOOLS_OUT/${TAG}_kernel_table_$1_72sims_mode$MODE.txt | head -8
  done
done
