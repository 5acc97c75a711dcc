#!/bin/bash
# 72 replicas (one GPU's share of 576 on 8 GPUs): PPPM next to the Ewald sum, kernel tables and idle gaps (on the GPU box)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
TAG=${1:-r02_l}; N=${2:-72}
C=$TOOLS_OUT/equil_pe10k.npz
for ks in pppm ewald; do
  python bench.py --full --sims $N --steps 8 --warmup 2 --no-cpu-baseline --equil-cache $C --kspace $ks 2>/dev/null | python -c "
import sys,json
d=json.loads(sys.stdin.read()); print('$ks', $N, round(d['value'],1), round(d['ms_per_step'],1))" || exit 1
  rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/pp_prof -- python bench.py --full --sims $N --steps 4 --warmup 1 --no-cpu-baseline --equil-cache $C --kspace $ks > $TOOLS_OUT/pp_prof.log 2>&1 || exit 1
  python tools/kernel_table.py $TOOLS_OUT/pp_prof > $TOOLS_OUT/${TAG}_kernel_table_bench_${N}sims_${ks}.txt
  python tools/kernel_gaps.py $TOOLS_OUT/pp_prof 8 > $TOOLS_OUT/${TAG}_kernel_gaps_${N}sims_${ks}.txt; cat $TOOLS_OUT/${TAG}_kernel_gaps_${N}sims_${ks}.txt
  rm -rf $TOOLS_OUT/pp_prof
  head -22 $TOOLS_OUT/${TAG}_kernel_table_bench_${N}sims_${ks}.txt
done
