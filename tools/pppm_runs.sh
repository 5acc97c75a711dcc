#!/bin/bash
# PPPM at full size next to the Ewald sum: bench lines and kernel tables (run on the GPU box; output under $TOOLS_OUT/)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
set -o pipefail
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
TAG=${1:-r02_k}
C=$TOOLS_OUT/equil_pe10k.npz
for ks in pppm ewald; do
  python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --equil-cache $C --kspace $ks 2>$TOOLS_OUT/${ks}_bench.err > $TOOLS_OUT/${TAG}_bench_576sims_${ks}.json || exit 1
  python -c "
import sys,json
d=json.loads(open('$TOOLS_OUT/${TAG}_bench_576sims_${ks}.json').read()); print('$ks', round(d['value'],1), round(d['ms_per_step'],1), d['config']['stress_zz_checksum_Pa'])"
  rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/pp_prof -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --equil-cache $C --kspace $ks > $TOOLS_OUT/pp_prof.log 2>&1 || exit 1
  python tools/kernel_table.py $TOOLS_OUT/pp_prof > $TOOLS_OUT/${TAG}_kernel_table_bench_576sims_${ks}.txt
  python tools/kernel_gaps.py $TOOLS_OUT/pp_prof > $TOOLS_OUT/${TAG}_kernel_gaps_576sims_${ks}.txt; cat $TOOLS_OUT/${TAG}_kernel_gaps_576sims_${ks}.txt
  rm -rf $TOOLS_OUT/pp_prof
  head -12 $TOOLS_OUT/${TAG}_kernel_table_bench_576sims_${ks}.txt
done
