#!/bin/bash
# kernel table + gaps of one GPU's share of the 8-GPU run (72 replicas) (usage on the GPU box: tools/r05_72_prof.sh <tag>)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
T=${1:-r05_x}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/${T}_prof72 -- python bench.py --full --sims 72 --steps 6 --warmup 4 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > $TOOLS_OUT/${T}_prof72_bench.json.log 2>&1
python tools/kernel_table.py $TOOLS_OUT/${T}_prof72 > $TOOLS_OUT/${T}_kernel_table_bench_72sims.txt
python tools/kernel_gaps.py $TOOLS_OUT/${T}_prof72 16 > $TOOLS_OUT/${T}_kernel_gaps_bench_72sims.txt
rm -rf $TOOLS_OUT/${T}_prof72
head -24 $TOOLS_OUT/${T}_kernel_table_bench_72sims.txt; head -12 $TOOLS_OUT/${T}_kernel_gaps_bench_72sims.txt
