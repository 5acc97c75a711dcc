#!/bin/bash
# kernel table + gaps of a single replica (BASELINE config 2) (usage on the GPU box: tools/r05_1_prof.sh <tag>)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
T=${1:-r05_x}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/${T}_prof1 -- python bench.py --full --sims 1 --steps 10 --warmup 4 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > $TOOLS_OUT/${T}_prof1_bench.json.log 2>&1
python tools/kernel_table.py $TOOLS_OUT/${T}_prof1 > $TOOLS_OUT/${T}_kernel_table_bench_1sim.txt
python tools/kernel_gaps.py $TOOLS_OUT/${T}_prof1 16 > $TOOLS_OUT/${T}_kernel_gaps_bench_1sim.txt
rm -rf $TOOLS_OUT/${T}_prof1
head -24 $TOOLS_OUT/${T}_kernel_table_bench_1sim.txt; head -14 $TOOLS_OUT/${T}_kernel_gaps_bench_1sim.txt
