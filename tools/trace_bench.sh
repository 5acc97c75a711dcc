#!/bin/bash
# usage (GPU box, repo root): tools/trace_bench.sh <tag> [extra bench args] -- rocprofv3 kernel trace of the default bench on a cached equilibrated state
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
TAG=$1; shift
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
[ -f $C ] || python bench.py --full --sims 1 --steps 1 --warmup 0 --nss 10 --no-cpu-baseline --equil-cache $C > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/trace_$TAG -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --equil-cache $C "$@" > $TOOLS_OUT/trace_$TAG.log 2>&1
tail -1 $TOOLS_OUT/trace_$TAG.log | cut -c1-300
python tools/kernel_table.py $TOOLS_OUT/trace_$TAG | tee $TOOLS_OUT/trace_$TAG.table.txt
cp $TOOLS_OUT/trace_$TAG/*/*kernel_stats.csv $TOOLS_OUT/trace_${TAG}_kernel_stats.csv
rm -rf $TOOLS_OUT/trace_$TAG
