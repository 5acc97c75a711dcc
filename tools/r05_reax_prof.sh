#!/bin/bash
# kernel table of the ReaxFF replica set (usage on the GPU box: tools/r05_reax_prof.sh <tag>)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
T=${1:-r05_x}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
mkdir -p $TOOLS_OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/${T}_rprof -- python bench.py --full --force-field reax --steps 4 --warmup 2 --no-cpu-baseline > $TOOLS_OUT/${T}_rprof_bench.json.log 2>&1
cp $TOOLS_OUT/${T}_rprof/*/*kernel_stats.csv $TOOLS_OUT/${T}_kernel_stats_bench_reax_72sims.csv
python tools/kernel_table.py $TOOLS_OUT/${T}_rprof > $TOOLS_OUT/${T}_kernel_table_bench_reax_72sims.txt 2>/dev/null || python tools/kernel_median.py $TOOLS_OUT/${T}_rprof > $TOOLS_OUT/${T}_kernel_table_bench_reax_72sims.txt
python tools/kernel_gaps.py $TOOLS_OUT/${T}_rprof 10 k_rx_hrow > $TOOLS_OUT/${T}_kernel_gaps_bench_reax_72sims.txt
rm -rf $TOOLS_OUT/${T}_rprof
head -12 $TOOLS_OUT/${T}_kernel_table_bench_reax_72sims.txt; head -11 $TOOLS_OUT/${T}_kernel_gaps_bench_reax_72sims.txt
python bench.py --full --force-field reax --steps 6 --warmup 2 --no-cpu-baseline 2>/dev/null | python -c "import sys,json; d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); print('reax', round(d['value'],1), 'evals/s')"
