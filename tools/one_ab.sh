#!/bin/bash
# usage (on the GPU box): tools/one_ab.sh  -- single replica and the headline batch under the profiler: launches and kernel time per step
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
python bench.py --full --sims 1 --steps 1 --warmup 0 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/one_prof -- python bench.py --full --sims 1 --steps 6 --warmup 2 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > $TOOLS_OUT/one.json.log 2>&1
echo "== 1 replica: $(grep '^{' $TOOLS_OUT/one.json.log | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(round(d["value"],2), "evals/s", round(d["ms_per_step"],3), "ms per update")')"
python tools/kernel_table.py $TOOLS_OUT/one_prof | head -24; rm -rf $TOOLS_OUT/one_prof
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/nab_prof -- python bench.py --full --steps 5 --warmup 4 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > $TOOLS_OUT/nab.json.log 2>&1
echo "== 576 replicas: $(grep '^{' $TOOLS_OUT/nab.json.log | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(round(d["value"],1), round(d["roofline"]["avg_launch_ms"],3))')"
python tools/kernel_table.py $TOOLS_OUT/nab_prof | head -24; rm -rf $TOOLS_OUT/nab_prof
