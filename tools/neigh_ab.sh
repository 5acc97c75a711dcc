#!/bin/bash
# usage (on the GPU box): tools/neigh_ab.sh  -- parity tests of the list build, then a sustained profile of the headline bench (k_neigh_build / k_pair per step), then the wave clocks
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
python -m pytest tests/test_gpu_parity.py tests/test_gpu_fullsize.py tests/test_gpu_edge_cases.py -x -q 2>&1 | tail -3 || exit 1
python bench.py --full --sims 1 --steps 1 --warmup 0 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $TOOLS_OUT/nab_prof -- python bench.py --full --steps 5 --warmup 4 --no-cpu-baseline --monotonic-updates 0 --equil-cache $C > $TOOLS_OUT/nab.json.log 2>&1
echo "== $(grep '^{' $TOOLS_OUT/nab.json.log | python -c 'import sys,json; d=json.loads(sys.stdin.read()); print(round(d["value"],1), round(d["roofline"]["avg_launch_ms"],3))')"
python tools/kernel_table.py $TOOLS_OUT/nab_prof | grep -E "k_neigh_build|k_pair<true|kernel time|k_cell_sort|k_pack"; rm -rf $TOOLS_OUT/nab_prof
bash tools/neigh_timing.sh 576 2>&1 | grep neigh_build | tail -2
