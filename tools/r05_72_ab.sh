#!/bin/bash
# 72 replicas (one GPU's share of 576 on 8): same-box A/B of environment variants (usage: tools/r05_72_ab.sh "name:ENV=.." ...)
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
C=$TOOLS_OUT/equil_pe10k.npz
python bench.py --full --sims 1 --steps 1 --warmup 0 --no-cpu-baseline --monotonic-updates 0 --reax-leg off --equil-cache $C > /dev/null 2>&1
for V in "$@"; do
  name=${V%%:*}; envs=${V#*:}
  env $envs python bench.py --full --sims 72 --steps 10 --warmup 3 --no-cpu-baseline --monotonic-updates 0 --reax-leg off --equil-cache $C 2>/dev/null | grep "^{" | python -c "
import sys,json; d=json.loads(sys.stdin.read()); print('$name', round(d['value'],1), 'evals/s', round(d['ms_per_step'],2), 'ms per update', d['config']['env_overrides'], flush=True)"
done
