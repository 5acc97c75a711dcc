#!/bin/bash
# the ReaxFF set with a larger replica (PE-2880: LDS tables past 64 kB): same-box A/B of environment variants
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
for V in "$@"; do
  name=${V%%:*}; envs=${V#*:}
  env $envs python bench.py --full --force-field reax --cells 4 6 10 --sims 48 --steps 3 --warmup 1 --no-cpu-baseline 2>/dev/null | python -c "
import sys,json
d=json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r=d['roofline']
print('$name', round(d['value'],1), 'evals/s; atoms', d['config']['atoms_per_replica'], 'sweep whole ms', round(r['whole_avg_launch_ms'],4), 'its/solve', round(r['qeq_iterations_per_solve'],2), d['config'].get('env_overrides'), flush=True)"
done
