#!/bin/bash
# same-box sensitivity: fit target of the real-space Ewald polynomial (number of Horner terms of the coulomb block)
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
for V in "tol2e-13:" "tol1e-9:SCEMA_MD_POLY_TOL=1e-9" "tol1e-6:SCEMA_MD_POLY_TOL=1e-6" "tol2e-13_again:" "tol1e-9_again:SCEMA_MD_POLY_TOL=1e-9"; do
  name=${V%%:*}; envs=${V#*:}
  env $envs python bench.py --full --steps 5 --warmup 3 --no-cpu-baseline --reax-leg off --monotonic-updates 0 --equil-cache $TOOLS_OUT/equil_pe10k.npz > $TOOLS_OUT/r04_n_$name.json.log 2> $TOOLS_OUT/r04_n_$name.err || exit 1
  python - <<PY
import json
d=json.loads(open('$TOOLS_OUT/r04_n_$name.json.log').read().strip().split('\n')[-1]); r=d['roofline']
print('$name', round(d['value'],1), 'evals/s; k_pair ms', round(r['avg_launch_ms'],3), d['config']['env_overrides'], flush=True)
PY
done
