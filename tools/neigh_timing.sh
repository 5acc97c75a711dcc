#!/bin/bash
# usage (on the GPU box, from the repo root): tools/neigh_timing.sh  -- clock-counter build (-DPAIR_TIMING): where the waves of k_neigh_build and k_pair spend their cycles
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
touch scema_amd/csrc/md_types.h
make -C scema_amd/csrc -j16 -s HIPFLAGS="--offload-arch=gfx950 -munsafe-fp-atomics -DPAIR_TIMING" 2>&1 | grep -E "error" | head
SCEMA_MD_TIMING=1 python bench.py --full --sims ${1:-72} --steps 2 --warmup 1 --no-cpu-baseline --monotonic-updates 0 > $TOOLS_OUT/neigh_timing.json.log 2> $TOOLS_OUT/neigh_timing.err
grep "clocks" $TOOLS_OUT/neigh_timing.err | tail -8
