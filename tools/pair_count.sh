#!/bin/bash
# usage (on the GPU box, from the repo root): tools/pair_count.sh  -- counting build of k_pair (-DPAIR_COUNT): where the lanes of the row loop are
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
touch scema_amd/csrc/md_types.h
make -C scema_amd/csrc -j16 -s HIPFLAGS="--offload-arch=gfx950 -munsafe-fp-atomics -DPAIR_COUNT" 2>&1 | grep -E "error" | head
SCEMA_MD_TIMING=1 python bench.py --full --sims 72 --steps 2 --warmup 1 --no-cpu-baseline --monotonic-updates 0 > $TOOLS_OUT/pair_count.json.log 2> $TOOLS_OUT/pair_count.err
grep "k_pair lanes\|far skin band\|row entries" $TOOLS_OUT/pair_count.err | tail -12
