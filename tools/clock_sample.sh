#!/bin/bash
# sustained clock and power of the headline loop: rocm-smi sampled every 2 s next to a short bench run (read-only queries)
cd "$(dirname "$0")/.."   # the repository root
TOOLS_OUT=${TOOLS_OUT:-tools_out}   # where the runs' logs and profiles go
mkdir -p $TOOLS_OUT
python bench.py --full --steps 12 --warmup 3 --no-cpu-baseline --reax-leg off --monotonic-updates 0 --equil-cache $TOOLS_OUT/equil_pe10k.npz > $TOOLS_OUT/r04_clock_bench.json.log 2>/dev/null &
BP=$!
: > $TOOLS_OUT/r04_clock_samples.txt
while kill -0 $BP 2>/dev/null; do
  (date +%s.%N; rocm-smi --showclocks --showpower --showuse 2>/dev/null | grep -E "sclk|mclk|Power|GPU use|fclk") >> $TOOLS_OUT/r04_clock_samples.txt
  sleep 2
done
wait $BP
grep -E "sclk" $TOOLS_OUT/r04_clock_samples.txt | sort | uniq -c | sort -rn | head -8
grep -E "Power" $TOOLS_OUT/r04_clock_samples.txt | sort | uniq -c | sort -rn | head -8
