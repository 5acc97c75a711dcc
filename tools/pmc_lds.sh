#!/bin/bash
# usage (on the GPU box, from the repo root): tools/pmc_lds.sh <tag> [kernel-regex] [sims]
# One rocprofv3 --pmc pass (no tracing domains) with the three LDS counters on a short headline-shaped bench (equilibrated replica,
# whole batch per launch); prints per-dispatch means of the batch launches only (as tools/pmc_pair.sh does) and, per kernel, the
# bank-conflict cycles per LDS instruction and their share of the LDS-array cycles.  Writes $TOOLS_OUT/pmc_lds_<tag>.txt.
TOOLS_OUT=${TOOLS_OUT:-tools_out}
TAG=${1:-x}; RE=${2:-k_pppm_force|k_pppm_spread_binned|k_pppm_bins|k_bonded}; SIMS=${3:-72}
cd "$(dirname "$0")/.." || exit 1
mkdir -p $TOOLS_OUT
CACHE=${EQUIL_CACHE:-$TOOLS_OUT/equil_pe10k.npz}
# the equilibration (2 000 single-replica steps) runs once, outside the profiler
[ -f $CACHE ] || timeout -k 10 300 python bench.py --full --sims 1 --steps 1 --warmup 0 --nss 10 --no-cpu-baseline --reax-leg off --monotonic-updates 0 --share8-updates 0 --equil-cache $CACHE > $TOOLS_OUT/pmc_lds_equil.log 2>&1 || exit 1
export SCEMA_MD_SPLIT=0   # whole batch per launch
timeout -k 10 400 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS --kernel-include-regex "$RE" --output-format csv -d $TOOLS_OUT/pmc_lds_$TAG -- \
  python bench.py --full --sims $SIMS --steps 1 --warmup 1 --nss 10 --no-cpu-baseline --reax-leg off --monotonic-updates 0 --share8-updates 0 --equil-cache $CACHE > $TOOLS_OUT/pmc_lds_$TAG.log 2>&1 || exit 1
python - <<PY | tee $TOOLS_OUT/pmc_lds_$TAG.txt
import csv, glob, collections
print("# rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS (one pass, no tracing) -- python bench.py --full --sims $SIMS --steps 1 --warmup 1 --nss 10, SCEMA_MD_SPLIT=0")
print("# per-dispatch means of the batch launches (largest grid of each kernel); conflict share = BANK_CONFLICT / IDX_ACTIVE")
for d in sorted(glob.glob('$TOOLS_OUT/pmc_lds_$TAG/*/*_counter_collection.csv')):
    rows = list(csv.DictReader(open(d)))
    gmax = collections.defaultdict(int)
    for r in rows:
        gmax[r['Kernel_Name']] = max(gmax[r['Kernel_Name']], int(r['Grid_Size']))
    agg = collections.defaultdict(lambda: collections.defaultdict(float)); disp = collections.defaultdict(set)
    for r in rows:
        if int(r['Grid_Size']) != gmax[r['Kernel_Name']]: continue
        k = r['Kernel_Name'].split('(')[0]; agg[k][r['Counter_Name']] += float(r['Counter_Value']); disp[k].add(r['Dispatch_Id'])
    for k in sorted(agg):
        n = len(disp[k]); c = {name: v / n for name, v in agg[k].items()}
        bc, ia, il = c.get('SQ_LDS_BANK_CONFLICT', 0.0), c.get('SQ_LDS_IDX_ACTIVE', 0.0), c.get('SQ_INSTS_LDS', 0.0)
        print(f"{k:48s} dispatches {n:3d}  SQ_LDS_BANK_CONFLICT {bc:14.0f}  SQ_LDS_IDX_ACTIVE {ia:14.0f}  SQ_INSTS_LDS {il:12.0f}"
              f"  conflict/inst {bc / max(il, 1):6.2f}  active/inst {ia / max(il, 1):6.2f}  conflict share {bc / max(ia, 1):5.2f}")
PY
