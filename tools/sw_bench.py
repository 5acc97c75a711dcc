"""Throughput of the Stillinger-Weber path on the shape of the reference's silicon example: N quadrature points (default 576) x one
192-atom replica (tests/golden/lammps_17Nov16_init.sic_1.bin with tests/golden/Si.sw), 10 straining + 100 sampling steps per evaluation.
One warm-up update, then the timed ones, each continuing from the states of the one before; a host clock around strain_batch, which ends
in a device synchronise.  Prints one JSON line.  For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python
tools/sw_bench.py --updates 2` (a run of its own: tracing slows the host).

  python tools/sw_bench.py [--sims 576] [--updates 5] [--nss 100] [--split 1] [--dump stress.npy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scema_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=576)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--nss", type=int, default=100)
    ap.add_argument("--split", type=int, default=-1, help="scema_md_batch_split: 0 whole, 1 part batches, -1 the default")
    ap.add_argument("--dump", default=None, metavar="FILE", help="write the stresses of the last update as FILE (.npy, float64, one row of six per quadrature point)")
    a = ap.parse_args()
    gold = os.path.join(ROOT, "tests", "golden")
    e = capi.Engine(capi.default_params())
    e.load_lammps_restart("sic", 1, os.path.join(gold, "lammps_17Nov16_init.sic_1.bin"), 192)
    e.sw_configure("sic", os.path.join(gold, "Si.sw"))
    e.batch_split(a.split)
    box, _, _ = e.get_state(capi.QP_NONE, "sic", 1)
    L = box[3:6] - box[:3]
    rng = np.random.default_rng(1)

    def sims(first):
        out = []
        for q in range(a.sims):
            ezz = rng.uniform(4e-4, 9e-4)      # 10 straining steps at 1e-4 per fs, dt 1 fs
            s = np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.1 * ezz * L[2], 0.0, 0.0])
            out.append(capi.make_sim(q, "sic", 1, s, nss=a.nss, dt=1.0, temperature=300.0, strain_rate=1e-4,
                                     most_recent=capi.QP_NONE if first else q))
        return out

    e.strain_batch(sims(True))                 # warm-up: code objects, slots, rows
    times = []
    for _ in range(a.updates):
        batch = sims(False)
        t0 = time.perf_counter()
        res = e.strain_batch(batch)
        times.append(time.perf_counter() - t0)
        assert all(o.stress_updated == 1 for o in res)
    if a.dump:
        np.save(a.dump, np.array([list(o.stress) for o in res], np.float64))
    prof = e.profile()
    best, med = min(times), sorted(times)[len(times) // 2]
    print(json.dumps({"workload": "sw_si_192", "sims": a.sims, "steps_per_eval": 10 + a.nss, "updates": a.updates, "split": e.concurrency()["split"],
                      "evals_per_s_median": a.sims / med, "evals_per_s_best": a.sims / best, "update_s": times,
                      "replica_steps_per_s_median": a.sims * (10 + a.nss) / med, "neigh_builds": prof["neigh_builds"], "md_steps": prof["md_steps"]}))
    e.close()


if __name__ == "__main__":
    main()
