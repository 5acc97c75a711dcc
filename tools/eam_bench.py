"""Throughput of the embedded-atom path on the shape of tools/tersoff_bench.py: N quadrature points (default 576) x one 256-atom fcc
replica of the fixture's first element (4 x 4 x 4 cells of copper, 3.615 A, thermal velocities at 300 K, tests/golden/CuAg.eam.alloy),
10 straining + 100 sampling steps per evaluation at 1 fs.  One warm-up update, then the timed ones, each continuing from the states of
the one before; a host clock around strain_batch, which ends in a device synchronise.  Prints one JSON line.

  python tools/eam_bench.py [--sims 576] [--updates 5] [--nss 100] [--split 1] [--dump stress.npy]
"""
import argparse
import itertools
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scema_amd import capi  # noqa: E402

A_CU, CU_MASS, BOLTZ, MVV2E = 3.615, 63.546, 0.0019872067, 48.88821291 ** 2


def copper(nx, ny, nz, temp, seed):
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0]], float) * 0.25
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * A_CU
    rng = np.random.default_rng(seed)
    v = rng.normal(size=x.shape) * math.sqrt(BOLTZ * temp / CU_MASS / MVV2E)
    return x, np.array([0.0, 0.0, 0.0, nx * A_CU, ny * A_CU, nz * A_CU, 0.0, 0.0, 0.0]), v - v.mean(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=576)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--nss", type=int, default=100)
    ap.add_argument("--split", type=int, default=-1, help="scema_md_batch_split: 0 whole, 1 part batches, -1 the default")
    ap.add_argument("--dump", default=None, metavar="FILE", help="write the stresses of the last update as FILE (.npy, float64, one row of six per quadrature point)")
    a = ap.parse_args()
    x, box, v = copper(4, 4, 4, 300.0, 1)
    e = capi.Engine(capi.default_params())
    e.register_replica("cu", 1, capi.bare_system(np.zeros(len(x), np.int32), x, box, v=v, masses=(CU_MASS,)))
    e.eam_configure("cu", os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy"), ("Cu",))
    e.batch_split(a.split)
    L = box[3:6] - box[:3]
    rng = np.random.default_rng(1)

    def sims(first):
        out = []
        for q in range(a.sims):
            ezz = rng.uniform(4e-4, 9e-4)      # 10 straining steps at 1e-4 per fs, dt 1 fs
            s = np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.1 * ezz * L[2], 0.0, 0.0])
            out.append(capi.make_sim(q, "cu", 1, s, nss=a.nss, dt=1.0, temperature=300.0, strain_rate=1e-4,
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
    print(json.dumps({"workload": "eam_cu_256", "sims": a.sims, "steps_per_eval": 10 + a.nss, "updates": a.updates, "split": e.concurrency()["split"],
                      "evals_per_s_median": a.sims / med, "evals_per_s_best": a.sims / best, "update_s": times,
                      "replica_steps_per_s_median": a.sims * (10 + a.nss) / med, "neigh_builds": prof["neigh_builds"], "md_steps": prof["md_steps"]}))
    e.close()


if __name__ == "__main__":
    main()
