#!/usr/bin/env python
"""Tiled PPPM kernels against the kernels without LDS on meshes beyond the LDS: PE-10k with its charges scaled so that the grid rule
gives a larger mesh, N replicas per strain_batch update as bench.py issues them (persistent states, load / unload strain draws),
scema_md_pppm_tiling mode 1 and mode 0 alternating in ONE process on one box, HIP events around every update.  One JSON line.

  python tools/pppm_tiled_ab.py --sims 72 --charge-scale 3 --accuracy 1e-5            # 30 x 30 x 30: both kernels tiled
  python tools/pppm_tiled_ab.py --sims 72 --charge-scale 4 --accuracy 1e-4            # 24 x 24 x 20: interpolation only
  python tools/pppm_tiled_ab.py --sims 72                                             # 12 x 12 x 12: control, nothing may move
  python tools/pppm_tiled_ab.py --sims 72 --charge-scale 3 --accuracy 1e-5 --only 1   # one mode only (under rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sims", type=int, default=72)
    ap.add_argument("--charge-scale", type=float, default=1.0)
    ap.add_argument("--accuracy", type=float, default=1e-4)
    ap.add_argument("--cells", type=int, nargs=3, default=[6, 9, 16])
    ap.add_argument("--nss", type=int, default=100)
    ap.add_argument("--updates", type=int, default=2, help="timed updates per mode and round")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of (mode 0, mode 1, mode 0 again)")
    ap.add_argument("--equil-steps", type=int, default=2000)
    ap.add_argument("--only", type=int, default=-1, help="run this mode only: one warm-up and --updates updates (for a profiler)")
    args = ap.parse_args()

    import torch
    from scema_amd import capi
    from scema_amd.systems import build_pe, synthetic_strains

    d = build_pe(*args.cells, shake_project=True)
    d["charge"] = np.asarray(d["charge"], float) * args.charge_scale
    P = capi.default_params(kspace_accuracy=args.accuracy)
    _, g, grid = capi.kspace_setup(P, np.asarray(d["box"], float), float((d["charge"] ** 2).sum()), d["natoms"])
    eng = capi.Engine(P)
    eng.register_replica("g0", 1, d)
    if args.equil_steps > 0:
        eng.set_state(1 << 20, "g0", 1, d["box"], d["x"], d["v"])
        eng.debug_run("g0", 1, args.equil_steps, 2.0, 300.0, qp=1 << 20, nvt=True, use_shake=True)
        box, x, v = eng.get_state(1 << 20, "g0", 1)
        d = dict(d, box=box, x=x, v=v)
        eng.register_replica("g0", 1, d)
    lens = d["box"][3:6] - d["box"][:3]
    n, istep = args.sims, [0]

    def update():
        k = istep[0]
        strains = synthetic_strains(n, lens, seed=2026 + k, scale=1.0, mode="balanced") * (-1.0 if k % 2 else 1.0)
        sims = [capi.make_sim(q, "g0", 1, strains[q], nss=args.nss, most_recent=capi.QP_NONE if k == 0 else q, strain_rate=1e-4, dt=2.0) for q in range(n)]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        out = eng.strain_batch(sims)
        t1.record()
        torch.cuda.synchronize()
        istep[0] += 1
        assert all(o.stress_updated for o in out)
        return t0.elapsed_time(t1), float(sum(o.stress[2] for o in out))

    res = dict(sims=n, charge_scale=args.charge_scale, accuracy=args.accuracy, grid=list(grid), g_ewald=g, natoms=int(d["natoms"]), nss=args.nss, runs=[])
    order = [args.only] if args.only >= 0 else [0, 1, 0] * args.rounds
    update()                                            # (lists, plans and LDS opt-ins of the first update)
    for mode in order:
        eng.pppm_tiling(mode, 0)
        update()
        ms = [update()[0] for _ in range(args.updates)]
        res["runs"].append(dict(mode=mode, ms_per_update=ms, paths=eng.pppm_paths()))
    for mode in sorted(set(order)):
        best = min(min(r["ms_per_update"]) for r in res["runs"] if r["mode"] == mode)
        mean = float(np.mean([t for r in res["runs"] if r["mode"] == mode for t in r["ms_per_update"]]))
        res[f"mode{mode}_ms"] = dict(best=best, mean=mean)
    if args.only < 0:
        first = [np.mean(r["ms_per_update"]) for r in res["runs"] if r["mode"] == 0]
        res["mode0_spread_between_runs"] = float((max(first) - min(first)) / np.mean(first))
        res["tiled_gain"] = float(res["mode0_ms"]["mean"] / res["mode1_ms"]["mean"] - 1.0)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
