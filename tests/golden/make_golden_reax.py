#!/usr/bin/env python3
"""Generates tests/golden/oracle_eval_reax.json: known answers of the CPU oracle (oracle/reax_md.py: the dynamics of
oracle/md_oracle.c around the reverse-mode forces of oracle/reax_torch.py and fix qeq/reax) for whole strained evaluations with
md_force_field "reax" -- BASELINE.json config 5, SURVEY.md 8(f) row f-4.  Settings of lammps_scripts_reax: ffield.reax.2 with
H C N O, QEq to 1e-6 every step, fix nvt 100 fs, fix deform erate remap x, no SHAKE, no k-space; dt 0.25 fs, 300 K, strain
rate 1e-3 /fs, 20 sampling steps (the replica-set workload of bench.py --force-field reax).

  pe1620   the 1 620-atom polyethylene replica of that workload (scema_amd.systems.build_pe(3, 5, 9), velocities seed 3):
           tension, shear-dominated, compression with nts = 20, each followed by a continued second evaluation
  mixture  864 atoms of water / ammonia / methane / formaldehyde (every element, hydrogen bonds; tests/test_reax_host.case_mixture,
           seed 10, velocities seed 2): two strains, each with a continuation

PARITY UNPINNED (no LAMMPS / USER-REAXC here).  ~25 s per evaluation; the chains run in a process pool.  From the repo root:
    python tests/golden/make_golden_reax.py
"""
import json
import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PARAMS = dict(dt=0.25, temperature=300.0, strain_rate=1e-3, nss=20, qeq_tol=1e-6)
ELEMENTS = ["H", "C", "N", "O"]
MASS = dict(H=1.008, C=12.011, N=14.007, O=15.999)
FFIELD = os.path.join(ROOT, "tests", "golden", "ffield.reax.2")


def velocities(sym, seed):
    m = np.array([MASS[s] for s in sym])
    v = np.random.default_rng(seed).standard_normal((len(sym), 3)) * np.sqrt(0.0019872067 * 300.0 / (m[:, None] * 48.88821291 ** 2))
    return v - (m[:, None] * v).sum(0) / m.sum()


def system(name):
    if name == "pe1620":
        from scema_amd.systems import build_pe
        d = build_pe(3, 5, 9)
        sym = ["C" if d["mass"][k] > 5 else "H" for k in d["type"]]
        return sym, np.array(d["x"], float), np.array(d["box"], float), velocities(sym, 3)
    from test_reax_host import case_mixture
    sym, x, box = case_mixture(seed=10)
    return sym, np.round(x, 10), box, velocities(sym, 2)   # rounded: the file stores exactly what was run


def strains(name, lens):
    lx, ly, lz = lens
    if name == "pe1620":
        tension = np.array([-4.0e-4 * lx, -4.0e-4 * ly, 1.25e-3 * lz, 6.0e-5 * lz, -3.0e-5 * ly, 4.0e-5 * lx])
        shear = np.array([1.0e-4 * lx, -1.0e-4 * ly, 2.0e-4 * lz, 1.0e-3 * lz, -4.0e-4 * ly, 5.0e-4 * lx])
        comp = np.array([0.9e-3 * lx, 0.9e-3 * ly, -3.0e-3 * lz, -5.0e-5 * lz, 8.0e-5 * ly, 2.0e-5 * lx])
        return dict(tension=tension, shear=shear, compression_nts20=comp)
    return dict(mixed=np.array([0.004 * lx, -0.001 * ly, 0.0, 0.002 * lz, 0.0, -0.001 * lx]),
                biaxial=np.array([-0.002 * lx, 0.003 * ly, 0.001 * lz, 0.0, 0.002 * ly, 0.0]))


def _chain(job):
    import torch
    torch.set_num_threads(max(1, (os.cpu_count() or 2) // 4))
    from oracle import reax_md
    name, chain_name, strain_list = job
    sym, x, box, v = system(name)
    lt = np.array([ELEMENTS.index(s) for s in sym])
    M = reax_md.ReaxMD(FFIELD, ELEMENTS, lt, [MASS[e] for e in ELEMENTS], box, x, v, qeq_tol=PARAMS["qeq_tol"])
    out = []
    for s in strain_list:
        st, nts = M.eval(np.array(s), PARAMS["dt"], PARAMS["temperature"], PARAMS["strain_rate"], PARAMS["nss"])
        out.append(dict(strain_len=[float(a) for a in s], nts=int(nts), stress=[float(a) for a in st]))
    return name, dict(name=chain_name, evals=out, qeq_iterations_per_solve=M.qeq_iters / max(M.qeq_solves, 1))


def main():
    jobs = []
    cases = {}
    for name in ("pe1620", "mixture"):
        sym, x, box, v = system(name)
        lens = box[3:6] - box[:3]
        cases[name] = dict(natoms=len(sym), box=[float(b) for b in box], x_checksum=float(np.abs(x).sum()), v_checksum=float(np.abs(v).sum()), chains=[])
        if name == "mixture":   # small enough to travel: the test rebuilds it from here, not from a random stream
            cases[name].update(sym=sym, x=x.tolist(), v=v.tolist())
        for cname, s in strains(name, lens).items():
            jobs.append((name, cname, [s.tolist(), (0.5 * s).tolist()]))
    with mp.Pool(min(len(jobs), 4)) as pool:
        for name, res in pool.map(_chain, jobs):
            cases[name]["chains"].append(res)
    out = dict(generator="tests/golden/make_golden_reax.py", params=PARAMS, elements=ELEMENTS,
               fixture="pe1620: scema_amd.systems.build_pe(3, 5, 9) + velocities(seed 3); mixture: stored", **cases)
    path = os.path.join(ROOT, "tests", "golden", "oracle_eval_reax.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    mp.set_start_method("spawn")
    main()
