"""Throughput of a force stage on full neighbour rows: N quadrature points (default 576) x one replica, 10 straining + 100 sampling steps
per evaluation at 1 fs.  The replica per potential:
  sw ....... the 192-atom silicon replica of the reference's example (tests/golden/lammps_17Nov16_init.sic_1.bin with tests/golden/Si.sw)
  edip ..... the same 192-atom silicon replica as sw, under tests/golden/Si.edip (pair_style edip)
  tersoff .. 192 atoms of diamond silicon (3 x 2 x 4 cells of 5.432 A, thermal velocities at 300 K, tests/golden/SiC.tersoff)
  tersoff_mod, tersoff_zbl .. the same 192 silicon atoms under tests/golden/Si.tersoff.mod (a = 5.429 A) and tests/golden/SiC.tersoff.zbl
  eam ...... 256 atoms of fcc copper, the fixture's first element (4 x 4 x 4 cells of 3.615 A, thermal velocities at 300 K,
             tests/golden/CuAg.eam.alloy)
  adp ...... the same 256 copper atoms under tests/golden/CuAg.adp (pair_style adp: the embedded-atom terms plus dipoles and quadrupoles)
  meam_spline  the 256-atom fcc replica of the eam leg scaled to 3.9 A, next to the fixture's own fcc minimum (twelve neighbours at 2.76 A inside the three-body range of 3.4 A, 42
             inside cutmax) with the mass of titanium, under the synthetic tests/golden/Ti.meam.spline (pair_style meam/spline)
  vashishta  512 atoms of zincblende SiC (4 x 4 x 4 cells of 4.3581 A: the box of 17.43 A is at least twice rc + skin = 8.35 A, so the rows
             are built by minimum image; masses 28.0855 and 12.011, thermal velocities at 300 K, tests/golden/SiC.vashishta)
  born_dsf   512 ions of rock-salt NaCl (4 x 4 x 4 cells of 5.64 A: the box of 22.56 A is at least twice cut_coul + skin = 11 A, so the
             rows are built by minimum image; charges +1 and -1, masses 22.98977 and 35.453, thermal velocities at 300 K,
             tests/golden/NaCl.born_dsf: pair_style born/coul/dsf 0.25 10.0, about 190 neighbours per ion)
  born_long  the born_dsf replica under tests/golden/NaCl.born_long: pair_style born/coul/long 10.0 with kspace_style ewald 1.0e-5, the
             same neighbours beside 709 k-vectors per replica; --kspace mesh puts the reciprocal part on the PPPM mesh (24^3) instead
  eam_coul   324 ions of fluorite UO2 (3 x 3 x 3 cells of 5.47 A, O -1.1104 and U +2.2208, masses 15.9994 and 238.02891, thermal velocities
             at 300 K) under tests/golden/UO2.eam_coul: pair_style hybrid/overlay coul/long 9.0 eam/alloy on the synthetic UO2.eam.alloy with
             kspace_style ewald 1.0e-5 (709 k-vectors); --kspace as for born_long.  Its two parents on the SAME replica, for the sum the
             fused stage is measured against: eam_coul_eam (the ions without their charges under pair_style eam/alloy on UO2.eam.alloy) and
             eam_coul_coul (pair_style born/coul/long 9.0 with every Born constant zero and the same kspace_style line, written to a
             temporary file; --kspace applies).  Point charges without a short-range term fall into each other under dynamics, so the
             Coulomb parent leaves the lattice and rebuilds its rows on most steps; --heavy multiplies the masses of these three legs
             by 1e8 (the thermal velocities shrink with them), so the ions of all three stay on their sites over the run, every leg
             walks the same rows and builds its lists equally often (neigh_builds of the JSON line), and the times compare kernels
One warm-up update, then the timed ones, each continuing from the states of the one before; a host clock around strain_batch, which ends
in a device synchronise.  Prints one JSON line.  For the per-kernel table run it under `rocprofv3 --kernel-trace --stats -- python
tools/rowpot_bench.py --potential sw --updates 2` (a run of its own: tracing slows the host).

  python tools/rowpot_bench.py --potential sw|edip|tersoff|tersoff_mod|tersoff_zbl|eam|adp|meam_spline|vashishta|born_dsf|born_long|eam_coul|eam_coul_eam|eam_coul_coul [--sims 576] [--updates 5] [--nss 100] [--split 1] [--cells K] [--kspace ewald|mesh] [--heavy] [--dump stress.npy]
"""
import argparse
import itertools
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scema_amd import capi  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
BOLTZ, MVV2E = 0.0019872067, 48.88821291 ** 2
DIAMOND = [[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]
FCC = DIAMOND[:4]
ZINCBLENDE = FCC + [[1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]]          # (the diamond sites: the fcc ones, then those a quarter diagonal further)


def register_lattice(e, matid, basis, cells, a, mass, temp=300.0, seed=1, basis_types=None, type_charges=None):
    """a cubic lattice of that basis (in quarters of the cell) with thermal velocities, as a bare replica; mass: one number, or with
    basis_types (the LAMMPS type, from 0, of every basis site) one per type; type_charges: a charge per type (an ionic replica)"""
    nx, ny, nz = cells
    grid = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (grid[:, None, :] + np.array(basis, float)[None, :, :] * 0.25).reshape(-1, 3) * a
    masses = (mass,) if basis_types is None else tuple(mass)
    types = np.tile(np.zeros(len(basis), np.int32) if basis_types is None else np.array(basis_types, np.int32), len(grid))
    rng = np.random.default_rng(seed)
    v = rng.normal(size=x.shape) * np.sqrt(BOLTZ * temp / np.array(masses)[types] / MVV2E)[:, None]
    box = np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0])
    if type_charges is None:
        e.register_replica(matid, 1, capi.bare_system(types, x, box, v=v - v.mean(axis=0), masses=masses))
    else:
        e.register_replica(matid, 1, capi.ionic_system(types, np.array(type_charges, float)[types], x, box, masses, v=v - v.mean(axis=0)))


def make_sw(e, cells=None):
    if cells is None:
        e.load_lammps_restart("sic", 1, os.path.join(GOLD, "lammps_17Nov16_init.sic_1.bin"), 192)
    else:
        register_lattice(e, "sic", DIAMOND, cells, 5.431, 28.0855)
    e.sw_configure("sic", os.path.join(GOLD, "Si.sw"))


def make_edip(e, cells=None):
    if cells is None:
        e.load_lammps_restart("sic", 1, os.path.join(GOLD, "lammps_17Nov16_init.sic_1.bin"), 192)
    else:
        register_lattice(e, "sic", DIAMOND, cells, 5.430, 28.0855)
    e.edip_configure("sic", os.path.join(GOLD, "Si.edip"))


def make_tersoff(e, cells=None):
    register_lattice(e, "si", DIAMOND, cells or (3, 2, 4), 5.432, 28.0855)
    e.tersoff_configure("si", os.path.join(GOLD, "SiC.tersoff"), ("Si",))


def make_tersoff_mod(e, cells=None):
    register_lattice(e, "si", DIAMOND, cells or (3, 2, 4), 5.429, 28.0855)
    e.tersoff_mod_configure("si", os.path.join(GOLD, "Si.tersoff.mod"), ("Si",))


def make_tersoff_zbl(e, cells=None):
    register_lattice(e, "si", DIAMOND, cells or (3, 2, 4), 5.432, 28.0855)
    e.tersoff_zbl_configure("si", os.path.join(GOLD, "SiC.tersoff.zbl"), ("Si",))


def make_eam(e, cells=None):
    register_lattice(e, "cu", FCC, cells or (4, 4, 4), 3.615, 63.546)
    e.eam_configure("cu", os.path.join(GOLD, "CuAg.eam.alloy"), ("Cu",))


def make_adp(e, cells=None):
    register_lattice(e, "cu", FCC, cells or (4, 4, 4), 3.615, 63.546)
    e.adp_configure("cu", os.path.join(GOLD, "CuAg.adp"), ("Cu",))


def make_meam_spline(e, cells=None):
    register_lattice(e, "ti", FCC, cells or (4, 4, 4), 3.9, 47.867)
    e.meam_spline_configure("ti", os.path.join(GOLD, "Ti.meam.spline"), ("Ti",))


def make_vashishta(e, cells=None):
    register_lattice(e, "sic", ZINCBLENDE, cells or (4, 4, 4), 4.3581, (28.0855, 12.011), basis_types=[0, 0, 0, 0, 1, 1, 1, 1])
    e.vashishta_configure("sic", os.path.join(GOLD, "SiC.vashishta"), ("Si", "C"))


ROCKSALT = FCC + [[2, 0, 0], [2, 2, 2], [0, 0, 2], [0, 2, 0]]              # (the fcc sites, then those half a cell edge further along x)


def make_born_dsf(e, cells=None):
    register_lattice(e, "nacl", ROCKSALT, cells or (4, 4, 4), 5.64, (22.98977, 35.453), basis_types=[0, 0, 0, 0, 1, 1, 1, 1], type_charges=(1.0, -1.0))
    e.born_dsf_configure("nacl", os.path.join(GOLD, "NaCl.born_dsf"))


def make_born_long(e, cells=None):
    register_lattice(e, "nacl", ROCKSALT, cells or (4, 4, 4), 5.64, (22.98977, 35.453), basis_types=[0, 0, 0, 0, 1, 1, 1, 1], type_charges=(1.0, -1.0))
    e.born_long_configure("nacl", os.path.join(GOLD, "NaCl.born_long"))


FLUORITE = FCC + [[i, j, k] for i in (1, 3) for j in (1, 3) for k in (1, 3)]   # (U on the fcc sites, O on the eight tetrahedral sites)
UO2 = dict(a=5.47, mass=(15.9994, 238.02891), basis_types=[1] * 4 + [0] * 8, type_charges=(-1.1104, 2.2208))
HEAVY = 1.0     # --heavy: 1e8


def uo2_mass():
    return tuple(m * HEAVY for m in UO2["mass"])


def make_eam_coul(e, cells=None):
    register_lattice(e, "uo2", FLUORITE, cells or (3, 3, 3), UO2["a"], uo2_mass(), basis_types=UO2["basis_types"], type_charges=UO2["type_charges"])
    e.eam_coul_configure("uo2", os.path.join(GOLD, "UO2.eam_coul"))


def make_eam_coul_eam(e, cells=None):
    register_lattice(e, "uo2", FLUORITE, cells or (3, 3, 3), UO2["a"], uo2_mass(), basis_types=UO2["basis_types"])
    e.eam_configure("uo2", os.path.join(GOLD, "UO2.eam.alloy"), ("O", "U"))


def make_eam_coul_coul(e, cells=None):
    register_lattice(e, "uo2", FLUORITE, cells or (3, 3, 3), UO2["a"], uo2_mass(), basis_types=UO2["basis_types"], type_charges=UO2["type_charges"])
    with tempfile.NamedTemporaryFile("w", suffix=".born_long") as f:
        f.write("units metal\npair_style born/coul/long 9.0\nkspace_style ewald 1.0e-5\npair_coeff * * 0.0 1.0 0.0 0.0 0.0\n")
        f.flush()
        e.born_long_configure("uo2", f.name)


# potential -> (workload of the JSON line, material id, what registers the one replica and attaches the potential)
POTENTIALS = {"sw": ("sw_si_192", "sic", make_sw), "tersoff": ("tersoff_si_192", "si", make_tersoff), "eam": ("eam_cu_256", "cu", make_eam),
              "tersoff_mod": ("tersoff_mod_si_192", "si", make_tersoff_mod), "tersoff_zbl": ("tersoff_zbl_si_192", "si", make_tersoff_zbl),
              "vashishta": ("vashishta_sic_512", "sic", make_vashishta), "adp": ("adp_cu_256", "cu", make_adp), "edip": ("edip_si_192", "sic", make_edip),
              "meam_spline": ("meam_spline_ti_256", "ti", make_meam_spline), "born_dsf": ("born_dsf_nacl_512", "nacl", make_born_dsf),
              "born_long": ("born_long_nacl_512", "nacl", make_born_long), "eam_coul": ("eam_coul_uo2_324", "uo2", make_eam_coul),
              "eam_coul_eam": ("eam_uo2_324", "uo2", make_eam_coul_eam), "eam_coul_coul": ("coul_long_uo2_324", "uo2", make_eam_coul_coul)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--potential", required=True, choices=sorted(POTENTIALS))
    ap.add_argument("--sims", type=int, default=576)
    ap.add_argument("--updates", type=int, default=5)
    ap.add_argument("--nss", type=int, default=100)
    ap.add_argument("--split", type=int, default=-1, help="scema_md_batch_split: 0 whole, 1 part batches, -1 the default")
    ap.add_argument("--cells", type=int, default=None, metavar="K", help="K x K x K lattice cells per replica instead of the potential's shape above (sw: diamond silicon of 5.431 A "
                    "instead of the example's file); the JSON line then names the atoms and the list builds through cells (SCEMA_MD_ROW_CELLS, DESIGN.md 7m)")
    ap.add_argument("--kspace", default=None, choices=("ewald", "mesh"), help="born_long, eam_coul and eam_coul_coul: the reciprocal solver of every replica, the Ewald sum (born_long_kspace "
                    "mode 2) or the PPPM mesh (mode 1); default: by the script and the Ewald limits (mode 0)")
    ap.add_argument("--heavy", action="store_true", help="eam_coul, eam_coul_eam and eam_coul_coul: masses times 1e8, so the ions stay on their sites and the "
                    "three legs build their rows equally often")
    ap.add_argument("--dump", default=None, metavar="FILE", help="write the stresses of the last update as FILE (.npy, float64, one row of six per quadrature point)")
    a = ap.parse_args()
    workload, mat, make = POTENTIALS[a.potential]
    if a.heavy:
        if not a.potential.startswith("eam_coul"):
            ap.error("--heavy needs --potential eam_coul, eam_coul_eam or eam_coul_coul")
        global HEAVY
        HEAVY = 1.0e8
    e = capi.Engine(capi.default_params())
    make(e, None if a.cells is None else (a.cells,) * 3)
    if a.kspace is not None:
        if a.potential not in ("born_long", "eam_coul", "eam_coul_coul"):
            ap.error("--kspace needs --potential born_long, eam_coul or eam_coul_coul")
        (e.eam_coul_kspace if a.potential == "eam_coul" else e.born_long_kspace)(mat, {"ewald": 2, "mesh": 1}[a.kspace])
    e.batch_split(a.split)
    box, _, _ = e.get_state(capi.QP_NONE, mat, 1)
    L = box[3:6] - box[:3]
    rng = np.random.default_rng(1)

    def sims(first):
        out = []
        for q in range(a.sims):
            ezz = rng.uniform(4e-4, 9e-4)      # 10 straining steps at 1e-4 per fs, dt 1 fs
            s = np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.1 * ezz * L[2], 0.0, 0.0])
            out.append(capi.make_sim(q, mat, 1, s, nss=a.nss, dt=1.0, temperature=300.0, strain_rate=1e-4,
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
    extra = {}
    if a.kspace is not None:
        extra["kspace"] = a.kspace
    if a.heavy:
        extra["heavy"] = True
    if a.cells is not None:
        natoms = e.natoms(mat, 1)
        workload = "%s_%d" % (workload.rsplit("_", 1)[0], natoms)
        extra = {**extra, "cells": a.cells, "atoms": natoms, "row_cell_builds": prof["row_cell_builds"], "row_cells_env": os.environ.get("SCEMA_MD_ROW_CELLS")}
    print(json.dumps({"workload": workload, "sims": a.sims, "steps_per_eval": 10 + a.nss, "updates": a.updates, "split": e.concurrency()["split"],
                      "evals_per_s_median": a.sims / med, "evals_per_s_best": a.sims / best, "update_s": times,
                      "replica_steps_per_s_median": a.sims * (10 + a.nss) / med, "neigh_builds": prof["neigh_builds"], "md_steps": prof["md_steps"], **extra}))
    e.close()


if __name__ == "__main__":
    main()
