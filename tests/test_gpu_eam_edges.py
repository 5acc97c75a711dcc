"""The embedded-atom kernels (k_eam_density, k_eam_force, md_eam.hip) where tests/test_gpu_eam.py does not take them, against the numpy
reference tests/eam_numpy.py, which tests/test_row_edges_host.py licenses on these inputs (supercell identity, central differences,
pinned counts, the host-compiled core):

  1  four elements, the most the tables hold (every off_rho / off_z lookup is [ti * EAM_MAXEL + tj]): the file's order, a permuted element
     list, a kept subset that skips a file element in the middle, three LAMMPS types on two elements (a many-to-one type map)
  2  some atoms above rhomax and some below in one launch
  3  15, 16 and 17 atoms: one round with a group idle, all sixteen busy, and a second round of one atom; 64, a full tile
  4  a cell two images deep tilted to xy = +-0.45 lx
  5  the state a sheared run leaves behind after a box flip
  6  dynamics with rebuilds in mid-run and atoms that leave the box, against the numpy stepper
  7  one launch over 4, 32, 108 and 1 200 atoms: the early return of whole workgroups, groups past n, the per-slot F' arrays

Budgets are the standing ones of tests/test_gpu_eam.py: static parity 1e-10 of the largest force component, energy term and virial
component, NVE 1e-9 A and 1e-11 A/fs, sampled pressure 1e-10, a batch against each member alone 1e-9; forces of one state evaluated twice
are equal bit for bit (the stage has no atomic on a force).  Each static check prints its errors and the longest row against the capacity.
"""
import numpy as np
import pytest

import eam_numpy as en
import rowkit as rk
from scema_amd import capi
from test_gpu_eam import CUAG, EAM, MASS, low_file, no_pairs, ref_cu, sheared  # noqa: F401  (fixtures)
from test_row_edges_host import EAM_COUNTS, NVE_STEPS, four_variants, moved_and_outside, nve_case

pytestmark = pytest.mark.gpu


_engine, _nts_and_rates = rk.engine, rk.nts_and_rates
_static = rk.static_of(EAM, CUAG, ("Cu",), MASS)


_check_static = rk.checker(EAM, "eam static", tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)      # the static budget of tests/test_gpu_eam.py


def _counts(ref):
    return ref["maxin"], ref["npairs"], ref["nabove"]


def _masses(elements):
    return tuple(en.JOHNSON[a]["mass"] for a in elements)


@pytest.fixture(scope="module")
def four_file(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("eam_edges") / "four.eam.alloy")
    en.write_johnson(p, en.FOUR)
    return p


# ---- 1. four elements ----
@pytest.mark.parametrize("name", ["four", "four_perm", "four_sub", "four_dup"])
def test_static_parity_four_element_file(four_file, name):
    elements, (x, box, t) = four_variants()[name]
    tab, tmap = en.read_setfl(four_file, elements)
    ref = en.EAM(tab).compute(x, box, np.array(tmap)[t])          # (the reference indexes its tables by element)
    assert _counts(ref) == EAM_COUNTS[name] and tab["n"] == len(set(elements)) and len(set(t)) == len(elements)
    got = _static(x, box, t, path=four_file, elements=tuple(elements), masses=_masses(elements))
    _check_static(got, ref, what=f"eam static {name}, elements {' '.join(elements)}")


# ---- 2. partly above rhomax ----
def test_static_parity_partly_above_rhomax(low_file):
    ref_e = en.EAM(en.read_setfl(low_file, ["Cu"])[0])
    x, box, t = en.case_partly_above()
    ref = ref_e.compute(x, box, t)
    assert _counts(ref) == EAM_COUNTS["partly"] and 0 < ref["nabove"] < len(x)
    _check_static(_static(x, box, t, path=low_file), ref, what="eam static partly above rhomax")


# ---- 3. group edges ----
@pytest.mark.parametrize("n", [15, 16, 17, 64])
def test_group_edges(ref_cu, n):
    x, box, t = en.case_count(n)
    ref = ref_cu.compute(x, box, t)
    assert _counts(ref) == EAM_COUNTS[f"count{n}"]
    _check_static(_static(x, box, t), ref, what=f"eam static n = {n}")


# ---- 4. tilted, two images deep ----
@pytest.mark.parametrize("sign", [+1, -1])
def test_static_parity_tilted_cell_two_images_deep(ref_cu, sign):
    x, box, t = en.case_cell4_tilted(sign)
    w = en.check_box(box)
    assert (w < 6.5).all() and (w > 3.25).all()
    ref = ref_cu.compute(x, box, t)
    assert _counts(ref) == EAM_COUNTS["tilted+" if sign > 0 else "tilted-"]
    _check_static(_static(x, box, t), ref, what=f"eam static cell4, xy = {box[6]:+.3f} A, widths {w[0]:.2f} / {w[1]:.2f} / {w[2]:.2f} A")


# ---- 5. a flipped state ----
def test_static_parity_of_a_flipped_state(ref_cu, sheared):
    """the last simulation of the sheared set of tests/test_gpu_eam.py alone: its box, written with xy = +0.4 lx, passes lx / 2 and flips;
    the forces on the state it leaves, in the box it leaves, against numpy"""
    fresh, sims = sheared[0], sheared[1]
    sim = sims[-1]
    e = fresh()
    try:
        e.strain_batch([sim])
        flips = e.profile()["box_flips"]
        box, x, _ = e.get_state(sim.qp_id, "cu", 1)
        print(f"eam flipped state: {flips} flip(s), xy {2.0 * en.A_CU:.3f} -> {box[6]:.3f} A of lx {box[3] - box[0]:.3f} A")
        assert flips >= 1 and abs(box[6]) <= 0.5 * (box[3] - box[0]) and box[6] < 0.0
        _check_static(e.eam_compute("cu", 1, qp=sim.qp_id), ref_cu.compute(x, box, en.zeros(len(x))), what="eam static flipped state")
    finally:
        e.close()


# ---- 6. dynamics with rebuilds ----
def test_nve_with_rebuilds_in_a_narrow_box(ref_cu):
    """eight copper atoms in 3.4 x 7.0 x 7.6 A, no two closer than 1.65 A (the lattice's neighbours are 2.556 A apart), 300 K, 40 steps:
    an atom moves 0.75 A -- past half the skin, so the rows are rebuilt in mid-run, two images deep -- and two end outside the box.  The
    reference's own reordering noise on this run is 1e-16 A and 1e-17 A/fs
    (tests/test_row_edges_host.py::test_reordering_noise_of_the_reference_trajectories).  Then one sampled step FROM the reference's end state"""
    x, box, t, masses, v = nve_case("hot")
    xr, vr = ref_cu.nve(x, v, box, t, masses, 1.0, NVE_STEPS)
    moved, outside = moved_and_outside(x, xr, box)
    assert moved > 0.5 and outside >= 1, (moved, outside)          # (else the test checks nothing new)
    e = _engine()
    try:
        e.eam_configure("cu", CUAG)
        e.register_replica("cu", 1, capi.bare_system(t, x, box, v=v, masses=MASS))
        e.set_state(0, "cu", 1, box, x, v)
        e.debug_run("cu", 1, NVE_STEPS, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        builds = e.profile()["neigh_builds"]
        _, xg, vg = e.get_state(0, "cu", 1)
        dx = np.abs(en.minimage_diff(xg, xr, box)).max()
        print(f"eam nve hot gas, {NVE_STEPS} steps: {builds} builds, largest move {moved:.2f} A, {outside} atom(s) outside; position difference "
              f"{dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert builds >= 2
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        e.set_state(1, "cu", 1, box, xr, vr)
        p = e.debug_run("cu", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref_cu.nve(xr, vr, box, t, masses, 1.0, 1)
        want = ref_cu.pressure_atm(x1, v1, box, t, masses)
        print(f"eam sampled pressure hot gas (atm): max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


# ---- 7. a launch ragged in atom count ----
@pytest.fixture(scope="module")
def ragged(four_file):
    """Eight simulations (the smallest batch that runs as two parts) over 4, 1 200, 32 and 108 atoms, the 32-atom ones under the
    four-element file; each material under its own id; 10 straining steps, nss 10; and each one's stress alone in a fresh engine"""
    mats = {"c4": (en.case_cell4(), CUAG, ("Cu",), MASS), "big": (en.case_count(1200), CUAG, ("Cu",), MASS),
            "four": (en.case_four(4), four_file, tuple(en.FOUR), _masses(en.FOUR)), "j108": (en.case_jitter(3), CUAG, ("Cu",), MASS)}
    vel = {m: rk.velocities(np.zeros(len(c[0][0]), int), MASS, 300.0, 60 + k) for k, (m, c) in enumerate(sorted(mats.items()))}
    sims = []
    for q, m in enumerate(["c4", "big", "four", "j108", "j108", "four", "big", "c4"]):      # (both parts hold every size)
        L = mats[m][0][1][3:6] - mats[m][0][1][:3]
        ezz = 4e-4 + 5e-5 * q          # norm below 1e-3 = 10 steps of dt 1 at the rate 1e-4
        sims.append((q, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))
        assert _nts_and_rates(sims[-1][2], mats[m][0][1], 1.0, 1e-4)[0] == 10
    assert sorted(len(c[0][0]) for c in mats.values()) == [4, 32, 108, 1200]

    def fresh(only=None):
        e = _engine()
        for m, ((x, box, t), path, el, masses) in mats.items():
            if only is None or m == only:
                e.eam_configure(m, path, el)
                e.register_replica(m, 1, capi.bare_system(t, x, box, v=vel[m], masses=masses))
        return e

    mk = lambda q, m, s: capi.make_sim(q, m, 1, s, nss=10, dt=1.0, temperature=300.0, strain_rate=1e-4, most_recent=capi.QP_NONE)
    alone = []
    for q, m, s in sims:
        e = fresh(m)
        alone.append(np.array(e.strain_batch([mk(q, m, s)])[0].stress[:]))
        e.close()
    return fresh, [mk(*s) for s in sims], np.array(alone), [m for _, m, _ in sims]


def _ragged_batch(ragged, split, forces=False):
    fresh, sims, alone, mat_of = ragged
    e = fresh()
    try:
        e.batch_split(split)
        out = np.array([list(o.stress) for o in e.strain_batch(sims)])
        err = np.abs(out - alone).max(axis=1) / np.abs(alone).max(axis=1)
        builds = e.profile()["neigh_builds"]
        print(f"eam ragged batch of 8 (split {split}): {builds} builds, rel err per simulation {' '.join('%.1e' % v for v in err)}")
        assert np.isfinite(out).all() and err.max() <= 1e-9
        if forces:
            g = fresh()
            try:
                for q, m in enumerate(mat_of):
                    box, x, v = e.get_state(q, m, 1)
                    g.set_state(q, m, 1, box, x, v)
                    a, b = e.eam_compute(m, 1, qp=q), g.eam_compute(m, 1, qp=q)
                    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]), (q, m)
                    assert a["npairs"] == b["npairs"] and a["nabove"] == b["nabove"]      # (the energies are atomic sums over workgroups: not compared by bit)
            finally:
                g.close()
        return builds
    finally:
        e.close()


@pytest.mark.parametrize("split", [0, 1])
def test_ragged_launch_equals_each_alone(ragged, split):
    """The batch against the SAME code in another launch shape: admissible only because tests/test_gpu_eam.py (the 4-atom cell, 108 and
    1 200 atoms) and test_static_parity_four_element_file pin each member's alone path against numpy.  Then the forces on every end state,
    evaluated in the engine that ran the batch (its slots hold rows and F' of simulations of other sizes) and in a fresh engine handed the
    same state: equal bit for bit"""
    _ragged_batch(ragged, split, forces=True)


def test_ragged_launch_overflows_and_retries(ragged, monkeypatch):
    """the same batch from row capacities forced low (the overflow test hook): every member overflows, the batch regrows and retries"""
    normal = _ragged_batch(ragged, 1)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    assert _ragged_batch(ragged, 1) >= normal + 8          # (the attempt that overflowed built every member's rows once, too)
