"""The mesh reciprocal solver of the Ewald ionic force stage on the GPU (md_born_long_mesh.hip, BlStage of engine_rowpot.cpp: PPPM on the
row driver, scema_md_born_long_kspace) against the independent FP64 numpy restatement tests/born_long_mesh_numpy.py, which
tests/test_born_long_mesh_host.py pins on the CPU.  numpy evaluates on the mesh and the g_ewald of its own copy of the rule, after the
device's mesh (exact) and g (1e-9 relative, the budget of two implementations of adjust_gewald's Newton step) are held against them, so
the budgets measure the kernels and not the accuracy of the method.

Budgets, those of tests/test_gpu_born_long.py: static parity 1e-10 of the largest force component, energy term and virial part; NVE after
20 steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; an update against its debug runs 1e-10; a batch against each simulation alone
1e-9, its forces bit for bit.  The forces of one ion are measured on K e^2/A^2 (1e-12).  The fixed-point charge grid resolves 2^-60 of its
largest possible value, seven digits below these budgets.

What the groups catch.  The needle: the replica the Ewald sum refuses (index 24 > 20) now computes under a `pppm` script, and is still
refused under `ewald` and under mode 2.  One ion: self, background and image energy on the mesh with no pair.  Two ions in a 6 A cube: an
8^3 mesh with every stencil wrapping.  63, 64, 65 ions: the edges of the atom tiles and of the 16-lane groups, cells that are not neutral
(the background term in energy and virial).  48 ions in a 1 x 2 x 3 box: a mesh that differs per dimension.  The triclinic cell: tilted
wave vectors and ions outside the box.  512 ions: 24^3, several workgroups per grid.  MgO: metal units, the table's K.  The batches: three
meshes in one launch (several transform runs), both part streams (a plan per stream), mesh and Ewald replicas side by side.  The
straining run: the influence function recomputed on every step, and the box of the step after a flip in xy and one in xz.
"""
import os

import numpy as np
import pytest

import born_long_mesh_numpy as bm
import born_long_numpy as bl
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_long")
MGO = os.path.join(ROOT, "tests", "golden", "MgO.buck_long")
MASS_NACL, MASS_MGO = (bl.NA_MASS, bl.CL_MASS), (bl.MG_MASS, bl.O_MASS)
EWALD_REFUSAL = r"rc=1: .*needs \d+ k-vectors \(indices up to 2 2 26\) at accuracy 1e-05: the Ewald sum of the row driver holds 4096 \(indices up to 20\); PPPM on the row driver is the follow-up for replicas of that size"

# mode 1 through the rows kit: configure attaches the material and asks for the mesh
MESH = rk.Pot("born/long mesh", "born_long_mesh_configure", "born_long_compute", "Born/long", ("e_born", "e_coul"), ("npairs", "ncoul"),
              counts="ordered pairs {npairs}, mesh {got[mesh]}, g {got[g_ewald]:.6f}", ionic=True,
              energy_scale=("e_born", "e_coul", "e_real", "e_recip", "e_self"))


@pytest.fixture(scope="module")
def ref_nacl():
    return bm.BornLongMesh(bl.read_born_long(NACL))


@pytest.fixture(scope="module")
def ref_mgo():
    return bm.BornLongMesh(bl.read_born_long(MGO))


def _mgo_case(seed=17):
    x, box, t, q = bl.case_jitter(2, seed, sigma=0.1, a=4.3)
    return x, box, t, 1.2 * q


def _static(case, path=NACL, masses=MASS_NACL, mode=1):
    """the static hook on one replica in a fresh engine under that solver mode, with the mesh it reports"""
    x, box, t, q = case
    e = rk.engine()
    try:
        e.born_long_configure("m", path)
        e.born_long_kspace("m", mode)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, masses))
        got = e.born_long_compute("m", 1)
        got["mesh"] = e.born_long_last_mesh()
        return got
    finally:
        e.close()


def _reference(ref, got, x, box, t, q):
    """numpy on the mesh and the g of its own rule, after holding the device's against them"""
    g, grid = ref.setup(box, q)
    assert got["nk"] == 0 and got["mesh"] == grid and abs(got["g_ewald"] - g) <= 1e-9 * g, (got["nk"], got["mesh"], grid, got["g_ewald"], g)
    return ref.compute(x, box, t, q, g, grid)


def _check(got, ref, what, K=None):
    rk.check_static(got, ref, MESH, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, what=what, fs=K * 1e-2 if K else None,
                    ws=max(np.abs(ref[k]).max() for k in ("w_born", "w_real", "w_recip")))


def _static_case(ref, case, what, path=NACL, masses=MASS_NACL, K=None, mode=1):
    got = _static(case, path, masses, mode)
    want = _reference(ref, got, *case)
    _check(got, want, what, K=K)
    return got, want


# ---- fails without the feature ----
def test_the_needle_the_ewald_sum_refuses_runs_on_the_mesh_under_a_pppm_script(ref_nacl, tmp_path):
    """the jittered 1 x 1 x 16 cell (128 ions; the kmax search of the Ewald rule gives 2 2 24, the list reaches index 26) under
    NaCl.born_long with `kspace_style pppm 1.0e-5`, mode 0: the mesh 9 x 9 x 60, static parity, and its force within 2.0 x accuracy x K
    (rms) of the Ewald sum at accuracy 1e-12; under `ewald`, and under mode 2, refused with the message of the Ewald sum"""
    case = bm.case_needle()
    x, box, t, q = case
    assert len(x) == 128
    pppm = tmp_path / "pppm.born_long"
    pppm.write_text(open(NACL).read().replace("kspace_style ewald 1.0e-5", "kspace_style pppm 1.0e-5"))
    got, want = _static_case(ref_nacl, case, "born/long mesh, the 1 x 1 x 16 needle under a pppm script (mode 0)", path=str(pppm), mode=0)
    assert got["mesh"] == (9, 9, 60)
    rms = bm.rms_force_error(got["f"], bl.BornLong(ref_nacl.p, accuracy=1e-12).compute(x, box, t, q)["f"], 1e-5, ref_nacl.K)
    print(f"needle: rms force error against the Ewald sum at 1e-12 over accuracy x K: {rms:.3f}")
    assert rms <= 2.0
    for path, mode in ((NACL, 0), (str(pppm), 2)):
        with pytest.raises(capi.EngineError, match=EWALD_REFUSAL):
            _static(case, path, MASS_NACL, mode)


# ---- mode 1, static parity ----
def test_one_ion_has_self_background_and_image_energy(ref_nacl):
    got, want = _static_case(ref_nacl, bl.case_single(), "born/long mesh one ion", K=ref_nacl.K)
    assert got["mesh"] == (9, 9, 9) and want["npairs"] == 0 and want["e_bg"] < 0.0 and want["e_recip"] > 0.0 and got["e_born"] == 0.0
    assert np.abs(got["f"]).max() <= 1e-12 * ref_nacl.K


def test_two_ions_in_a_six_angstrom_cube(ref_nacl):
    got, _ = _static_case(ref_nacl, bl.case_two(), "born/long mesh two ions, 6 A cube")
    assert got["mesh"] == (8, 8, 8)


def test_the_eight_ion_cell(ref_nacl):
    got, _ = _static_case(ref_nacl, bl.case_jitter(1, 1), "born/long mesh 8-ion cell, jittered")
    assert got["mesh"] == (8, 8, 8)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_around_the_atom_tile_width(ref_nacl, n):
    j64 = bl.case_jitter(2, 1)
    case = {63: bl.case_without(j64, [37]), 64: j64, 65: bl.case_with_extra(j64)}[n]
    assert len(case[0]) == n and (abs(np.sum(case[3])) == 1.0) == (n != 64)
    got, want = _static_case(ref_nacl, case, f"born/long mesh {n} ions")
    assert got["mesh"] == (15, 15, 15)
    if n != 64:
        assert abs(want["e_bg"]) > 0.0


def test_48_ions_on_a_mesh_that_differs_per_dimension(ref_nacl):
    case = bl.case_jitter((1, 2, 3), 3)
    got, _ = _static_case(ref_nacl, case, "born/long mesh 48 ions, 5.64 x 11.28 x 16.92 A")
    assert got["mesh"] == (8, 15, 16)


def test_triclinic_box_with_ions_outside(ref_nacl):
    case = bl.case_triclinic()
    s = (case[0] - case[1][:3]) @ np.linalg.inv(bl.h_matrix(case[1]))
    assert ((s < 0.0) | (s >= 1.0)).any(axis=1).sum() >= 8
    got, _ = _static_case(ref_nacl, case, "born/long mesh triclinic, ions outside the box")
    assert got["mesh"] == (15, 15, 12)


def test_512_ions_on_24_cubed(ref_nacl):
    got, _ = _static_case(ref_nacl, bl.case_jitter(4, 2), "born/long mesh 512 ions")
    assert got["mesh"] == (24, 24, 24)


def test_buckingham_fixture_in_metal_units(ref_mgo):
    got, _ = _static_case(ref_mgo, _mgo_case(), "buck/long mesh MgO, 64 ions", path=MGO, masses=MASS_MGO)
    assert ref_mgo.p["style"] == "buck" and ref_mgo.p["unit"] == 0 and abs(ref_mgo.K - bl.K_EV * bl.EV_TO_KCALMOL) < 1e-12


def test_the_default_is_untouched():
    """mode 0 inside the Ewald limits: the `pppm` script of MgO.buck_long keeps its 61 k-vectors, the 64-ion cell its 128, no mesh"""
    for case, path, masses, nk in ((_mgo_case(), MGO, MASS_MGO, 61), (bl.case_jitter(2, 1), NACL, MASS_NACL, 128)):
        got = _static(case, path, masses, mode=0)
        assert got["nk"] == nk and got["mesh"] == (0, 0, 0)


# ---- bits ----
def test_two_evaluations_of_one_state_agree_bit_for_bit():
    case = bl.case_jitter(2, 7)
    e = rk.engine()
    try:
        e.born_long_mesh_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(case[2], case[3], case[0], case[1], MASS_NACL))
        a, b = e.born_long_compute("m", 1), e.born_long_compute("m", 1)
    finally:
        e.close()
    c = _static(case)
    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]) and np.array_equal(a["f"], c["f"])


def _batch(mats, n, seed):
    """n simulations dealt over the materials of `mats` (name -> (case, path, masses, solver mode)) in the sorted order of the names,
    velocities of 300 K from the seeds 7, 8, .., strains of 10 to 30 straining steps: a ragged batch; and each one's stress alone"""
    names = sorted(mats)
    vel = {m: rk.velocities(mats[m][0][2], mats[m][2], 300.0, 7 + k) for k, m in enumerate(names)}
    rng = np.random.default_rng(seed)
    sims = []
    for q in range(n):
        m = names[q % len(names)]
        box = mats[m][0][1]
        L = box[3:6] - box[:3]
        ezz = rng.uniform(5e-4, 2.5e-3)
        sims.append((q, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))

    def fresh():
        e = rk.engine()
        for m, (case, path, masses, mode) in mats.items():
            e.born_long_configure(m, path)
            e.born_long_kspace(m, mode)
            e.register_replica(m, 1, capi.ionic_system(case[2], case[3], case[0], case[1], masses, v=vel[m]))
        return e

    mk = lambda q, m, s: capi.make_sim(q, m, 1, s, most_recent=capi.QP_NONE, **rk.UPDATE)
    alone = []
    for q, m, s in sims:
        e = fresh()
        alone.append(np.array(e.strain_batch([mk(q, m, s)])[0].stress[:]))
        e.close()
    return rk.Batch(fresh, [mk(*s) for s in sims], np.array(alone), [m for _, m, _ in sims])


@pytest.fixture(scope="module")
def nine():
    """9 simulations (two part streams) in mode 1 over both fixtures and three sizes: 64 ions of NaCl (15^3), 48 ions of NaCl in the
    1 x 2 x 3 box (8 x 15 x 16), 64 ions under MgO.buck_long (its mesh at accuracy 1e-4): three meshes in one launch"""
    return _batch({"nacl64": (bl.case_jitter(2, 6, sigma=0.08), NACL, MASS_NACL, 1), "nacl48": (bl.case_jitter((1, 2, 3), 3, sigma=0.08), NACL, MASS_NACL, 1),
                   "mgo64": (_mgo_case(), MGO, MASS_MGO, 1)}, 9, 21)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_nine_on_three_meshes_equals_each_alone(nine, split):
    """whole (split 0) and as part batches on two streams (split 1): stresses 1e-9, the forces on every end state bit for bit"""
    rk.assert_batch_vs_alone(MESH, nine, split, what="born/long mesh batch of 9 on three meshes", tol=1e-9, bitwise_forces=True)


def test_a_plan_per_stream_and_no_more_on_a_repeat(nine):
    """the batch whole uses the plans of the main stream; as two parts it adds those of the second stream (and of the parts' batch
    counts); the same batch again adds none"""
    e = nine.fresh()
    try:
        e.batch_split(0)
        e.strain_batch(nine.sims)
        whole = e.pppm_plan_count()
        e.batch_split(1)
        e.strain_batch(nine.sims)
        parts = e.pppm_plan_count()
        e.strain_batch(nine.sims)
        print(f"born/long mesh hipFFT plans: whole {whole}, as two parts {parts}, repeated {e.pppm_plan_count()}")
        assert whole > 0 and parts > whole and e.pppm_plan_count() == parts
    finally:
        e.close()


@pytest.fixture(scope="module")
def mixed():
    """9 simulations, mesh and Ewald replicas side by side in one launch: NaCl 64 ions on the mesh (mode 1), MgO 64 ions on its Ewald sum
    (mode 0, nk 61), NaCl 48 ions forced to the Ewald sum (mode 2)"""
    return _batch({"nacl64": (bl.case_jitter(2, 6, sigma=0.08), NACL, MASS_NACL, 1), "mgo64": (_mgo_case(), MGO, MASS_MGO, 0),
                   "nacl48": (bl.case_jitter((1, 2, 3), 3, sigma=0.08), NACL, MASS_NACL, 2)}, 9, 22)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_mesh_and_ewald_replicas_equals_each_alone(mixed, split):
    rk.assert_batch_vs_alone(MESH, mixed, split, what="born/long batch of mesh and Ewald replicas", tol=1e-9, bitwise_forces=True)


# ---- dynamics ----
def test_nve_dynamics_and_sampled_pressure(ref_nacl):
    x, box, t, q = bl.case_jitter(2, 6, sigma=0.08)
    v = rk.velocities(t, MASS_NACL, 300.0, 1)
    e = rk.engine()
    try:
        e.born_long_mesh_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        e.debug_run("nacl", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "nacl", 1)
        xr, vr = ref_nacl.nve(x, v, box, t, q, MASS_NACL, 1.0, 20)
        dx = np.abs(bl.minimage_diff(xg, xr, box)).max()
        print(f"born/long mesh nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        # the virial -> pressure conversion on a strained cell: one step with sampling gives (sum m v v + W) / V of the state after it, in atm
        xs, bs = bl.strained(x, box, np.array([[0.01, 0.004, 0.0], [0.0, -0.006, 0.003], [0.0, 0.0, 0.008]]))
        e.set_state(1, "nacl", 1, bs, xs, v)
        p = e.debug_run("nacl", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        g, grid = ref_nacl.setup(bs, q)
        x1, v1 = ref_nacl.nve(xs, v, bs, t, q, MASS_NACL, 1.0, 1)
        want = ref_nacl.pressure_atm(x1, v1, bs, t, q, MASS_NACL, g, grid)
        print(f"born/long mesh sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


def test_a_straining_run_whose_box_flips_in_xy_and_in_xz(ref_nacl):
    """16 steps of NVE under fix deform from a box tilted close to both flips: xy passes half a box length after step 6, xz after step 10.
    numpy takes the box of each step, the flipped one after a flip, as the device does: the mesh 15 x 18 x 18 of the start box stays, the
    influence function follows the box.  End box, end positions and the pressure sampled at every step"""
    (x, box, t, q), rates = bl.case_flip()
    nsteps, L = 16, box[3] - box[0]
    ratio = lambda k, step: (box[6 + k] + rates[3 + k] * L * step) / L
    cross = [min(s for s in range(1, nsteps) if ratio(k, s) > 0.50001) for k in (0, 1)]
    assert cross == [6, 10] and ratio(0, 0) < 0.5 and ratio(1, 0) < 0.5
    v = rk.velocities(t, MASS_NACL, 300.0, 9)
    xr, vr, box_r, p_r, flips_r = ref_nacl.nve(x, v, box, t, q, MASS_NACL, 1.0, nsteps, rates=rates)
    assert flips_r == 2 and ref_nacl.setup(box, q)[1] == (15, 18, 18)
    e = rk.engine()
    try:
        e.born_long_mesh_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        p = e.debug_run("nacl", 1, nsteps, 1.0, 300.0, qp=0, nvt=False, use_shake=False, rates=rates, sample=True)
        bg, xg, vg = e.get_state(0, "nacl", 1)
        flips = e.profile()["box_flips"]
    finally:
        e.close()
    print(f"born/long mesh flips {flips}, end tilts device {bg[6:9]}, numpy {box_r[6:9]}")
    assert flips == 2 and np.abs(bg[6:9] - box_r[6:9]).max() < 1e-9 and np.abs(bg[:6] - box_r[:6]).max() < 1e-12
    dx = np.abs(bl.minimage_diff(xg, xr, box_r)).max()
    dp = np.abs(p - p_r).max() / np.abs(p_r).max()
    print(f"born/long mesh straining run with two flips: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs, pressure {dp:.2e}")
    assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11 and dp <= 1e-10


def test_strain_batch_equals_the_two_runs_and_a_second_update_continues():
    """an update against the straining run and the sampling run issued through the parity hooks; then a second update from the stored
    states: qp 0 continues from its own, qp 1 branches from qp 0's"""
    x, box, t, q = bl.case_jitter(2, 8, sigma=0.08)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s2 = np.array([1.0e-3 * L[0], 0.0, 1.0e-3 * L[2], 0.0, 0.0, 0.0])
    s = rk.Setup("nacl", NACL, None, MASS_NACL, (x, box, t, q), rk.velocities(t, MASS_NACL, 300.0, 2))
    rk.strain_batch_and_a_second_update(MESH, s, s1, s2, tol=1e-10)


# ---- rows through cells ----
def _cells_static(monkeypatch, cells, case):
    monkeypatch.setenv("SCEMA_MD_ROW_CELLS", str(cells))     # (the engine has no parameter for it: the switch is read when the engine is made)
    x, box, t, q = case
    e = rk.engine()
    try:
        e.born_long_mesh_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS_NACL))
        out = e.born_long_compute("m", 1)
        out["rows"], out["prof"], out["mesh"] = e.debug_rows(0, rows=False), e.profile(), e.born_long_last_mesh()
        return out
    finally:
        e.close()


def test_cell_binned_row_build_under_the_mesh(monkeypatch):
    """SCEMA_MD_ROW_CELLS=1 on 1 728 ions (36^3): the same rows in the same order and the same mesh chain, so the forces of the N^2 rows
    bit for bit"""
    case = bl.case_jitter(6, 9, sigma=0.08)
    assert len(case[0]) == 1728
    on, off = _cells_static(monkeypatch, 1, case), _cells_static(monkeypatch, 0, case)
    assert (on["rows"]["cells"], off["rows"]["cells"]) == (1, 0) and on["prof"]["row_cell_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0
    assert on["mesh"] == off["mesh"] == (36, 36, 36) and on["nk"] == off["nk"] == 0
    assert (on["npairs"], on["ncoul"]) == (off["npairs"], off["ncoul"]) and np.abs(off["f"]).max() > 0.0
    assert np.array_equal(on["f"], off["f"])


# ---- refusals ----
def test_refusals(tmp_path):
    x, box, t, q = bl.case_jitter(4, 2)
    tight = tmp_path / "tight.born_long"
    tight.write_text(open(NACL).read().replace("kspace_style ewald 1.0e-5", "kspace_style pppm 1.0e-12"))
    e = rk.engine()
    try:
        e.born_long_configure("big", str(tight))
        e.register_replica("big", 1, capi.ionic_system(t, q, x, box, MASS_NACL))
        # mode 0: the k list of 512 ions at 1e-12 is over the Ewald limit and the script says pppm, so the mesh is tried: 800^3
        for mode in (0, 1):
            e.born_long_kspace("big", mode)
            with pytest.raises(capi.EngineError, match=r"rc=1: a Born/long replica of 512 atoms needs a mesh of 800 x 800 x 800 = 512000000 points at accuracy 1e-12: "
                                                       r"the mesh solver of the row driver holds 4194304"):
                e.born_long_compute("big", 1)
        for mode in (-1, 3):
            with pytest.raises(capi.EngineError, match=rf"rc=1: reciprocal solver mode {mode} "):
                e.born_long_kspace("big", mode)
        with pytest.raises(capi.EngineError, match=r"rc=1: no Born/long potential attached to material none \(scema_md_born_long_configure\)"):
            e.born_long_kspace("none", 1)
    finally:
        e.close()
