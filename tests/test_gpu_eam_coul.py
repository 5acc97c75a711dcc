"""The EAM + long-range Coulomb stage on the GPU (md_eam_coul.hip, engine_rowpot.cpp: `pair_style hybrid/overlay coul/long <cut_coul>
eam/alloy` with `kspace_style ewald|pppm <accuracy>`) against the FP64 numpy restatement tests/eam_coul_numpy.py, the sum of
tests/eam_numpy.py on the setfl cutoff and tests/born_long_numpy.py with all Born constants zero (no LAMMPS exists to compare with).  numpy
evaluates on the g_ewald and the integer triples the device reports having used (nk and g are compared with numpy's own copy of the rule
first), so the budgets measure the kernels and not the accuracy of the Ewald sum.

Budgets, those of tests/test_gpu_born_long.py: static parity 1e-10 of the largest force component, energy term and virial part; NVE after 20
steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; whole evaluations 1e-10 (an update against its two runs) and 1e-9 (a batch against
each simulation alone).  The forces of one ion are measured on K e^2/A^2 (1e-12).  Composition on the device: the stage against the sum
of the EAM stage and the Born/long stage with zero Born constants, 2e-10 (the sum of the two parents' 1e-10), and against the EAM stage
alone with all charges zero, 1e-13; the scales are per quantity, as in the parents' parity budgets: forces on the largest force component,
the virial on the largest virial component, the energy on the largest energy term of the two parents: the same table records go through the same arithmetic in the same order, what is left is the
rounding of one sum against two.  The mesh against the Ewald sum at accuracy 1e-12: an rms force error of 2.0 x accuracy x K, the bound
of tests/test_gpu_born_long_mesh.py.

The static hook returns one virial, the sum of its parts; it is held on the largest of the reference's three parts (EAM, real space,
reciprocal), as the Born/long file holds its own.

What the groups catch.  One ion: self and image energy with no pair and no density.  The O-U-O trimers: each term is exactly zero beyond
its own cutoff, whichever of the two is larger (UO2.eam_coul: cut_coul 9 above the setfl cutoff 7; UO2_short.eam_coul: 6 below it).  One
fluorite cell of 12 ions: both cutoffs exceed the box, an atom pairs with its own images.  96 ions with a tilt: the k-vectors of a
triclinic box.  97 and 65 ions: a net charge (the background term), the ragged tail of a tile of 64.
"""
import os

import numpy as np
import pytest

import born_long_mesh_numpy as bm
import eam_coul_numpy as ec
import eam_numpy as en
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LONG, SHORT, SETFL = (os.path.join(GOLDEN, n) for n in ("UO2.eam_coul", "UO2_short.eam_coul", "UO2.eam.alloy"))
CUAG = os.path.join(GOLDEN, "CuAg.eam.alloy")
MASS = (ec.O_MASS, ec.U_MASS)
ROW_TILE = 64

EAM_COUL = rk.Pot("eam/coul", "eam_coul_configure", "eam_coul_compute", "EAM/coul", ("e_eam", "e_coul"), ("npairs", "ncoul"),
                  counts="ordered pairs {npairs} / {ncoul}, nk {got[nk]}, g {got[g_ewald]:.6f}", ionic=True,
                  energy_scale=("e_pair", "e_embed", "e_coul", "e_real", "e_recip", "e_self"))


@pytest.fixture(scope="module")
def refs():
    return {LONG: ec.EamCoul(ec.read_eam_coul(LONG)), SHORT: ec.EamCoul(ec.read_eam_coul(SHORT))}


@pytest.fixture(scope="module")
def c96():
    """2 x 2 x 2 fluorite cells, 96 ions, rattled by 0.1 A, xy tilt 0.3 lx"""
    return ec.case_rattled(2, 5, tilt_xy=0.3)


def _static(case, path=LONG, mode=0):
    x, box, t, q = case
    e = rk.engine()
    try:
        e.eam_coul_configure("m", path)
        e.eam_coul_kspace("m", mode)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS))
        got = e.eam_coul_compute("m", 1)
        got["mesh"] = e.eam_coul_last_mesh()
        return got
    finally:
        e.close()


def _reference(ref, got, x, box, t, q):
    """numpy on the g and the triples of the rule, after holding the device's nk and g against them"""
    g, tr = ref.setup(box, q)
    assert got["nk"] == len(tr) and abs(got["g_ewald"] - g) <= 1e-14 * g, (got["nk"], len(tr), got["g_ewald"], g)
    return ref.compute(x, box, t, q, g, tr)


def _check(got, ref, what, K=None):
    rk.check_static(got, ref, EAM_COUL, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, what=what, fs=K * 1e-2 if K else None,
                    ws=max(np.abs(ref[k]).max() for k in ("w_eam", "w_real", "w_recip")))


def _static_case(refs, case, what, path=LONG, K=None):
    got = _static(case, path)
    want = _reference(refs[path], got, *case)
    _check(got, want, what, K=K)
    return got, want


# ---- 1. static parity ----
def test_one_ion_has_self_and_image_energy_and_no_force(refs):
    K = refs[LONG].K
    got, want = _static_case(refs, ec.case_single(), "eam/coul one ion", K=K)
    assert (got["npairs"], got["ncoul"]) == (0, 0) and got["e_eam"] == 0.0 and want["e_self"] < 0.0 and want["e_recip"] > 0.0
    assert abs(want["e_bg"]) > 0.0 and np.abs(got["f"]).max() <= 1e-12 * K


@pytest.mark.parametrize("path,cut,npairs,ncoul", [(LONG, 7.0, 2, 4), (LONG, 9.0, 0, 2), (SHORT, 7.0, 2, 0), (SHORT, 6.0, 4, 2)],
                         ids=["long-eam", "long-coul", "short-eam", "short-coul"])
def test_trimer_with_one_arm_inside_and_one_outside_a_cutoff(refs, path, cut, npairs, ncoul):
    """O-U-O in a 30 A box, one arm 0.05 A inside and one 0.05 A outside `cut`: the term of that cutoff counts one arm (both ends), the
    other term what its own cutoff says; a term is exactly 0 beyond its cutoff, so a trimer outside cut_coul (inside the setfl cutoff)
    has exactly no real-space Coulomb energy, and the other way round"""
    case = ec.case_trimer(cut, cut)
    got, want = _static_case(refs, case, f"eam/coul trimer at {cut} A under {os.path.basename(path)}", path=path)
    assert (got["npairs"], got["ncoul"]) == (npairs, ncoul) == (want["npairs"], want["ncoul"])
    if npairs == 0:
        # (no pair inside the setfl cutoff: no density, F(0) = 0, no phi)
        assert got["e_eam"] == 0.0 and want["e_eam"] == 0.0
    if ncoul == 0:
        # (no pair inside cut_coul: E_coul is the reciprocal sum, self and background alone; numpy's real-space part is exactly 0)
        assert want["e_real"] == 0.0 and not want["w_real"].any()
        assert abs(got["e_coul"] - (want["e_recip"] + want["e_self"] + want["e_bg"])) <= 1e-10 * abs(want["e_self"])


@pytest.mark.parametrize("path", [LONG, SHORT], ids=["long", "short"])
def test_one_fluorite_cell_narrower_than_both_cutoffs(refs, path):
    case = ec.case_rattled(1, 3)
    assert len(case[0]) == 12 and case[1][3] < 6.0
    got, _ = _static_case(refs, case, f"eam/coul 12-ion cell under {os.path.basename(path)}", path=path)
    assert got["npairs"] > 12 * 60 and got["maxrow"] > 12          # (an atom pairs with its own images)


@pytest.mark.parametrize("path", [LONG, SHORT], ids=["long", "short"])
def test_96_ions_in_a_tilted_box(refs, c96, path):
    assert len(c96[0]) == 96 and c96[1][6] == 0.3 * (c96[1][3] - c96[1][0])
    got, _ = _static_case(refs, c96, f"eam/coul 96 ions, xy tilt 0.3, under {os.path.basename(path)}", path=path)
    assert got["mesh"] == (0, 0, 0) and got["nk"] > 128


@pytest.mark.parametrize("n", [ROW_TILE + 1, 97])
def test_a_net_charge_and_the_ragged_tail_of_a_tile(refs, c96, n):
    """97: the 96-ion replica with one interstitial O; 65: the same with 32 ions taken out, one more than a tile"""
    case = ec.case_with_interstitial(c96)
    if n == ROW_TILE + 1:
        keep = np.ones(97, bool)
        keep[np.random.default_rng(8).choice(96, 32, replace=False)] = False
        case = (case[0][keep], case[1], case[2][keep], case[3][keep])
    assert len(case[0]) == n and abs(np.sum(case[3])) > 1.0
    _, want = _static_case(refs, case, f"eam/coul {n} ions, net charge {np.sum(case[3]):+.4f}")
    assert abs(want["e_bg"]) > 0.0


def test_two_evaluations_of_one_state_agree_bit_for_bit(c96):
    x, box, t, q = c96
    e = rk.engine()
    try:
        e.eam_coul_configure("m", LONG)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS))
        a, b = e.eam_coul_compute("m", 1), e.eam_coul_compute("m", 1)
    finally:
        e.close()
    c = _static(c96)
    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]) and np.array_equal(a["f"], c["f"])


# ---- 2. composition on the device ----
def test_the_stage_equals_the_sum_of_its_two_parents_on_the_device(c96, tmp_path):
    """the 96-ion replica under UO2.eam_coul against scema_md_eam_debug_compute on the same setfl file plus
    scema_md_born_long_debug_compute on a script of the same cut_coul, accuracy and solver with zero Born constants: forces, virial and
    E_eam + E_coul to 2e-10 of the largest force component, virial component and energy term of the two parents"""
    x, box, t, q = c96
    zero = tmp_path / "zero.born_long"
    zero.write_text("units metal\npair_style born/coul/long 9.0\nkspace_style ewald 1.0e-5\npair_coeff * * 0.0 1.0 0.0 0.0 0.0\n")
    got = _static(c96)
    e = rk.engine()
    try:
        e.eam_configure("eam", SETFL, ("O", "U"))
        e.register_replica("eam", 1, capi.bare_system(t, x, box, masses=MASS))
        a = e.eam_compute("eam", 1)
        e.born_long_configure("coul", str(zero))
        e.register_replica("coul", 1, capi.ionic_system(t, q, x, box, MASS))
        b = e.born_long_compute("coul", 1)
    finally:
        e.close()
    assert b["e_born"] == 0.0 and (b["nk"], b["g_ewald"]) == (got["nk"], got["g_ewald"]) and (a["npairs"], b["ncoul"]) == (got["npairs"], got["ncoul"])
    fs = max(np.abs(a["f"]).max(), np.abs(b["f"]).max())
    ws = max(np.abs(a["w"]).max(), np.abs(b["w"]).max())
    es = max(abs(a["e_pair"]), abs(a["e_embed"]), abs(b["e_coul"]))
    df = np.abs(got["f"] - (a["f"] + b["f"])).max() / fs
    dw = np.abs(got["w"] - (a["w"] + b["w"])).max() / ws
    de = abs(got["e_eam"] + got["e_coul"] - (a["e_pair"] + a["e_embed"] + b["e_coul"])) / es
    print(f"eam/coul against eam + born/long on the device: force {df:.2e}, virial {dw:.2e}, energy {de:.2e}")
    assert df <= 2e-10 and dw <= 2e-10 and de <= 2e-10


def test_with_all_charges_zero_the_stage_is_the_eam_stage(c96):
    x, box, t, q = c96
    got = _static((x, box, t, np.zeros(len(q))))
    e = rk.engine()
    try:
        e.eam_configure("eam", SETFL, ("O", "U"))
        e.register_replica("eam", 1, capi.bare_system(t, x, box, masses=MASS))
        a = e.eam_compute("eam", 1)
    finally:
        e.close()
    df = np.abs(got["f"] - a["f"]).max() / np.abs(a["f"]).max()
    dw = np.abs(got["w"] - a["w"]).max() / np.abs(a["w"]).max()
    de = abs(got["e_eam"] - (a["e_pair"] + a["e_embed"])) / max(abs(a["e_pair"]), abs(a["e_embed"]))
    print(f"eam/coul with zero charges against eam: force {df:.2e}, virial {dw:.2e}, energy {de:.2e}")
    assert got["e_coul"] == 0.0 and got["npairs"] == a["npairs"] and got["nk"] == 0
    assert df <= 1e-13 and dw <= 1e-13 and de <= 1e-13


def test_the_force_pass_applies_the_setfl_cutoff_to_tables_that_go_on_beyond_it(c96, tmp_path):
    """The fixture's tables are exactly 0 from its cutoff on, so a force pass that forgot its own `r^2 < cut^2` test under a larger
    cut_coul would still agree with numpy.  Here the same tables stand under a STATED cutoff of 5.0 A, where phi and rho are far from
    zero, with cut_coul 9.0: numpy's EAM stops at 5.0 A, and so must both passes on the device (the counter is the density pass's, the
    forces and the virial are the force pass's)"""
    names = ["O", "U"]
    tabs = list(ec.crg_tables(names))
    tabs[4] = 5.0
    en.write_setfl(str(tmp_path / "UO2cut5.eam.alloy"), names, [8, 92], [ec.O_MASS, ec.U_MASS], [ec.A_UO2] * 2, *tabs,
                      ["the tables of UO2.eam.alloy under a stated cutoff of 5.0 A", "written at test time", "units metal"])
    script = tmp_path / "cut5.eam_coul"
    script.write_text(open(LONG).read().replace("UO2.eam.alloy O U", "UO2cut5.eam.alloy O U"))
    ref = ec.EamCoul(ec.read_eam_coul(str(script)))
    assert ref.cutoff == 5.0 and ref.rc == 9.0
    got = _static(c96, str(script))
    want = _reference(ref, got, *c96)
    _check(got, want, "eam/coul 96 ions, tables that go on beyond a stated cutoff of 5.0 A")
    # (what a force pass without the test would add: the EAM force of the whole tables against that of the stated cutoff)
    full = ec.EamCoul(ec.read_eam_coul(LONG)).eam.compute(c96[0], c96[1], ref.tmap[c96[2]])
    assert got["npairs"] == want["npairs"] < full["npairs"] and np.abs(full["f"] - want["f_eam"]).max() > 1e-3 * np.abs(want["f"]).max()


# ---- 3. both solvers and both cutoff orders ----
@pytest.mark.parametrize("path", [LONG, SHORT], ids=["long", "short"])
def test_mesh_and_ewald_modes(refs, c96, path):
    """mode 2: the Ewald sum, static parity, no mesh reported.  mode 1: the mesh numpy's copy of the rule gives, nk 0, and a force within
    2.0 x accuracy x K (rms) of the Ewald sum at accuracy 1e-12"""
    ref = refs[path]
    x, box, t, q = c96
    ew = _static(c96, path, mode=2)
    _check(ew, _reference(ref, ew, *c96), f"eam/coul 96 ions, mode 2, under {os.path.basename(path)}")
    assert ew["mesh"] == (0, 0, 0)
    mesh = _static(c96, path, mode=1)
    g, grid = bm.mesh_rule(box, len(x), float(np.sum(q * q)), ref.rc, ref.p["accuracy"])
    assert mesh["nk"] == 0 and mesh["mesh"] == tuple(grid) and abs(mesh["g_ewald"] - g) <= 1e-9 * g, (mesh["mesh"], grid, mesh["g_ewald"], g)
    assert (mesh["npairs"], mesh["ncoul"]) == (ew["npairs"], ew["ncoul"])
    exact = ec.EamCoul(ref.p, accuracy=1e-12).compute(x, box, t, q)
    rms = bm.rms_force_error(mesh["f"], exact["f"], ref.p["accuracy"], ref.K)
    print(f"eam/coul mesh {mesh['mesh']} under {os.path.basename(path)}: rms force error against the Ewald sum at 1e-12 over accuracy x K: {rms:.3f}")
    assert rms <= 2.0


# ---- 4. dynamics ----
def test_nve_dynamics_and_sampled_pressure(refs):
    """the scenario of rowkit.nve_and_sampled_pressure with the charges the ionic reference takes: 20 steps of NVE against the numpy
    velocity-Verlet stepper, then one step with sampling"""
    ref = refs[LONG]
    x, box, t, q = ec.case_rattled(2, 6, sigma=0.08)
    v = rk.velocities(t, MASS, 300.0, 1)
    s = rk.Setup("uo2", LONG, None, MASS, (x, box, t, q), v)
    e = rk.registered(EAM_COUL, s)
    try:
        e.set_state(0, "uo2", 1, box, x, v)
        e.debug_run("uo2", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "uo2", 1)
        xr, vr = ref.nve(x, v, box, t, q, MASS, 1.0, 20)
        dx = np.abs(ec.minimage_diff(xg, xr, box)).max()
        print(f"eam/coul nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        e.set_state(1, "uo2", 1, box, x, v)
        p = e.debug_run("uo2", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        g, tr = ref.setup(box, q)
        x1, v1 = ref.nve(x, v, box, t, q, MASS, 1.0, 1)
        want = ref.pressure_atm(x1, v1, box, t, q, MASS, g, tr)
        print(f"eam/coul sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


# ---- 5. whole evaluations ----
def test_strain_batch_equals_the_two_runs_and_a_second_update_continues():
    x, box, t, q = ec.case_rattled(2, 8, sigma=0.08)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s2 = np.array([1.0e-3 * L[0], 0.0, 1.0e-3 * L[2], 0.0, 0.0, 0.0])
    s = rk.Setup("uo2", LONG, None, MASS, (x, box, t, q), rk.velocities(t, MASS, 300.0, 2))
    rk.strain_batch_and_a_second_update(EAM_COUL, s, s1, s2, tol=1e-10)


@pytest.fixture(scope="module")
def nine(c96):
    """9 simulations (the smallest batch that runs as two parts) over both scripts, dealt in the sorted order of the names: 96 ions under
    UO2.eam_coul on the Ewald sum, 96 ions under UO2_short.eam_coul on the mesh (mode 1), 97 ions under UO2_short.eam_coul on the Ewald
    sum: one launch holds Ewald and mesh replicas and both cutoff orders; and each one's stress alone in a fresh engine"""
    mats = {"a_long": (ec.case_rattled(2, 6, sigma=0.08), LONG, 0), "b_short_mesh": (ec.case_rattled(2, 7, sigma=0.08), SHORT, 1),
            "c_short": (ec.case_with_interstitial(ec.case_rattled(2, 9, sigma=0.08)), SHORT, 2)}
    names = sorted(mats)
    vel = {m: rk.velocities(mats[m][0][2], MASS, 300.0, 7 + k) for k, m in enumerate(names)}
    rng = np.random.default_rng(21)
    sims = []
    for k in range(9):
        m = names[k % 3]
        L = mats[m][0][1][3:6] - mats[m][0][1][:3]
        ezz = rng.uniform(5e-4, 2.5e-3)
        sims.append((k, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))

    def fresh():
        e = rk.engine()
        for m, (case, path, mode) in mats.items():
            e.eam_coul_configure(m, path)
            e.eam_coul_kspace(m, mode)
            e.register_replica(m, 1, capi.ionic_system(case[2], case[3], case[0], case[1], MASS, v=vel[m]))
        return e

    mk = lambda k, m, s: capi.make_sim(k, m, 1, s, most_recent=capi.QP_NONE, **rk.UPDATE)
    alone = []
    for k, m, s in sims:
        e = fresh()
        alone.append(np.array(e.strain_batch([mk(k, m, s)])[0].stress[:]))
        e.close()
    return rk.Batch(fresh, [mk(*s) for s in sims], np.array(alone), [m for _, m, _ in sims])


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_nine_over_both_scripts_and_solvers_equals_each_alone(nine, split):
    """whole (split 0) and as part batches on two streams (split 1): stresses 1e-9, the forces on every end state bit for bit"""
    rk.assert_batch_vs_alone(EAM_COUL, nine, split, what="eam/coul batch of 9 over both scripts, Ewald and mesh", tol=1e-9, bitwise_forces=True)


@pytest.fixture(scope="module")
def sheared():
    """Eight simulations of a 5 x 2 x 2 fluorite cell (240 ions) written with xy = 2 a = 0.4 lx (the same crystal: a lattice translation),
    each sheared by 0.105 to 0.14 lx in xy, so that every one crosses +lx / 2 and flips once; each one's stress, flips and box alone"""
    x, box, t, q = ec.fluorite(5, 2, 2)
    box[6] = 2.0 * ec.A_UO2
    x = x + np.random.default_rng(12).normal(0.0, 0.05, x.shape)
    return rk.sheared_fixture(EAM_COUL, rk.Setup("uo2", LONG, None, MASS, (x, box, t, q), rk.velocities(t, MASS, 300.0, 31)))


def test_box_flips_inside_a_split_batch(sheared):
    rk.assert_flips_in_split_batch(sheared, "uo2", 1, what="eam/coul sheared batch of 8 (split)", tol=1e-9)


# ---- 6. self-configuration and refusals ----
def test_self_configuration_from_the_scripts_folder(refs, tmp_path):
    """a `pair_style hybrid/overlay` line in in.strain.lammps configures a charged topology-free replica whose material has nothing
    attached, after the two ionic styles found nothing: the update equals the configured one to the batch budget"""
    scripts = tmp_path / "lammps_scripts_uo2"
    scripts.mkdir()
    (scripts / "UO2.eam.alloy").write_bytes(open(SETFL, "rb").read())
    (scripts / "in.strain.lammps").write_text("# straining run\nread_restart ${loco}/init.restart\n" + open(SHORT).read() + "fix 1 all nvt temp 300 300 100\nrun 100\n")
    x, box, t, q = ec.case_rattled(2, 9, sigma=0.08)
    v = rk.velocities(t, MASS, 300.0, 3)
    L = box[3:6] - box[:3]
    ref = ec.EamCoul(ec.read_eam_coul(str(scripts / "in.strain.lammps")))
    outs = []
    for configure in (False, True):
        e = rk.engine()
        try:
            if configure:
                e.eam_coul_configure("ion", str(scripts / "in.strain.lammps"))
            e.register_replica("ion", 1, capi.ionic_system(t, q, x, box, MASS, v=v))
            if not configure:
                rk.assert_not_attached(EAM_COUL, e, "ion")
            o = e.strain_batch([rk.self_configuring_sim("ion", np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), scripts, temperature=300.0, strain_rate=1e-4)])[0]
            assert o.stress_updated == 1
            outs.append(np.array(o.stress[:]))
            got = e.eam_coul_compute("ion", 1)
            _check(got, _reference(ref, got, x, box, t, q), f"eam/coul {'configured' if configure else 'self-configured'}")
        finally:
            e.close()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0] - outs[1]).max() <= 1e-9 * np.abs(outs[1]).max()


def test_refusals(c96, tmp_path):
    x, box, t, q = c96
    (tmp_path / "UO2.eam.alloy").write_bytes(open(SETFL, "rb").read())
    pppm = tmp_path / "pppm.eam_coul"
    pppm.write_text(open(LONG).read().replace("kspace_style ewald 1.0e-5", "kspace_style pppm 1.0e-5"))
    nok = tmp_path / "nokspace.eam_coul"
    nok.write_text(open(LONG).read().replace("kspace_style ewald 1.0e-5\n", ""))
    e = rk.engine()
    try:
        e.register_replica("uo2", 1, capi.ionic_system(t, q, x, box, MASS))
        with pytest.raises(capi.EngineError, match=r"no EAM/coul potential attached to material uo2 \(scema_md_eam_coul_configure\)"):
            e.eam_coul_compute("uo2", 1)
        with pytest.raises(capi.EngineError, match=r"no EAM/coul potential attached to material uo2 \(scema_md_eam_coul_configure\)"):
            e.eam_coul_kspace("uo2", 1)
        with pytest.raises(capi.EngineError, match=r"rc=5: .*nokspace\.eam_coul line 0: no `kspace_style ewald\|pppm <accuracy>` line"):
            e.eam_coul_configure("uo2", str(nok))
        with pytest.raises(capi.EngineError, match=r"rc=5: .*UO2\.eam_coul line 4: units metal contradicts energy unit 1"):
            e.eam_coul_configure("uo2", LONG, energy_unit=1)
        # the material holds one attachment: Born/long's entry points refuse an EAM/coul material by name, and the other way round
        e.eam_coul_configure("uo2", LONG)
        with pytest.raises(capi.EngineError, match=r"no Born/long potential attached to material uo2"):
            e.born_long_kspace("uo2", 1)
        with pytest.raises(capi.EngineError, match=r"reciprocal solver mode 3"):
            e.eam_coul_kspace("uo2", 3)
        # a k list over the limit: the rattled 1 x 1 x 12 needle (144 ions, 65.64 A long) reaches an index beyond 20 at accuracy 1e-5; under
        # `ewald` it is refused, under `pppm` it runs on the mesh
        big = ec.case_rattled((1, 1, 12), 2)
        assert len(big[0]) == 144
        for m, path in (("big_e", LONG), ("big_p", str(pppm))):
            e.eam_coul_configure(m, path)
            e.register_replica(m, 1, capi.ionic_system(big[2], big[3], big[0], big[1], MASS))
        with pytest.raises(capi.EngineError, match=r"rc=1: a EAM/coul replica of 144 atoms needs \d+ k-vectors .* holds 4096 \(indices up to 20\)"):
            e.eam_coul_compute("big_e", 1)
        got = e.eam_coul_compute("big_p", 1)
        assert got["nk"] == 0 and min(e.eam_coul_last_mesh()) > 0 and np.isfinite(got["f"]).all() and np.abs(got["f"]).max() > 0.0
        # an update mixing this kind with another
        e.eam_configure("cu", CUAG, ("Cu",))
        e.register_replica("cu", 1, capi.bare_system(np.zeros(len(x), np.int32), x, box, masses=(63.546,)))
        mk = lambda k, m: capi.make_sim(k, m, 1, np.array([1e-3 * (box[3] - box[0]), 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "uo2"), mk(1, "cu")], [mk(1, "cu"), mk(0, "uo2")]):
            with pytest.raises(capi.EngineError, match="rc=1: .*mixes EAM materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "uo2", 1) and not e.has_state(1, "cu", 1)
        assert e.strain_batch([mk(0, "uo2")])[0].stress_updated == 1
    finally:
        e.close()
