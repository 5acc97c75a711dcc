"""The spline-MEAM force stage on the GPU (md_meam_spline.hip, engine_rowpot.cpp) against the independent FP64 numpy restatement
tests/meam_spline_numpy.py, which tests/test_meam_spline_host.py pins on the CPU (no LAMMPS exists to compare with): static parity on the
smallest shapes at which the kernels take another path, dynamics, the virial -> pressure conversion, whole evaluations, batches over two
materials, refusals, replaced attachments, self-configuration from the scripts folder.

Budgets, the standing ones (tests/test_gpu_vashishta.py, tests/test_gpu_adp.py): static parity 1e-10 of the largest force component, 1e-9
of the largest energy term and virial component; NVE after 20 steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; whole evaluations and a batch against each
simulation alone 1e-9 relative.  The perfect cell has no force by symmetry, so its forces are measured on the scale of its jittered twin.

Energy drift.  The embedded-atom tests hold no drift bound to borrow, so the bound is the reference's own: after 200 NVE steps the total
energy on the device may have moved from its start by no more than the numpy velocity-Verlet integrator's own drift on the same input
plus the static energy budget (1e-9 of the largest energy term).

What the groups catch.  Dimers: the strict tests at the last knots of f, rho and phi, a value exactly on a knot.  Trimers: f's last knot,
g's end knots and its linear continuation.  Densities outside U's knots: the continuation of U both ways.  Clusters: the ballot rank
across a trip of 16, the limit of 32 on f's range alone.  Atom counts: a short last tile, a second tile, the force table past the LDS
limit.  Two elements: a swapped pair index, rho or f of the wrong end.  Whole evaluations: rows kept or rebuilt under the wrong
material, part streams.
"""
import os
import shutil

import numpy as np
import pytest

import meam_spline_numpy as mn
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TI = os.path.join(ROOT, "tests", "golden", "Ti.meam.spline")
TIO = os.path.join(ROOT, "tests", "golden", "TiO.meam.spline")
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
EL1, MASS1 = ("Ti",), (mn.TI_MASS,)
EL2, MASS2 = ("Ti", "O"), (mn.TI_MASS, mn.O_MASS)
RLIST = mn.TI_CUT + 1.0


@pytest.fixture(scope="module")
def ref_ti():
    return mn.MeamSpline(mn.read_meam_spline(TI, list(EL1))[0])


@pytest.fixture(scope="module")
def ref_tio():
    return mn.MeamSpline(mn.read_meam_spline(TIO, list(EL2))[0])


MEAM = rk.Pot("meam/spline", "meam_spline_configure", "meam_spline_compute", "MEAM/spline", ("e_pair", "e_embed"), ("npairs", "ntriplets"),
              counts="ordered pairs {npairs}, triplets {ntriplets}")


_engine = rk.engine
_static = rk.static_of(MEAM, TI, EL1, MASS1)


def no_pairs(got, ref, scale, what):
    """nothing inside cutmax, or inside it but beyond every function of the pair: exactly zero, U(0) - U(0) included"""
    if ref["npairs"] != 0 and np.abs(scale["f"]).max() > 0.0:
        return False
    rk.all_exactly_zero(got, ref, MEAM, what, head=f"{ref['npairs']} ordered pairs")
    return True


_check_static = rk.checker(MEAM, tol_f=1e-10, tol_e=1e-9, tol_w=1e-9, no_pairs=no_pairs)


# ---- dimers ----
def test_dimers_of_one_element(ref_ti):
    """inside f's range, between f's and rho's last knot, between rho's and phi's, 0.05 A inside cutmax, exactly at cutmax and 1e-9 beyond
    (nothing counted, everything exactly zero), and exactly on an interior knot of rho"""
    for r in (2.9, 4.0, 5.2, mn.TI_CUT - 0.05, mn.TI_CUT, mn.TI_CUT + 1e-9, mn.TI_KNOT):
        x, box, t = mn.case_dimer(r)
        assert x[1, 0] - x[0, 0] == r
        ref = ref_ti.compute(x, box, t)
        assert ref["npairs"] == (2 if r < mn.TI_CUT else 0) and ref["ntriplets"] == 0 and ref["maxin"] == (1 if r < mn.TI_CUT_F else 0)
        assert (ref["rho"].max() > 0.0) == (r < mn.TI_CUT_RHO)
        _check_static(_static(x, box, t), ref, f"meam/spline dimer at {r!r}")
    assert mn.TI_KNOT in ref_ti.s["rho"][0].x[1:-1]


@pytest.mark.parametrize("pair", [(0, 0), (0, 1), (1, 1)])
def test_dimers_of_each_pair_of_elements(ref_tio, pair):
    """Ti-Ti, Ti-O and O-O under the two-element file: inside both f ranges, between them, beyond rho of oxygen (4.4 A), beyond phi of the
    pair where it ends before cutmax (O-O: 4.6 A, Ti-O: 5.0 A; the pair is still counted: it lies inside cutmax), at cutmax and beyond"""
    for r in (2.5, 3.2, 4.5, 4.8, 5.2, mn.TI_CUT - 0.05, mn.TI_CUT, mn.TI_CUT + 1e-9):
        x, box, t = mn.case_dimer(r, *pair)
        ref = ref_tio.compute(x, box, t)
        assert ref["npairs"] == (2 if r < mn.TI_CUT else 0)
        _check_static(_static(x, box, t, path=TIO, elements=EL2, masses=MASS2), ref, f"meam/spline dimer {pair} at {r!r}")


# ---- trimers ----
def test_trimers_at_the_last_knot_of_f(ref_ti):
    for r2, ntrip in ((mn.TI_CUT_F - 1e-6, 1), (mn.TI_CUT_F, 0), (2.9, 1)):
        x, box, t = mn.case_trimer(2.6, r2)
        ref = ref_ti.compute(x, box, t)
        assert ref["ntriplets"] >= ntrip and ref["maxin"] == (2 if ntrip else 1)
        _check_static(_static(x, box, t), ref, f"meam/spline trimer, second arm {r2!r}")


def test_trimers_at_the_ends_of_g(ref_ti, ref_tio):
    x, box, t = mn.case_collinear()
    d1, d2 = x[1] - x[0], x[2] - x[0]
    assert np.dot(d1, d2) / (np.linalg.norm(d1) * np.linalg.norm(d2)) == -1.0
    _check_static(_static(x, box, t), ref_ti.compute(x, box, t), "meam/spline collinear trimer, cos = -1")
    x, box, t = mn.case_near_degenerate()
    d1, d2 = x[1] - x[0], x[2] - x[0]
    assert 1.0 - np.dot(d1, d2) / (np.linalg.norm(d1) * np.linalg.norm(d2)) < 1e-12
    ref = ref_ti.compute(x, box, t)
    assert ref["ntriplets"] >= 1
    _check_static(_static(x, box, t), ref, "meam/spline near-degenerate trimer, cos -> 1")
    x, box, t = mn.case_trimer(2.4, 2.7, 95.0, (1, 0, 1))
    _check_static(_static(x, box, t, path=TIO, elements=EL2, masses=MASS2), ref_tio.compute(x, box, t), "meam/spline O-Ti-O trimer")


# ---- densities outside U's knots ----
def test_densities_outside_the_knots_of_u(ref_ti):
    U = ref_ti.s["U"][0]
    x, box, t = mn.case_dimer(mn.TI_CUT_RHO - 0.2)
    ref = ref_ti.compute(x, box, t)
    assert (ref["rho"] > 0.0).all() and (ref["rho"] < U.x[1]).all() and U.x[0] < 0.0     # below U's first interior knot
    _check_static(_static(x, box, t), ref, "meam/spline distant pair")
    x, box, t = mn.case_bcc(2, 2, 2, 2.8, 0.03, 2)
    ref = ref_ti.compute(x, box, t)
    assert ref["rho"].min() > U.x[-1]                                                       # beyond U's last knot
    _check_static(_static(x, box, t), ref, f"meam/spline compressed lattice, rho {ref['rho'].min():.1f} > {U.x[-1]}")


# ---- list limits ----
@pytest.mark.parametrize("m", [15, 16, 17, 31, 32])
def test_list_lengths(ref_ti, m):
    """an atom inside m atoms on a sphere of 3.2 A, inside f's range: the centre's list holds m entries (one trip of 16 short of one, full,
    one more, two trips short of one and full); the counts are pinned"""
    x, box, t = mn.case_cluster(m)
    ref = ref_ti.compute(x, box, t)
    assert ref["maxin"] == m and ref["npairs"] >= 2 * m and ref["ntriplets"] >= m * (m - 1) // 2
    got = _static(x, box, t)
    assert (got["npairs"], got["ntriplets"]) == (ref["npairs"], ref["ntriplets"])
    _check_static(got, ref, f"meam/spline cluster of {m}")


def test_more_than_32_inside_the_range_of_f_is_an_error(ref_ti):
    x, box, t = mn.case_cluster(33)
    assert ref_ti.compute(x, box, t)["maxin"] == 33
    with pytest.raises(capi.EngineError, match=r"more than 32 neighbours inside the last knot of f, the three-body range of the MEAM/spline potential"):
        _static(x, box, t)


def test_more_than_32_between_the_range_of_f_and_cutmax_is_taken(ref_ti):
    x, box, t = mn.case_cluster(6, outer=40)
    ref = ref_ti.compute(x, box, t)
    r0 = np.linalg.norm(x[1:] - x[0], axis=1)
    assert ((r0 > mn.TI_CUT_F) & (r0 < mn.TI_CUT)).sum() == 40 and ref["maxin"] <= 32
    _check_static(_static(x, box, t), ref, "meam/spline shell of 40 beyond f's range")


# ---- lattices ----
def test_a_cell_narrower_than_the_list_radius(ref_ti):
    """1 x 1 x 2 bcc cells of 3.3 A: the box is narrower than cutmax + skin = 6.5 A (and barely wider than half of it, the narrowest the
    image search takes), so an atom's row holds its own images and partners through both faces; perfect (measured on the scale of its
    jittered twin) and jittered"""
    x, box, t = mn.case_bcc(1, 1, 2, 3.3)
    xj, _, _ = mn.case_bcc(1, 1, 2, 3.3, 0.05)
    assert RLIST / 2.0 < box[3] - box[0] < RLIST
    ref, refj = ref_ti.compute(x, box, t), ref_ti.compute(xj, box, t)
    assert ref["maxin"] == 14 and ref["ntriplets"] == 4 * 91
    _check_static(_static(x, box, t), ref, "meam/spline four-atom cell", scale=refj)
    _check_static(_static(xj, box, t), refj, "meam/spline four-atom cell, jittered")


def test_triclinic_box_with_atoms_outside(ref_ti):
    x, box, t = mn.case_triclinic()
    s = (x - box[:3]) @ np.linalg.inv(mn.h_matrix(box))
    assert ((s < 0.0) | (s >= 1.0)).any(axis=1).sum() > 10 and box[6] != 0.0 and box[7] != 0.0 and box[8] != 0.0
    _check_static(_static(x, box, t), ref_ti.compute(x, box, t), "meam/spline triclinic")


# ---- atom counts ----
@pytest.mark.parametrize("n", [63, 64, 65])
def test_atom_counts(ref_ti, n):
    x, box, t = mn.case_count(n)
    assert len(x) == n
    _check_static(_static(x, box, t), ref_ti.compute(x, box, t), f"meam/spline n = {n}")


def test_a_block_past_the_lds_force_table(ref_ti):
    """1 025 atoms of jittered bcc at 3.8 A (eight arms inside f's range each) with vacancies: the instance that adds partner forces to
    global memory directly"""
    x, box, t = mn.case_block(1025, a=3.8)
    ref = ref_ti.compute(x, box, t)
    assert len(x) == 1025 and ref["ntriplets"] > 1025 * 10
    _check_static(_static(x, box, t), ref, "meam/spline 1 025 atoms")


# ---- two elements ----
@pytest.mark.parametrize("order", ["Ti O", "O Ti", "Ti Ti O"])
@pytest.mark.parametrize("occupation", ["ordered", "random"])
def test_two_elements(ref_tio, order, occupation):
    """an ordered compound (B2) and a random occupation under both element orders of pair_coeff (the types swapped with them: the same
    crystal), and with three LAMMPS types of which the first and the second are titanium"""
    x, box, t = mn.case_bcc(2, 2, 2, 3.3, 0.06, 3 if occupation == "ordered" else 4, occupation)
    ref = ref_tio.compute(x, box, t)
    assert len(set(t)) == 2 and ref["ntriplets"] > 0
    if order == "Ti O":
        types, masses = t, MASS2
    elif order == "O Ti":
        types, masses = 1 - t, MASS2[::-1]
    else:
        types, masses = np.where(t == 1, 2, np.arange(len(t)) % 2), (mn.TI_MASS, mn.TI_MASS, mn.O_MASS)
        assert set(types) == {0, 1, 2}
    _check_static(_static(x, box, types, path=TIO, elements=tuple(order.split()), masses=masses), ref, f"meam/spline {occupation} Ti-O, elements {order}")


# ---- dynamics ----
def test_nve_dynamics_and_sampled_pressure(ref_ti):
    x, box, t = mn.case_bcc(2, 2, 2, 3.2, 0.05, 6)
    v = rk.velocities(t, MASS1, 300.0, 1)
    e = _engine()
    try:
        e.meam_spline_configure("ti", TI, EL1)
        e.register_replica("ti", 1, capi.bare_system(t, x, box, v=v, masses=MASS1))
        e.set_state(0, "ti", 1, box, x, v)
        e.debug_run("ti", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "ti", 1)
        xr, vr = ref_ti.nve(x, v, box, t, MASS1, 1.0, 20)
        dx = np.abs(mn.minimage_diff(xg, xr, box)).max()
        print(f"meam/spline nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        # the virial -> pressure conversion on a strained cell: one step with sampling gives (sum m v v + W) / V of the state after it, in atm
        xs, bs = mn.strained(x, box, np.array([[0.01, 0.004, 0.0], [0.0, -0.006, 0.003], [0.0, 0.0, 0.008]]))
        e.set_state(1, "ti", 1, bs, xs, v)
        p = e.debug_run("ti", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref_ti.nve(xs, v, bs, t, MASS1, 1.0, 1)
        want = ref_ti.pressure_atm(x1, v1, bs, t, MASS1)
        print(f"meam/spline sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


def test_energy_drift_over_200_steps(ref_ti):
    """total energy after 200 NVE steps of the jittered four-atom cell: no further from its start than the numpy integrator's own drift
    plus the static energy budget"""
    x, box, t = mn.case_bcc(1, 1, 2, 3.3, 0.05)
    v = rk.velocities(t, MASS1, 300.0, 5)
    m = np.asarray(MASS1)[t]
    total = lambda c, vel: c["e_pair"] + c["e_embed"] + 0.5 * mn.MVV2E * np.sum(m[:, None] * vel * vel)
    ref0 = ref_ti.compute(x, box, t)
    xr, vr = ref_ti.nve(x, v, box, t, MASS1, 1.0, 200)
    drift_ref = abs(total(ref_ti.compute(xr, box, t), vr) - total(ref0, v))
    e = _engine()
    try:
        e.meam_spline_configure("ti", TI, EL1)
        e.register_replica("ti", 1, capi.bare_system(t, x, box, v=v, masses=MASS1))
        e.set_state(0, "ti", 1, box, x, v)
        e0 = total(e.meam_spline_compute("ti", 1, qp=0), v)
        e.debug_run("ti", 1, 200, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, _, vg = e.get_state(0, "ti", 1)
        drift = abs(total(e.meam_spline_compute("ti", 1, qp=0), vg) - e0)
        es = max(abs(ref0["e_pair"]), abs(ref0["e_embed"]))
        print(f"meam/spline energy drift over 200 steps: device {drift:.3e}, numpy integrator {drift_ref:.3e} kcal/mol of {es:.1f}")
        assert drift <= drift_ref + 1e-9 * es
    finally:
        e.close()


# ---- whole evaluations ----
def test_strain_batch_equals_the_two_runs_and_a_second_update_continues(ref_ti):
    """an update against the straining run and the sampling run issued through the parity hooks; then a second update from the stored
    states: qp 0 continues from its own, qp 1 branches from qp 0's"""
    x, box, t = mn.case_count(64)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s2 = np.array([1.0e-3 * L[0], 0.0, 1.0e-3 * L[2], 0.0, 0.0, 0.0])
    s = rk.Setup("ti", TI, EL1, MASS1, (x, box, t), rk.velocities(t, MASS1, 300.0, 2))
    rk.strain_batch_and_a_second_update(MEAM, s, s1, s2, tol=1e-9)


@pytest.fixture(scope="module")
def nine():
    """9 simulations (two part streams) over titanium under Ti.meam.spline and the Ti-O compound under TiO.meam.spline, and each one's
    stress alone in a fresh engine"""
    mats = {"ti": (mn.case_bcc(2, 2, 2, 3.2, 0.05, 6), TI, EL1, MASS1), "tio": (mn.case_bcc(2, 2, 2, 3.3, 0.06, 3, "ordered"), TIO, EL2, MASS2)}
    return rk.batch_vs_alone_fixture(MEAM, mats, 9, 21)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_nine_over_two_materials_equals_each_alone(nine, split):
    """whole (split 0) and as part batches on two streams (split 1)"""
    rk.assert_batch_vs_alone(MEAM, nine, split, what="meam/spline batch of 9 over two materials", tol=1e-9)


def test_a_replaced_potential_rebuilds_the_rows(ref_ti, ref_tio):
    """a material holds one attachment: the two-element file configured over Ti.meam.spline (every atom now oxygen, another cutmax and
    other lists) gives the forces of a fresh engine, not those of kept rows; an EAM attachment over it and back likewise"""
    x, box, t = mn.case_count(64)
    ref_o = mn.MeamSpline(mn.read_meam_spline(TIO, ["O"])[0])
    e = _engine()
    try:
        e.meam_spline_configure("m", TI, EL1)
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS1))
        _check_static(e.meam_spline_compute("m", 1), ref_ti.compute(x, box, t), "meam/spline before the replacement")
        e.meam_spline_configure("m", TIO, ("O",))
        _check_static(e.meam_spline_compute("m", 1), ref_o.compute(x, box, t), "meam/spline after the replacement")
        e.eam_configure("m", CUAG, ("Cu",))
        rk.assert_not_attached(MEAM, e, "m")
        assert e.eam_compute("m", 1)["npairs"] > 0
        e.meam_spline_configure("m", TI, EL1)
        with pytest.raises(capi.EngineError, match="no EAM potential"):
            e.eam_compute("m", 1)
        _check_static(e.meam_spline_compute("m", 1), ref_ti.compute(x, box, t), "meam/spline over an EAM attachment")
    finally:
        e.close()


def test_self_configuration_from_the_scripts_folder(ref_ti, tmp_path):
    """`pair_coeff * * ${locs}/Ti.meam.spline Ti` in in.strain.lammps configures a bare replica whose material has nothing attached: the
    update equals the configured one to the batch budget, and the material then computes"""
    scripts = tmp_path / "lammps_scripts_ti"
    scripts.mkdir()
    shutil.copy(TI, scripts / "Ti.meam.spline")
    (scripts / "in.strain.lammps").write_text("# straining run\npair_style meam/spline\n#pair_coeff * * ${locs}/other.meam.spline Zr\n"
                                              "pair_coeff * * ${locs}/Ti.meam.spline Ti   # the potential\nfix 1 all nvt temp 300 300 100\n")
    x, box, t = mn.case_count(64)
    v = rk.velocities(t, MASS1, 300.0, 3)
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "ti", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    outs = []
    for configure in (False, True):
        e = _engine()
        try:
            if configure:
                e.meam_spline_configure("ti", TI, EL1)
            e.register_replica("ti", 1, capi.bare_system(t, x, box, v=v, masses=MASS1))
            if not configure:
                rk.assert_not_attached(MEAM, e, "ti")
            o = e.strain_batch([mk(scripts)])[0]
            assert o.stress_updated == 1
            outs.append(np.array(o.stress[:]))
            _check_static(e.meam_spline_compute("ti", 1), ref_ti.compute(x, box, t), f"meam/spline {'configured' if configure else 'self-configured'}")
        finally:
            e.close()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0] - outs[1]).max() <= 1e-9 * np.abs(outs[1]).max()
    rk.assert_malformed_pair_coeff_lines(MEAM, rk.Setup("ti", TI, EL1, MASS1, (x, box, t)), tmp_path, ".meam.spline", "Ti", match_head="rc=1: .*", lines=1)


def _cells_static(monkeypatch, cells, case):
    monkeypatch.setenv("SCEMA_MD_ROW_CELLS", str(cells))     # (the engine has no parameter for it: the switch is read when the engine is made)
    x, box, t = case
    e = _engine()
    try:
        e.meam_spline_configure("m", TI, EL1)
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS1))
        out = e.meam_spline_compute("m", 1)
        out["rows"], out["prof"] = e.debug_rows(0), e.profile()
        return out
    finally:
        e.close()


def test_cell_binned_row_build(monkeypatch):
    """SCEMA_MD_ROW_CELLS=1 on a box of 19.8 A (three cells of the list radius 6.5 A per dimension): rows entry for entry those of the N^2
    build, forces, energies and virial equal to its result within the static budgets"""
    x, box, t = mn.case_bcc(6, 6, 6, 3.3, 0.08, 9)
    on, off = _cells_static(monkeypatch, 1, (x, box, t)), _cells_static(monkeypatch, 0, (x, box, t))
    a, b = on["rows"], off["rows"]
    assert (a["cells"], b["cells"]) == (1, 0) and min(a["ncell"]) >= 3 and a["cap"] == b["cap"]
    assert np.array_equal(a["cnt"], b["cnt"])
    live = np.arange(a["cap"])[None, :] < a["cnt"][:, None]
    assert np.array_equal(a["rows"][live], b["rows"][live]) and a["cnt"].sum() > 0
    assert on["prof"]["row_cell_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0
    assert off["ntriplets"] > 0 and np.abs(off["f"]).max() > 0.0
    _check_static(on, dict(off, e=off["e_pair"] + off["e_embed"]), "meam/spline 432 atoms, rows through cells against N^2 rows")


# ---- refusals ----
def test_refusals(ref_ti):
    x, box, t = mn.case_count(64)
    e = _engine()
    try:
        e.register_replica("ti", 1, capi.bare_system(t, x, box, masses=MASS1))
        with pytest.raises(capi.EngineError, match=r"no MEAM/spline potential attached to material ti \(scema_md_meam_spline_configure\)"):
            e.meam_spline_compute("ti", 1)
        # an update mixing this kind with another
        e.meam_spline_configure("ti", TI, EL1)
        e.eam_configure("cu", CUAG, ("Cu",))
        e.register_replica("cu", 1, capi.bare_system(t, x, box, masses=(63.546,)))
        mk = lambda q, m: capi.make_sim(q, m, 1, np.array([1e-3 * (box[3] - box[0]), 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "ti"), mk(1, "cu")], [mk(1, "cu"), mk(0, "ti")]):
            with pytest.raises(capi.EngineError, match="rc=1: .*mixes EAM materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "ti", 1) and not e.has_state(1, "cu", 1)
        assert e.strain_batch([mk(0, "ti")])[0].stress_updated == 1
        # an atom type beyond the element list
        t2 = t.copy()
        t2[5] = 1
        e.register_replica("ti", 2, capi.bare_system(t2, x, box, masses=(mn.TI_MASS, mn.O_MASS)))
        with pytest.raises(capi.EngineError, match=r"atom 5 has type 2 but the MEAM/spline element list names 1 types"):
            e.meam_spline_compute("ti", 2)
    finally:
        e.close()
