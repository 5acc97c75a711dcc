"""The Ewald ionic force stage on the GPU (md_born_long.hip, engine_rowpot.cpp: `pair_style born/coul/long`, `buck/coul/long` with
`kspace_style ewald|pppm <accuracy>`) against the independent FP64 numpy restatement tests/born_long_numpy.py, which
tests/test_born_long_host.py pins on the CPU (no LAMMPS exists to compare with).  numpy evaluates on the g_ewald and the integer triples the
device reports having used (nk and g are compared with numpy's own copy of the rule first), so the budgets measure the kernels and not the
accuracy of the Ewald sum.

Budgets, those of tests/test_gpu_born_dsf.py: static parity 1e-10 of the largest force component, energy term and virial part; NVE after 20
steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; whole evaluations 1e-10 (an update against its two runs) and 1e-9 (a batch against
each simulation alone).  The forces of one ion are measured on K e^2/A^2 (1e-12).  Energy drift after 200 NVE steps: no more than the numpy
integrator's own drift on the same input plus the static energy budget.

What the groups catch.  One ion: self, background and image energy with no pair.  Two ions in a 6 A cube: the image search two deep.  63,
64, 65 ions: the edges of the atom staging of k_bl_sfac (32) and of the 16-lane groups, cells that are not neutral (the background term in
energy and virial).  48 ions in a 1 x 2 x 3 box: kmax differs per dimension.  512 ions: more than one k chunk (709 k-vectors).  The
straining run: triples that stay while the box deforms, and their re-expression at a flip in xy and one in xz.
"""
import os

import numpy as np
import pytest

import born_long_numpy as bl
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_long")
MGO = os.path.join(ROOT, "tests", "golden", "MgO.buck_long")
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
MASS_NACL, MASS_MGO = (bl.NA_MASS, bl.CL_MASS), (bl.MG_MASS, bl.O_MASS)


@pytest.fixture(scope="module")
def ref_nacl():
    return bl.BornLong(bl.read_born_long(NACL))


@pytest.fixture(scope="module")
def ref_mgo():
    return bl.BornLong(bl.read_born_long(MGO))


BORN_LONG = rk.Pot("born/long", "born_long_configure", "born_long_compute", "Born/long", ("e_born", "e_coul"), ("npairs", "ncoul"),
                   counts="ordered pairs {npairs}, nk {got[nk]}, g {got[g_ewald]:.6f}", ionic=True,
                   energy_scale=("e_born", "e_coul", "e_real", "e_recip", "e_self"))


def _mgo_case(seed=17):
    x, box, t, q = bl.case_jitter(2, seed, sigma=0.1, a=4.3)
    return x, box, t, 1.2 * q


_engine = rk.engine
_static = rk.static_of(BORN_LONG, NACL, None, MASS_NACL)


def _reference(ref, got, x, box, t, q):
    """numpy on the g and the triples of the rule, after holding the device's nk and g against them"""
    g, tr = ref.setup(box, q)
    assert got["nk"] == len(tr) and abs(got["g_ewald"] - g) <= 1e-14 * g, (got["nk"], len(tr), got["g_ewald"], g)
    return ref.compute(x, box, t, q, g, tr)


def _check(got, ref, what, scale=None, K=None):
    """the virial on the largest of its three parts; one ion, which has no force by symmetry, on K e^2/A^2 with the budget 1e-12"""
    sc = scale or ref
    rk.check_static(got, ref, BORN_LONG, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, what=what, scale=scale, fs=K * 1e-2 if K else None,
                    ws=max(np.abs(sc[k]).max() for k in ("w_born", "w_real", "w_recip")))


def _static_case(ref, case, what, path=NACL, masses=MASS_NACL, scale_case=None, K=None):
    got = _static(*case, path=path, masses=masses)
    want = _reference(ref, got, *case)
    scale = None
    if scale_case is not None:
        scale = ref.compute(*scale_case)
    _check(got, want, what, scale=scale, K=K)
    return got, want


# ---- static parity ----
def test_one_ion_has_self_background_and_image_energy(ref_nacl):
    case = bl.case_single()
    got, want = _static_case(ref_nacl, case, "born/long one ion", K=ref_nacl.K)
    assert want["npairs"] == 0 and want["e_bg"] < 0.0 and want["e_recip"] > 0.0 and got["e_born"] == 0.0
    assert np.abs(got["f"]).max() <= 1e-12 * ref_nacl.K


def test_two_ions_in_a_six_angstrom_cube(ref_nacl):
    got, want = _static_case(ref_nacl, bl.case_two(), "born/long two ions, 6 A cube")
    assert want["maxrow"] > 20      # (an ion meets its own images and its partner's, two boxes deep)


def test_the_eight_ion_cell(ref_nacl):
    got, _ = _static_case(ref_nacl, bl.rocksalt(1, 1, 1), "born/long 8-ion cell", scale_case=bl.case_jitter(1, 1))
    assert got["nk"] == 16
    m = -got["e_coul"] / 4.0 * (bl.A_NACL / 2.0) / ref_nacl.K
    print(f"Madelung constant on the device: {m:.7f}")
    assert abs(m - bl.MADELUNG_NACL) < 3e-5
    _static_case(ref_nacl, bl.case_jitter(1, 1), "born/long 8-ion cell, jittered")


@pytest.mark.parametrize("n", [63, 64, 65])
def test_around_the_atom_staging_width(ref_nacl, n):
    j64 = bl.case_jitter(2, 1)
    case = {63: bl.case_without(j64, [37]), 64: j64, 65: bl.case_with_extra(j64)}[n]
    assert len(case[0]) == n and (abs(np.sum(case[3])) == 1.0) == (n != 64)
    got, want = _static_case(ref_nacl, case, f"born/long {n} ions")
    assert got["nk"] == 128 or n != 64
    if n != 64:
        assert abs(want["e_bg"]) > 0.0


def test_48_ions_in_a_box_of_three_different_edges(ref_nacl):
    case = bl.case_jitter((1, 2, 3), 3)
    assert len(case[0]) == 48
    _, tr = ref_nacl.setup(case[1], case[3])
    assert len(set(np.abs(tr).max(axis=0))) == 3
    _static_case(ref_nacl, case, "born/long 48 ions, 5.64 x 11.28 x 16.92 A")


def test_triclinic_box_with_ions_outside(ref_nacl):
    case = bl.case_triclinic()
    s = (case[0] - case[1][:3]) @ np.linalg.inv(bl.h_matrix(case[1]))
    assert ((s < 0.0) | (s >= 1.0)).any(axis=1).sum() >= 8
    _static_case(ref_nacl, case, "born/long triclinic, ions outside the box")


def test_512_ions_beyond_one_k_chunk(ref_nacl):
    case = bl.case_jitter(4, 2)
    got, _ = _static_case(ref_nacl, case, "born/long 512 ions")
    assert got["nk"] == 709


def test_buckingham_fixture(ref_mgo):
    got, _ = _static_case(ref_mgo, _mgo_case(), "buck/long MgO, 64 ions", path=MGO, masses=MASS_MGO)
    assert ref_mgo.p["style"] == "buck" and ref_mgo.p["solver"] == "pppm" and got["ncoul"] == got["npairs"]


def test_two_evaluations_of_one_state_agree_bit_for_bit():
    case = bl.case_jitter(2, 7)
    e = _engine()
    try:
        e.born_long_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(case[2], case[3], case[0], case[1], MASS_NACL))
        a, b = e.born_long_compute("m", 1), e.born_long_compute("m", 1)
    finally:
        e.close()
    c = _static(*case)
    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]) and np.array_equal(a["f"], c["f"])


# ---- dynamics ----
def test_nve_dynamics_and_sampled_pressure(ref_nacl):
    x, box, t, q = bl.case_jitter(2, 6, sigma=0.08)
    v = rk.velocities(t, MASS_NACL, 300.0, 1)
    e = _engine()
    try:
        e.born_long_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        e.debug_run("nacl", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "nacl", 1)
        xr, vr = ref_nacl.nve(x, v, box, t, q, MASS_NACL, 1.0, 20)
        dx = np.abs(bl.minimage_diff(xg, xr, box)).max()
        print(f"born/long nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        # the virial -> pressure conversion on a strained cell: one step with sampling gives (sum m v v + W) / V of the state after it, in atm
        xs, bs = bl.strained(x, box, np.array([[0.01, 0.004, 0.0], [0.0, -0.006, 0.003], [0.0, 0.0, 0.008]]))
        e.set_state(1, "nacl", 1, bs, xs, v)
        p = e.debug_run("nacl", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        g, tr = ref_nacl.setup(bs, q)
        x1, v1 = ref_nacl.nve(xs, v, bs, t, q, MASS_NACL, 1.0, 1)
        want = ref_nacl.pressure_atm(x1, v1, bs, t, q, MASS_NACL, g, tr)
        print(f"born/long sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


def test_energy_drift_over_200_steps(ref_nacl):
    """total energy after 200 NVE steps of the jittered 8-ion cell: no further from its start than the numpy integrator's own drift plus
    the static energy budget"""
    x, box, t, q = bl.case_jitter(1, 4, sigma=0.05)
    v = rk.velocities(t, MASS_NACL, 300.0, 5)
    m = np.asarray(MASS_NACL)[t]
    total = lambda c, vel: c["e_born"] + c["e_coul"] + 0.5 * bl.MVV2E * np.sum(m[:, None] * vel * vel)
    g, tr = ref_nacl.setup(box, q)
    ref0 = ref_nacl.compute(x, box, t, q, g, tr)
    xr, vr = ref_nacl.nve(x, v, box, t, q, MASS_NACL, 1.0, 200)
    drift_ref = abs(total(ref_nacl.compute(xr, box, t, q, g, tr), vr) - total(ref0, v))
    e = _engine()
    try:
        e.born_long_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        e0 = total(e.born_long_compute("nacl", 1, qp=0), v)
        e.debug_run("nacl", 1, 200, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, _, vg = e.get_state(0, "nacl", 1)
        drift = abs(total(e.born_long_compute("nacl", 1, qp=0), vg) - e0)
        es = max(abs(ref0[k]) for k in ("e_born", "e_coul", "e_real", "e_recip", "e_self"))
        print(f"born/long energy drift over 200 steps: device {drift:.3e}, numpy integrator {drift_ref:.3e} kcal/mol of {es:.1f}")
        assert drift <= drift_ref + 1e-10 * es
    finally:
        e.close()


def test_a_straining_run_whose_box_flips_in_xy_and_in_xz(ref_nacl):
    """16 steps of NVE under fix deform from a box tilted close to both flips: xy passes half a box length after step 6, xz after step 10
    (checked here on the tilt ratios of the unflipped path).  numpy keeps the unflipped box and the triples of the start box; the device
    flips twice and re-expresses its triples.  End positions (as lattice points of the end box) and the pressure sampled at every step"""
    (x, box, t, q), rates = bl.case_flip()
    nsteps, L = 16, box[3] - box[0]
    ratio = lambda k, step: (box[6 + k] + rates[3 + k] * L * step) / L
    cross = [min(s for s in range(1, nsteps) if ratio(k, s) > 0.50001) for k in (0, 1)]
    assert cross == [6, 10] and ratio(0, 0) < 0.5 and ratio(1, 0) < 0.5
    v = rk.velocities(t, MASS_NACL, 300.0, 9)
    xr, vr, box_r, p_r = ref_nacl.nve(x, v, box, t, q, MASS_NACL, 1.0, nsteps, rates=rates)
    e = _engine()
    try:
        e.born_long_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        p = e.debug_run("nacl", 1, nsteps, 1.0, 300.0, qp=0, nvt=False, use_shake=False, rates=rates, sample=True)
        bg, xg, vg = e.get_state(0, "nacl", 1)
        flips = e.profile()["box_flips"]
    finally:
        e.close()
    print(f"born/long flips {flips}, end tilts device {bg[6:9]}, numpy {box_r[6:9]}")
    assert flips == 2
    assert abs(bg[6] - (box_r[6] - L)) < 1e-9 and abs(bg[7] - (box_r[7] - L)) < 1e-9 and np.abs(bg[:6] - box_r[:6]).max() < 1e-12
    dx = np.abs(bl.minimage_diff(xg, xr, box_r)).max()
    dp = np.abs(p - p_r).max() / np.abs(p_r).max()
    print(f"born/long straining run with two flips: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs, pressure {dp:.2e}")
    assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11 and dp <= 1e-10


# ---- whole evaluations ----
def test_strain_batch_equals_the_two_runs_and_a_second_update_continues():
    """an update against the straining run and the sampling run issued through the parity hooks; then a second update from the stored
    states: qp 0 continues from its own, qp 1 branches from qp 0's"""
    x, box, t, q = bl.case_jitter(2, 8, sigma=0.08)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s2 = np.array([1.0e-3 * L[0], 0.0, 1.0e-3 * L[2], 0.0, 0.0, 0.0])
    s = rk.Setup("nacl", NACL, None, MASS_NACL, (x, box, t, q), rk.velocities(t, MASS_NACL, 300.0, 2))
    rk.strain_batch_and_a_second_update(BORN_LONG, s, s1, s2, tol=1e-10)


@pytest.fixture(scope="module")
def nine():
    """9 simulations (two part streams) over both fixtures and three sizes -- 64 ions of NaCl (nk 128), 48 ions of NaCl in the 1 x 2 x 3 box,
    64 ions under MgO.buck_long (nk of accuracy 1e-4) -- so one launch holds different nk; and each one's stress alone in a fresh engine"""
    mats = {"nacl64": (bl.case_jitter(2, 6, sigma=0.08), NACL, None, MASS_NACL), "nacl48": (bl.case_jitter((1, 2, 3), 3, sigma=0.08), NACL, None, MASS_NACL),
            "mgo64": (_mgo_case(), MGO, None, MASS_MGO)}
    return rk.batch_vs_alone_fixture(BORN_LONG, mats, 9, 21, pick=lambda k: sorted(mats)[k % 3])


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_nine_over_both_fixtures_equals_each_alone(nine, split):
    """whole (split 0) and as part batches on two streams (split 1)"""
    rk.assert_batch_vs_alone(BORN_LONG, nine, split, what="born/long batch of 9 over both fixtures", tol=1e-9)


def _real_units_copy(path, buck):
    """the fixture with its energies converted to kcal/mol by hand, under `units real`"""
    lines = []
    for raw in open(path):
        w = raw.split("#")[0].split()
        if w and w[0] == "units":
            lines.append("units real\n")
        elif w and w[0] == "pair_coeff":
            v = [float(s) for s in w[3:]]
            for k in ((0, 2) if buck else (0, 3, 4)):
                v[k] *= bl.EV_TO_KCALMOL
            lines.append(" ".join(w[:3] + [repr(s) for s in v]) + "\n")
        else:
            lines.append(raw)
    return "".join(lines)


@pytest.mark.parametrize("style,units", [("born", "metal"), ("born", "real"), ("buck", "metal"), ("buck", "real")])
def test_self_configuration_from_the_scripts_folder(style, units, tmp_path):
    """`pair_style born/coul/long` or `buck/coul/long` in in.strain.lammps configures a topology-free replica with charges whose material has
    nothing attached, from the script's own lines: the update equals the configured one to the batch budget, and the material then
    computes.  With `units real` the numbers are taken as kcal/mol."""
    path, masses = (NACL, MASS_NACL) if style == "born" else (MGO, MASS_MGO)
    scripts = tmp_path / "lammps_scripts_ionic"
    scripts.mkdir()
    frag = open(path).read() if units == "metal" else _real_units_copy(path, style == "buck")
    (scripts / "in.strain.lammps").write_text("# straining run\nread_restart ${loco}/init.restart\n" + frag + "fix 1 all nvt temp 300 300 100\nrun 100\n")
    ref = bl.BornLong(bl.read_born_long(str(scripts / "in.strain.lammps")))
    assert ref.p["unit"] == (1 if units == "real" else 0) and ref.p["style"] == style
    x, box, t, q = bl.case_jitter(2, 9, sigma=0.08) if style == "born" else _mgo_case()
    v = rk.velocities(t, masses, 300.0, 3)
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "ion", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    outs = []
    for configure in (False, True):
        e = _engine()
        try:
            if configure:
                e.born_long_configure("ion", str(scripts / "in.strain.lammps"), energy_unit=ref.p["unit"])
            e.register_replica("ion", 1, capi.ionic_system(t, q, x, box, masses, v=v))
            if not configure:
                rk.assert_not_attached(BORN_LONG, e, "ion")
            o = e.strain_batch([mk(scripts)])[0]
            assert o.stress_updated == 1
            outs.append(np.array(o.stress[:]))
            got = e.born_long_compute("ion", 1)
            _check(got, _reference(ref, got, x, box, t, q), f"{style}/long {'configured' if configure else 'self-configured'}, units {units}")
        finally:
            e.close()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0] - outs[1]).max() <= 1e-9 * np.abs(outs[1]).max()


def _cells_static(monkeypatch, cells, case):
    monkeypatch.setenv("SCEMA_MD_ROW_CELLS", str(cells))     # (the engine has no parameter for it: the switch is read when the engine is made)
    x, box, t, q = case
    e = _engine()
    try:
        e.born_long_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS_NACL))
        out = e.born_long_compute("m", 1)
        out["rows"], out["prof"] = e.debug_rows(0, rows=False), e.profile()
        return out
    finally:
        e.close()


def test_cell_binned_row_build(monkeypatch):
    """SCEMA_MD_ROW_CELLS=1 on 1 728 ions in a box of 33.84 A: the same rows in the same order, so the forces of the N^2 rows bit for bit"""
    case = bl.case_jitter(6, 9, sigma=0.08)
    assert len(case[0]) == 1728
    on, off = _cells_static(monkeypatch, 1, case), _cells_static(monkeypatch, 0, case)
    assert (on["rows"]["cells"], off["rows"]["cells"]) == (1, 0) and on["prof"]["row_cell_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0
    assert off["npairs"] > 1728 * 150 and np.abs(off["f"]).max() > 0.0 and on["nk"] == off["nk"] > 709
    assert (on["npairs"], on["ncoul"]) == (off["npairs"], off["ncoul"])
    assert np.array_equal(on["f"], off["f"])


# ---- refusals ----
def test_refusals(tmp_path):
    x, box, t, q = bl.case_jitter(2, 4, sigma=0.08)
    text = open(NACL).read()
    nok = tmp_path / "nokspace.born_long"
    nok.write_text(text.replace("kspace_style ewald 1.0e-5\n", ""))
    kmod = tmp_path / "kmod.born_long"
    kmod.write_text(text + "kspace_modify mesh 16 16 16\n")
    tight = tmp_path / "tight.born_long"
    tight.write_text(text.replace("kspace_style ewald 1.0e-5", "kspace_style ewald 1.0e-12"))
    e = _engine()
    try:
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS_NACL))
        with pytest.raises(capi.EngineError, match=r"no Born/long potential attached to material nacl \(scema_md_born_long_configure\)"):
            e.born_long_compute("nacl", 1)
        with pytest.raises(capi.EngineError, match=r"rc=5: .*nokspace\.born_long line 0: no `kspace_style ewald\|pppm <accuracy>` line"):
            e.born_long_configure("nacl", str(nok))
        with pytest.raises(capi.EngineError, match=r"rc=5: .*kmod\.born_long line 11: a kspace_modify line: none of its options is honoured"):
            e.born_long_configure("nacl", str(kmod))
        with pytest.raises(capi.EngineError, match=r"rc=5: .*NaCl\.born_long line 4: units metal contradicts energy unit 1"):
            e.born_long_configure("nacl", NACL, energy_unit=1)
        # a k list over the limit: 512 ions at accuracy 1e-12
        xb, bb, tb, qb = bl.case_jitter(4, 2)
        e.born_long_configure("big", str(tight))
        e.register_replica("big", 1, capi.ionic_system(tb, qb, xb, bb, MASS_NACL))
        with pytest.raises(capi.EngineError, match=r"rc=1: .*needs \d+ k-vectors .* holds 4096 .*PPPM on the row driver is the follow-up"):
            e.born_long_compute("big", 1)
        # an update mixing this kind with another
        e.born_long_configure("nacl", NACL)
        e.eam_configure("cu", CUAG, ("Cu",))
        e.register_replica("cu", 1, capi.bare_system(np.zeros(len(x), np.int32), x, box, masses=(63.546,)))
        mk = lambda k, m: capi.make_sim(k, m, 1, np.array([1e-3 * (box[3] - box[0]), 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "nacl"), mk(1, "cu")], [mk(1, "cu"), mk(0, "nacl")]):
            with pytest.raises(capi.EngineError, match="rc=1: .*mixes EAM materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "nacl", 1) and not e.has_state(1, "cu", 1)
        assert e.strain_batch([mk(0, "nacl")])[0].stress_updated == 1
    finally:
        e.close()
