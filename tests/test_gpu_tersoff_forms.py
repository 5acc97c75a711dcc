"""The force stages of the Tersoff forms on the GPU (k_ts_force<TsModTable, .> and k_ts_force<TsZblTable, .> of md_tersoff.hip, the entries
"Tersoff/mod" and "Tersoff/ZBL" of row_pots in engine_rowpot.cpp) against the FP64 numpy restatement tests/tersoff_forms_numpy.py, which
tests/test_tersoff_forms_host.py pins on the CPU.  No LAMMPS exists here to compare with.

Budgets (the project's standing ones): static parity 1e-10 of the largest force component, energy term and virial component; NVE after
20 steps 1e-9 A and 1e-11 A/fs; whole evaluations 1e-10 / 1e-9 relative; elastic constants within 0.1 % of second differences of the
numpy energy, as for plain Tersoff.

Shapes: the CPU inputs of tests/test_tersoff_forms_host.py (single atom to the 216-atom gas, both forms, the synthetic two-element file
and its clamped variant, SiC in both element orders); the 8-atom cell under a list radius wider than the box (images two boxes away); a
triclinic box with atoms outside it; lists of 16, 17 and 32 neighbours and the refusal at 33; 1 024 atoms (the largest LDS force table,
which both forms keep) and 1 025 (the instances without it); rows regrown after a forced overflow; dimers around R + D.
"""
import os
import re
import shutil

import numpy as np
import pytest

import rowkit as rk
import tersoff_forms_numpy as tf
import tersoff_numpy as tsn
from scema_amd import capi
from test_tersoff_forms_host import MOD, MODC, NAMES, SIC, ZBL, files, inputs, mod_ref, zbl_ref  # noqa: F401  (files: a fixture)

pytestmark = pytest.mark.gpu

MASSES = {"Si": tsn.SI_MASS, "C": tsn.C_MASS, "X": 28.0, "Y": 20.0}
FORMS = {"mod": (MOD, ("Si",), 3.3), "zbl": (ZBL, ("Si",), 3.0)}


COUNTS = "pairs {npairs}, (j, k) {nzeta}"
POTS = {"mod": rk.Pot("mod", "tersoff_mod_configure", "tersoff_mod_compute", "Tersoff/mod", ("e_rep", "e_att"), ("npairs", "nzeta"), counts=COUNTS),
        "zbl": rk.Pot("zbl", "tersoff_zbl_configure", "tersoff_zbl_compute", "Tersoff/ZBL", ("e_rep", "e_att"), ("npairs", "nzeta"), counts=COUNTS)}
SI1 = (tsn.SI_MASS,)

_engine = rk.engine


def _eval(form, x, box, t, path=None, elements=("Si",), skin=-1.0):
    return rk.static(POTS[form], x, box, t, path or FORMS[form][0], elements, tuple(MASSES[el] for el in elements), skin=skin)


def no_pairs(got, ref, scale, what):
    """no pair, so no term at all: everything is exactly zero, and there is no scale to divide by"""
    if ref["npairs"] != 0:
        return False
    rk.all_exactly_zero(got, ref, POTS["mod"], what)
    return True


# (plain Tersoff and the two forms report the same terms and counters: one descriptor serves the check of all three)
_check_static = rk.checker(POTS["mod"], tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)


def _ref(form, path=None, elements=("Si",)):
    return (mod_ref if form == "mod" else zbl_ref)(path or FORMS[form][0], list(elements))


@pytest.fixture(scope="module")
def ref_of():
    """the numpy objects of the two silicon fixtures, read once"""
    return {form: _ref(form) for form in FORMS}


# ---- static parity ----
@pytest.mark.parametrize("name", NAMES)
def test_static_parity_of_the_cpu_inputs(files, name):
    form, path, el, (x, box, t) = inputs(files)[name]
    ref = _ref(form, path, el).compute(x, box, t)
    _check_static(_eval(form, x, box, t, path, tuple(el)), ref, what=f"tersoff forms static {name}")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_static_parity_cell8_two_images_deep(ref_of, form):
    """the 8-atom cell (5.432 A) under a list radius of 5.5 A: the row build searches images two boxes away"""
    x, box, t = tsn.case_cell8()
    skin = 5.5 - FORMS[form][2]
    assert FORMS[form][2] + skin > box[3] - box[0] >= (FORMS[form][2] + skin) / 2.0
    got = _eval(form, x, box, t, skin=skin)
    _check_static(got, ref_of[form].compute(x, box, t), what=f"{form} static cell8, list radius 5.5 A")
    assert got["maxrow"] > _eval(form, x, box, t)["maxrow"]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_static_parity_triclinic(ref_of, form):
    x, box, t = tsn.case_triclinic()
    tsn.check_box(box, FORMS[form][2], FORMS[form][2] + 1.0)
    _check_static(_eval(form, x, box, t), ref_of[form].compute(x, box, t), what=f"{form} static triclinic")


@pytest.mark.parametrize("k", [16, 17, 32])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_static_parity_list_lengths(ref_of, form, k):
    """a centre atom with k atoms on a sphere of 2.6 A around it: one pass of 16 lanes, one lane into the second, the full list"""
    x, box, t = tsn.case_crowded(k)
    ref = ref_of[form].compute(x, box, t)
    assert ref["maxin"] == k
    _check_static(_eval(form, x, box, t), ref, what=f"{form} static {k} neighbours")


@pytest.mark.parametrize("form,name", [("mod", "Tersoff/mod"), ("zbl", "Tersoff/ZBL")])
def test_thirty_three_neighbours_are_refused(ref_of, form, name):
    x, box, t = tsn.case_crowded(33)
    assert ref_of[form].compute(x, box, t)["maxin"] == 33
    with pytest.raises(capi.EngineError, match=re.escape(f"more than 32 neighbours inside the {name} cutoff")):
        _eval(form, x, box, t)


@pytest.mark.parametrize("n", [1024, 1025])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_atom_count_edges(ref_of, form, n):
    """1 024 atoms: the largest replica whose forces are summed in the LDS table (static + dynamic LDS 63 936 B for mod, 63 424 B for zbl);
    1 025: the instance that adds to global memory"""
    x, box, t = tsn.case_count(n)
    _check_static(_eval(form, x, box, t), ref_of[form].compute(x, box, t), what=f"{form} static n = {n}")


@pytest.mark.parametrize("form", sorted(FORMS))
def test_row_overflow_regrows_and_retries(ref_of, form, monkeypatch):
    x, box, t = tsn.case_scaled()
    ref = ref_of[form].compute(x, box, t)
    normal = _eval(form, x, box, t)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    got = _eval(form, x, box, t)
    _check_static(got, ref, what=f"{form} static after a row overflow")
    assert got["rowcap"] < normal["rowcap"]


@pytest.mark.parametrize("form", sorted(FORMS))
def test_dimer_around_the_cutoff(ref_of, form):
    """at R + D - 1e-6, exactly R + D, and + 1e-6: finite values just inside, exactly zero from the cutoff on.  Just inside, the mod energy
    is of order fC ~ (1e-6)^4, the ZBL one keeps its step (1 - F) V_ZBL ~ 1e-11 kcal/mol"""
    cut = FORMS[form][2]
    for d in (-1e-6, 0.0, 1e-6):
        x, box, t = tsn.case_dimer(cut + d)
        assert x[1, 0] - x[0, 0] == cut + d
        got, ref = _eval(form, x, box, t), ref_of[form].compute(x, box, t)
        assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and np.isfinite(got["e_rep"]) and np.isfinite(got["e_att"])
        assert got["npairs"] == ref["npairs"] == (2 if d < 0 else 0)
        if d < 0:
            # (parity on the scale of the terms that cancel there is what _check cannot give: hold the values to their own smallness)
            print(f"{form} dimer just inside R + D: e {got['e_rep'] + got['e_att']:.3e} (numpy {ref['e']:.3e}), |f| {np.abs(got['f']).max():.3e}")
            assert abs(got["e_rep"] + got["e_att"]) < 1e-8 and np.abs(got["f"]).max() < 1e-2
            assert abs(got["e_rep"] + got["e_att"] - ref["e"]) < 1e-10 and np.abs(got["f"] - ref["f"]).max() < 1e-10
        else:
            assert got["e_rep"] == 0.0 and got["e_att"] == 0.0 and not got["f"].any() and not got["w"].any()


# ---- dynamics and plumbing ----
@pytest.mark.parametrize("form", sorted(FORMS))
def test_nve_dynamics(ref_of, form):
    x, box, t = tsn.case_a()
    v = rk.velocities(t, SI1, 300.0, 1)
    e = _engine()
    try:
        rk.configure(POTS[form], e, "si", FORMS[form][0])
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=v))
        e.set_state(0, "si", 1, box, x, v)
        e.debug_run("si", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "si", 1)
        xr, vr = ref_of[form].nve(x, v, box, t, (tsn.SI_MASS,), 1.0, 20)
        dx = np.abs(tsn.minimage_diff(xg, xr, box)).max()
        print(f"{form} nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
    finally:
        e.close()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_strain_batch_equals_the_two_runs(form):
    x, box, t = tsn.case_a()
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s = rk.Setup("si", FORMS[form][0], None, None, (x, box, t), rk.velocities(t, SI1, 300.0, 2))
    rk.strain_batch_vs_debug_runs(POTS[form], s, s1, expect_nts=30, tol=1e-10)


@pytest.fixture(scope="module")
def eleven():
    """11 simulations over a tersoff/mod and a tersoff/mod/c material (one kind, two tables), and each one's stress alone in a fresh engine"""
    mats = {"mod": (tsn.case_a(), MOD, None, None), "modc": (tsn.case_scaled(), MODC, None, None)}
    return rk.batch_vs_alone_fixture(POTS["mod"], mats, 11, 21, thermal_masses=SI1)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_eleven_equals_each_alone(eleven, split):
    rk.assert_batch_vs_alone(POTS["mod"], eleven, split, what="batch of 11 over a mod and a mod/c material", tol=1e-9)


def _two_atom_update(form, path, scripts, configure):
    """one update of a two-atom replica (bit-reproducible: every force component is the sum of two terms), and the static hook on the
    registered dimer"""
    dimer = rk.Setup("si", path, None, None, (np.array([[5.0, 6.0, 6.0], [7.3, 6.1, 5.9]]), np.array([0.0, 0.0, 0.0, 12.0, 12.0, 12.0, 0.0, 0.0, 0.0]), tsn.zeros(2)),
                     np.array([[1e-3, 2e-3, -1e-3], [-1e-3, -2e-3, 1e-3]]))
    return rk.dimer_update(POTS[form], dimer, scripts, configure, 1.2e-2, compute_qp=capi.QP_NONE)


@pytest.mark.parametrize("form,path,style", [("mod", MOD, "tersoff/mod"), ("mod", MODC, "tersoff/mod/c"), ("zbl", ZBL, "tersoff/zbl")])
def test_self_configuration_from_the_scripts_folder(tmp_path, form, path, style):
    """`pair_coeff * * ${locs}/<name>.tersoff.mod|.tersoff.modc|.tersoff.zbl Si` in in.strain.lammps configures a bare replica whose material
    has nothing attached: the update and the state equal those of the configured run bit for bit; a malformed line is SCEMA_MD_ERR_ARG"""
    name = os.path.basename(path)
    scripts = tmp_path / "scripts"
    scripts.mkdir()
    shutil.copy(path, scripts / name)
    (scripts / "in.strain.lammps").write_text(f"# straining run\npair_style {style}\n#pair_coeff * * ${{locs}}/other.tersoff C\n"
                                              f"pair_coeff * * ${{locs}}/{name} Si   # the potential\nfix 1 all nvt temp 300 300 100\n")
    a, sa, ca = _two_atom_update(form, path, scripts, configure=False)
    b, sb, cb = _two_atom_update(form, path, scripts, configure=True)
    assert np.isfinite(a).all() and np.abs(a).max() > 0.0
    assert np.array_equal(a, b) and all(np.array_equal(p, q) for p, q in zip(sa, sb))
    assert ca["e_rep"] == cb["e_rep"] and ca["npairs"] == 2
    if path == MODC:          # (the file was read as mod/c: the registered dimer, 2.3 A apart, carries 1/2 c0 fC per ordered pair)
        plain = _two_atom_update("mod", MOD, tmp_path / "none", configure=True)[2]
        assert abs((ca["e_rep"] - plain["e_rep"]) + 0.0251 * tf.EV_TO_KCALMOL) < 1e-12
    ext = name[name.index(".tersoff"):]
    rk.assert_malformed_pair_coeff_lines(POTS[form], rk.Setup("si", path, None, None, tsn.case_dimer(2.3)), tmp_path, ext, "Si", match_head="rc=1.*",
                                         match_tail=" ", lines=3, strain_x=1e-2)


# ---- replacement and mixing ----
def test_configuring_replaces_a_plain_tersoff_attachment_and_back(ref_of):
    x, box, t = tsn.case_a()
    plain = tsn.Tersoff(tsn.read_tersoff(SIC, ["Si"])[0]).compute(x, box, t)
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        _check_static(e.tersoff_compute("si", 1), plain, what="plain tersoff")
        e.tersoff_mod_configure("si", MOD)
        with pytest.raises(capi.EngineError, match=r"no Tersoff potential attached to material si \(scema_md_tersoff_configure\)"):
            e.tersoff_compute("si", 1)
        with pytest.raises(capi.EngineError, match=r"no Tersoff/ZBL potential attached to material si \(scema_md_tersoff_zbl_configure\)"):
            e.tersoff_zbl_compute("si", 1)
        _check_static(e.tersoff_mod_compute("si", 1), ref_of["mod"].compute(x, box, t), what="tersoff/mod over a plain attachment")
        e.tersoff_zbl_configure("si", ZBL)
        rk.assert_not_attached(POTS["mod"], e, "si")
        _check_static(e.tersoff_zbl_compute("si", 1), ref_of["zbl"].compute(x, box, t), what="tersoff/zbl over a mod attachment")
        e.tersoff_configure("si", SIC)
        rk.assert_not_attached(POTS["zbl"], e, "si")
        _check_static(e.tersoff_compute("si", 1), plain, what="plain tersoff over a zbl attachment")
    finally:
        e.close()


def test_mixed_kinds_are_refused_in_table_order():
    """Tersoff + Tersoff/mod and Tersoff/mod + Tersoff/ZBL in one update, both list orders: the kind earlier in the table is named, no state
    is stored; each alone runs"""
    xs = tsn.diamond(1, 1, 1, tsn.A_SI)[0] + 12.0
    box = tsn.BIG_BOX.copy()
    e = _engine()
    try:
        e.tersoff_configure("ts", SIC)
        e.tersoff_mod_configure("mod", MOD)
        e.tersoff_zbl_configure("zbl", ZBL)
        for m in ("ts", "mod", "zbl"):
            e.register_replica(m, 1, capi.bare_system(tsn.zeros(8), xs, box))
        s = np.array([1e-3 * 30.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        mk = lambda q, m: capi.make_sim(q, m, 1, s, nss=10, most_recent=capi.QP_NONE)
        for (a, b), name in {("ts", "mod"): "Tersoff", ("mod", "zbl"): "Tersoff/mod", ("ts", "zbl"): "Tersoff"}.items():
            msg = f"one update mixes {name} materials (1 of 2 simulations) with others"
            for first, second in ((a, b), (b, a)):
                with pytest.raises(capi.EngineError, match="rc=1.*" + re.escape(msg)):
                    e.strain_batch([mk(0, first), mk(1, second)])
                assert not e.has_state(0, first, 1) and not e.has_state(1, second, 1)
        for q, m in enumerate(("ts", "mod", "zbl")):
            assert e.strain_batch([mk(q, m)])[0].stress_updated == 1 and e.has_state(q, m, 1)
    finally:
        e.close()


# ---- elastic constants ----
def test_elastic_constants_of_the_mod_fixture(ref_of):
    """C11 and C12 of the mod fixture from the GPU virials at +-1e-3 strain against second differences of the numpy energy within 0.1 %, the
    agreement asserted for plain Tersoff (both are finite differences with a relative truncation of order 1e-5).  No literature value is pinned"""
    ref = ref_of["mod"]
    x, box = tsn.diamond(2, 2, 2, 5.429)
    t = tsn.zeros(len(x))
    h, vol = 1e-3, tsn.volume(box)
    E = lambda e1, e2: ref.energy(*tsn.strained(x, box, np.diag([e1, e2, 0.0])), t)
    n11 = (E(h, 0.0) - 2.0 * E(0.0, 0.0) + E(-h, 0.0)) / h ** 2 / vol * tsn.KCALMOL_A3_TO_GPA
    n12 = (E(h, h) - E(h, -h) - E(-h, h) + E(-h, -h)) / (4.0 * h ** 2) / vol * tsn.KCALMOL_A3_TO_GPA
    e = _engine()
    try:
        e.tersoff_mod_configure("si", MOD)
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        sig = {}
        for s in (+1, -1):
            xs, bs = tsn.strained(x, box, np.diag([s * h, 0.0, 0.0]))
            e.set_state(5, "si", 1, bs, xs, np.zeros_like(xs))
            sig[s] = -e.tersoff_mod_compute("si", 1, qp=5)["w"] / tsn.volume(bs) * tsn.KCALMOL_A3_TO_GPA
        c11, c12 = (sig[+1][0] - sig[-1][0]) / (2 * h), (sig[+1][1] - sig[-1][1]) / (2 * h)
        print(f"tersoff/mod elastic constants on the device: C11 {c11:.3f} GPa, C12 {c12:.3f} GPa; numpy energy: C11 {n11:.3f}, C12 {n12:.3f}")
        assert abs(c11 / n11 - 1.0) < 1e-3 and abs(c12 / n12 - 1.0) < 1e-3
    finally:
        e.close()
