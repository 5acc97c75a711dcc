"""The Tersoff force stage on the GPU (md_tersoff.hip, engine_rowpot.cpp) against the independent FP64 numpy restatement
tests/tersoff_numpy.py, which tests/test_tersoff_host.py pins on the CPU (no LAMMPS and no reference Tersoff file exist to compare with):
static parity on the shapes at which the kernels take another path, dynamics, the virial -> pressure conversion, elastic constants, whole
evaluations, batches over two materials, box flips inside a split batch, refusals, self-configuration from the scripts folder.

Budgets: static parity 1e-10 of the largest force component, energy term and virial component (the project's standing budget: FP64 sums
of a few hundred terms in another order); NVE after 20 steps 1e-9 A and 1e-11 A/fs; whole evaluations 1e-10 / 1e-9 relative (the same
arithmetic in another launch shape).

What the groups catch.  Static parity: a pair term owned by one end only (every jittered case: forces, energies and the count of ordered
pairs), the cutoff of fC(r_ik) from the wrong entry (from i j j: jittered SiC and the synthetic files; from i k k: the synthetic files, whose
i j k entries carry their own R, D), a swapped [i][j][k] index (SiC in both element orders), a wrong image shift (the 8-atom cell, the triclinic box),
a force table indexed past the LDS limit or a short last tile (the atom counts), a truncated neighbour list (the crowded cluster must be
an error).  Dynamics and pressure: the sign and the 1/2 of the virial, its split over two engine parts.  Whole evaluations: rows kept or
rebuilt under the wrong material, part streams, flips.  The wrong builds named first -- the pair term owned by one end; R, D of fC(r_ik) from entry
i j j, and from entry i k k -- were tried on the CPU driver (tests/test_tersoff_host.py::test_wrong_builds_are_caught says what failed).
A list that stops at the pair's own cutoff is NOT caught here: no case of this file has an entry between the pair's R + D and cutin (the
synthetic cell's bonds end at 2.8 A, its next shell starts at 3.84 A).  The shell case of tests/test_gpu_tersoff_edges.py, with 60 such
entries, catches it (tests/test_row_edges_host.py::test_list_cut_at_the_pair_cutoff_is_caught).
"""
import math
import os
import shutil

import numpy as np
import pytest

import rowkit as rk
import sw_numpy as swn
import tersoff_numpy as tsn
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.tersoff")
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")
MASS = (tsn.SI_MASS,)
MASS2 = (tsn.SI_MASS, tsn.C_MASS)


@pytest.fixture(scope="module")
def ref_si():
    return tsn.Tersoff(tsn.read_tersoff(SIC, ["Si"])[0])


@pytest.fixture(scope="module")
def ref_sic():
    return tsn.Tersoff(tsn.read_tersoff(SIC, ["Si", "C"])[0])


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tersoff")
    (d / "synth.tersoff").write_text(tsn.SYNTH)
    (d / "clamp.tersoff").write_text(tsn.SYNTH_CLAMP)
    return {"synth": str(d / "synth.tersoff"), "clamp": str(d / "clamp.tersoff")}


TERSOFF = rk.Pot("tersoff", "tersoff_configure", "tersoff_compute", "Tersoff", ("e_rep", "e_att"), ("npairs", "nzeta"), counts="pairs {npairs}, (j, k) {nzeta}")


_engine = rk.engine
_static = rk.static_of(TERSOFF, SIC, ("Si",), MASS)


def no_pairs(got, ref, scale, what):
    """no pair, so no term at all: everything is exactly zero, and there is no scale to divide by"""
    if ref["npairs"] != 0:
        return False
    rk.all_exactly_zero(got, ref, TERSOFF, what)
    return True


_check_static = rk.checker(TERSOFF, "tersoff static", tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)


# the smallest shapes at which a path changes: no pair; zeta = 0; one (j, k) per pair; the image search with an atom's own images' neighbours;
# minimum image with 4 neighbours; 16 neighbours, the second shell inside R - D .. R + D; a triclinic box with atoms outside it
SILICON = {"single": tsn.case_single, "dimer": tsn.case_dimer, "trimer": tsn.case_trimer, "cell8": tsn.case_cell8, "a": tsn.case_a,
           "scaled": tsn.case_scaled, "triclinic": tsn.case_triclinic}


@pytest.mark.parametrize("name", sorted(SILICON))
def test_static_parity_silicon(ref_si, name):
    x, box, t = SILICON[name]()
    ref = ref_si.compute(x, box, t)
    if name == "scaled":
        assert ref["maxin"] == 16 and ref["npairs"] == 64 * 16 and ref["nshell"] == 384 and box[3] == 8.148 >= 2 * 4.0
    if name == "a":
        assert ref["maxin"] == 4 and ref["nzeta"] == 64 * 12
    if name == "cell8":
        assert box[3] == 5.432 < 2 * 4.0 and ref["npairs"] == 8 * 4
    if name == "dimer":
        assert ref["nzeta"] == 0 and ref["npairs"] == 2
    _check_static(_static(x, box, t), ref, what=f"tersoff static {name}")


def test_dimer_around_the_cutoff(ref_si):
    """at R + D - 1e-6, exactly R + D = 3 A, and + 1e-6: finite values just inside, exactly zero from the cutoff on"""
    for d in (-1e-6, 0.0, 1e-6):
        x, box, t = tsn.case_dimer(3.0 + d)
        assert x[1, 0] - x[0, 0] == 3.0 + d
        got, ref = _static(x, box, t), ref_si.compute(x, box, t)
        assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and math.isfinite(got["e_rep"]) and math.isfinite(got["e_att"])
        _check_static(got, ref, what=f"tersoff dimer at R + D {d:+.0e}")
        assert got["npairs"] == (2 if d < 0 else 0)
        if d < 0:
            assert 0.0 < abs(got["e_rep"] + got["e_att"]) < 1e-8


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_static_parity_gas(ref_si, seed):
    """216 atoms at random, 16.3 A box, minimum separation 2.0 A: ragged lists of up to 10 neighbours, some 190 pairs inside the switching shell"""
    x, box, t = tsn.case_gas(seed)
    ref = ref_si.compute(x, box, t)
    print(f"tersoff gas seed {seed}: most neighbours {ref['maxin']}, pairs in the switching shell {ref['nshell']}")
    assert 8 <= ref["maxin"] <= 10 and 175 <= ref["nshell"] <= 205
    _check_static(_static(x, box, t), ref, what=f"tersoff static gas {seed}")


@pytest.mark.parametrize("order", ["Si C", "C Si"])
def test_static_parity_silicon_carbide(ref_sic, order):
    """64-atom zincblende SiC, a = 4.36 A, with both element orders in `elements` (the types swapped with them: the same crystal)"""
    x, box, t = tsn.case_sic()
    ref = ref_sic.compute(x, box, t)
    # (the jitter brings some Si-Si second neighbours, 3.08 A apart on the lattice, inside their 3.0 A: pairs without a bond between them)
    assert ref["npairs"] > 64 * 4 and len(set(t)) == 2
    got = _static(x, box, t if order == "Si C" else 1 - t, elements=tuple(order.split()), masses=MASS2 if order == "Si C" else MASS2[::-1])
    _check_static(got, ref, what=f"tersoff static SiC, elements {order}")


@pytest.mark.parametrize("which", ["synth", "clamp"])
def test_static_parity_synthetic_file(synth_files, which):
    """m = 1 and m = 3 with lambda3 = 1.3 and gamma = 0.7, R, D of the i j k entries their own; `clamp`: lambda3 = 40, both clamps of the
    exponent and the large-zeta end of b"""
    ref_ts = tsn.Tersoff(tsn.read_tersoff(synth_files[which], ["X", "Y"])[0])
    x, box, t = tsn.case_synth()
    ref = ref_ts.compute(x, box, t)
    assert len(set(t)) == 2 and ref["nzeta"] > 0
    _check_static(_static(x, box, t, path=synth_files[which], elements=("X", "Y"), masses=(28.0, 20.0)), ref, what=f"tersoff static {which}")


@pytest.mark.parametrize("n", [63, 65, 1025, 1200])
def test_atom_count_edges(ref_si, n):
    """a partial only tile, a second tile of one atom, one atom past the LDS force table (1 024), and 1 200 atoms: a partial last tile"""
    x, box, t = tsn.case_count(n)
    _check_static(_static(x, box, t), ref_si.compute(x, box, t), what=f"tersoff static n = {n}")


def test_row_overflow_regrows_and_retries(ref_si, monkeypatch):
    """the scaled cell with the row capacity forced low through the overflow test hook: fault bit 1, the retry recovers"""
    x, box, t = tsn.case_scaled()
    ref = ref_si.compute(x, box, t)
    normal = _static(x, box, t)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    got = _static(x, box, t)
    _check_static(got, ref, what="tersoff static after a row overflow")
    assert got["rowcap"] < normal["rowcap"]          # it started at 8 entries and grew to what the rows asked for, not to the default


def test_more_than_32_neighbours_is_an_error():
    """a centre atom with 33 atoms on a sphere of 2.6 A around it: one more than the force kernel lists -- an error, never a wrong force"""
    x, box, t = tsn.case_crowded(33)
    assert (np.linalg.norm(x[1:] - x[0], axis=1) < 3.0).sum() == 33
    with pytest.raises(capi.EngineError, match="more than 32 neighbours"):
        _static(x, box, t)
    x, box, t = tsn.case_crowded(20)                 # (the same generator below the limit runs)
    assert np.isfinite(_static(x, box, t)["f"]).all()


def test_nve_dynamics_and_sampled_pressure(ref_si):
    x, box, t = tsn.case_a()
    s = rk.Setup("si", SIC, None, MASS, (x, box, t), rk.velocities(t, MASS, 300.0, 1))
    rk.nve_and_sampled_pressure(TERSOFF, ref_si, s, steps=20, tol_x=1e-9, tol_v=1e-11, tol_p=1e-10)


@pytest.fixture(scope="module")
def static_constants(ref_si):
    """C11 and C12 of silicon (GPa) from second differences of the numpy energy under +-1e-3 homogeneous strain of the perfect lattice"""
    x, box = tsn.diamond(2, 2, 2, tsn.A_SI)
    t = tsn.zeros(len(x))
    h, v = 1e-3, tsn.volume(box)
    E = lambda e1, e2: ref_si.energy(*tsn.strained(x, box, np.diag([e1, e2, 0.0])), t)
    c11 = (E(h, 0.0) - 2.0 * E(0.0, 0.0) + E(-h, 0.0)) / h ** 2 / v
    c12 = (E(h, h) - E(h, -h) - E(-h, h) + E(-h, -h)) / (4.0 * h ** 2) / v
    return c11 * tsn.KCALMOL_A3_TO_GPA, c12 * tsn.KCALMOL_A3_TO_GPA


def test_elastic_constants(static_constants):
    """C11 and C12 of silicon from the GPU virials at +-1e-3 strain, through set_state, against second differences of the numpy energy
    within 0.1 % (both are finite differences with a relative truncation of order h^2 C''' / C ~ 1e-5).  No literature value is asserted."""
    x, box = tsn.diamond(2, 2, 2, tsn.A_SI)
    t = tsn.zeros(len(x))
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        h = 1e-3
        sig = {}
        for s in (+1, -1):
            xs, bs = tsn.strained(x, box, np.diag([s * h, 0.0, 0.0]))
            e.set_state(5, "si", 1, bs, xs, np.zeros_like(xs))
            sig[s] = -e.tersoff_compute("si", 1, qp=5)["w"] / tsn.volume(bs) * tsn.KCALMOL_A3_TO_GPA
        c11 = (sig[+1][0] - sig[-1][0]) / (2 * h)
        c12 = (sig[+1][1] - sig[-1][1]) / (2 * h)
        print(f"tersoff elastic constants on the device: C11 {c11:.3f} GPa, C12 {c12:.3f} GPa; numpy energy: C11 {static_constants[0]:.3f}, C12 {static_constants[1]:.3f}")
        assert abs(c11 / static_constants[0] - 1.0) < 1e-3 and abs(c12 / static_constants[1] - 1.0) < 1e-3
    finally:
        e.close()


def test_strain_batch_equals_the_two_runs():
    """tension plus a shear component, nss = 10: the update against the straining run and the sampling run issued through the parity hooks"""
    x, box, t = tsn.case_a()
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s = rk.Setup("si", SIC, None, MASS, (x, box, t), rk.velocities(t, MASS, 300.0, 2))
    rk.strain_batch_vs_debug_runs(TERSOFF, s, s1, expect_nts=30, tol=1e-10)


@pytest.fixture(scope="module")
def eleven():
    """11 simulations over two Tersoff materials (silicon, and silicon carbide with two elements), and each one's stress alone in a fresh engine"""
    mats = {"si": (tsn.case_a(), SIC, ("Si",), MASS), "sic": (tsn.case_sic(), SIC, ("Si", "C"), MASS2)}
    return rk.batch_vs_alone_fixture(TERSOFF, mats, 11, 21, thermal_masses=MASS)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_eleven_equals_each_alone(eleven, split):
    rk.assert_batch_vs_alone(TERSOFF, eleven, split, what="tersoff batch of 11 over two materials", tol=1e-9)


@pytest.fixture(scope="module")
def sheared():
    """Eight simulations of a 5 x 2 x 2 silicon cell (160 atoms) written with xy = 2 a = 0.4 lx (the same crystal: a lattice translation),
    each sheared by 0.105 to 0.14 lx in xy, so that every one crosses +lx / 2 and flips once; each one's stress, flips and box alone"""
    x, box = tsn.diamond(5, 2, 2, tsn.A_SI)
    box[6] = 2.0 * tsn.A_SI
    t = tsn.zeros(len(x))
    return rk.sheared_fixture(TERSOFF, rk.Setup("si", SIC, None, None, (x, box, t), rk.velocities(t, MASS, 300.0, 31)))


def test_box_flips_inside_a_split_batch(sheared):
    """eight is the smallest batch that runs as two parts: same stresses as each simulation alone, as many flips, every box back inside"""
    rk.assert_flips_in_split_batch(sheared, "si", 1, what="tersoff sheared batch of 8 (split)", tol=1e-9)


def test_mixed_updates_are_refused(small_pe):
    """Tersoff + Stillinger-Weber and Tersoff + OPLS in one update: SCEMA_MD_ERR_ARG before anything is planned; each alone runs"""
    x, box, t = tsn.case_a()
    e = _engine(cut_lj=5.0, cut_coul=4.0, skin=1.0, kspace_accuracy=1e-5)
    try:
        e.tersoff_configure("ts", SIC)
        e.sw_configure("sw", SI_SW)
        e.register_replica("ts", 1, capi.bare_system(t, x, box))
        e.register_replica("sw", 1, capi.bare_system(t, x, box))
        e.register_replica("pe", 1, small_pe)
        L = box[3:6] - box[:3]
        s = np.array([1e-3 * L[0], 0.0, 0.0, 0.0, 0.0, 0.0])
        mk = lambda q, m: capi.make_sim(q, m, 1, s, nss=10, most_recent=capi.QP_NONE)
        for other in ("sw", "pe"):
            with pytest.raises(capi.EngineError, match="rc=1.*mixes"):
                e.strain_batch([mk(0, "ts"), mk(1, other)])
            assert not e.has_state(0, "ts", 1) and not e.has_state(1, other, 1)
        assert e.strain_batch([mk(0, "ts")])[0].stress_updated == 1
        rk.assert_not_attached(TERSOFF, e, "pe")
        rk.assert_not_attached(TERSOFF, e, "sw")
    finally:
        e.close()


def test_configuring_replaces_the_other_attachment(ref_si):
    """a material holds one attachment: a Tersoff potential configured over a Stillinger-Weber one replaces it (rows and element arrays are
    rebuilt: the forces are those of a fresh engine), and the other way round"""
    x, box, t = tsn.case_a()
    ref = ref_si.compute(x, box, t)
    ref_sw = swn.SW(swn.read_sw(SI_SW, ["Si"])[0]).compute(x, box, t)
    e = _engine()
    try:
        e.sw_configure("si", SI_SW)
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        sw0 = e.sw_compute("si", 1)
        e.tersoff_configure("si", SIC)
        with pytest.raises(capi.EngineError, match="no Stillinger-Weber potential"):
            e.sw_compute("si", 1)
        _check_static(e.tersoff_compute("si", 1), ref, what="tersoff over an SW attachment")
        e.sw_configure("si", SI_SW)
        rk.assert_not_attached(TERSOFF, e, "si")
        sw1 = e.sw_compute("si", 1)
        assert sw1["npairs"] == sw0["npairs"] == ref_sw["npairs"]
        assert np.abs(sw1["f"] - ref_sw["f"]).max() <= 1e-10 * np.abs(ref_sw["f"]).max()
    finally:
        e.close()


DIMER = rk.Setup("si", SIC, ("Si",), None, (np.array([[5.0, 6.0, 6.0], [7.3, 6.1, 5.9]]), np.array([0.0, 0.0, 0.0, 12.0, 12.0, 12.0, 0.0, 0.0, 0.0]), tsn.zeros(2)),
                 np.array([[1e-3, 2e-3, -1e-3], [-1e-3, -2e-3, 1e-3]]))


def test_self_configuration_from_the_scripts_folder(ref_si, tmp_path):
    """`pair_coeff * * ${locs}/SiC.tersoff Si` in in.strain.lammps configures a bare replica whose material has nothing attached; a folder
    that also holds Si.sw still takes Stillinger-Weber; a malformed line is an error"""
    scripts = tmp_path / "lammps_scripts_tersoff"
    scripts.mkdir()
    shutil.copy(SIC, scripts / "SiC.tersoff")
    (scripts / "in.strain.lammps").write_text("# straining run\npair_style tersoff\n#pair_coeff * * ${locs}/other.tersoff C\n"
                                              "pair_coeff * * ${locs}/SiC.tersoff Si   # the potential\nfix 1 all nvt temp 300 300 100\n")
    # (a two-atom replica: every force component is the sum of two terms, so two runs of the same configuration agree bit for bit)
    a, sa = rk.dimer_update(TERSOFF, DIMER, scripts, False, 1.2e-2)
    b, sb = rk.dimer_update(TERSOFF, DIMER, scripts, True, 1.2e-2)
    assert np.isfinite(a).all() and np.abs(a).max() > 0.0
    assert np.array_equal(a, b) and all(np.array_equal(p, q) for p, q in zip(sa, sb))
    # the update configured the material: static forces of the 64-atom cell against the numpy helper
    x, box, t = tsn.case_a()
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "si", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    e = _engine()
    try:
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS, 300.0, 3)))
        rk.assert_not_attached(TERSOFF, e, "si")
        assert e.strain_batch([mk(scripts)])[0].stress_updated == 1
        _check_static(e.tersoff_compute("si", 1), ref_si.compute(x, box, t), what="tersoff self-configured")
    finally:
        e.close()
    # Si.sw in the folder keeps its precedence
    both = tmp_path / "both"
    shutil.copytree(scripts, both)
    shutil.copy(SI_SW, both / "Si.sw")
    e = _engine()
    try:
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS, 300.0, 3)))
        assert e.strain_batch([mk(both)])[0].stress_updated == 1
        assert e.sw_compute("si", 1)["npairs"] >= 2 * len(x)      # (the Stillinger-Weber hook answers: that potential is attached)
        rk.assert_not_attached(TERSOFF, e, "si")
    finally:
        e.close()
    # malformed lines, and a line that names a file the folder lacks: the reader's message
    rk.assert_malformed_pair_coeff_lines(TERSOFF, rk.Setup("si", SIC, None, None, (x, box, t)), tmp_path, ".tersoff", "Si", missing_file=True)


def test_init_material_runs_for_a_tersoff_material(static_constants):
    """scema_md_init_material through the same switch: homogenisation run + 12 strained runs of the jittered 64-atom cell at 10 K with 20
    sampling steps.  A plumbing check: finite C11 and C12 within 2 % of the static ones"""
    x, box, t = tsn.case_a()
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS, 10.0, 9)))
        length, stress, stiff = e.init_material("si", 1, dt=1.0, temperature=10.0, nss=20, strain_ampl=0.005, strain_rate=1e-4)
        assert np.allclose(length, box[3:6] - box[:3]) and np.isfinite(stress).all() and np.isfinite(stiff).all()
        c11, c12 = stiff[0, 0] / 1e9, stiff[0, 3] / 1e9        # file order 00, 01, 02, 11, 12, 22
        print(f"tersoff init_material: C11 {c11:.2f} GPa, C12 {c12:.2f} GPa (static lattice: {static_constants[0]:.2f}, {static_constants[1]:.2f})")
        assert abs(c11 / static_constants[0] - 1.0) < 0.02 and abs(c12 / static_constants[1] - 1.0) < 0.02
    finally:
        e.close()
