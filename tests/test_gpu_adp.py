"""The force stage of the angular-dependent potential on the GPU (md_adp.hip, engine_rowpot.cpp) against the independent FP64 numpy
restatement tests/adp_numpy.py, which tests/test_adp_host.py pins on the CPU (no LAMMPS exists to compare with): static parity on the
shapes at which the kernels or the driver take another path, forces equal bit for bit between evaluations, the embedded-atom stage on
a file without angular terms, shear constants, dynamics, the virial -> pressure conversion, whole evaluations, batches over two
materials, box flips inside a split batch, refusals, replaced attachments, self-configuration from the scripts folder.

Budgets, those of tests/test_gpu_eam.py: static parity 1e-10 of the largest force component, 1e-9 of the largest energy term and of the
largest virial component (FP64 sums of a few hundred terms in another order); NVE after 20 steps 1e-9 A and 1e-11 A/fs; the sampled
pressure 1e-10 relative; whole evaluations 1e-10 / 1e-9 relative (the same arithmetic in another launch shape).  Forces carry no atomic
sum in this stage: where two evaluations see the same state they are compared bit for bit.

The trap: in a perfect cubic lattice mu = 0 and lam is a multiple of the unit tensor, the angular energy and forces vanish, and a
perfect cell tests nothing of this stage.  Every parity case is a cluster, jittered, strained or an alloy; _check asserts that
the angular part of the reference force is at least a hundredth of the embedded-atom part wherever there is a pair.

What the groups catch.  Static parity: mu_j with the wrong sign, the trace left in Lambda, the w' term, a pair index mixed up (both
alloy orders, the three-type map), the record of the wrong atom gathered (the alloy: every atom's record differs), the extrapolation
above rhomax, a wrong image shift or a missed self-image (the 4-atom cell, the triclinic box), a short last tile or group and rows
longer than one trip of 16 lanes (the atom counts), rows that overflow.  The wrong builds named first were tried on the CPU driver
(tests/test_adp_host.py::test_wrong_builds_are_caught says what failed).
"""
import math
import os
import shutil

import numpy as np
import pytest

import adp_numpy as an
import eam_numpy as en
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.adp")
CUAG_EAM = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
MASS = (an.CU_MASS,)
MASS2 = (an.CU_MASS, an.AG_MASS)


@pytest.fixture(scope="module")
def ref_cu():
    return an.ADP(an.read_adp(CUAG, ["Cu"])[0])


@pytest.fixture(scope="module")
def ref_cuag():
    return an.ADP(an.read_adp(CUAG, ["Cu", "Ag"])[0])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """copper with rhomax at 1.1 times the lattice's density (a cell compressed by 5 % passes it); the fixture with u = w = 0 and the
    plain setfl file with the same F, rho and r phi"""
    d = tmp_path_factory.mktemp("adp")
    an.write_fixture(str(d / "CuLow.adp"), ["Cu"], rhomax_over_rhoe=1.1)
    an.write_fixture(str(d / "zero.adp"), ["Cu", "Ag"], angular=False)
    an.write_eam_twin(str(d / "twin.eam.alloy"), ["Cu", "Ag"])
    return {"low": str(d / "CuLow.adp"), "zero": str(d / "zero.adp"), "twin": str(d / "twin.eam.alloy")}


ADP = rk.Pot("adp", "adp_configure", "adp_compute", "ADP", ("e_pair", "e_manybody"), ("npairs", "nabove"), counts="pairs {npairs}, above rhomax {nabove}",
             energy_scale=("e_pair", "e_embed", "e_angular"))


_engine = rk.engine
_static = rk.static_of(ADP, CUAG, ("Cu",), MASS)


def no_pairs(got, ref, scale, what):
    """no pair: the embedding energy of bare atoms, no force at all"""
    if ref["npairs"] != 0:
        return False
    assert not ref["f"].any() and (got["f"] == 0.0).all() and (got["w"] == 0.0).all() and got["e_pair"] == 0.0 and got["e_manybody"] == ref["e_embed"]
    print(f"{what}: no pairs, forces exactly zero, rows {got['maxrow']}/{got['rowcap']}")
    return True


def _check(got, ref, what="adp static", angular=True):
    """angular: the case tests the angular terms -- their share of the reference force is asserted wherever there is a pair"""
    share = np.abs(ref["f_angular"]).max() / np.abs(ref["f_eam"]).max() if ref["npairs"] else None
    rk.check_static(got, ref, ADP, tol_f=1e-10, tol_e=1e-9, tol_w=1e-9, what=what, no_pairs=no_pairs,
                    tail=f", angular / embedded-atom force {share:.3f}" if ref["npairs"] else "")
    if angular and ref["npairs"]:
        assert 0.01 <= share


# the shapes at which a path changes: no pair; three atoms; the image search two boxes deep with an atom's own images; a triclinic box
# with atoms outside it; one image deep with 54 neighbours in range (32, 108 and 256 atoms); ragged rows (the gas)
COPPER = {"single": an.case_single, "trimer": an.case_trimer, "cell4": an.case_cell4, "triclinic": an.case_triclinic, "j32": lambda: an.case_jitter(2),
          "j108": lambda: an.case_jitter(3), "j256": lambda: an.case_jitter(4), "gas": an.case_gas}


@pytest.mark.parametrize("name", sorted(COPPER))
def test_static_parity_copper(ref_cu, name):
    x, box, t = COPPER[name]()
    ref = ref_cu.compute(x, box, t)
    if name in ("j32", "j108", "j256", "triclinic"):
        assert ref["maxin"] > 32          # rows longer than two trips of 16 lanes
    if name == "cell4":
        assert box[3] == an.A_CU < 6.5 and ref["maxin"] >= 50
    if name == "single":
        assert ref["npairs"] == 0 and ref["e_embed"] == ref_cu.t["F"][0][0]
    _check(_static(x, box, t), ref, what=f"adp static {name}")


@pytest.mark.parametrize("pair", ["cucu", "cuag", "agag"])
def test_static_parity_dimers(ref_cuag, pair):
    """a dimer of each pair along a general direction: mu = +-u d and lam = w d (x) d, so the pair's own u, u', w, w' are all that acts"""
    types, r = {"cucu": ((0, 0), 2.5037), "cuag": ((0, 1), 2.7), "agag": ((1, 1), 2.9)}[pair]
    x, box, t = an.case_dimer(r, types)
    ref = ref_cuag.compute(x, box, t)
    got = _static(x, box, t, elements=("Cu", "Ag"), masses=MASS2)
    _check(got, ref, what=f"adp dimer {pair}")
    assert np.abs(got["f"][0] + got["f"][1]).max() <= 1e-13 * np.abs(got["f"]).max()          # each end sums its own force: the exact negative to rounding


def test_a_cell_below_the_two_image_limit_is_refused():
    x, box, t = an.case_cell4(3.24)
    with pytest.raises(capi.EngineError, match=r"box width 3.240 < \(cutoff\+skin\)/2 = 3.250"):
        _static(x, box, t)


def test_dimer_around_the_cutoff(ref_cu):
    """at 5.5 A - 1e-6, exactly 5.5 A, and + 1e-6: finite values just inside, exactly zero and not counted from the cutoff on"""
    f0 = ref_cu.t["F"][0][0]
    for d in (-1e-6, 0.0, 1e-6):
        x, box, t = en.case_dimer(5.5 + d)          # (along x from x = 0: r is the distance to the bit)
        assert x[1, 0] - x[0, 0] == 5.5 + d
        got, ref = _static(x, box, t), ref_cu.compute(x, box, t)
        assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and math.isfinite(got["e_pair"]) and math.isfinite(got["e_manybody"])
        _check(got, ref, what=f"adp dimer at the cutoff {d:+.0e}", angular=False)
        assert got["npairs"] == (2 if d < 0 else 0)
        if d >= 0:
            assert not got["f"].any() and not got["w"].any() and got["e_pair"] == 0.0 and got["e_manybody"] == 2.0 * f0


@pytest.mark.parametrize("order", ["Cu Ag", "Ag Cu", "Cu Ag Cu"])
def test_static_parity_alloy(ref_cuag, order):
    """32 atoms, the two elements at random, with both element orders in `elements` (the types swapped with them: the same crystal), and
    with three LAMMPS types of which the first and the third are copper (every second copper atom takes the third)"""
    x, box, t = an.case_alloy()
    ref = ref_cuag.compute(x, box, t)
    assert len(set(t)) == 2 and ref["maxin"] > 32
    if order == "Cu Ag":
        types, masses = t, MASS2
    elif order == "Ag Cu":
        types, masses = 1 - t, MASS2[::-1]
    else:
        types = t.copy()
        types[np.nonzero(t == 0)[0][::2]] = 2
        masses = (an.CU_MASS, an.AG_MASS, an.CU_MASS)
        assert len(set(types)) == 3
    _check(_static(x, box, types, elements=tuple(order.split()), masses=masses), ref, what=f"adp static alloy, elements {order}")


def test_static_parity_above_rhomax(files):
    ref_e = an.ADP(an.read_adp(files["low"], ["Cu"])[0])
    x, box, t = an.case_jitter(2, a=0.95 * an.A_CU)
    ref = ref_e.compute(x, box, t)
    assert ref["nabove"] == 32
    _check(_static(x, box, t, path=files["low"]), ref, what="adp static above rhomax")


@pytest.mark.parametrize("n", [63, 65, 1025])
def test_atom_count_edges(ref_cu, n):
    """a partial only tile, a second tile of one atom, and 1 025 atoms (a group of the last round alone); rows of up to 54 entries: four
    trips of 16 lanes"""
    x, box, t = an.case_count(n)
    ref = ref_cu.compute(x, box, t)
    assert ref["maxin"] > 16
    _check(_static(x, box, t), ref, what=f"adp static n = {n}")


def test_reproducible_bits_and_rows_regrown_after_an_overflow(ref_cu, monkeypatch):
    """one 108-atom state: two evaluations in one engine, a fresh engine, and an engine whose row capacity was forced low through the
    overflow test hook (fault bit 1, the retry regrows the rows) -- the same rows in the same order, neither kernel has an atomic on a
    force, a density, a dipole or a quadrupole: the same bits everywhere"""
    x, box, t = an.case_jitter(3)
    ref = ref_cu.compute(x, box, t)
    a = _static(x, box, t)
    e = _engine()
    try:
        e.adp_configure("m", CUAG, ("Cu",))
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS))
        b, c = e.adp_compute("m", 1), e.adp_compute("m", 1)
    finally:
        e.close()
    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]) and np.array_equal(b["f"], c["f"])
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    got = _static(x, box, t)
    _check(got, ref, what="adp static after a row overflow")
    assert got["rowcap"] < a["rowcap"]          # it started at 8 entries and grew to what the rows asked for, not to the default
    assert np.array_equal(got["f"], a["f"])


def test_without_angular_terms_it_is_the_embedded_atom_stage(files):
    """u = w = 0: the ADP stage on that file against the EAM stage on the plain setfl file with the same F, rho and r phi"""
    x, box, t = an.case_alloy()
    got = _static(x, box, t, path=files["zero"], elements=("Cu", "Ag"), masses=MASS2)
    e = _engine()
    try:
        e.eam_configure("m", files["twin"], ("Cu", "Ag"))
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS2))
        twin = e.eam_compute("m", 1)
    finally:
        e.close()
    fs, ws = np.abs(twin["f"]).max(), np.abs(twin["w"]).max()
    es = max(abs(twin["e_pair"]), abs(twin["e_embed"]))
    df, dw = np.abs(got["f"] - twin["f"]).max(), np.abs(got["w"] - twin["w"]).max()
    de = max(abs(got["e_pair"] - twin["e_pair"]), abs(got["e_manybody"] - twin["e_embed"]))
    print(f"adp with u = w = 0 vs the eam stage: force {df / fs:.2e}, energy {de / es:.2e}, virial {dw / ws:.2e}")
    assert got["npairs"] == twin["npairs"] and df <= 1e-10 * fs and de <= 1e-9 * es and dw <= 1e-9 * ws


def _shear_constants(pot):
    """C44 and C' = (C11 - C12) / 2 of copper (GPa) from second differences of a numpy energy under +-1e-3 homogeneous strain of the
    perfect lattice, as slopes of the stress (tests/test_gpu_eam.py::static_constants says why C12 carries the lattice's stress)"""
    x, box = an.fcc(2, 2, 2, an.A_CU)
    t = an.zeros(len(x))
    h, v = 1e-3, an.volume(box)
    E = lambda eps: pot.energy(*an.strained(x, box, eps), t)
    d = lambda e1, e2: np.diag([e1, e2, 0.0])
    s = np.zeros((3, 3))
    s[0, 1] = h
    e0 = E(d(0.0, 0.0))
    c11 = (E(d(h, 0.0)) - 2.0 * e0 + E(d(-h, 0.0))) / h ** 2 / v
    c12 = (E(d(h, h)) - E(d(h, -h)) - E(d(-h, h)) + E(d(-h, -h))) / (4.0 * h ** 2) / v
    c44 = (E(s) - 2.0 * e0 + E(-s)) / h ** 2 / v
    sigma0 = -pot.compute(x, box, t)["w"][1] / v
    return c44 * an.KCALMOL_A3_TO_GPA, 0.5 * (c11 - (c12 - sigma0)) * an.KCALMOL_A3_TO_GPA


def test_shear_constants_feel_the_angular_terms(ref_cu, files):
    """C44 and C' as slopes of the stress from the GPU virials at +-1e-3 strain of the perfect lattice (strained, it is cubic no more:
    lam is no multiple of the unit tensor), against second differences of the numpy energy within 0.1 % (both are finite differences
    with a relative truncation of order h^2 C''' / C ~ 1e-5); and both differ from the constants of the file with u = w = 0 by more
    than that: the angular terms show under strain.  No literature value is asserted."""
    want = _shear_constants(ref_cu)
    plain = _shear_constants(an.ADP(an.read_adp(files["zero"], ["Cu"])[0]))
    x, box = an.fcc(2, 2, 2, an.A_CU)
    t = an.zeros(len(x))
    e = _engine()
    try:
        e.adp_configure("cu", CUAG)
        e.register_replica("cu", 1, capi.bare_system(t, x, box, masses=MASS))
        h = 1e-3
        sig = {}
        shear = np.zeros((3, 3))
        shear[0, 1] = h
        for name, eps in (("n", np.diag([h, 0.0, 0.0])), ("s", shear)):
            for s in (+1, -1):
                xs, bs = an.strained(x, box, s * eps)
                e.set_state(5, "cu", 1, bs, xs, np.zeros_like(xs))
                sig[name, s] = -e.adp_compute("cu", 1, qp=5)["w"] / an.volume(bs) * an.KCALMOL_A3_TO_GPA
        c11 = (sig["n", +1][0] - sig["n", -1][0]) / (2 * h)
        c12 = (sig["n", +1][1] - sig["n", -1][1]) / (2 * h)
        c44 = (sig["s", +1][3] - sig["s", -1][3]) / (2 * h)
        got = (c44, 0.5 * (c11 - c12))
        print(f"adp shear constants on the device: C44 {got[0]:.3f}, C' {got[1]:.3f} GPa; numpy energy: {want[0]:.3f}, {want[1]:.3f}; "
              f"with u = w = 0: {plain[0]:.3f}, {plain[1]:.3f}")
        for g, w, p in zip(got, want, plain):
            assert abs(g / w - 1.0) < 1e-3 and abs(w / p - 1.0) > 1e-3
    finally:
        e.close()


def test_nve_dynamics_and_sampled_pressure(ref_cu):
    x, box, t = an.case_jitter(2)
    s = rk.Setup("cu", CUAG, None, MASS, (x, box, t), rk.velocities(t, MASS, 300.0, 1))
    rk.nve_and_sampled_pressure(ADP, ref_cu, s, steps=20, tol_x=1e-9, tol_v=1e-11, tol_p=1e-10)


def test_strain_batch_equals_the_two_runs():
    """tension plus a shear component, nss = 10: the update against the straining run and the sampling run issued through the parity hooks"""
    x, box, t = an.case_jitter(2)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s = rk.Setup("cu", CUAG, None, MASS, (x, box, t), rk.velocities(t, MASS, 300.0, 2))
    rk.strain_batch_vs_debug_runs(ADP, s, s1, expect_nts=30, tol=1e-10)


@pytest.fixture(scope="module")
def eleven():
    """11 simulations over two ADP materials (copper, and the alloy with two elements), each one's stress alone in a fresh engine"""
    mats = {"cu": (an.case_jitter(2), CUAG, ("Cu",), MASS), "cuag": (an.case_alloy(), CUAG, ("Cu", "Ag"), MASS2)}
    return rk.batch_vs_alone_fixture(ADP, mats, 11, 21, thermal_masses=MASS)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_eleven_equals_each_alone(eleven, split):
    """the stresses of the batch, whole and as part batches, against each simulation alone; and the forces on every end state, evaluated
    in the engine that ran the batch (its slots hold rows and records of other simulations) and in a fresh engine handed the same
    state: equal bit for bit"""
    rk.assert_batch_vs_alone(ADP, eleven, split, what="adp batch of 11 over two materials", tol=1e-9, bitwise_forces=True)


@pytest.fixture(scope="module")
def sheared():
    """Eight simulations of a jittered 5 x 2 x 2 copper cell (80 atoms) written with xy = 2 a = 0.4 lx, each sheared by 0.105 to 0.14 lx
    in xy, so that every one crosses +lx / 2 and flips once; each one's stress, flips and box alone"""
    x, box = an.fcc(5, 2, 2, an.A_CU)
    x = x + np.random.default_rng(17).uniform(-0.1, 0.1, x.shape)
    box[6] = 2.0 * an.A_CU
    t = an.zeros(len(x))
    return rk.sheared_fixture(ADP, rk.Setup("cu", CUAG, None, MASS, (x, box, t), rk.velocities(t, MASS, 300.0, 31)))


def test_box_flips_inside_a_split_batch(sheared):
    """eight is the smallest batch that runs as two parts: same stresses as each simulation alone, as many flips, every box back inside"""
    rk.assert_flips_in_split_batch(sheared, "cu", 1, what="adp sheared batch of 8 (split)", tol=1e-9)


def test_an_update_mixed_with_eam_is_refused():
    """ADP + EAM in one update: SCEMA_MD_ERR_ARG before anything is planned, naming EAM, the first of the two kinds in the table, and
    leaving no state; each alone runs"""
    x, box, t = an.case_jitter(2)
    e = _engine()
    try:
        e.adp_configure("adp", CUAG)
        e.eam_configure("eam", CUAG_EAM)
        e.register_replica("adp", 1, capi.bare_system(t, x, box, masses=MASS))
        e.register_replica("eam", 1, capi.bare_system(t, x, box, masses=MASS))
        L = box[3:6] - box[:3]
        s = np.array([1e-3 * L[0], 0.0, 0.0, 0.0, 0.0, 0.0])
        mk = lambda q, m: capi.make_sim(q, m, 1, s, nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "adp"), mk(1, "eam")], [mk(0, "eam"), mk(1, "adp")]):
            with pytest.raises(capi.EngineError, match="rc=1.*mixes EAM materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "adp", 1) and not e.has_state(1, "eam", 1) and not e.has_state(0, "eam", 1) and not e.has_state(1, "adp", 1)
        assert e.strain_batch([mk(0, "adp")])[0].stress_updated == 1
        assert e.strain_batch([mk(1, "eam")])[0].stress_updated == 1
        with pytest.raises(capi.EngineError, match=r"no ADP potential attached to material eam \(scema_md_adp_configure\)"):
            e.adp_compute("eam", 1)
        with pytest.raises(capi.EngineError, match="no EAM potential"):
            e.eam_compute("adp", 1)
    finally:
        e.close()


def test_configuring_over_an_eam_attachment_and_back(ref_cu):
    """a material holds one attachment: an ADP potential configured over an EAM one replaces it (rows and element arrays are rebuilt:
    the forces are those of a fresh engine, bit for bit), and the other way round"""
    x, box, t = an.case_jitter(2)
    fresh = _static(x, box, t)
    ref_eam = en.EAM(en.read_setfl(CUAG_EAM, ["Cu"])[0]).compute(x, box, t)
    e = _engine()
    try:
        e.eam_configure("m", CUAG_EAM)
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS))
        eam0 = e.eam_compute("m", 1)
        e.adp_configure("m", CUAG)
        with pytest.raises(capi.EngineError, match="no EAM potential"):
            e.eam_compute("m", 1)
        got = e.adp_compute("m", 1)
        _check(got, ref_cu.compute(x, box, t), what="adp over an EAM attachment")
        assert np.array_equal(got["f"], fresh["f"])
        e.eam_configure("m", CUAG_EAM)
        rk.assert_not_attached(ADP, e, "m")
        eam1 = e.eam_compute("m", 1)
        assert np.array_equal(eam1["f"], eam0["f"]) and np.abs(eam1["f"] - ref_eam["f"]).max() <= 1e-10 * np.abs(ref_eam["f"]).max()
    finally:
        e.close()


DIMER = rk.Setup("cu", CUAG, ("Cu",), MASS, (np.array([[5.0, 6.0, 6.0], [7.4, 6.1, 5.9]]), np.array([0.0, 0.0, 0.0, 14.0, 14.0, 14.0, 0.0, 0.0, 0.0]), an.zeros(2)),
                 np.array([[1e-3, 2e-3, -1e-3], [-1e-3, -2e-3, 1e-3]]))


def test_self_configuration_from_the_scripts_folder(ref_cu, tmp_path):
    """`pair_coeff * * ${locs}/CuAg.adp Cu` in in.strain.lammps configures a bare replica whose material has nothing attached: the end
    stress, the end state and the forces on it equal those of the configured run bit for bit; an EAM line in the same script keeps its
    precedence; a malformed line is an error"""
    scripts = tmp_path / "lammps_scripts_adp"
    scripts.mkdir()
    shutil.copy(CUAG, scripts / "CuAg.adp")
    (scripts / "in.strain.lammps").write_text("# straining run\npair_style adp\n#pair_coeff * * ${locs}/other.adp Ag\n"
                                              "pair_coeff * * ${locs}/CuAg.adp Cu   # the potential\nfix 1 all nvt temp 300 300 100\n")
    # (a two-atom replica -- mu = +-u d, lam = w d (x) d: the angular terms act -- whose every sum has two terms: two runs of the same
    # configuration agree bit for bit; the third result is the force on the end state)
    a, sa, fa = rk.dimer_update(ADP, DIMER, scripts, False, 1.4e-2, compute_qp=0)
    b, sb, fb = rk.dimer_update(ADP, DIMER, scripts, True, 1.4e-2, compute_qp=0)
    fa, fb = fa["f"], fb["f"]
    assert np.isfinite(a).all() and np.abs(a).max() > 0.0 and np.abs(fa).max() > 0.0
    assert np.array_equal(a, b) and all(np.array_equal(p, q) for p, q in zip(sa, sb)) and np.array_equal(fa, fb)
    # the update configured the material: static forces of the 32-atom cell against the numpy helper
    x, box, t = an.case_jitter(2)
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "cu", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    e = _engine()
    try:
        e.register_replica("cu", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS, 300.0, 3), masses=MASS))
        rk.assert_not_attached(ADP, e, "cu")
        assert e.strain_batch([mk(scripts)])[0].stress_updated == 1
        _check(e.adp_compute("cu", 1), ref_cu.compute(x, box, t), what="adp self-configured")
    finally:
        e.close()
    # an EAM line keeps its precedence: the table is searched in its order
    both = tmp_path / "both"
    shutil.copytree(scripts, both)
    shutil.copy(CUAG_EAM, both / "CuAg.eam.alloy")
    (both / "in.strain.lammps").write_text("pair_coeff * * ${locs}/CuAg.adp Cu\npair_coeff * * ${locs}/CuAg.eam.alloy Cu\n")
    e = _engine()
    try:
        e.register_replica("cu", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS, 300.0, 3), masses=MASS))
        assert e.strain_batch([mk(both)])[0].stress_updated == 1
        assert e.eam_compute("cu", 1)["npairs"] > 0
        rk.assert_not_attached(ADP, e, "cu")
    finally:
        e.close()
    # malformed lines, and a line that names a file the folder lacks: the reader's message
    rk.assert_malformed_pair_coeff_lines(ADP, rk.Setup("cu", CUAG, None, MASS, (x, box, t)), tmp_path, ".adp", "Cu", missing_file=True)
