"""The EDIP force stage on the GPU (md_edip.hip, engine_rowpot.cpp) against the independent FP64 numpy restatement tests/edip_numpy.py, which
tests/test_edip_host.py pins on the CPU (no LAMMPS exists to compare with): static parity on the smallest shapes at which the kernel takes
another path, dynamics, the virial -> pressure conversion, elastic constants, whole evaluations, batches over two materials, refusals,
replaced attachments, self-configuration from the scripts folder.

Budgets, the standing ones: static parity 1e-10 of the largest force component, 1e-9 of the largest energy term and virial
component (FP64 sums of a few hundred terms in another order); NVE after 20 steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; whole
evaluations and a batch against each simulation alone 1e-9 relative (the partner forces go through atomics).  The perfect 8-atom cell
sits at the potential's own minimum, so its forces and virial are measured on the scale of its jittered twin.

"Coordination" inputs.  A perfect or lightly jittered diamond cell has every neighbour inside c and none between c and a: f' = 0 and the
third pass of the kernel, the coordination force, does nothing.  Every input called a coordination input here -- simple-cubic silicon
at 2.8 A with 0.1 A Gaussian jitter, six neighbours at f ~ 0.77 -- has at least half of its ordered pairs in (c, a); `_soft` asserts it on
the numpy reference before anything is compared.

"Bit for bit".  Forces on partners are summed by atomic adds (LDS, then global memory), and atomics of different waves arrive in no fixed
order: the forces of two evaluations of the same rows agree to the last bit only where one wave does all the adding.  A wave holds the
groups of four central atoms, so the inputs compared bit for bit have four atoms (`case_cell4`: a periodic cell whose row entries are all
images, `case_tetramer`); the same properties are then held to the static budget on inputs of 64 and 125 atoms.

What the groups catch.  Dimers and the trimer: the strict tests at c and a, f' next to a.  Atom counts: a short last tile, a second
tile, the force table past the LDS limit.  Clusters: the ballot rank across a trip of 16, the limit of 32.  Element orders and the
synthetic file: a swapped [i][j][k] index, pair numbers from the wrong end.  Dynamics and pressure: the sign of the coordination part in
the virial.  Whole evaluations: rows kept or rebuilt under the wrong material, part streams.
"""
import os
import shutil

import numpy as np
import pytest

import edip_numpy as en
import rowkit as rk
import sw_numpy as swn
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI = os.path.join(ROOT, "tests", "golden", "Si.edip")
SIC = os.path.join(ROOT, "tests", "golden", "SiC.edip")
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")
EL1, MASS1 = ("Si",), (en.SI_MASS,)
EL2, MASS2 = ("Si", "C"), (en.SI_MASS, en.C_MASS)
RLIST = en.SI_A + 1.0


@pytest.fixture(scope="module")
def ref_si():
    return en.Edip(en.read_edip(SI, list(EL1))[0])


@pytest.fixture(scope="module")
def ref_sic():
    return en.Edip(en.read_edip(SIC, list(EL2))[0])


EDIP = rk.Pot("edip", "edip_configure", "edip_compute", "EDIP", ("e2", "e3"), ("npairs", "ntriplets"),
              counts="ordered pairs {npairs} ({ref[soft]} in (c, a)), triplets {ntriplets}")


_engine = rk.engine
_static = rk.static_of(EDIP, SI, EL1, MASS1)


def _soft(ref):
    """the condition of a coordination input, on the reference alone"""
    assert 2 * ref["soft"] >= ref["npairs"] > 0, (ref["soft"], ref["npairs"])


def no_pairs(got, ref, scale, what):
    """no term at all (or all of them underflow to zero): exactly zero, and no scale to divide by"""
    if ref["npairs"] != 0 and np.abs(scale["f"]).max() > 0.0:
        return False
    rk.all_exactly_zero(got, ref, EDIP, what, head=f"{ref['npairs']} ordered pairs")
    return True


_check_static = rk.checker(EDIP, tol_f=1e-10, tol_e=1e-9, tol_w=1e-9, no_pairs=no_pairs)


def test_dimers(ref_si):
    """inside c, between c and a, 1e-6 A inside a (every exponential underflows: exactly zero, but counted), and exactly at a and beyond,
    where the pair is not counted"""
    for r in (2.4, 2.9, en.SI_A - 1e-6, en.SI_A, en.SI_A + 1e-9):
        x, box, t = en.case_dimer(r)
        assert x[1, 0] - x[0, 0] == r
        got, ref = _static(x, box, t), ref_si.compute(x, box, t)
        assert ref["npairs"] == (2 if r < en.SI_A else 0) and ref["ntriplets"] == 0
        assert ref["soft"] == (2 if en.SI_C < r < en.SI_A else 0)
        _check_static(got, ref, f"edip dimer at {r}")


def test_trimer_and_tetramer(ref_si):
    for what, (x, box, t) in (("trimer", en.case_trimer()), ("tetramer", en.case_tetramer())):
        ref = ref_si.compute(x, box, t)
        assert ref["ntriplets"] >= 1 and ref["soft"] >= 2 and ref["e3"] > 0.0
        _check_static(_static(x, box, t), ref, f"edip {what}")


def test_the_eight_atom_cell(ref_si):
    """the diamond cell of 5.43 A is narrower than two list radii: the rows come from the image search.  Z = 4, no pair in (c, a): the
    coordination pass runs over nothing here"""
    x, box, t = en.case_diamond(1)
    ref = ref_si.compute(x, box, t)
    xj, _, _ = en.case_diamond_jitter(1, 4, 0.02)
    refj = ref_si.compute(xj, box, t)
    for r in (ref, refj):
        assert (r["maxin"], r["npairs"], r["ntriplets"], r["soft"]) == (4, 8 * 4, 8 * 6, 0)
    assert box[3] < 2.0 * RLIST
    got = _static(x, box, t)
    _check_static(got, ref, "edip 8-atom cell", scale=refj)
    assert abs(got["e2"] / 8.0 / en.EV_TO_KCALMOL - (-4.649953)) < 1e-6
    _check_static(_static(xj, box, t), refj, "edip 8-atom cell, jittered")


@pytest.mark.parametrize("n", [27, 63, 64, 65])
def test_coordination_inputs(ref_si, n):
    """27: a box of 8.4 A, barely two list radii (8.24 A) wide; 63, 64, 65: a short only tile, a full one, a second tile of one atom"""
    x, box, t = en.case_coordination(n)
    assert len(x) == n
    ref = ref_si.compute(x, box, t)
    _soft(ref)
    _check_static(_static(x, box, t), ref, f"edip coordination input, n = {n}")


def test_a_block_past_the_lds_force_table(ref_si):
    """1 025 atoms of jittered diamond with vacancies: the instance that adds to global memory directly"""
    x, box, t = en.case_block(1025)
    assert len(x) == 1025
    _check_static(_static(x, box, t), ref_si.compute(x, box, t), "edip 1 025 atoms")


def test_a_strongly_jittered_diamond_cell(ref_si):
    """64 diamond atoms with 0.35 A jitter: neighbours on both sides of c, second neighbours inside a"""
    x, box, t = en.case_diamond_jitter(2, 1, 0.35)
    ref = ref_si.compute(x, box, t)
    assert 0 < ref["soft"] < ref["npairs"] and ref["maxin"] > 4
    _check_static(_static(x, box, t), ref, "edip diamond, 0.35 A jitter")


@pytest.mark.parametrize("m", [15, 16, 17, 32])
def test_list_lengths(ref_si, m):
    """an atom inside m atoms on a sphere of 2.9 A: the centre's list holds m entries (one trip of 16 short of one, full, one more, two
    trips to the last slot), all of them between c and a"""
    x, box, t = en.case_cluster(m)
    ref = ref_si.compute(x, box, t)
    assert ref["maxin"] == m and ref["soft"] >= 2 * m
    _check_static(_static(x, box, t), ref, f"edip cluster of {m}")


def test_more_than_32_inside_a_is_an_error(ref_si):
    x, box, t = en.case_cluster(33)
    assert ref_si.compute(x, box, t)["maxin"] == 33
    with pytest.raises(capi.EngineError, match=r"more than 32 neighbours inside a \(cutoffA\), the range of the EDIP potential"):
        _static(x, box, t)


def test_rows_regrown_after_an_overflow(ref_si, monkeypatch):
    """the row capacity forced low through the overflow hook: fault bit 1, and the retry recovers the forces of the unforced run -- bit
    for bit on the four-atom cell (more than the floor of 8 entries a row, all of them images; one wave does all the adding), within the static budget on 64 atoms"""
    x4, box4, t4 = en.case_cell4()
    x64, box64, t64 = en.case_coordination(64)
    ref4, ref64 = ref_si.compute(x4, box4, t4), ref_si.compute(x64, box64, t64)
    _soft(ref4)
    _soft(ref64)
    normal4, normal64 = _static(x4, box4, t4), _static(x64, box64, t64)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    got4, got64 = _static(x4, box4, t4), _static(x64, box64, t64)
    _check_static(got4, ref4, "edip four-atom cell after a row overflow")
    _check_static(got64, ref64, "edip 64 atoms after a row overflow")
    # (under the hook a row starts at the floor of 8 entries, fewer than either input's longest row: the first build overflows)
    print(f"edip overflow: four atoms rows {got4['maxrow']}/{got4['rowcap']} (unforced {normal4['rowcap']}), 64 atoms {got64['maxrow']}/{got64['rowcap']} (unforced {normal64['rowcap']})")
    assert normal4["maxrow"] > 8 and normal64["maxrow"] > 8 and got4["rowcap"] >= got4["maxrow"] == normal4["maxrow"]
    assert np.array_equal(got4["f"], normal4["f"]) and np.abs(got4["f"]).max() > 0.0
    assert got64["rowcap"] >= got64["maxrow"] == normal64["maxrow"]
    assert np.abs(got64["f"] - normal64["f"]).max() <= 1e-10 * np.abs(ref64["f"]).max()


def test_triclinic_box_with_atoms_outside(ref_si):
    x, box, t = en.case_triclinic()
    H = en.h_matrix(box)
    s = (x - box[:3]) @ np.linalg.inv(H)
    assert ((s < 0.0) | (s >= 1.0)).any(axis=1).sum() > 10 and box[6] != 0.0 and box[7] != 0.0 and box[8] != 0.0
    ref = ref_si.compute(x, box, t)
    _soft(ref)
    _check_static(_static(x, box, t), ref, "edip triclinic")


def test_static_parity_of_a_flipped_state(ref_si):
    """a 5 x 2 x 2 diamond cell written with xy = 2 a = 0.4 lx (a lattice translation: the same crystal), sheared by 0.12 lx so that it
    passes lx / 2 and flips; the forces on the state it leaves, in the box it leaves, against numpy"""
    x, box = en.diamond(5, 2, 2, en.A_SI)
    t = np.zeros(len(x), int)
    x = x + np.random.default_rng(5).normal(0.0, 0.05, x.shape)
    box[6] = 2.0 * en.A_SI
    lx, ly, lz = box[3:6] - box[:3]
    e = _engine()
    try:
        e.edip_configure("si", SI, EL1)
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS1, 300.0, 31), masses=MASS1))
        s = np.array([0.0, 0.0, 0.0, 0.12 * lx * lz / ly, 0.0, 0.0])
        e.strain_batch([capi.make_sim(0, "si", 1, s, nss=10, dt=1.0, temperature=300.0, strain_rate=3.4e-3, most_recent=capi.QP_NONE)])
        flips = e.profile()["box_flips"]
        b, xs, _ = e.get_state(0, "si", 1)
        print(f"edip flipped state: {flips} flip(s), xy {box[6]:.3f} -> {b[6]:.3f} A of lx {b[3] - b[0]:.3f} A")
        assert flips >= 1 and abs(b[6]) <= 0.5 * (b[3] - b[0]) and b[6] < 0.0
        _check_static(e.edip_compute("si", 1, qp=0), ref_si.compute(xs, b, t), "edip flipped state")
    finally:
        e.close()


@pytest.mark.parametrize("order", ["Si C", "C Si", "Si C Si"])
def test_synthetic_file_element_orders_and_a_many_to_one_type_map(ref_sic, order):
    """the two-element coordination input under both element orders of pair_coeff (the types swapped with them: the same crystal), and
    with three LAMMPS types of which the first and the third are silicon"""
    x, box, t = en.case_coordination(27, two_elements=True)
    ref = ref_sic.compute(x, box, t)
    _soft(ref)
    assert len(set(t)) == 2 and ref["e3"] > 0.0
    if order == "Si C":
        types, masses = t, MASS2
    elif order == "C Si":
        types, masses = 1 - t, MASS2[::-1]
    else:
        types, masses = np.where((t == 0) & (np.arange(len(t)) % 3 == 0), 2, t), (en.SI_MASS, en.C_MASS, en.SI_MASS)
        assert set(types) == {0, 1, 2}
    _check_static(_static(x, box, types, path=SIC, elements=tuple(order.split()), masses=masses), ref, f"edip synthetic file, elements {order}")


def _shear(h):
    e = np.zeros((3, 3))
    e[1, 2] = h
    return e


@pytest.fixture(scope="module")
def static_constants(ref_si):
    """C11, C12 and C44 (unrelaxed: homogeneous strain of every atom) of diamond silicon in GPa from second differences of the numpy energy
    under +-1e-3 strain of the perfect cell"""
    x, box, t = en.case_diamond(1)
    h, v = 1e-3, en.volume(box)
    E = lambda eps: ref_si.energy(*en.strained(x, box, eps), t)
    E0 = E(np.zeros((3, 3)))
    c11 = (E(np.diag([h, 0.0, 0.0])) - 2.0 * E0 + E(np.diag([-h, 0.0, 0.0]))) / h ** 2 / v
    c12 = (E(np.diag([h, h, 0.0])) - E(np.diag([h, -h, 0.0])) - E(np.diag([-h, h, 0.0])) + E(np.diag([-h, -h, 0.0]))) / (4.0 * h ** 2) / v
    c44 = (E(_shear(h)) - 2.0 * E0 + E(_shear(-h))) / h ** 2 / v
    return np.array([c11, c12, c44]) * en.KCALMOL_A3_TO_GPA


def test_elastic_constants(static_constants):
    """C11, C12 and C44 from the GPU virials at +-1e-3 strain, through set_state, against second differences of the numpy energy within
    0.1 % (both are finite differences with a relative truncation of order h^2 C''' / C ~ 1e-5)"""
    x, box, t = en.case_diamond(1)
    e = _engine()
    try:
        e.edip_configure("si", SI, EL1)
        e.register_replica("si", 1, capi.bare_system(t, x, box, masses=MASS1))
        h = 1e-3

        def stress(eps):
            xs, bs = en.strained(x, box, eps)
            e.set_state(5, "si", 1, bs, xs, np.zeros_like(xs))
            return -e.edip_compute("si", 1, qp=5)["w"] / en.volume(bs) * en.KCALMOL_A3_TO_GPA

        sp, sm = stress(np.diag([h, 0.0, 0.0])), stress(np.diag([-h, 0.0, 0.0]))
        c11, c12 = (sp[0] - sm[0]) / (2 * h), (sp[1] - sm[1]) / (2 * h)
        c44 = (stress(_shear(h))[5] - stress(_shear(-h))[5]) / (2 * h)
        got = np.array([c11, c12, c44])
        print(f"edip elastic constants on the device: C11 {c11:.3f}, C12 {c12:.3f}, C44 (unrelaxed) {c44:.3f} GPa; numpy energy: {static_constants}")
        assert abs(static_constants[0] / 172.04 - 1.0) < 1e-3
        assert (np.abs(got / static_constants - 1.0) < 1e-3).all()
    finally:
        e.close()


def test_nve_dynamics_and_sampled_pressure(ref_si):
    x, box, t = en.case_coordination(27)
    _soft(ref_si.compute(x, box, t))
    s = rk.Setup("si", SI, EL1, MASS1, (x, box, t), rk.velocities(t, MASS1, 300.0, 1))
    rk.nve_and_sampled_pressure(EDIP, ref_si, s, steps=20, tol_x=1e-9, tol_v=1e-11, tol_p=1e-10)


def test_strain_batch_equals_the_two_runs():
    """tension plus a shear component, nss = 10: the update against the straining run and the sampling run issued through the parity hooks"""
    x, box, t = en.case_coordination(64)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s = rk.Setup("si", SI, EL1, MASS1, (x, box, t), rk.velocities(t, MASS1, 300.0, 2))
    rk.strain_batch_vs_debug_runs(EDIP, s, s1, expect_nts=30, tol=1e-9)


@pytest.fixture(scope="module")
def eleven():
    """11 simulations over silicon and the synthetic two-element material, and each one's stress alone in a fresh engine"""
    mats = {"si": (en.case_coordination(27), SI, EL1, MASS1), "sic": (en.case_coordination(27, two_elements=True), SIC, EL2, MASS2)}
    return rk.batch_vs_alone_fixture(EDIP, mats, 11, 21)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_eleven_equals_each_alone(eleven, split):
    """whole (split 0) and as part batches on two streams (split 1)"""
    rk.assert_batch_vs_alone(EDIP, eleven, split, what="edip batch of 11 over two materials", tol=1e-9)


def _cells_static(monkeypatch, cells, case):
    monkeypatch.setenv("SCEMA_MD_ROW_CELLS", str(cells))
    x, box, t = case
    e = _engine()
    try:
        e.edip_configure("m", SI, EL1)
        e.register_replica("m", 1, capi.bare_system(t, x, box, masses=MASS1))
        out = e.edip_compute("m", 1)
        out["rows"], out["prof"] = e.debug_rows(0), e.profile()
        return out
    finally:
        e.close()


def test_cell_binned_row_build(ref_si, monkeypatch):
    """SCEMA_MD_ROW_CELLS=1 on boxes of 14 A (three cells of the list radius 4.12 A and more per dimension): rows entry for entry those of
    the N^2 build; forces bit for bit on the four-atom cluster, within the static budget on 125 atoms of the coordination lattice"""
    x, box = np.array(list(np.ndindex(5, 5, 5)), float) * 2.8, np.array([0.0, 0.0, 0.0, 14.0, 14.0, 14.0, 0.0, 0.0, 0.0])
    big = (x + np.random.default_rng(9).normal(0.0, 0.1, x.shape), box, np.zeros(125, int))
    for what, case, bits in (("tetramer", en.case_tetramer(14.0), True), ("125 atoms", big, False)):
        ref = ref_si.compute(*case)
        _soft(ref)
        on, off = _cells_static(monkeypatch, 1, case), _cells_static(monkeypatch, 0, case)
        a, b = on["rows"], off["rows"]
        assert (a["cells"], b["cells"]) == (1, 0) and min(a["ncell"]) >= 3 and a["cap"] == b["cap"]
        assert np.array_equal(a["cnt"], b["cnt"])
        live = np.arange(a["cap"])[None, :] < a["cnt"][:, None]
        assert np.array_equal(a["rows"][live], b["rows"][live]) and a["cnt"].sum() > 0
        assert on["prof"]["row_cell_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0
        _check_static(on, ref, f"edip {what}, rows through cells")
        _check_static(off, ref, f"edip {what}, N^2 rows")
        if bits:
            assert np.array_equal(on["f"], off["f"]) and np.abs(on["f"]).max() > 0.0
        else:
            assert np.abs(on["f"] - off["f"]).max() <= 1e-10 * np.abs(ref["f"]).max()


def test_self_configuration_from_the_scripts_folder(ref_si, tmp_path):
    """`pair_coeff * * ${locs}/Si.edip Si` in in.strain.lammps configures a bare replica whose material has nothing attached, bit for bit
    as the configured run; a malformed line of that kind is SCEMA_MD_ERR_ARG"""
    scripts = tmp_path / "lammps_scripts_edip"
    scripts.mkdir()
    shutil.copy(SI, scripts / "Si.edip")
    (scripts / "in.strain.lammps").write_text("# straining run\npair_style edip\n#pair_coeff * * ${locs}/other.edip C\n"
                                              "pair_coeff * * ${locs}/Si.edip Si   # the potential\nfix 1 all nvt temp 300 300 100\n")
    # (the four-atom cluster: one wave does all the adding, so two runs of the same configuration agree bit for bit)
    case = en.case_tetramer(12.0)
    tetramer = rk.Setup("si", SI, EL1, MASS1, case, rk.velocities(case[2], MASS1, 300.0, 4))
    a, sa = rk.dimer_update(EDIP, tetramer, scripts, False, 1.2e-2)
    b, sb = rk.dimer_update(EDIP, tetramer, scripts, True, 1.2e-2)
    assert np.isfinite(a).all() and np.abs(a).max() > 0.0
    assert np.array_equal(a, b) and all(np.array_equal(p, q) for p, q in zip(sa, sb))
    # the update configured the material: static forces of the 64-atom coordination input against the numpy helper
    x, box, t = en.case_coordination(64)
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "si", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    e = _engine()
    try:
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(t, MASS1, 300.0, 3), masses=MASS1))
        rk.assert_not_attached(EDIP, e, "si")
        assert e.strain_batch([mk(scripts)])[0].stress_updated == 1
        _check_static(e.edip_compute("si", 1), ref_si.compute(x, box, t), "edip self-configured")
    finally:
        e.close()
    rk.assert_malformed_pair_coeff_lines(EDIP, rk.Setup("si", SI, EL1, MASS1, (x, box, t)), tmp_path, ".edip", "Si", match_head="rc=1: .*")


def test_configuring_replaces_a_stillinger_weber_attachment_and_back(ref_si):
    """a material holds one attachment: EDIP configured over Stillinger-Weber replaces it (rows and element arrays are rebuilt: the forces
    are those of a fresh engine), and the other way round"""
    x, box, t = en.case_diamond_jitter(2, 1, 0.1)
    ref = ref_si.compute(x, box, t)
    e = _engine()
    try:
        e.sw_configure("si", SI_SW)
        e.register_replica("si", 1, capi.bare_system(t, x, box, masses=MASS1))
        sw0 = e.sw_compute("si", 1)
        e.edip_configure("si", SI, EL1)
        with pytest.raises(capi.EngineError, match="no Stillinger-Weber potential"):
            e.sw_compute("si", 1)
        _check_static(e.edip_compute("si", 1), ref, "edip over a Stillinger-Weber attachment")
        e.sw_configure("si", SI_SW)
        rk.assert_not_attached(EDIP, e, "si")
        sw1 = e.sw_compute("si", 1)
        assert sw1["npairs"] == sw0["npairs"] > 0 and np.abs(sw1["f"] - sw0["f"]).max() <= 1e-10 * np.abs(sw0["f"]).max()
    finally:
        e.close()


def test_an_update_mixed_with_stillinger_weber_is_refused():
    """EDIP + Stillinger-Weber in one update: SCEMA_MD_ERR_ARG before anything is planned, naming the earlier kind of the table; no state
    is left behind; each alone runs"""
    x, box, t = en.case_coordination(64)
    xs, boxs, ts = swn.case_a()
    e = _engine()
    try:
        e.edip_configure("ed", SI, EL1)
        e.sw_configure("sw", SI_SW)
        e.register_replica("ed", 1, capi.bare_system(t, x, box, masses=MASS1))
        e.register_replica("sw", 1, capi.bare_system(ts, xs, boxs))
        mk = lambda q, m, b: capi.make_sim(q, m, 1, np.array([1e-3 * (b[3] - b[0]), 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "ed", box), mk(1, "sw", boxs)], [mk(1, "sw", boxs), mk(0, "ed", box)]):
            with pytest.raises(capi.EngineError, match="rc=1: .*mixes Stillinger-Weber materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "ed", 1) and not e.has_state(1, "sw", 1)
        assert e.strain_batch([mk(0, "ed", box)])[0].stress_updated == 1
        assert e.strain_batch([mk(1, "sw", boxs)])[0].stress_updated == 1
        rk.assert_not_attached(EDIP, e, "sw")
    finally:
        e.close()
