"""The ionic force stage on the GPU (md_born_dsf.hip, engine_rowpot.cpp: `pair_style born/coul/dsf`) against the independent FP64 numpy
restatement tests/born_dsf_numpy.py, which tests/test_born_dsf_host.py pins on the CPU (no LAMMPS exists to compare with): static parity
on the smallest shapes at which a path changes, bitwise repeatability, dynamics, the virial -> pressure conversion, whole evaluations,
batches over two materials, rows through cells, refusals, replaced attachments, self-configuration from the scripts folder.

Budgets, those of tests/test_gpu_tersoff.py: static parity 1e-10 of the largest force component, energy term and virial component; NVE
after 20 steps 1e-9 A and 1e-11 A/fs, the sampled pressure 1e-10; whole evaluations 1e-10 (an update against its two runs) and 1e-9 (a
batch against each simulation alone).  The perfect cell has no force by symmetry, so its forces are measured on the scale of its
jittered twin.

Energy drift.  No row stage holds a drift bound to borrow, so the bound is the reference's own, as in tests/test_gpu_meam_spline.py:
after 200 NVE steps the total energy on the device may have moved from its start by no more than the numpy velocity-Verlet integrator's
own drift on the same input plus the static energy budget (1e-10 of the largest energy term).

What the groups catch.  One ion: the self term, a row of no entries.  Dimers: the sign of q_i q_j, a charge of zero, the strict tests at
cut_coul and cut_lj.  The 8-ion cells: the image search two boxes deep, an ion's own images.  63 ions: a short last group, a cell that
is not neutral.  KNaCl: a swapped type index, per-pair Born cutoffs below cut_coul.  The gas: rows from none to many entries, the
regrowth of the row capacity.
"""
import math
import os

import numpy as np
import pytest

import born_dsf_numpy as bn
import rowkit as rk
from scema_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_dsf")
KNACL = os.path.join(ROOT, "tests", "golden", "KNaCl.born_dsf")
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")
MASS2, MASS3 = (bn.NA_MASS, bn.CL_MASS), (bn.NA_MASS, bn.CL_MASS, bn.K_MASS)
RLIST = 10.0 + 1.0


@pytest.fixture(scope="module")
def ref_nacl():
    return bn.BornDsf(bn.read_born_dsf(NACL))


@pytest.fixture(scope="module")
def ref_knacl():
    return bn.BornDsf(bn.read_born_dsf(KNACL))


BORN_DSF = rk.Pot("born/dsf", "born_dsf_configure", "born_dsf_compute", "Born/DSF", ("e_born", "e_coul"), ("npairs", "ncoul"),
                  counts="ordered pairs {npairs}, inside cut_coul {ncoul}", ionic=True)


_engine = rk.engine
_static = rk.static_of(BORN_DSF, NACL, None, MASS2)


def no_pairs(got, ref, scale, what):
    """no pair: the self energy alone, every force and the virial exactly zero"""
    if ref["npairs"] != 0:
        return False
    es = max(abs(scale["e_born"]), abs(scale["e_coul"]))
    de = max(abs(got["e_born"] - ref["e_born"]), abs(got["e_coul"] - ref["e_coul"]))
    assert not ref["f"].any() and not ref["w"].any() and ref["e_born"] == 0.0
    assert got["e_born"] == 0.0 and (got["f"] == 0.0).all() and (got["w"] == 0.0).all()
    print(f"{what}: no pairs, forces and virial exactly zero, self energy err {de / max(es, 1e-300):.2e}, rows {got['maxrow']}/{got['rowcap']}")
    assert de <= 1e-10 * es
    return True


_check_static = rk.checker(BORN_DSF, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)


# ---- one ion, dimers ----
def test_one_ion_has_its_self_energy_alone(ref_nacl):
    case = bn.case_single()
    ref = ref_nacl.compute(*case)
    assert ref["npairs"] == 0 and ref["e_coul"] == ref["e_self"] < 0.0
    got = _static(*case)
    assert got["e_coul"] < 0.0
    _check_static(got, ref, "born/dsf one ion")


@pytest.mark.parametrize("name,ti,tj,qi,qj", [("+/-", 0, 1, 1.0, -1.0), ("+/+", 0, 0, 1.0, 1.0), ("ion next to an uncharged atom", 0, 1, 1.0, 0.0)])
def test_dimers(ref_nacl, name, ti, tj, qi, qj):
    for r in (2.4, 6.0):
        case = bn.case_dimer(ti, tj, qi, qj, r)
        ref = ref_nacl.compute(*case)
        assert ref["npairs"] == 2
        got = _static(*case)
        _check_static(got, ref, f"born/dsf dimer {name} at {r}")
        if qj == 0.0:      # Coulomb exactly zero: Born alone, and the one self energy
            assert not ref["w_coul"].any() and ref["e_coul"] == ref["e_self"]
            born = ref_nacl.born(ti, tj, np.array([r]))
            assert abs(got["f"][0, 0] - born[1][0]) <= 1e-10 * abs(born[1][0])
        else:
            assert (ref["e_coul"] - ref["e_self"] < 0.0) == (qi * qj < 0.0)


def test_dimers_at_cut_coul(ref_nacl):
    """cut_coul = cut_lj = cutmax = 10 A in this file: finite just inside, no pair from the cutoff on (the self energies remain)"""
    rc = ref_nacl.rc
    for r, n in ((rc - 1e-6, 2), (rc, 0), (rc + 1e-6, 0)):
        case = bn.case_dimer(0, 1, 1.0, -1.0, r)
        assert case[0][1, 0] - case[0][0, 0] == r
        ref = ref_nacl.compute(*case)
        assert ref["npairs"] == n and ref["ncoul"] == n
        _check_static(_static(*case), ref, f"born/dsf dimer at cut_coul {r - rc:+.0e}")


def test_dimers_at_cut_lj(ref_knacl):
    """the pair 1-1 of KNaCl: cut_lj 7 A below cut_coul 10 A; just inside the unshifted Born term is finite, from 7 A on exactly zero while
    the pair is still counted and its Coulomb term runs on"""
    cut = ref_knacl.p["cut_lj"][0, 0]
    assert cut == 7.0
    for r in (cut - 1e-6, cut, cut + 1e-6):
        case = bn.case_dimer(0, 0, 1.0, 1.0, r)
        ref = ref_knacl.compute(*case)
        assert ref["npairs"] == 2 and ref["ncoul"] == 2 and (ref["e_born"] != 0.0) == (r < cut)
        got = _static(*case, path=KNACL, masses=MASS3)
        _check_static(got, ref, f"born/dsf dimer at cut_lj {r - cut:+.0e}")
        assert (got["e_born"] != 0.0) == (r < cut)


def test_a_born_cutoff_beyond_cut_coul(tmp_path):
    """a fragment whose cut_lj (12 A) lies beyond cut_coul (9 A), so that cutmax is a Born cutoff: a dimer between the two is counted
    inside cutmax but not inside cut_coul, with the Born term alone; a lattice has pairs of both kinds"""
    p = tmp_path / "long_born.born_dsf"
    p.write_text(open(NACL).read().replace("born/coul/dsf 0.25 10.0", "born/coul/dsf 0.25 12.0 9.0"))
    ref_bd = bn.BornDsf(bn.read_born_dsf(str(p)))
    assert ref_bd.cutmax == 12.0 and ref_bd.rc == 9.0
    case = bn.case_dimer(0, 1, 1.0, -1.0, 10.5)
    ref = ref_bd.compute(*case)
    assert (ref["npairs"], ref["ncoul"]) == (2, 0) and ref["e_born"] != 0.0 and ref["e_coul"] == ref["e_self"]
    _check_static(_static(*case, path=str(p)), ref, "born/dsf dimer between cut_coul and cut_lj")
    case = bn.case_jitter(2, 3)
    ref = ref_bd.compute(*case)
    assert 0 < ref["ncoul"] < ref["npairs"]
    _check_static(_static(*case, path=str(p)), ref, "born/dsf 64 ions, cut_lj beyond cut_coul")


# ---- lattices ----
@pytest.mark.parametrize("a", [5.64, 5.51])
def test_the_eight_ion_cell(ref_nacl, a):
    """the list radius is 11 A, so the image search is two boxes deep (5.51 A: barely wider than half of it, the narrowest it takes) and an
    ion meets its own images; perfect (measured on the scale of its jittered twin) and jittered"""
    case, twin = bn.case_cell8(a), bn.case_cell8(a, jitter=0.05)
    assert RLIST / 2.0 < a < RLIST
    ref, reft = ref_nacl.compute(*case), ref_nacl.compute(*twin)
    assert ref["maxrow"] > 150
    _check_static(_static(*case), ref, f"born/dsf 8-ion cell at {a}", scale=reft)
    _check_static(_static(*twin), reft, f"born/dsf 8-ion cell at {a}, jittered")


def test_a_cell_narrower_than_half_the_list_radius_is_refused():
    with pytest.raises(capi.EngineError, match=r"rc=4: .*box width 5\.490 < \(cutoff\+skin\)/2 = 5\.500"):
        _static(*bn.case_cell8(5.49))


def test_triclinic_box_with_ions_outside(ref_nacl):
    x, box, t, q = bn.case_triclinic()
    s = (x - box[:3]) @ np.linalg.inv(bn.h_matrix(box))
    assert len(x) == 64 and ((s < 0.0) | (s >= 1.0)).any(axis=1).sum() > 5 and box[6] != 0.0 and box[7] != 0.0 and box[8] != 0.0
    _check_static(_static(x, box, t, q), ref_nacl.compute(x, box, t, q), "born/dsf triclinic")


@pytest.mark.parametrize("ncell", [2, 3])
def test_jittered_lattices(ref_nacl, ncell):
    case = bn.case_jitter(ncell, ncell)
    assert len(case[0]) == 8 * ncell ** 3
    _check_static(_static(*case), ref_nacl.compute(*case), f"born/dsf {len(case[0])} jittered ions")


def test_63_ions_of_a_cell_that_is_not_neutral(ref_nacl):
    case = bn.case_63()
    assert len(case[0]) == 63 and case[3].sum() == 1.0
    _check_static(_static(*case), ref_nacl.compute(*case), "born/dsf 63 ions, net charge +1")


def test_a_ragged_gas(ref_nacl):
    case = bn.case_gas()
    ref = ref_nacl.compute(*case)
    I = ref_nacl.ordered_pairs(case[0], case[1])[0]
    cnt = np.bincount(I, minlength=len(case[0]))
    assert cnt.min() <= 3 and cnt.max() >= 12
    _check_static(_static(*case), ref, f"born/dsf gas, rows of {cnt.min()} to {cnt.max()} entries inside cutmax")


def test_rows_that_overflow_their_first_capacity(ref_nacl):
    """60 ions in a 40 A box, a third of them in one corner: the first capacity follows the mean density (8 entries), the crowded rows
    need several times that, so the evaluation regrows them and repeats"""
    case = bn.case_gas(n=60, seed=9, L=40.0)
    rho = 60 / 40.0 ** 3
    first = max(8, (int(math.ceil(rho * 4.0 / 3.0 * math.pi * RLIST ** 3 * 1.5)) + 7) // 8 * 8)
    got = _static(*case)
    assert got["maxrow"] > first and got["rowcap"] > first, (got["maxrow"], got["rowcap"], first)
    _check_static(got, ref_nacl.compute(*case), f"born/dsf regrown rows (first capacity {first})")


@pytest.mark.parametrize("order", ["Na Cl K", "K Cl Na"])
def test_three_types_in_both_orders(ref_knacl, order, tmp_path):
    """KNaCl as written, and with the first and the third type swapped in the replica and in a rewritten fragment: the same crystal"""
    x, box, t, q = bn.case_knacl()
    ref = ref_knacl.compute(x, box, t, q)
    assert set(t) == {0, 1, 2} and ref["ncoul"] <= ref["npairs"]
    if order == "Na Cl K":
        _check_static(_static(x, box, t, q, path=KNACL, masses=MASS3), ref, "born/dsf KNaCl")
        return
    swap = {"1": "3", "3": "1", "2": "2", "*": "*"}
    lines = []
    for raw in open(KNACL):
        w = raw.split("#")[0].split()
        if w and w[0] == "pair_coeff":
            i, j = swap[w[1]], swap[w[2]]
            if "*" not in (i, j) and int(i) > int(j):
                i, j = j, i
            lines.append(" ".join(["pair_coeff", i, j] + w[3:]) + "\n")
        else:
            lines.append(raw)
    p = tmp_path / "swapped.born_dsf"
    p.write_text("".join(lines))
    got = _static(x, box, 2 - t, q, path=str(p), masses=MASS3[::-1])
    _check_static(got, ref, "born/dsf KNaCl, types 1 and 3 swapped")


def test_two_evaluations_of_one_state_agree_bit_for_bit():
    case = bn.case_jitter(3, 7)
    e = _engine()
    try:
        e.born_dsf_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(case[2], case[3], case[0], case[1], MASS2))
        a, b = e.born_dsf_compute("m", 1), e.born_dsf_compute("m", 1)
    finally:
        e.close()
    c = _static(*case)
    assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]) and np.array_equal(a["f"], c["f"])


# ---- dynamics ----
def test_nve_dynamics_and_sampled_pressure(ref_nacl):
    x, box, t, q = bn.case_jitter(2, 6)
    v = rk.velocities(t, MASS2, 300.0, 1)
    e = _engine()
    try:
        e.born_dsf_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        e.debug_run("nacl", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "nacl", 1)
        xr, vr = ref_nacl.nve(x, v, box, t, q, MASS2, 1.0, 20)
        dx = np.abs(bn.minimage_diff(xg, xr, box)).max()
        print(f"born/dsf nve 20 steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        # the virial -> pressure conversion on a strained cell: one step with sampling gives (sum m v v + W) / V of the state after it, in atm
        xs, bs = bn.strained(x, box, np.array([[0.01, 0.004, 0.0], [0.0, -0.006, 0.003], [0.0, 0.0, 0.008]]))
        e.set_state(1, "nacl", 1, bs, xs, v)
        p = e.debug_run("nacl", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref_nacl.nve(xs, v, bs, t, q, MASS2, 1.0, 1)
        want = ref_nacl.pressure_atm(x1, v1, bs, t, q, MASS2)
        print(f"born/dsf sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


def test_energy_drift_over_200_steps(ref_nacl):
    """total energy after 200 NVE steps of the jittered 8-ion cell: no further from its start than the numpy integrator's own drift plus
    the static energy budget"""
    x, box, t, q = bn.case_cell8(jitter=0.05)
    v = rk.velocities(t, MASS2, 300.0, 5)
    m = np.asarray(MASS2)[t]
    total = lambda c, vel: c["e_born"] + c["e_coul"] + 0.5 * bn.MVV2E * np.sum(m[:, None] * vel * vel)
    ref0 = ref_nacl.compute(x, box, t, q)
    xr, vr = ref_nacl.nve(x, v, box, t, q, MASS2, 1.0, 200)
    drift_ref = abs(total(ref_nacl.compute(xr, box, t, q), vr) - total(ref0, v))
    e = _engine()
    try:
        e.born_dsf_configure("nacl", NACL)
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2, v=v))
        e.set_state(0, "nacl", 1, box, x, v)
        e0 = total(e.born_dsf_compute("nacl", 1, qp=0), v)
        e.debug_run("nacl", 1, 200, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, _, vg = e.get_state(0, "nacl", 1)
        drift = abs(total(e.born_dsf_compute("nacl", 1, qp=0), vg) - e0)
        es = max(abs(ref0["e_born"]), abs(ref0["e_coul"]))
        print(f"born/dsf energy drift over 200 steps: device {drift:.3e}, numpy integrator {drift_ref:.3e} kcal/mol of {es:.1f}")
        assert drift <= drift_ref + 1e-10 * es
    finally:
        e.close()


# ---- whole evaluations ----
def test_strain_batch_equals_the_two_runs_and_a_second_update_continues():
    """an update against the straining run and the sampling run issued through the parity hooks; then a second update from the stored
    states: qp 0 continues from its own, qp 1 branches from qp 0's"""
    x, box, t, q = bn.case_jitter(2, 8)
    L = box[3:6] - box[:3]
    s1 = np.array([2.0e-3 * L[0], -5e-4 * L[1], -5e-4 * L[2], 8e-4 * L[2], 0.0, 0.0])
    s2 = np.array([1.0e-3 * L[0], 0.0, 1.0e-3 * L[2], 0.0, 0.0, 0.0])
    s = rk.Setup("nacl", NACL, None, MASS2, (x, box, t, q), rk.velocities(t, MASS2, 300.0, 2))
    rk.strain_batch_and_a_second_update(BORN_DSF, s, s1, s2, tol=1e-10)


@pytest.fixture(scope="module")
def nine():
    """9 simulations (two part streams) over sodium chloride under NaCl.born_dsf and the three-type crystal under KNaCl.born_dsf, and
    each one's stress alone in a fresh engine"""
    mats = {"nacl": (bn.case_jitter(2, 6), NACL, None, MASS2), "knacl": (bn.case_knacl(), KNACL, None, MASS3)}
    return rk.batch_vs_alone_fixture(BORN_DSF, mats, 9, 21)


@pytest.mark.parametrize("split", [0, 1])
def test_batch_of_nine_over_two_materials_equals_each_alone(nine, split):
    """whole (split 0) and as part batches on two streams (split 1)"""
    rk.assert_batch_vs_alone(BORN_DSF, nine, split, what="born/dsf batch of 9 over two materials", tol=1e-9)


def test_a_replaced_attachment_rebuilds_the_rows(ref_nacl, ref_knacl):
    """a material holds one attachment: KNaCl.born_dsf configured over NaCl.born_dsf (another alpha, other Born cutoffs) gives the forces
    of a fresh engine, not those of kept rows; an EAM attachment over it and back likewise"""
    x, box, t, q = bn.case_jitter(2, 4)
    e = _engine()
    try:
        e.born_dsf_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS2))
        _check_static(e.born_dsf_compute("m", 1), ref_nacl.compute(x, box, t, q), "born/dsf before the replacement")
        e.born_dsf_configure("m", KNACL)
        _check_static(e.born_dsf_compute("m", 1), ref_knacl.compute(x, box, t, q), "born/dsf after the replacement")
        e.eam_configure("m", CUAG, ("Cu", "Ag"))
        rk.assert_not_attached(BORN_DSF, e, "m")
        assert e.eam_compute("m", 1)["npairs"] > 0
        e.born_dsf_configure("m", NACL)
        with pytest.raises(capi.EngineError, match="no EAM potential"):
            e.eam_compute("m", 1)
        _check_static(e.born_dsf_compute("m", 1), ref_nacl.compute(x, box, t, q), "born/dsf over an EAM attachment")
    finally:
        e.close()


def _real_units_copy(path):
    """the fixture with its energies converted to kcal/mol by hand, under `units real`"""
    lines = []
    for raw in open(path):
        w = raw.split("#")[0].split()
        if w and w[0] == "units":
            lines.append("units real\n")
        elif w and w[0] == "pair_coeff":
            v = [float(s) for s in w[3:]]
            for k in (0, 3, 4):
                v[k] *= bn.EV_TO_KCALMOL
            lines.append(" ".join(w[:3] + [repr(s) for s in v]) + "\n")
        else:
            lines.append(raw)
    return "".join(lines)


@pytest.mark.parametrize("units", ["metal", "real"])
def test_self_configuration_from_the_scripts_folder(units, tmp_path):
    """`pair_style born/coul/dsf` in in.strain.lammps configures a topology-free replica with charges whose material has nothing attached,
    from the script's own lines: the update equals the configured one to the batch budget, and the material then computes.  With `units
    real` the numbers are taken as kcal/mol."""
    scripts = tmp_path / "lammps_scripts_nacl"
    scripts.mkdir()
    frag = open(NACL).read() if units == "metal" else _real_units_copy(NACL)
    (scripts / "in.strain.lammps").write_text("# straining run\nread_restart ${loco}/init.restart\n" + frag + "fix 1 all nvt temp 300 300 100\nrun 100\n")
    ref = bn.BornDsf(bn.read_born_dsf(str(scripts / "in.strain.lammps")))
    assert ref.p["unit"] == (1 if units == "real" else 0)
    x, box, t, q = bn.case_jitter(2, 9)
    v = rk.velocities(t, MASS2, 300.0, 3)
    L = box[3:6] - box[:3]
    mk = lambda folder: capi.make_sim(0, "nacl", 1, np.array([1e-3 * L[0], 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls",
                                      scripts_folder=str(folder))
    outs = []
    for configure in (False, True):
        e = _engine()
        try:
            if configure:
                e.born_dsf_configure("nacl", str(scripts / "in.strain.lammps"), energy_unit=ref.p["unit"])
            e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2, v=v))
            if not configure:
                rk.assert_not_attached(BORN_DSF, e, "nacl")
            o = e.strain_batch([mk(scripts)])[0]
            assert o.stress_updated == 1
            outs.append(np.array(o.stress[:]))
            _check_static(e.born_dsf_compute("nacl", 1), ref.compute(x, box, t, q), f"born/dsf {'configured' if configure else 'self-configured'}, units {units}")
        finally:
            e.close()
    assert np.isfinite(outs[0]).all() and np.abs(outs[0] - outs[1]).max() <= 1e-9 * np.abs(outs[1]).max()


def test_self_configuration_refuses_lines_the_reader_refuses(tmp_path):
    bad = tmp_path / "bad"
    bad.mkdir()
    (bad / "in.strain.lammps").write_text("pair_style born/coul/dsf 0.25 10.0\npair_coeff 1 1 0.2637 0.317 2.340 1.05 -0.499\npair_coeff 2 2 0.1582 0.317 3.170 72.40 -145.427\n")
    x, box, t, q = bn.case_jitter(2, 9)
    e = _engine()
    try:
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2))
        sim = capi.make_sim(0, "nacl", 1, np.array([1e-3 * (box[3] - box[0]), 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, scripts_folder=str(bad))
        with pytest.raises(capi.EngineError, match=r"rc=1: .*in\.strain\.lammps line 1: no pair_coeff line sets the pair 1 2"):
            e.strain_batch([sim])
    finally:
        e.close()


def test_a_charged_replica_whose_script_lacks_the_line_is_not_attached(tmp_path):
    """a topology-free replica with charges and a script of another style: no row potential is attached, whatever the update then does
    with the replica (the molecular path takes it, or refuses its box)"""
    scripts = tmp_path / "other"
    scripts.mkdir()
    (scripts / "in.strain.lammps").write_text("pair_style lj/cut/coul/long 12.0 9.0\nkspace_style pppm 1e-4\n")
    x, box, t, q = bn.case_jitter(2, 9)
    e = _engine()
    try:
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2))
        sim = capi.make_sim(0, "nacl", 1, np.array([1e-3 * (box[3] - box[0]), 0, 0, 0, 0, 0]), nss=10, dt=1.0, most_recent=capi.QP_NONE, scripts_folder=str(scripts))
        try:
            e.strain_batch([sim])
        except capi.EngineError as err:
            assert "born" not in str(err).lower() and "Born" not in str(err)
        with pytest.raises(capi.EngineError, match=r"no Born/DSF potential attached to material nacl \(scema_md_born_dsf_configure\)"):
            e.born_dsf_compute("nacl", 1)
        for name in ("eam_compute", "sw_compute", "vashishta_compute"):
            with pytest.raises(capi.EngineError, match="potential attached to material nacl"):
                getattr(e, name)("nacl", 1)
    finally:
        e.close()


def _cells_static(monkeypatch, cells, case):
    monkeypatch.setenv("SCEMA_MD_ROW_CELLS", str(cells))     # (the engine has no parameter for it: the switch is read when the engine is made)
    x, box, t, q = case
    e = _engine()
    try:
        e.born_dsf_configure("m", NACL)
        e.register_replica("m", 1, capi.ionic_system(t, q, x, box, MASS2))
        out = e.born_dsf_compute("m", 1)
        out["rows"], out["prof"] = e.debug_rows(0), e.profile()
        return out
    finally:
        e.close()


def test_cell_binned_row_build(monkeypatch):
    """SCEMA_MD_ROW_CELLS=1 on 1 728 ions in a box of 33.84 A (three cells of the list radius 11 A per dimension): rows entry for entry
    those of the N^2 build, forces, energies and virial equal to its result within the static budgets"""
    case = bn.case_jitter(6, 9)
    assert len(case[0]) == 1728
    on, off = _cells_static(monkeypatch, 1, case), _cells_static(monkeypatch, 0, case)
    a, b = on["rows"], off["rows"]
    assert (a["cells"], b["cells"]) == (1, 0) and min(a["ncell"]) >= 3 and a["cap"] == b["cap"]
    assert np.array_equal(a["cnt"], b["cnt"])
    live = np.arange(a["cap"])[None, :] < a["cnt"][:, None]
    assert np.array_equal(a["rows"][live], b["rows"][live]) and a["cnt"].sum() > 0
    assert on["prof"]["row_cell_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0
    assert off["npairs"] > 1728 * 150 and np.abs(off["f"]).max() > 0.0
    _check_static(on, off, "born/dsf 1 728 ions, rows through cells against N^2 rows")
    assert np.array_equal(on["f"], off["f"])      # (the same rows in the same order: the same sums)


# ---- refusals ----
def test_refusals():
    x, box, t, q = bn.case_jitter(2, 4)
    e = _engine()
    try:
        e.register_replica("nacl", 1, capi.ionic_system(t, q, x, box, MASS2))
        with pytest.raises(capi.EngineError, match=r"no Born/DSF potential attached to material nacl \(scema_md_born_dsf_configure\)"):
            e.born_dsf_compute("nacl", 1)
        with pytest.raises(capi.EngineError, match=r"rc=5: .*nowhere\.born_dsf: cannot open"):
            e.born_dsf_configure("nacl", os.path.join(ROOT, "tests", "golden", "nowhere.born_dsf"))
        with pytest.raises(capi.EngineError, match=r"rc=5: .*NaCl\.born_dsf line 4: units metal contradicts energy unit 1"):
            e.born_dsf_configure("nacl", NACL, energy_unit=1)
        # an update mixing this kind with another
        e.born_dsf_configure("nacl", NACL)
        e.eam_configure("cu", CUAG, ("Cu",))
        e.register_replica("cu", 1, capi.bare_system(np.zeros(len(x), np.int32), x, box, masses=(63.546,)))
        mk = lambda k, m: capi.make_sim(k, m, 1, np.array([1e-3 * (box[3] - box[0]), 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, most_recent=capi.QP_NONE)
        for sims in ([mk(0, "nacl"), mk(1, "cu")], [mk(1, "cu"), mk(0, "nacl")]):
            with pytest.raises(capi.EngineError, match="rc=1: .*mixes EAM materials"):
                e.strain_batch(sims)
            assert not e.has_state(0, "nacl", 1) and not e.has_state(1, "cu", 1)
        assert e.strain_batch([mk(0, "nacl")])[0].stress_updated == 1
        # an atom type beyond the fragment's
        t2 = t.copy()
        t2[5] = 2
        e.register_replica("nacl", 2, capi.ionic_system(t2, q, x, box, MASS3))
        with pytest.raises(capi.EngineError, match=r"atom 5 has type 3 but the Born/DSF element list names 2 types"):
            e.born_dsf_compute("nacl", 2)
    finally:
        e.close()
