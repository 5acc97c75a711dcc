"""The EDIP arithmetic of the product (scema_amd/csrc/edip/edip_core.h, the functions the HIP kernel of md_edip.hip runs, with the tables
of host/edip_params.cpp), compiled for the host as the stand-alone program tests/edip_host_driver.cpp and held against the independent
numpy restatement tests/edip_numpy.py: energies, forces and virial to 1e-12 relative; the numpy forces against central differences of the
numpy energy, its virial against the strain derivative, and the published figures of silicon.  No GPU needed: this is where every
derivative is pinned; the `-m gpu` tests then compare the kernel's output with the same helper.  No LAMMPS exists here to compare with:
parity with `pair_style edip` is unpinned (it interpolates grids; here the functions are evaluated in closed form).

Silicon: with the numbers of tests/golden/Si.edip the diamond lattice has -4.649953 eV per atom at 5.430 A, Z = 4, a three-body term of
zero (tau(4) = 1/3 to the digits of the published constants), its minimum between 5.42 and 5.44 A and C11 = 172.04 GPa; Justo et al.
(1998) give -4.650 eV, 5.430 A and 172 GPa.  A slip in the form or in a number of the fixture shows there.

"Coordination" inputs.  In a perfect or lightly jittered diamond cell every neighbour stands inside c (2.35 < 2.56 A) and none between c
and a: f' = 0 everywhere and the part of the force that is new with this potential, (dE_i/dZ_i) f'(r_im), is never computed.  Every input
called a coordination input below has at least half of its ordered pairs in (c, a); `test_coordination_inputs_are_soft` asserts it.

Wrong builds of the driver (-DEDH_WRONG=k, switches of the driver, not of the product), each with the case that fails; every one of them
still passes the diamond cell (build 3 to 1e-10, since tau(4) is 1/3 only to the digits of the published constants: the test says how
much that is), which is why that cell alone pins so little:
  1  the coordination force left out .................. coord27 (forces and virial; the energy is untouched)
  2  f = 1 inside a ................................... coord27
  3  tau = 1/3 at every Z ............................. coord27 (Z ~ 3.9 there)
  4  the pair sum over the pairs an atom owns, twice .. coord27 (V2(r_ij, Z_i) != V2(r_ji, Z_j) as soon as Z_i != Z_j)
  5  the triplet numbers of i j j for those of i j k .. the synthetic file
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import edip_numpy as en
import hostdrv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI = os.path.join(ROOT, "tests", "golden", "Si.edip")
SIC = os.path.join(ROOT, "tests", "golden", "SiC.edip")


def driver_exe(wrong=0):
    return hostdrv.build(f"edip_host_driver_{wrong}", ["tests/edip_host_driver.cpp", "scema_amd/csrc/host/edip_params.cpp"], shared=False,
                         defines=(f"EDH_WRONG={wrong}",))


def _run(exe, path, elements, x, box, types, energy_unit=0):
    text = f"{len(x)}\n" + " ".join(repr(float(b)) for b in box) + "\n"
    text += "".join(f"{int(t)} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for t, p in zip(types, x))
    out = subprocess.run([exe, path, str(energy_unit)] + list(elements), input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = out[0].split()
    w9 = np.array([float(v) for v in out[1].split()]).reshape(3, 3)
    f = np.array([[float(v) for v in line.split()] for line in out[2:2 + len(x)]])
    e2, e3 = float(head[0]), float(head[1])
    return dict(e2=e2, e3=e3, e=e2 + e3, npairs=int(head[2]), ntriplets=int(head[3]), maxin=int(head[4]), w33=w9,
                w=np.array([w9[0, 0], w9[1, 1], w9[2, 2], w9[0, 1], w9[0, 2], w9[1, 2]]), f=f)


COORDINATION = ["coord27", "coord64", "coord27_sic", "triclinic"]


def _inputs():
    """name -> (file, elements, case): every static input of the CPU tests"""
    out = {}
    for rn, r in (("inside_c", 2.4), ("between", 2.9), ("next_to_a", en.SI_A - 1e-6)):
        out[f"dimer_{rn}"] = (SI, ["Si"], en.case_dimer(r))
    out["trimer"] = (SI, ["Si"], en.case_trimer())
    out["cell8"] = (SI, ["Si"], en.case_diamond(1))
    out["cell8j"] = (SI, ["Si"], en.case_diamond_jitter(1, 4, 0.02))
    out["coord27"] = (SI, ["Si"], en.case_coordination(27))
    out["coord64"] = (SI, ["Si"], en.case_coordination(64))
    out["triclinic"] = (SI, ["Si"], en.case_triclinic())
    out["jitter64"] = (SI, ["Si"], en.case_diamond_jitter(2, 1, 0.35))
    out["coord27_sic"] = (SIC, ["Si", "C"], en.case_coordination(27, two_elements=True))
    out["dimer_sic"] = (SIC, ["Si", "C"], en.case_dimer(2.7, 0, 1))
    return out


NAMES = sorted(_inputs())


@pytest.fixture(scope="module")
def refs():
    """per input: (numpy object, file, elements, case, numpy result, driver result), each computed once"""
    exe = driver_exe()
    out = {}
    for name, (path, el, case) in _inputs().items():
        ref = en.Edip(en.read_edip(path, el)[0])
        out[name] = (ref, path, el, case, ref.compute(*case), _run(exe, path, el, *case))
    return out


# what differs beyond 1e-12 of the largest force component, energy term and virial component of ref, or of `scale` (the perfect cell,
# whose forces and virial cancel, is measured on its jittered twin: its energy terms too)
mismatch = functools.partial(hostdrv.mismatch, counters=("npairs", "ntriplets", "maxin"), energies=("e2", "e3"), tol=1e-12, energy_scale_of_scale=True)


@pytest.mark.parametrize("name", COORDINATION)
def test_coordination_inputs_are_soft(refs, name):
    """at least half of the ordered pairs inside a stand in (c, a): the reference alone says so, before anything is compared"""
    ref = refs[name][4]
    print(f"{name}: {ref['soft']} of {ref['npairs']} ordered pairs in (c, a), mean Z {ref['z'].mean():.3f}")
    assert 2 * ref["soft"] >= ref["npairs"] > 0


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    _, _, _, case, ref, got = refs[name]
    assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and np.isfinite(got["e"])
    scale = refs["cell8j"][4] if name == "cell8" else ref
    assert mismatch(got, ref, scale=scale) == [], mismatch(got, ref, scale=scale)
    assert abs(ref["f"].sum(axis=0)).max() <= 1e-10 * max(np.abs(scale["f"]).max(), 1e-300)
    if name in ("cell8", "cell8j"):
        assert (ref["maxin"], ref["npairs"], ref["ntriplets"], ref["soft"]) == (4, 8 * 4, 8 * 6, 0)
    if name.startswith("dimer"):
        assert ref["npairs"] == 2 and ref["ntriplets"] == 0
    if name == "dimer_inside_c":
        assert list(ref["z"]) == [1.0, 1.0] and ref["soft"] == 0
    if name == "dimer_between":
        assert ref["soft"] == 2 and 0.0 < ref["z"][0] < 1.0 and np.abs(ref["f"]).max() > 0.0
    if name == "dimer_next_to_a":      # exp(-5e5) = 0 times derivatives of 1e12: finite, and zero
        assert ref["soft"] == 2 and got["e2"] == 0.0 and not got["f"].any()
    if name == "trimer":
        assert (ref["npairs"], ref["ntriplets"], ref["soft"]) == (4, 1, 2) and ref["e3"] > 0.0      # (the two ends are 3.99 A apart)
    if name == "jitter64":
        assert 0 < ref["soft"] < ref["npairs"] and ref["maxin"] > 4


@pytest.mark.parametrize("r", [en.SI_A, en.SI_A + 1e-9, en.SI_A + 1.0])
def test_a_dimer_at_or_beyond_a_is_exactly_zero(r):
    case = en.case_dimer(r)
    ref = en.Edip(en.read_edip(SI, ["Si"])[0])
    for got in (ref.compute(*case), _run(driver_exe(), SI, ["Si"], *case)):
        assert got["npairs"] == 0 and got["e2"] == 0.0 and got["e3"] == 0.0 and not got["f"].any() and not got["w"].any()


def test_diamond_silicon(refs):
    ref_ed, _, _, case, ref, _ = refs["cell8"]
    ecoh = ref["e"] / 8.0 / en.EV_TO_KCALMOL
    print(f"diamond silicon at {en.A_SI} A: {ecoh:.6f} eV per atom, E3 {ref['e3']:.3e} kcal/mol, tau(4) - 1/3 = {en.tau(ref_ed.p[(0, 0, 0)], 4.0) - 1.0 / 3.0:.2e}")
    assert abs(ecoh - (-4.649953)) < 1e-6
    assert abs(ref["e3"]) <= 1e-10 * abs(ref["e2"])
    assert (ref["z"] == 4.0).all()
    assert np.abs(ref["f"]).max() < 1e-10      # (every atom sits on a centre of tetrahedral symmetry)
    e = {a: ref_ed.energy(*en.case_diamond(1, a)) for a in (5.42, 5.43, 5.44)}
    assert e[5.43] < e[5.42] and e[5.43] < e[5.44]
    amin = 5.43 - 0.01 * (e[5.44] - e[5.42]) / (2.0 * (e[5.44] - 2.0 * e[5.43] + e[5.42]))      # the parabola through the three
    print(f"minimum of the diamond lattice near {amin:.4f} A")
    assert 5.42 < amin < 5.44


def test_c11_of_silicon(refs):
    """second difference of the energy at +-1e-3 strain of the perfect cell: 172.04 GPa (published: 172)"""
    ref_ed = refs["cell8"][0]
    x, box, t = en.case_diamond(1)
    h, v = 1e-3, en.volume(box)
    E = lambda eps: ref_ed.energy(*en.strained(x, box, eps), t)
    c11 = (E(np.diag([h, 0.0, 0.0])) - 2.0 * E(np.zeros((3, 3))) + E(np.diag([-h, 0.0, 0.0]))) / h ** 2 / v * en.KCALMOL_A3_TO_GPA
    print(f"C11 = {c11:.3f} GPa")
    assert abs(c11 / 172.04 - 1.0) < 1e-3


@pytest.mark.parametrize("name", ["coord27", "coord64", "coord27_sic", "jitter64", "trimer", "triclinic"])
def test_numpy_forces_are_the_gradient_of_its_energy(refs, name):
    """central differences of the numpy energy, h = 1e-5 A, within 1e-6 of the largest force: truncation h^2 f'''/6 ~ 1e-10 f, rounding
    1e-16 E / h ~ 1e-8 kcal/mol/A; every input keeps 1e-4 A from every c and a, so no pair changes sides within h"""
    ref_ed, _, _, (x, box, t), ref, _ = refs[name]
    assert ref_ed.margin(x, box, t) >= 1e-4
    assert abs(ref_ed.energy(x, box, t) - ref["e"]) <= 1e-13 * max(abs(ref["e2"]), abs(ref["e3"]))
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(3):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(ref_ed.energy(x + h * u, box, t) - ref_ed.energy(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(ref["f"] * u)) < 1e-6 * np.abs(ref["f"]).max(), name


@pytest.mark.parametrize("name", ["coord27", "coord27_sic"])
def test_numpy_virial_is_the_strain_derivative_of_its_energy(refs, name):
    ref_ed, _, _, (x, box, t), ref, _ = refs[name]
    h = 1e-6
    for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        e = np.zeros((3, 3))
        e[a, b] = h
        ep = ref_ed.energy(*en.strained(x, box, e), t)
        em = ref_ed.energy(*en.strained(x, box, -e), t)
        assert abs(-(ep - em) / (2 * h) - ref["w"][k]) < 1e-5 * np.abs(ref["w"]).max(), k      # W_ab = sum d_a f_b = -dE/d eps_ab


@pytest.mark.parametrize("name", COORDINATION + ["jitter64"])
def test_the_sum_of_the_per_pair_virials_is_symmetric(refs, name):
    """W = sum over neighbours of d (x) (force on the neighbour), all nine components summed apart (numpy and driver): the pair and the
    coordination terms are d (x) d, the triplet terms are not, and only their sum over a triplet is symmetric"""
    _, _, _, _, ref, got = refs[name]
    for w in (ref["w33"], got["w33"]):
        assert np.abs(w - w.T).max() <= 1e-10 * np.abs(w).max()


@pytest.mark.parametrize("order", ["Si C", "C Si", "Si C Si"])
def test_element_orders_and_a_many_to_one_type_map(refs, order):
    """the synthetic file under both element orders of pair_coeff (the types swapped with them: the same crystal), and with three LAMMPS
    types of which the first and the third are silicon"""
    _, path, _, (x, box, t), ref, _ = refs["coord27_sic"]
    if order == "Si C":
        types = t
    elif order == "C Si":
        types = 1 - t
    else:
        types = np.where((t == 0) & (np.arange(len(t)) % 3 == 0), 2, t)
        assert set(types) == {0, 1, 2}
    assert mismatch(_run(driver_exe(), path, order.split(), x, box, types), ref) == []


def test_both_energy_units(refs):
    """energy_unit 1 takes A and lambda as written: the fixture read that way is 23 times weaker, and driver and numpy agree on it"""
    _, _, _, case, ref, _ = refs["coord27"]
    p, _ = en.read_edip(SI, ["Si"], energy_unit=1)
    assert p[(0, 0, 0)]["A"] == 7.9821730 and p[(0, 0, 0)]["lambda"] == 1.4533108
    got = _run(driver_exe(), SI, ["Si"], *case, energy_unit=1)
    assert mismatch(got, en.Edip(p).compute(*case)) == []
    assert abs(got["e"] * en.EV_TO_KCALMOL / ref["e"] - 1.0) < 1e-12


WRONG = {1: ("coord27", ["forces", "virial"]), 2: ("coord27", None), 3: ("coord27", None), 4: ("coord27", None), 5: ("coord27_sic", None)}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_builds_are_caught(refs, wrong):
    exe = driver_exe(wrong)
    name, what = WRONG[wrong]
    _, path, el, case, ref, _ = refs[name]
    bad = mismatch(_run(exe, path, el, *case), ref)
    print(f"wrong build {wrong} on {name}: {bad}")
    assert bad and (what is None or bad == what)
    # ... and the diamond cell sees none of them.  Build 3 at 1e-10: the published constants give tau(4) = 1/3 - 2.6e-7, not 1/3, so
    # the right three-body energy of the cell is 48 g^2 lambda (1 + eta) Q(4) (2.6e-7)^2 = 1.4e-10 kcal/mol where build 3 has exactly 0,
    # and its radial derivative, 1.4e-10 x 2 r gamma / (r - a)^2 ~ 1e-9 in the trace of the virial, is 1e-11 of the jittered twin's
    # virial: above the 1e-12 of rounding, below anything a test of the cell could tell from noise in FP64 sums at the GPU's budget
    _, path, el, case, ref, _ = refs["cell8"]
    assert mismatch(_run(exe, path, el, *case), ref, tol=1e-10 if wrong == 3 else 1e-12, scale=refs["cell8j"][4]) == []
