"""The arithmetic of the angular-dependent potential (scema_amd/csrc/eam/adp_core.h, the functions the HIP kernels of md_adp.hip run),
compiled for the host as the stand-alone program tests/adp_host_driver.cpp and held against the independent numpy restatement
tests/adp_numpy.py: energies, forces and virial to 1e-12 relative (the budget of test_eam_host.py), forces against central differences
of the energy (h = 1e-5 A, 1e-6 of the largest force), the virial against the strain derivative of the energy.  No GPU needed: this is
where the arithmetic is pinned; the `-m gpu` tests then compare the kernels with the same helper.  No LAMMPS exists to compare with.

The trap: in a perfect cubic lattice mu = 0 and lam is a multiple of the unit tensor, so the angular energy and forces vanish.  That
case appears once, on purpose (it pins the -nu^2 / 6 term and the factor on the off-diagonal squares); every other input is a cluster,
jittered or an alloy.

Wrong builds (the driver's third argument), each failing a named case (test_wrong_builds_are_caught):
  1  mu_j taken with the sign of mu_i: the forces of j32 (and of every other input with a pair)
  2  Lambda without the trace removed: the forces of j32
  3  u and w looked up by the partner's element alone, [tj][tj]: the alloy, while every single-element input passes.  (The transposition
     [tj][ti] itself cannot show: the file holds one table per unordered pair.  The amplitude of its own that every pair has in the
     fixture is what makes a wrong pair index visible.)
  4  the off-diagonal lam^2 counted once in the energy: the angular energy of the trimer and of j32, not the perfect cell's, no force
  5  the w' term left out: the forces of j32
"""
import os
import subprocess

import numpy as np
import pytest

import adp_numpy as an
import eam_numpy as en
import hostdrv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.adp")


@pytest.fixture(scope="module")
def exe():
    return hostdrv.build("adp_host_driver", ["tests/adp_host_driver.cpp", "scema_amd/csrc/host/eam_setfl.cpp"], shared=False)


class Driver:
    def __init__(self, exe, path, elements, wrong=0, energy_unit=0):
        self.cmd = [exe, path, str(energy_unit), str(wrong)] + list(elements)

    def __call__(self, x, box, types):
        text = "%d\n%s\n" % (len(x), " ".join("%.17g" % b for b in box)) + "".join("%d %.17g %.17g %.17g\n" % (t, *p) for t, p in zip(types, np.asarray(x, float)))
        out = subprocess.run(self.cmd, input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        e = [float(v) for v in out[0].split()[1:]]
        w = np.array([float(v) for v in out[1].split()[1:]])
        c = [int(v) for v in out[2].split()[1:]]
        a = np.array([[float(v) for v in ln.split()[1:]] for ln in out[3:3 + len(x)]])
        lam6 = a[:, 7:13]
        lam = np.zeros((len(x), 3, 3))
        for k, (p, q) in enumerate([(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]):          # xx yy zz yz xz xy
            lam[:, p, q] = lam[:, q, p] = lam6[:, k]
        return dict(f=a[:, :3], e_pair=e[0], e_embed=e[1], e_angular=e[2], e_manybody=e[1] + e[2], e=sum(e), w=w, npairs=c[0], nabove=c[1], maxin=c[2],
                    rho=a[:, 3], mu=a[:, 4:7], lam=lam)

    def energy(self, x, box, types):
        return self(x, box, types)["e"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the files written at test time: copper with rhomax at 1.1 times the lattice's density; the fixture with u = w = 0 and its EAM twin"""
    d = tmp_path_factory.mktemp("adp")
    an.write_fixture(str(d / "CuLow.adp"), ["Cu"], rhomax_over_rhoe=1.1)
    an.write_fixture(str(d / "zero.adp"), ["Cu", "Ag"], angular=False)
    an.write_eam_twin(str(d / "twin.eam.alloy"), ["Cu", "Ag"])
    return {"low": str(d / "CuLow.adp"), "zero": str(d / "zero.adp"), "twin": str(d / "twin.eam.alloy")}


def _inputs(files):
    al = an.case_alloy()
    return {
        "dimer_cucu": (CUAG, ["Cu", "Ag"], an.case_dimer(2.5037, (0, 0))),
        "dimer_cuag": (CUAG, ["Cu", "Ag"], an.case_dimer(2.7, (0, 1))),
        "dimer_agag": (CUAG, ["Cu", "Ag"], an.case_dimer(2.9, (1, 1))),
        "trimer": (CUAG, ["Cu"], an.case_trimer()),
        "trimer_mixed": (CUAG, ["Cu", "Ag"], an.case_trimer((0, 1, 0))),
        "cell4": (CUAG, ["Cu"], an.case_cell4()),
        "j32": (CUAG, ["Cu"], an.case_jitter(2)),
        "j108": (CUAG, ["Cu"], an.case_jitter(3)),
        "silver": (CUAG, ["Ag"], an.case_jitter(2, a=an.A_AG)),
        "alloy": (CUAG, ["Cu", "Ag"], al),
        "alloy_ac": (CUAG, ["Ag", "Cu"], (al[0], al[1], 1 - al[2])),
        "gas": (CUAG, ["Cu"], an.case_gas()),
        "rhomax": (files["low"], ["Cu"], an.case_jitter(2, a=0.95 * an.A_CU)),
        "zero": (files["zero"], ["Cu", "Ag"], al),
    }


NAMES = ["dimer_cucu", "dimer_cuag", "dimer_agag", "trimer", "trimer_mixed", "cell4", "j32", "j108", "silver", "alloy", "alloy_ac", "gas", "rhomax", "zero"]
SINGLE_ELEMENT = ["trimer", "cell4", "j32", "silver", "gas"]


@pytest.fixture(scope="module")
def refs(exe, files):
    """per input: (numpy object, driver, case, numpy result, driver result), each computed once"""
    out = {}
    for name, (path, el, case) in _inputs(files).items():
        ref = an.ADP(an.read_adp(path, el)[0])
        drv = Driver(exe, path, el)
        out[name] = (ref, drv, case, ref.compute(*case), drv(*case))
    return out


def _same(got, ref, tol=1e-12):
    assert got["npairs"] == ref["npairs"] and got["nabove"] == ref["nabove"], (got["npairs"], ref["npairs"], got["nabove"], ref["nabove"])
    es = max(abs(ref["e_pair"]), abs(ref["e_embed"]), abs(ref["e_angular"]))
    for k in ("e_pair", "e_embed", "e_angular"):
        assert abs(got[k] - ref[k]) <= tol * es, (k, got[k], ref[k])
    fs = np.abs(ref["f"]).max()
    assert np.abs(got["f"] - ref["f"]).max() <= tol * fs, np.abs(got["f"] - ref["f"]).max() / fs
    assert np.abs(got["w"] - ref["w"]).max() <= tol * np.abs(ref["w"]).max()
    assert np.abs(got["mu"] - ref["mu"]).max() <= tol * max(np.abs(ref["mu"]).max(), np.abs(ref["lam"]).max())
    assert np.abs(got["lam"] - ref["lam"]).max() <= tol * np.abs(ref["lam"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, files, name):
    ref_e, drv, case, ref, got = refs[name]
    _same(got, ref)
    assert abs(ref["f"].sum(axis=0)).max() <= 1e-10 * np.abs(ref["f"]).max()
    assert np.abs(ref["w33"] - ref["w33"].T).max() <= 1e-10 * np.abs(ref["w33"]).max()       # pair by pair it is not symmetric, the sum is
    if name.startswith("dimer"):    # closed forms: mu_0 = u d, mu_1 = -mu_0, lam_0 = lam_1 = w d (x) d
        x, _, t = case
        d = x[1] - x[0]
        r = np.linalg.norm(d)
        u = en.lookup(ref_e.su[t[0]][t[1]], ref_e.t["dr"], r)[0]
        w = en.lookup(ref_e.sw[t[0]][t[1]], ref_e.t["dr"], r)[0]
        assert abs(u) > 1e-2 and abs(w) > 1e-2
        assert np.abs(got["mu"][0] - u * d).max() <= 1e-13 * abs(u) * r and np.abs(got["mu"][1] + u * d).max() <= 1e-13 * abs(u) * r
        for k in (0, 1):
            assert np.abs(got["lam"][k] - w * np.outer(d, d)).max() <= 1e-13 * abs(w) * r * r
        # E_angular = 2 [1/2 u^2 r^2 + 1/2 w^2 r^4 - w^2 r^4 / 6]
        assert abs(got["e_angular"] - (u * u * r * r + 2.0 / 3.0 * w * w * r ** 4)) <= 1e-13 * got["e_angular"]
    if name in ("j32", "j108", "alloy"):
        assert ref["maxin"] > 32
        ratio = np.abs(ref["f_angular"]).max() / np.abs(ref["f_eam"]).max()
        assert 0.01 < ratio < 1.0, ratio          # the angular forces are neither noise nor the whole force
    if name == "cell4":             # images of the atom itself and of the others, two boxes away
        assert ref["maxin"] >= 50 and case[1][3] < 5.5
    if name == "rhomax":
        assert ref["nabove"] == 32
    if name == "alloy_ac":          # the same crystal under the other element order: the same numbers
        _same(got, refs["alloy"][3], tol=1e-13)
    if name == "zero":              # u = w = 0: the embedded-atom method on the twin file
        twin = en.EAM(en.read_setfl(files["twin"], ["Cu", "Ag"])[0]).compute(*case)
        assert got["e_angular"] == 0.0 and not got["mu"].any() and not got["lam"].any()
        assert abs(got["e_pair"] - twin["e_pair"]) <= 1e-12 * abs(twin["e_pair"]) and abs(got["e_embed"] - twin["e_embed"]) <= 1e-12 * abs(twin["e_embed"])
        assert np.abs(got["f"] - twin["f"]).max() <= 1e-12 * np.abs(twin["f"]).max() and np.abs(got["w"] - twin["w"]).max() <= 1e-12 * np.abs(twin["w"]).max()


def test_perfect_cell_has_no_angular_energy(exe):
    """the perfect 4-atom cell, two images deep: mu = 0, lam = (nu / 3) I, so 1/2 sum lam^2 = nu^2 / 6 and the angular energy is zero to
    rounding (of the two terms that cancel) -- in numpy and in the driver; the forces vanish too"""
    x, box = an.fcc(1, 1, 1, an.A_CU)
    t = an.zeros(4)
    ref_e = an.ADP(an.read_adp(CUAG, ["Cu"])[0])
    for o in (ref_e.compute(x, box, t), Driver(exe, CUAG, ["Cu"])(x, box, t)):
        nu = np.trace(o["lam"], axis1=1, axis2=2)
        assert np.abs(nu).min() > 1.0                                   # the terms that cancel are not small
        assert abs(o["e_angular"]) <= 1e-13 * np.sum(nu * nu) / 6.0
        assert np.abs(o["mu"]).max() <= 1e-13 * np.abs(nu).max() and np.abs(o["f"]).max() <= 1e-11 * np.abs(nu).max() ** 2
    assert abs(ref_e.energy(x, box, t) - ref_e.compute(x, box, t)["e"]) <= 1e-12 * abs(ref_e.compute(x, box, t)["e_embed"])


def test_energy_loop_equals_compute(refs):
    for name in ("trimer_mixed", "cell4", "j32", "alloy", "rhomax"):
        ref_e, _, case, ref, _ = refs[name]
        assert abs(ref_e.energy(*case) - ref["e"]) <= 1e-13 * max(abs(ref["e_pair"]), abs(ref["e_embed"]))


@pytest.mark.parametrize("name", ["trimer_mixed", "cell4", "j32", "alloy", "rhomax"])
@pytest.mark.parametrize("which", ["numpy", "driver"])
def test_forces_are_the_gradient_of_the_energy(refs, name, which):
    """central differences of the energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A"""
    ref_e, drv, (x, box, t), ref, got = refs[name]
    fn, f = (ref_e.energy, ref["f"]) if which == "numpy" else (drv.energy, got["f"])
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(4):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), (name, which)
    # one atom alone, along each axis: a sum over all atoms could hide an error that cancels between the two ends of a pair
    for c in range(3):
        u = np.zeros_like(x)
        u[1, c] = 1.0
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - f[1, c]) < 1e-6 * np.abs(f).max(), (name, which, c)


@pytest.mark.parametrize("name", ["j32", "alloy"])
def test_virial_is_the_strain_derivative_of_the_energy(refs, name):
    ref_e, drv, (x, box, t), ref, got = refs[name]
    h = 1e-6
    for obj, w in ((drv, got["w"]), (ref_e, ref["w"])):
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            e = np.zeros((3, 3))
            e[a, b] = h
            ep = obj.energy(*an.strained(x, box, e), t)
            em = obj.energy(*an.strained(x, box, -e), t)
            assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)      # W_ab = -dE/d eps_ab


def test_energy_unit(exe):
    """energy_unit 1 takes everything as written: the energies of unit 0 are 23.060549 times those (F and r phi by the factor, u and w
    by its square root, and mu^2, lam^2 are the energies); the density has no unit"""
    x, box, t = an.case_alloy()
    e0, e1 = Driver(exe, CUAG, ["Cu", "Ag"])(x, box, t), Driver(exe, CUAG, ["Cu", "Ag"], energy_unit=1)(x, box, t)
    for k in ("e_pair", "e_embed", "e_angular"):
        assert abs(e0[k] / e1[k] / an.EV_TO_KCALMOL - 1.0) < 1e-13, k
    assert abs(e0["f"] / e1["f"] / an.EV_TO_KCALMOL - 1.0).max() < 1e-10
    assert abs(e0["mu"] / e1["mu"] / np.sqrt(an.EV_TO_KCALMOL) - 1.0).max() < 1e-12
    assert np.array_equal(e0["rho"], e1["rho"])


def test_wrong_builds_are_caught(exe, refs, files):
    """the wrong builds of the module docstring fail where it says"""
    inputs = _inputs(files)

    def run(wrong, name):
        path, el, case = inputs[name]
        return Driver(exe, path, el, wrong=wrong)(*case)

    def fails(wrong, name, got=None):
        try:
            _same(got or run(wrong, name), refs[name][3])
        except AssertionError:
            return True
        return False

    def force_err(got, name):
        return np.abs(got["f"] - refs[name][3]["f"]).max() / np.abs(refs[name][3]["f"]).max()
    for wrong in (1, 2, 5):
        got = run(wrong, "j32")
        assert force_err(got, "j32") > 1e-4, wrong
        assert abs(got["e"] - refs["j32"][3]["e"]) <= 1e-12 * abs(refs["j32"][3]["e_embed"])       # the energy is not what they break
    assert fails(1, "dimer_cuag") and fails(1, "alloy")
    for name in SINGLE_ELEMENT:
        assert not fails(3, name), name
    assert fails(3, "alloy") and fails(3, "alloy_ac") and fails(3, "dimer_cuag") and fails(3, "trimer_mixed")
    for name in ("trimer", "j32"):
        got = run(4, name)
        ref = refs[name][3]
        assert abs(got["e_angular"] - ref["e_angular"]) > 1e-3 * abs(ref["e_angular"]) and force_err(got, name) <= 1e-12
    x, box = an.fcc(1, 1, 1, an.A_CU)
    assert abs(Driver(exe, CUAG, ["Cu"], wrong=4)(x, box, an.zeros(4))["e_angular"]) < 1e-10       # lam is diagonal there: nothing to count
    assert not fails(2, "zero") and not fails(5, "zero")
