"""The embedded-atom arithmetic of the product (scema_amd/csrc/eam/eam_core.h, the functions the HIP kernels of md_eam.hip run), compiled
for the host by tests/eam_host_driver.cpp and held against the independent numpy restatement tests/eam_numpy.py: energies, forces and
virial to 1e-12 relative, forces and virial against central differences of the energy, and the spline formulae against tables of cubic
polynomials, which they reproduce exactly wherever the five-point slope is used.  No GPU needed: this is where the arithmetic is pinned;
the `-m gpu` tests then compare the kernels' output with the same helper.  No LAMMPS exists to compare with.

Wrong builds (eamh_create's `wrong`), tried on this driver:
  1  F'_i and F'_j swapped in the pair term: with one element rho'_j = rho'_i, the sum is the same and every single-element case passes;
     the alloy fails in forces and virial
  2  the density taken from the central atom's element: the same, the single-element cases pass, the alloy fails (energies too)
  3  the extrapolation above rhomax left out: only the embedding energy of the `rhomax` case fails
test_wrong_builds_are_caught asserts all three.
"""
import ctypes as C
import os

import numpy as np
import pytest

import eam_numpy as en
import hostdrv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUAG = os.path.join(ROOT, "tests", "golden", "CuAg.eam.alloy")


def driver_lib():
    L = C.CDLL(hostdrv.build("libeam_host.so", ["tests/eam_host_driver.cpp", "scema_amd/csrc/host/eam_setfl.cpp"], shared=True))
    L.eamh_create.restype = C.c_void_p
    L.eamh_create.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]
    L.eamh_destroy.argtypes = [C.c_void_p]
    L.eamh_cutoff.restype = C.c_double
    L.eamh_cutoff.argtypes = [C.c_void_p]
    L.eamh_compute.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    return L


class Driver:
    def __init__(self, L, path, elements, wrong=0, energy_unit=0):
        self.L = L
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self.h = L.eamh_create(path.encode(), arr, len(elements), energy_unit, wrong)
        assert self.h

    def __call__(self, x, box, types):
        n = len(x)
        x = np.ascontiguousarray(x, float); box = np.ascontiguousarray(box, float); t = np.ascontiguousarray(types, np.int32)
        f, e, w, cnt, rho = np.zeros((n, 3)), np.zeros(2), np.zeros(6), np.zeros(3, np.int32), np.zeros(n)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert self.L.eamh_compute(self.h, n, p(t), p(x), p(box), p(f), p(e), p(w), p(cnt), p(rho)) == 0
        return dict(f=f, e_pair=e[0], e_embed=e[1], e=e[0] + e[1], w=w, npairs=int(cnt[0]), nabove=int(cnt[1]), maxin=int(cnt[2]), rho=rho)

    def energy(self, x, box, types):
        return self(x, box, types)["e"]


@pytest.fixture(scope="module")
def lib():
    return driver_lib()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the files written at test time: copper alone; copper with rhomax at 1.1 times the lattice's density; cubic polynomials"""
    d = tmp_path_factory.mktemp("eam")
    en.write_johnson(str(d / "Cu.eam.alloy"), ["Cu"])
    en.write_johnson(str(d / "CuLow.eam.alloy"), ["Cu"], rhomax_over_rhoe=1.1)
    en.write_poly(str(d / "poly.eam.alloy"))
    return {"cu": str(d / "Cu.eam.alloy"), "low": str(d / "CuLow.eam.alloy"), "poly": str(d / "poly.eam.alloy")}


def _inputs(files):
    al = en.case_alloy()
    knot = 223 * 0.0112                     # a knot of the fixture's r grid
    return {
        "single": (CUAG, ["Cu"], en.case_single()),
        "dimer_knot": (CUAG, ["Cu"], en.case_dimer(knot)),
        "dimer_between": (CUAG, ["Cu"], en.case_dimer(2.5037)),
        "cell4": (CUAG, ["Cu"], en.case_cell4()),
        "j32": (CUAG, ["Cu"], en.case_jitter(2)),
        "j108": (CUAG, ["Cu"], en.case_jitter(3)),
        "gas": (CUAG, ["Cu"], en.case_gas()),
        "silver": (CUAG, ["Ag"], en.case_jitter(2, a=en.A_AG)),
        "one_file": (files["cu"], ["Cu"], en.case_jitter(2)),
        "alloy": (CUAG, ["Cu", "Ag"], al),
        "alloy_ac": (CUAG, ["Ag", "Cu"], (al[0], al[1], 1 - al[2])),
        "rhomax": (files["low"], ["Cu"], en.case_jitter(2, a=0.95 * en.A_CU)),
    }


NAMES = ["single", "dimer_knot", "dimer_between", "cell4", "j32", "j108", "gas", "silver", "one_file", "alloy", "alloy_ac", "rhomax"]
SINGLE_ELEMENT = ["dimer_between", "cell4", "j32", "gas", "silver", "one_file"]


@pytest.fixture(scope="module")
def refs(lib, files):
    """per input: (numpy object, driver, case, numpy result, driver result), each computed once"""
    out = {}
    for name, (path, el, case) in _inputs(files).items():
        ref = en.EAM(en.read_setfl(path, el)[0])
        drv = Driver(lib, path, el)
        out[name] = (ref, drv, case, ref.compute(*case), drv(*case))
    return out


def same(got, ref, tol=1e-12):
    assert got["npairs"] == ref["npairs"] and got["nabove"] == ref["nabove"], (got["npairs"], ref["npairs"], got["nabove"], ref["nabove"])
    es = max(abs(ref["e_pair"]), abs(ref["e_embed"]))
    for k in ("e_pair", "e_embed"):
        assert abs(got[k] - ref[k]) <= tol * es, k
    if ref["npairs"] == 0:
        assert not ref["f"].any() and not got["f"].any() and not got["w"].any()
        return
    fs = np.abs(ref["f"]).max()
    assert np.abs(got["f"] - ref["f"]).max() <= tol * fs, np.abs(got["f"] - ref["f"]).max() / fs
    assert np.abs(got["w"] - ref["w"]).max() <= tol * np.abs(ref["w"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    ref_e, drv, case, ref, got = refs[name]
    same(got, ref)
    assert abs(ref["f"].sum(axis=0)).max() <= 1e-10 * max(np.abs(ref["f"]).max(), 1e-300)
    if name == "single":            # no neighbour: rho = 0, E = F[0] exactly
        assert got["e_embed"] == ref_e.t["F"][0][0] and got["e_pair"] == 0.0 and got["npairs"] == 0
    if name in ("j32", "j108"):
        assert ref["maxin"] > 32
    if name == "cell4":             # images of the atom itself and of the others, two boxes away
        assert ref["maxin"] >= 50 and case[1][3] < 5.5
    if name == "rhomax":
        assert ref["nabove"] == 32
    if name == "alloy_ac":          # the same crystal under the other element order: the same numbers
        same(got, refs["alloy"][3], tol=1e-13)
    if name == "one_file":          # a file of copper alone holds the same copper
        same(got, refs["j32"][3], tol=1e-13)


def test_dimer_at_the_cutoff_to_the_bit(lib):
    """at 5.5 A exactly and beyond nothing is in range: E = 2 F[0], forces exactly zero; just inside the terms are finite and small -- not
    zero: the cubic of the interval that holds the cutoff interpolates the switching function between its knots, off by some (dr)^2 of
    its curvature, and F' is at its largest at rho = 0"""
    drv, ref_e = Driver(lib, CUAG, ["Cu"]), en.EAM(en.read_setfl(CUAG, ["Cu"])[0])
    assert lib.eamh_cutoff(drv.h) == 5.5
    f0 = ref_e.t["F"][0][0]
    for obj in (drv, ref_e.compute):
        for d in (0.0, 1e-6):
            o = obj(*en.case_dimer(5.5 + d))
            assert o["npairs"] == 0 and o["e_pair"] == 0.0 and o["e_embed"] == 2.0 * f0 and not o["f"].any() and not o["w"].any()
        o = obj(*en.case_dimer(5.5 - 1e-6))
        assert o["npairs"] == 2 and np.isfinite(o["f"]).all() and np.abs(o["f"]).max() < 1e-2 and abs(o["e_pair"]) < 1e-5
    same(drv(*en.case_dimer(5.5 - 1e-6)), ref_e.compute(*en.case_dimer(5.5 - 1e-6)))


def test_spline_reproduces_cubic_polynomials(files):
    """tables of cubic polynomials: away from the two intervals at either end, where the slopes are three-point or one-sided, the
    five-point slope is exact for a cubic and so is the Hermite cubic between two knots -- values and derivatives to rounding"""
    tab = en.read_setfl(files["poly"], ["X"], energy_unit=1)[0]
    for key, f, delta in (("F", tab["F"][0], tab["drho"]), ("rho", tab["rho"][0], tab["dr"]), ("z", tab["z"][0][0], tab["dr"])):
        s = en.spline(f, delta)
        n = len(f)
        xs = np.linspace(2.0 * delta, (n - 3) * delta, 997)
        c = en.POLY[key]
        vs = max(abs(en.poly(c, x)) for x in xs)
        ds = max(abs(en.dpoly(c, x)) for x in xs)
        for x in xs:
            v, d = en.lookup(s, delta, x, floor0=key == "F")
            assert abs(v - en.poly(c, x)) <= 1e-13 * vs and abs(d - en.dpoly(c, x)) <= 1e-13 * ds, (key, x)
        # in the end intervals the spline still interpolates the knots
        for k in (0, 1, n - 2, n - 1):
            assert en.lookup(s, delta, k * delta)[0] == pytest.approx(f[k], rel=1e-14)


def test_energy_loop_equals_compute(refs):
    for name in ("cell4", "j32", "alloy", "rhomax"):
        ref_e, _, case, ref, _ = refs[name]
        assert abs(ref_e.energy(*case) - ref["e"]) <= 1e-13 * max(abs(ref["e_pair"]), abs(ref["e_embed"]))


@pytest.mark.parametrize("name", ["cell4", "j32", "alloy", "rhomax"])
@pytest.mark.parametrize("which", ["numpy", "driver"])
def test_forces_are_the_gradient_of_the_energy(refs, name, which):
    """central differences of the energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A"""
    ref_e, drv, (x, box, t), ref, got = refs[name]
    fn, f = (ref_e.energy, ref["f"]) if which == "numpy" else (drv.energy, got["f"])
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(6 if which == "driver" else 2):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), (name, which)


@pytest.mark.parametrize("name", ["j32", "alloy"])
def test_virial_is_the_strain_derivative_of_the_energy(refs, name):
    ref_e, drv, (x, box, t), ref, got = refs[name]
    h = 1e-6
    for obj, w in ((drv, got["w"]),) + (((ref_e, ref["w"]),) if name == "alloy" else ()):
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            e = np.zeros((3, 3))
            e[a, b] = h
            ep = obj.energy(*en.strained(x, box, e), t)
            em = obj.energy(*en.strained(x, box, -e), t)
            assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)      # W_ab = sum d_a f_b = -dE/d eps_ab


def test_energy_unit(lib):
    """energy_unit 1 takes F and r phi as written: the energies of unit 0 are 23.060549 times those; the density has no unit"""
    x, box, t = en.case_jitter(2)
    e0, e1 = Driver(lib, CUAG, ["Cu"])(x, box, t), Driver(lib, CUAG, ["Cu"], energy_unit=1)(x, box, t)
    assert abs(e0["e"] / e1["e"] / en.EV_TO_KCALMOL - 1.0) < 1e-13 and abs(e0["f"] / e1["f"] / en.EV_TO_KCALMOL - 1.0).max() < 1e-11
    assert np.array_equal(e0["rho"], e1["rho"])


def test_wrong_builds_are_caught(lib, refs, files):
    """the wrong builds of the module docstring fail where it says"""
    inputs = _inputs(files)

    def fails(wrong, name):
        path, el, case = inputs[name]
        got = Driver(lib, path, el, wrong=wrong)(*case)
        try:
            same(got, refs[name][3])
        except AssertionError:
            return True
        return False
    for wrong in (1, 2):
        for name in SINGLE_ELEMENT:
            assert not fails(wrong, name), (wrong, name)
        assert fails(wrong, "alloy") and fails(wrong, "alloy_ac"), wrong
    for name in NAMES:
        assert fails(3, name) == (name == "rhomax"), name
    path, el, case = inputs["rhomax"]
    bad, ref = Driver(lib, path, el, wrong=3)(*case), refs["rhomax"][3]
    assert np.abs(bad["f"] - ref["f"]).max() <= 1e-12 * np.abs(ref["f"]).max() and abs(bad["e_embed"] - ref["e_embed"]) > 1e-6 * abs(ref["e_embed"])
