"""The Stillinger-Weber arithmetic of the product (scema_amd/csrc/sw/sw_core.h, the functions the HIP kernels of md_sw.hip run), compiled
for the host by tests/sw_host_driver.cpp and held against the independent numpy restatement tests/sw_numpy.py: energies, forces and
virial to 1e-12 relative, forces against central differences of the energy, and the closed forms of the silicon parameters.  No GPU
needed: this is where every derivative is pinned; the `-m gpu` tests then compare the kernels' output with the same helper.

Closed forms (Stillinger and Weber's silicon, tests/golden/Si.sw): the perfect diamond lattice at a = 4 2^(1/6) sigma / sqrt 3 has
E/N = -2 eps to the digits of A and B (1e-9) and no forces; C11 = 151.42 GPa and C12 = 76.42 GPa, which are free of internal relaxation
by symmetry, from second differences of the energy under +-1e-3 homogeneous strain, to 0.1 %.
"""
import ctypes as C
import os

import numpy as np
import pytest

import hostdrv
import sw_numpy as swn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SI_SW = os.path.join(ROOT, "tests", "golden", "Si.sw")
EPS = 2.1683 * swn.EV_TO_KCALMOL


def driver_lib():
    L = C.CDLL(hostdrv.build("libsw_host.so", ["tests/sw_host_driver.cpp", "scema_amd/csrc/host/sw_params.cpp"], shared=True))
    L.swh_create.restype = C.c_void_p
    L.swh_create.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]
    L.swh_destroy.argtypes = [C.c_void_p]
    L.swh_cutmax.restype = C.c_double
    L.swh_cutmax.argtypes = [C.c_void_p]
    L.swh_fast_pairs.argtypes = [C.c_void_p]
    L.swh_compute.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    return L


class Driver:
    def __init__(self, L, path, elements, general=False, energy_unit=0):
        self.L = L
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self.h = L.swh_create(path.encode(), arr, len(elements), energy_unit, 1 if general else 0)
        assert self.h

    def __call__(self, x, box, types):
        n = len(x)
        x = np.ascontiguousarray(x, float); box = np.ascontiguousarray(box, float); t = np.ascontiguousarray(types, np.int32)
        f, e, w, cnt = np.zeros((n, 3)), np.zeros(2), np.zeros(6), np.zeros(3, np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert self.L.swh_compute(self.h, n, p(t), p(x), p(box), p(f), p(e), p(w), p(cnt)) == 0
        return dict(f=f, e2=e[0], e3=e[1], e=e[0] + e[1], w=w, npairs=int(cnt[0]), ntriplets=int(cnt[1]), maxin=int(cnt[2]))

    def energy(self, x, box, types):
        return self(x, box, types)["e"]


@pytest.fixture(scope="module")
def lib():
    return driver_lib()


@pytest.fixture(scope="module")
def two_sw(tmp_path_factory):
    p = tmp_path_factory.mktemp("sw") / "two.sw"
    p.write_text(swn.TWO_ELEMENT_SW)
    return str(p)


@pytest.fixture(scope="module")
def si(lib):
    """(numpy helper, driver with the p = 4, q = 0 fast path, driver with pow) for silicon"""
    prm, _ = swn.read_sw(SI_SW, ["Si"])
    fast, general = Driver(lib, SI_SW, ["Si"]), Driver(lib, SI_SW, ["Si"], general=True)
    assert lib.swh_fast_pairs(fast.h) == 1 and lib.swh_fast_pairs(general.h) == 0
    assert lib.swh_cutmax(fast.h) == 1.80 * 2.0951
    return swn.SW(prm), fast, general


@pytest.fixture(scope="module")
def two(lib, two_sw):
    prm, _ = swn.read_sw(two_sw, ["Si", "X"])
    d = Driver(lib, two_sw, ["Si", "X"])
    assert lib.swh_fast_pairs(d.h) == 1          # Si-Si alone has p = 4, q = 0: the other pairs take pow
    return swn.SW(prm), d


def same(got, ref, tol=1e-12):
    assert got["npairs"] == ref["npairs"] and got["ntriplets"] == ref["ntriplets"] and got["maxin"] == ref["maxin"]
    fs = max(np.abs(ref["f"]).max(), 1e-300)
    assert np.abs(got["f"] - ref["f"]).max() <= tol * fs
    for k in ("e2", "e3"):
        assert abs(got[k] - ref[k]) <= tol * max(abs(ref["e2"]), abs(ref["e3"]))
    assert np.abs(got["w"] - ref["w"]).max() <= tol * np.abs(ref["w"]).max()


CASES = {"a": swn.case_a, "b": swn.case_b, "c": swn.case_c, "h": swn.case_h}


@pytest.mark.parametrize("name", sorted(CASES))
def test_static_cases_match_numpy(si, name):
    ref_sw, fast, general = si
    x, box, t = CASES[name]()
    ref = ref_sw.compute(x, box, t)
    same(fast(x, box, t), ref)
    same(general(x, box, t), ref)
    if name == "c":
        assert ref["maxin"] == 16 and ref["ntriplets"] == 64 * 120
    assert abs(ref["f"].sum(axis=0)).max() < 1e-10 * np.abs(ref["f"]).max()


def test_two_elements_match_numpy(two):
    ref_sw, d = two
    x, box, t = swn.case_e()
    ref = ref_sw.compute(x, box, t)
    assert ref["ntriplets"] > 0 and len(set(t)) == 2
    same(d(x, box, t), ref)


@pytest.mark.parametrize("which", ["numpy", "fast", "general", "two"])
def test_forces_are_the_gradient_of_the_energy(si, two, which):
    """central differences of the energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A"""
    if which == "two":
        ref_sw, d = two
        x, box, t = swn.case_e()
        fn, f = d.energy, d(x, box, t)["f"]
    else:
        ref_sw, fast, general = si
        x, box, t = swn.case_a()
        obj = dict(numpy=ref_sw, fast=fast, general=general)[which]
        fn, f = obj.energy, (ref_sw.compute(x, box, t) if which == "numpy" else obj(x, box, t))["f"]
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(6):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), which


def test_virial_is_the_strain_derivative_of_the_energy(si):
    ref_sw, fast, _ = si
    x, box, t = swn.case_b()
    h = 1e-6
    for obj, w in ((ref_sw, ref_sw.compute(x, box, t)["w"]), (fast, fast(x, box, t)["w"])):
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            e = np.zeros((3, 3))
            e[a, b] = h
            ep = obj.energy(*swn.strained(x, box, e), t)
            em = obj.energy(*swn.strained(x, box, -e), t)
            # W_ab = sum d_a f_b = -dE/d eps_ab
            assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)


def test_cutoff_is_exact_and_continuous(si):
    """a pair at a sigma - 1e-6, at a sigma + 1e-6 and exactly at the cutoff: finite, continuous, and exactly zero from the cutoff on"""
    ref_sw, fast, general = si
    cut = 1.80 * 2.0951
    base = fast(*swn.case_d(+0.5))                       # the pair well outside: what the third atom contributes alone
    for obj in (ref_sw.compute, fast, general):
        out = {d: obj(*swn.case_d(d)) for d in (-1e-6, 0.0, +1e-6, +0.5)}
        for d, o in out.items():
            assert np.isfinite(o["f"]).all() and np.isfinite(o["w"]).all() and np.isfinite(o["e2"]) and np.isfinite(o["e3"])
        for d in (0.0, +1e-6):                           # from the cutoff on: bitwise what is there without the pair
            assert out[d]["npairs"] == out[+0.5]["npairs"] and out[d]["ntriplets"] == out[+0.5]["ntriplets"]
            assert out[d]["e2"] == out[+0.5]["e2"] and out[d]["e3"] == out[+0.5]["e3"]
            assert (out[d]["f"][[0, 2, 3]] == out[+0.5]["f"][[0, 2, 3]]).all()
        assert out[-1e-6]["npairs"] == out[0.0]["npairs"] + 1
        # just inside the pair's terms carry exp(-sigma / 1e-6): continuous to the last bit of the sums
        assert abs(out[-1e-6]["e"] - out[0.0]["e"]) <= 1e-15 * abs(out[0.0]["e"])
        assert np.abs(out[-1e-6]["f"] - out[0.0]["f"]).max() <= 1e-15 * np.abs(out[0.0]["f"]).max()
        assert out[-1e-6]["ntriplets"] == out[0.0]["ntriplets"] + 1
    assert abs(base["e"]) > 0.0 and base["npairs"] == 1 and base["ntriplets"] == 0
    assert swn.case_d(0.0)[0][1, 0] - swn.case_d(0.0)[0][0, 0] == cut


@pytest.mark.parametrize("which", ["numpy", "fast", "general"])
def test_perfect_lattice_energy_and_forces(si, which):
    ref_sw, fast, general = si
    x, box = swn.diamond(2, 2, 2, swn.si_lattice_constant())
    assert abs(swn.si_lattice_constant() - 5.430950) < 1e-6
    t = np.zeros(len(x), int)
    o = ref_sw.compute(x, box, t) if which == "numpy" else dict(fast=fast, general=general)[which](x, box, t)
    assert abs(o["e"] / len(x) / EPS + 2.0) < 1e-9, o["e"] / len(x) / EPS
    assert np.abs(o["f"]).max() < 1e-9 * EPS
    assert o["npairs"] == 2 * len(x) and o["ntriplets"] == 6 * len(x)


def _c11_c12(energy, x, box, t, h=1e-3):
    v = swn.volume(box)
    def E(e1, e2):
        return energy(*swn.strained(x, box, np.diag([e1, e2, 0.0])), t)
    e0 = E(0.0, 0.0)
    c11 = (E(h, 0.0) - 2.0 * e0 + E(-h, 0.0)) / h ** 2 / v
    c12 = (E(h, h) - E(h, -h) - E(-h, h) + E(-h, -h)) / (4.0 * h ** 2) / v
    return c11 * swn.KCALMOL_A3_TO_GPA, c12 * swn.KCALMOL_A3_TO_GPA


@pytest.mark.parametrize("which", ["numpy", "fast"])
def test_elastic_constants(si, which):
    ref_sw, fast, _ = si
    x, box = swn.diamond(2, 2, 2, swn.si_lattice_constant())
    t = np.zeros(len(x), int)
    c11, c12 = _c11_c12(ref_sw.energy if which == "numpy" else fast.energy, x, box, t)
    assert abs(c11 / 151.42 - 1.0) < 1e-3, c11
    assert abs(c12 / 76.42 - 1.0) < 1e-3, c12
