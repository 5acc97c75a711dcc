"""The Tersoff arithmetic of the product (scema_amd/csrc/tersoff/ts_core.h, the functions the HIP kernels of md_tersoff.hip run), compiled
for the host by tests/tersoff_host_driver.cpp and held against the independent numpy restatement tests/tersoff_numpy.py: energies, forces
and virial to 1e-12 relative, forces against central differences of the energy, the two numerical forms of b_ij and of g, and the closed
form of the diamond lattice.  No GPU needed: this is where every derivative is pinned; the `-m gpu` tests then compare the kernels'
output with the same helper.  No LAMMPS and no reference Tersoff file exist to compare with: these three are the parity there is.

Closed form (tests/golden/SiC.tersoff, Tersoff 1989): on perfect diamond E/N = 2 [A e^{-lambda1 r} - b B e^{-lambda2 r}], r = a sqrt3/4,
zeta = 3 g(-1/3); its minimum lies at a = 5.432 A with -4.62959501 eV/atom for Si and at 3.5656 A with -7.37051421 eV/atom for C.

Wrong builds (tsh_create's `wrong`), tried on this driver:
  1  the pair term owned by the lower index only, and doubled: the single-element lattices still pass to 1e-16 in the energy of the
     PERFECT lattice (V_ij = V_ji by symmetry) but every jittered case fails _same in forces, energy and counts (half the ordered pairs);
     zincblende SiC fails by 4 % in the bond-order energy even unjittered, since b_SiC != b_CSi
  2  R, D of fC(r_ik) from entry i k k: tests/golden/SiC.tersoff writes the same R, D in both entries, so every silicon and SiC case
     passes; the synthetic file, whose i j k entries carry their own R, D, fails _same (count of (j, k) and forces)
  3  R, D of fC(r_ik) from entry i j j (the pair's own parameter set where pair_tersoff.cpp uses that of i j k): the single-element
     cases pass (one entry); jittered SiC fails -- around Si a carbon third atom is cut at the Si-Si 3.0 A instead of 2.51 A and the
     other way round: another count of (j, k) and forces off by more than their size -- and so does the synthetic file
test_wrong_builds_are_caught asserts all three.  A fourth, the neighbour list cut at the pair's own R + D instead of cutin, passes every
input of this file; tests/test_row_edges_host.py has the case that catches it.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import hostdrv
import tersoff_numpy as tsn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.tersoff")


def driver_lib():
    L = C.CDLL(hostdrv.build("libtersoff_host.so", ["tests/tersoff_host_driver.cpp", "scema_amd/csrc/host/tersoff_params.cpp"], shared=True))
    L.tsh_create.restype = C.c_void_p
    L.tsh_create.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]
    L.tsh_destroy.argtypes = [C.c_void_p]
    L.tsh_cutmax.restype = C.c_double
    L.tsh_cutmax.argtypes = [C.c_void_p]
    L.tsh_bond_order.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tsh_slot.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.tsh_g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tsh_compute.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    return L


class Driver:
    def __init__(self, L, path, elements, wrong=0, energy_unit=0):
        self.L = L
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self.h = L.tsh_create(path.encode(), arr, len(elements), energy_unit, wrong)
        assert self.h

    def __call__(self, x, box, types):
        n = len(x)
        x = np.ascontiguousarray(x, float); box = np.ascontiguousarray(box, float); t = np.ascontiguousarray(types, np.int32)
        f, e, w, cnt, z = np.zeros((n, 3)), np.zeros(2), np.zeros(6), np.zeros(3, np.int32), np.zeros((n, 32))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert self.L.tsh_compute(self.h, n, p(t), p(x), p(box), p(f), p(e), p(w), p(cnt), p(z)) == 0
        return dict(f=f, e_rep=e[0], e_att=e[1], e=e[0] + e[1], w=w, npairs=int(cnt[0]), nzeta=int(cnt[1]), maxin=int(cnt[2]), t=z[z >= 0.0])

    def energy(self, x, box, types):
        return self(x, box, types)["e"]

    def bond_order(self, i, j, zeta):
        out = np.zeros(6)
        self.L.tsh_bond_order(self.h, i, j, zeta, out.ctypes.data_as(C.c_void_p))
        return out

    def g(self, i, j, k, c):
        out = np.zeros(2)
        self.L.tsh_g(self.h, i, j, k, c, out.ctypes.data_as(C.c_void_p))
        return out


@pytest.fixture(scope="module")
def lib():
    return driver_lib()


@pytest.fixture(scope="module")
def synth_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("tersoff")
    (d / "synth.tersoff").write_text(tsn.SYNTH)
    (d / "clamp.tersoff").write_text(tsn.SYNTH_CLAMP)
    return str(d / "synth.tersoff"), str(d / "clamp.tersoff")


# name -> (file, elements, case): every static input of the CPU tests.  "sic_cs" names the elements in the other order (types swapped
# with them: the same crystal)
def inputs(synth_files):
    sic = tsn.case_sic()
    return {
        "dimer": (SIC, ["Si"], tsn.case_dimer()),
        "trimer": (SIC, ["Si"], tsn.case_trimer()),
        "cell8": (SIC, ["Si"], tsn.case_cell8()),
        "a": (SIC, ["Si"], tsn.case_a()),
        "scaled": (SIC, ["Si"], tsn.case_scaled()),
        "gas1": (SIC, ["Si"], tsn.case_gas(1)),
        "triclinic": (SIC, ["Si"], tsn.case_triclinic()),
        "carbon": (SIC, ["C"], tsn.case_a(a=tsn.A_C)),
        "sic": (SIC, ["Si", "C"], sic),
        "sic_cs": (SIC, ["C", "Si"], (sic[0], sic[1], 1 - sic[2])),
        "synth": (synth_files[0], ["X", "Y"], tsn.case_synth()),
        "clamp": (synth_files[1], ["X", "Y"], tsn.case_synth()),
    }


NAMES = ["dimer", "trimer", "cell8", "a", "scaled", "gas1", "triclinic", "carbon", "sic", "sic_cs", "synth", "clamp"]


@pytest.fixture(scope="module")
def refs(lib, synth_files):
    """per input: (numpy object, driver, case, numpy result, driver result), each computed once"""
    out = {}
    for name, (path, el, case) in inputs(synth_files).items():
        ref = tsn.Tersoff(tsn.read_tersoff(path, el)[0])
        drv = Driver(lib, path, el)
        out[name] = (ref, drv, case, ref.compute(*case), drv(*case))
    return out


def same(got, ref, tol=1e-12):
    assert got["npairs"] == ref["npairs"] and got["nzeta"] == ref["nzeta"], (got["npairs"], ref["npairs"], got["nzeta"], ref["nzeta"])
    fs = max(np.abs(ref["f"]).max(), 1e-300)
    assert np.abs(got["f"] - ref["f"]).max() <= tol * fs, np.abs(got["f"] - ref["f"]).max() / fs
    for k in ("e_rep", "e_att"):
        assert abs(got[k] - ref[k]) <= tol * max(abs(ref["e_rep"]), abs(ref["e_att"])), k
    assert np.abs(got["w"] - ref["w"]).max() <= tol * np.abs(ref["w"]).max()


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    ref_ts, drv, case, ref, got = refs[name]
    same(got, ref)
    assert abs(ref["f"].sum(axis=0)).max() < 1e-10 * np.abs(ref["f"]).max()
    if name == "scaled":
        assert ref["maxin"] == 16 and ref["npairs"] == 64 * 16 and ref["nshell"] == 384
    if name == "a":
        assert ref["maxin"] == 4 and ref["nzeta"] == 64 * 12
    if name == "gas1":
        assert 8 <= ref["maxin"] <= 10 and 175 <= ref["nshell"] <= 205
    if name == "clamp":          # both clamps and the large-zeta end of b are reached
        assert got["t"].max() > 1e20
    if name == "sic_cs":         # the same crystal under the other element order: the same numbers
        same(got, refs["sic"][3], tol=1e-13)


def test_energy_loop_equals_compute(refs):
    """the energy-first loop of the numpy helper and the energies its force routine sums"""
    for name in ("trimer", "cell8", "sic", "synth"):
        ref_ts, _, case, ref, _ = refs[name]
        assert abs(ref_ts.energy(*case) - ref["e"]) <= 1e-13 * abs(ref["e_att"])


@pytest.mark.parametrize("name", ["a", "scaled", "sic", "synth"])
@pytest.mark.parametrize("which", ["numpy", "driver"])
def test_forces_are_the_gradient_of_the_energy(refs, name, which):
    """central differences of the energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A"""
    ref_ts, drv, (x, box, t), ref, got = refs[name]
    fn, f = (ref_ts.energy, ref["f"]) if which == "numpy" else (drv.energy, got["f"])
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(6 if which == "driver" else 2):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), (name, which)


@pytest.mark.parametrize("name", ["triclinic", "synth"])
def test_virial_is_the_strain_derivative_of_the_energy(refs, name):
    ref_ts, drv, (x, box, t), ref, got = refs[name]
    h = 1e-6
    for obj, w in ((drv, got["w"]),) + (((ref_ts, ref["w"]),) if name == "synth" else ()):
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            e = np.zeros((3, 3))
            e[a, b] = h
            ep = obj.energy(*tsn.strained(x, box, e), t)
            em = obj.energy(*tsn.strained(x, box, -e), t)
            assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)      # W_ab = sum d_a f_b = -dE/d eps_ab


def test_bond_order_end_forms_equal_the_exact_expression(refs):
    """ts_bond_order switches b and b' to their leading terms below c3, c4 and above c2, c1 (as LAMMPS does); the numpy helper evaluates
    the exact expression everywhere.  The two agree to 1e-12 on every beta zeta the test inputs produce (the static cases and the synthetic file; the
    clamped variant of that file, which drives zeta to both ends on purpose, counts as part of the sweep below c3).  On a sweep across the four
    switch points of every pair of both files b agrees to 1e-12 as well; b' is held to 1e-7 there: below c3 its leading term drops the
    factor (1 + t^n)^(-1 - 1/(2n)), which at t = c3 is 1 - (2n + 1) 1e-8 -- the accuracy the switch points were chosen for"""
    seen = 0
    for name in NAMES:
        ref_ts, drv, (x, box, t), _, got = refs[name]
        types = sorted(set(int(v) for v in t))
        for ti in types:
            for tj in types:
                p = ref_ts.p[(ti, tj, tj)]
                sw = drv.bond_order(ti, tj, 1.0)[2:]
                assert sw[0] > sw[1] > 1.0 > sw[2] > sw[3] > 0.0
                sweep = [s * k for s in sw for k in (0.5, 0.999999, 1.000001, 2.0)] + [0.0]
                # (the clamped file pushes beta zeta below c3 on purpose: its values there belong to the sweep)
                mine = [(v, 1e-7 if name == "clamp" and v < sw[2] else 1e-12) for v in got["t"]]
                for tval, dtol in mine + [(v, 1e-7) for v in sweep]:
                    zeta = tval / p["beta"]
                    b, db = drv.bond_order(ti, tj, zeta)[:2]
                    eb, edb = tsn.bond_order(p, zeta)
                    assert abs(b - eb) <= 1e-12 * eb, (name, tval, b, eb)
                    if tval < sw[3]:          # below c4 (1e-20 for silicon) b' is 0 by construction: for n < 1 the exact one is singular at 0
                        assert db == 0.0 and b == 1.0
                    else:
                        assert abs(db - edb) <= dtol * abs(edb) + 1e-300, (name, tval, db, edb)
                    seen += 1
    assert seen > 5000


def test_g_forms(refs):
    """the textbook form of g subtracts c^2/d^2 and c^2/(d^2 + x^2), both near 3.8e7 for silicon, to get values between 1 and 1e5: its
    rounding is ABSOLUTE, 1.1e-16 * 3.8e7 = 4e-9.  It holds the form without cancellation to 1e-9 of the largest g on the grid, and to
    1e-9 of g itself at the tetrahedral angle, where g = 1e4; the stable form's derivative is its own central difference"""
    for name, ti in (("a", 0), ("carbon", 0), ("synth", 0), ("synth", 1)):
        ref_ts, drv, _, _, _ = refs[name]
        p = ref_ts.p[(ti, ti, ti)]
        grid = np.linspace(-1.0, 1.0, 401)
        gmax = max(tsn.g_stable(p, c)[0] for c in grid)
        for c in list(grid) + [-1.0 / 3.0]:
            g, dg = drv.g(ti, ti, ti, c)
            assert abs(g - tsn.g_stable(p, c)[0]) <= 1e-14 * g
            assert abs(g - tsn.g_textbook(p, c)) <= 1e-9 * (g if c == -1.0 / 3.0 else gmax), (name, c)
            h = 1e-6
            num = (drv.g(ti, ti, ti, c + h)[0] - drv.g(ti, ti, ti, c - h)[0]) / (2 * h)
            assert abs(num - dg) <= 1e-6 * max(abs(dg), g)


@pytest.mark.parametrize("el,a0,e0", [("Si", 5.432, -4.62959501), ("C", 3.5656, -7.37051421)])
def test_perfect_diamond_closed_form(lib, el, a0, e0):
    p = tsn.read_tersoff(SIC, [el])[0][(0, 0, 0)]
    drv, ref_ts = Driver(lib, SIC, [el]), tsn.Tersoff(tsn.read_tersoff(SIC, [el])[0])
    x, box = tsn.diamond(2, 2, 2, a0)
    t = tsn.zeros(len(x))
    r = a0 * math.sqrt(3.0) / 4.0
    zeta = 3.0 * p["gamma"] * (1.0 + p["c"] ** 2 / p["d"] ** 2 - p["c"] ** 2 / (p["d"] ** 2 + (-1.0 / 3.0 - p["costheta0"]) ** 2))
    b = (1.0 + (p["beta"] * zeta) ** p["n"]) ** (-0.5 / p["n"])
    closed = 2.0 * (p["A"] * math.exp(-p["lambda1"] * r) - b * p["B"] * math.exp(-p["lambda2"] * r))
    assert abs(closed / tsn.EV_TO_KCALMOL - e0) < 1e-8
    for o in (drv(x, box, t), ref_ts.compute(x, box, t)):
        assert abs(o["e"] / len(x) / closed - 1.0) < 1e-9
        assert np.abs(o["f"]).max() < 1e-9 * abs(closed)
        assert o["npairs"] == 4 * len(x) and o["nzeta"] == 12 * len(x)
    # the minimum over a: golden section on the closed form (it is smooth and single-welled between +-5 %)
    lo, hi = 0.95 * a0, 1.05 * a0
    gr = (math.sqrt(5.0) - 1.0) / 2.0
    for _ in range(60):
        m1, m2 = hi - gr * (hi - lo), lo + gr * (hi - lo)
        if tsn.diamond_energy_per_atom(p, m1) < tsn.diamond_energy_per_atom(p, m2):
            hi = m2
        else:
            lo = m1
    assert abs(0.5 * (lo + hi) - a0) < 1e-3, 0.5 * (lo + hi)


def test_cutoff_is_exact_and_continuous(lib):
    """a dimer at R + D - 1e-6, exactly at R + D = 3 A, and beyond: finite, continuous (fC = (pi/2 1e-6 / D)^2 / 4 = 2.7e-11 just
    inside, times a pair term of some 40 kcal/mol), exactly zero from the cutoff on"""
    drv, ref_ts = Driver(lib, SIC, ["Si"]), tsn.Tersoff(tsn.read_tersoff(SIC, ["Si"])[0])
    assert lib.tsh_cutmax(drv.h) == 2.85 + 0.15 == 3.0
    for obj in (drv, ref_ts.compute):
        out = {d: obj(*tsn.case_dimer(3.0 + d)) for d in (-1e-6, 0.0, 1e-6)}
        for d in (0.0, 1e-6):
            assert out[d]["npairs"] == 0 and out[d]["e"] == 0.0 and not out[d]["f"].any() and not out[d]["w"].any()
        o = out[-1e-6]
        assert o["npairs"] == 2 and np.isfinite(o["f"]).all() and 0.0 < abs(o["e"]) < 1e-8 and np.abs(o["f"]).max() < 1e-2
    inside = drv(*tsn.case_dimer(2.3))
    assert inside["nzeta"] == 0 and inside["npairs"] == 2 and list(inside["t"]) == [0.0, 0.0]        # zeta = 0, b = 1
    p = ref_ts.p[(0, 0, 0)]
    assert abs(inside["e"] - (p["A"] * math.exp(-p["lambda1"] * 2.3) - p["B"] * math.exp(-p["lambda2"] * 2.3))) <= 1e-13 * abs(inside["e_att"])


def test_energy_unit(lib):
    """energy_unit 1 takes A and B as written: the energies of unit 0 are 23.060549 times those"""
    x, box, t = tsn.case_a()
    e0, e1 = Driver(lib, SIC, ["Si"])(x, box, t), Driver(lib, SIC, ["Si"], energy_unit=1)(x, box, t)
    assert abs(e0["e"] / e1["e"] / tsn.EV_TO_KCALMOL - 1.0) < 1e-14 and abs(e0["f"] / e1["f"] / tsn.EV_TO_KCALMOL - 1.0).max() < 1e-12


def test_wrong_builds_are_caught(lib, refs, synth_files):
    """the wrong builds of the module docstring fail where it says"""
    def fails(drv, name):
        try:
            same(drv(*refs[name][2]), refs[name][3])
        except AssertionError:
            return True
        return False
    owner = Driver(lib, SIC, ["Si"], wrong=1)
    owner2 = Driver(lib, SIC, ["Si", "C"], wrong=1)
    assert fails(owner, "a") and fails(owner, "scaled") and fails(owner2, "sic")
    x, box = tsn.diamond(2, 2, 2, tsn.A_SIC)
    t = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), 8)
    good = Driver(lib, SIC, ["Si", "C"])(x, box, t)
    assert abs(owner2(x, box, t)["e_att"] / good["e_att"] - 1.0) > 1e-3          # b_SiC != b_CSi even on the perfect lattice
    assert not fails(Driver(lib, SIC, ["Si"], wrong=2), "scaled") and not fails(Driver(lib, SIC, ["Si", "C"], wrong=2), "sic")
    assert fails(Driver(lib, synth_files[0], ["X", "Y"], wrong=2), "synth")
    # 3: the cutoff of the third atom from entry i j j
    assert not fails(Driver(lib, SIC, ["Si"], wrong=3), "scaled") and not fails(Driver(lib, SIC, ["Si"], wrong=3), "gas1")
    bad = Driver(lib, SIC, ["Si", "C"], wrong=3)(*refs["sic"][2])
    assert bad["nzeta"] != refs["sic"][3]["nzeta"]
    assert np.abs(bad["f"] - refs["sic"][3]["f"]).max() > 0.1 * np.abs(refs["sic"][3]["f"]).max()
    assert fails(Driver(lib, SIC, ["Si", "C"], wrong=3), "sic") and fails(Driver(lib, synth_files[0], ["X", "Y"], wrong=3), "synth")
