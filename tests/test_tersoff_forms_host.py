"""The arithmetic of the Tersoff forms tersoff/mod, tersoff/mod/c and tersoff/zbl (scema_amd/csrc/tersoff/ts_core.h, what the instances
k_ts_force<TsModTable, .> and k_ts_force<TsZblTable, .> of md_tersoff.hip run), compiled for the host by
tests/tersoff_forms_host_driver.cpp and held against the independent numpy restatement tests/tersoff_forms_numpy.py: energies, forces and
virial to 1e-12 relative.  The numpy restatement itself is pinned first: its forces and virial against central differences of its own
energy (step and budget of tests/test_tersoff_host.py), the cohesive energy of diamond silicon under the mod fixture, the c0 shift
identity, and the two limits of the ZBL form.  No GPU needed; the `-m gpu` tests of tests/test_gpu_tersoff_forms.py compare the kernels
with the same helper.  No LAMMPS exists here to compare with: parity with it stays unpinned, as for every stage.

Every finite-difference input keeps each pair at least 1e-3 A from every R + D it can be held against (the ZBL energy has a step there,
and so has any energy under a displacement that moves a pair across); the tests assert it on the input (tersoff_forms_numpy.cut_margin).

Wrong builds (tfh_create's `wrong`), tried on this driver; test_wrong_builds_are_caught asserts every line:
  1  the plain fC for the pair in the mod form: passes the dimer below R - D and the jittered 64-atom cell (every bond below R - D = 2.7 A,
     where both are 1); fails the dimer inside the switching region, the scaled cell (384 pairs in the shell) and the gas
  2  eta and 1/(2n) exchanged: passes every input whose zeta is 0 (dimers); fails the synthetic file (eta 0.8 .. 1.3, n 0.9 .. 1.1) and
     also the silicon fixture (eta = 1, 1/(2n) = 0.533) wherever zeta > 0
  3  F left off fA (energy and zeta prefactor alike): the ZBL trimer with arms of 1.0 and 1.2 A (F = 0.67 and 0.97) fails, by more than
     10 % in e_att.  (At crystal distances 1 - F is 6e-9 at 2.3 A: silicon and SiC inputs would show it at the 1e-8 level only.)
  4  F left off the zeta prefactor only: the ZBL trimer's energies agree to 1e-12, its forces are off by more than 1e-3 of the largest
  5  c0 multiplied by b: passes every input of the 17-column fixture (c0 = 0); with the mod/c fixture the shift E(mod/c) - E(mod) is no
     longer 1/2 c0 sum fC
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import hostdrv
import tersoff_forms_numpy as tf
import tersoff_numpy as tsn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MOD, MODC, ZBL, SIC = (os.path.join(GOLD, n) for n in ("Si.tersoff.mod", "Si.tersoff.modc", "SiC.tersoff.zbl", "SiC.tersoff"))


def driver_lib():
    L = C.CDLL(hostdrv.build("libtersoff_forms_host.so", ["tests/tersoff_forms_host_driver.cpp", "scema_amd/csrc/host/tersoff_params.cpp"], shared=True))
    L.tfh_create.restype = C.c_void_p
    L.tfh_create.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]
    L.tfh_destroy.argtypes = [C.c_void_p]
    L.tfh_cutmax.restype = C.c_double
    L.tfh_cutmax.argtypes = [C.c_void_p]
    L.tfh_bond_order.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tfh_g.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tfh_fc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tfh_zbl.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    L.tfh_compute.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
    return L


class Driver:
    def __init__(self, L, form, path, elements, wrong=0, energy_unit=0):
        self.L = L
        arr = (C.c_char_p * len(elements))(*[e.encode() for e in elements])
        self.h = L.tfh_create({"mod": 0, "zbl": 1}[form], path.encode(), arr, len(elements), energy_unit, wrong)
        assert self.h

    def __call__(self, x, box, types):
        n = len(x)
        x = np.ascontiguousarray(x, float); box = np.ascontiguousarray(box, float); t = np.ascontiguousarray(types, np.int32)
        f, e, w, cnt, z, fs = np.zeros((n, 3)), np.zeros(2), np.zeros(6), np.zeros(3, np.int32), np.zeros((n, 32)), np.zeros(1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert self.L.tfh_compute(self.h, n, p(t), p(x), p(box), p(f), p(e), p(w), p(cnt), p(z), p(fs)) == 0
        return dict(f=f, e_rep=e[0], e_att=e[1], e=e[0] + e[1], w=w, npairs=int(cnt[0]), nzeta=int(cnt[1]), maxin=int(cnt[2]), t=z[z >= 0.0], fcsum=fs[0])

    def energy(self, x, box, types):
        return self(x, box, types)["e"]

    def fn(self, name, *args, nout=2):
        out = np.zeros(4)
        getattr(self.L, name)(self.h, *args, out.ctypes.data_as(C.c_void_p))
        return out[:nout]


@pytest.fixture(scope="module")
def lib():
    return driver_lib()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """the synthetic mod/c files, and two variants of the ZBL fixture: `late` (F = 1 to the bit at every crystal distance: r_C = 0.1 A,
    A_F = 60 / A, the clamp is passed from 1.26 A on) and `early` (F = 0 to the bit: r_C = 5 A)"""
    d = tmp_path_factory.mktemp("tersoff_forms")
    (d / "synth.tersoff.modc").write_text(tf.SYNTH_MOD)
    (d / "clamp.tersoff.modc").write_text(tf.SYNTH_MOD_CLAMP)
    text = open(ZBL).read()
    assert text.count(" 0.95 14.0") == 8
    (d / "late.tersoff.zbl").write_text(text.replace(" 0.95 14.0", " 0.1 60.0"))
    (d / "early.tersoff.zbl").write_text(text.replace(" 0.95 14.0", " 5.0 60.0"))
    return {k: str(d / n) for k, n in (("synth", "synth.tersoff.modc"), ("clamp", "clamp.tersoff.modc"), ("late", "late.tersoff.zbl"), ("early", "early.tersoff.zbl"))}


def mod_ref(path, el):
    return tf.TersoffMod(tf.read_mod(path, el)[0])


def zbl_ref(path, el):
    return tf.TersoffZbl(tf.read_zbl(path, el)[0])


# The static inputs, name -> (form, file, elements, case).  Si fixture of the mod form: R - D = 2.7 A, R + D = 3.3 A.
def inputs(files):
    sic = tsn.case_sic(19)
    zt = lambda r1, r2: tf.case_arm_trimer(r1, r2, types=[0, 1, 0])
    return {
        "mod_single": ("mod", MOD, ["Si"], tsn.case_single()),
        "mod_dimer_inner": ("mod", MOD, ["Si"], tsn.case_dimer(2.3)),          # below R - D
        "mod_dimer_shell": ("mod", MOD, ["Si"], tsn.case_dimer(3.1)),          # inside the switching region
        "mod_dimer_cut": ("mod", MOD, ["Si"], tsn.case_dimer(3.3)),            # at R + D to the bit: no pair
        "mod_trimer_h": ("mod", MOD, ["Si"], tf.case_h_trimer()),              # cos theta = h: g = c1, dg = 0
        "mod_trimer_small": ("mod", MOD, ["Si"], tf.case_arm_trimer(2.35, 3.3 - 7e-5)),   # zeta below ca4 (fC = 3e-15 there; 2e-5 from R + D it rounds to -5e-17)
        "mod_trimer_big": ("mod", files["clamp"], ["X", "Y"], tf.case_arm_trimer(2.6, 2.0)),   # zeta beyond ca1 (the clamp of the exponent)
        "mod_cell8": ("mod", MOD, ["Si"], tsn.case_cell8()),
        "mod_a": ("mod", MOD, ["Si"], tsn.case_a()),
        "modc_a": ("mod", MODC, ["Si"], tsn.case_a()),
        "mod_scaled": ("mod", MOD, ["Si"], tsn.case_scaled()),
        "modc_scaled": ("mod", MODC, ["Si"], tsn.case_scaled()),
        "mod_gas": ("mod", MOD, ["Si"], tsn.case_gas(1)),
        "mod_synth": ("mod", files["synth"], ["X", "Y"], tsn.case_synth()),
        "mod_clamp": ("mod", files["clamp"], ["X", "Y"], tsn.case_synth()),
        "zbl_single": ("zbl", ZBL, ["Si"], tsn.case_single()),
        "zbl_dimer_03": ("zbl", ZBL, ["Si"], tsn.case_dimer(0.3)),
        "zbl_dimer_rc": ("zbl", ZBL, ["Si"], tsn.case_dimer(0.95)),            # at r_C exactly: F = 1/2
        "zbl_dimer_23": ("zbl", ZBL, ["Si"], tsn.case_dimer(2.3)),
        "zbl_dimer_cut": ("zbl", ZBL, ["Si"], tsn.case_dimer(3.0)),
        "zbl_trimer": ("zbl", ZBL, ["Si", "C"], zt(1.0, 1.2)),                  # arms around r_C: F = 0.67 and 0.97
        "zbl_cell8": ("zbl", ZBL, ["Si"], tsn.case_cell8()),
        "zbl_a": ("zbl", ZBL, ["Si"], tsn.case_a()),
        "zbl_gas": ("zbl", ZBL, ["Si"], tsn.case_gas(1)),
        "zbl_sic": ("zbl", ZBL, ["Si", "C"], sic),
        "zbl_sic_cs": ("zbl", ZBL, ["C", "Si"], (sic[0], sic[1], 1 - sic[2])),
    }


NAMES = ["mod_single", "mod_dimer_inner", "mod_dimer_shell", "mod_dimer_cut", "mod_trimer_h", "mod_trimer_small", "mod_trimer_big", "mod_cell8", "mod_a", "modc_a",
         "mod_scaled", "modc_scaled", "mod_gas", "mod_synth", "mod_clamp", "zbl_single", "zbl_dimer_03", "zbl_dimer_rc", "zbl_dimer_23", "zbl_dimer_cut",
         "zbl_trimer", "zbl_cell8", "zbl_a", "zbl_gas", "zbl_sic", "zbl_sic_cs"]


@pytest.fixture(scope="module")
def refs(lib, files):
    """per input: (numpy object, driver, case, numpy result, driver result), each computed once"""
    out = {}
    for name, (form, path, el, case) in inputs(files).items():
        ref = mod_ref(path, el) if form == "mod" else zbl_ref(path, el)
        drv = Driver(lib, form, path, el)
        out[name] = (ref, drv, case, ref.compute(*case), drv(*case))
    return out


def _same(got, ref, tol=1e-12):
    assert got["npairs"] == ref["npairs"] and got["nzeta"] == ref["nzeta"], (got["npairs"], ref["npairs"], got["nzeta"], ref["nzeta"])
    if ref["npairs"] == 0:
        assert got["e"] == 0.0 and not got["f"].any() and not got["w"].any() and ref["e"] == 0.0 and not ref["f"].any()
        return
    fs = np.abs(ref["f"]).max()
    assert np.abs(got["f"] - ref["f"]).max() <= tol * fs, np.abs(got["f"] - ref["f"]).max() / fs
    for k in ("e_rep", "e_att"):
        assert abs(got[k] - ref[k]) <= tol * max(abs(ref["e_rep"]), abs(ref["e_att"])), k
    assert np.abs(got["w"] - ref["w"]).max() <= tol * np.abs(ref["w"]).max()
    assert abs(got["fcsum"] - ref["fcsum"]) <= tol * ref["fcsum"]


# ---- 1. the reference ----
def test_counts_under_the_mod_cutoff(refs):
    """the generators of tests/tersoff_numpy.py keep their licence under R + D = 3.3 A: neighbours in range, ordered pairs, ordered (j, k)"""
    want = {"mod_cell8": (4, 32, 96), "mod_a": (4, 256, 768), "mod_scaled": (16, 1024, 15360), "mod_gas": (11, 1490, 9312), "mod_dimer_cut": (0, 0, 0),
            "mod_dimer_shell": (1, 2, 0), "mod_trimer_h": (2, 4, 2)}
    for name, w in want.items():
        ref = refs[name][3]
        assert (ref["maxin"], ref["npairs"], ref["nzeta"]) == w, (name, ref["maxin"], ref["npairs"], ref["nzeta"])
        tsn.check_box(refs[name][2][1], tf.MOD_CUT, tf.MOD_CUT + 1.0)
    x, box, t = tsn.case_triclinic()
    tsn.check_box(box, tf.MOD_CUT, tf.MOD_CUT + 1.0)
    o = refs["mod_a"][0].compute(x, box, t)
    assert (o["maxin"], o["npairs"], o["nzeta"]) == (4, 768, 2304)
    s = refs["mod_synth"][3]
    assert s["nzeta"] > 0 and len(set(refs["mod_synth"][2][2])) == 2


FD = ["mod_a", "modc_scaled", "mod_synth", "zbl_a", "zbl_sic", "zbl_trimer"]


@pytest.mark.parametrize("name", FD)
@pytest.mark.parametrize("which", ["numpy", "driver"])
def test_forces_are_the_gradient_of_the_energy(refs, name, which):
    """central differences of the energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A"""
    ref_o, drv, (x, box, t), ref, got = refs[name]
    assert tf.cut_margin(ref_o, x, box, t) >= 1e-3
    fn, f = (ref_o.energy, ref["f"]) if which == "numpy" else (drv.energy, got["f"])
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(6 if which == "driver" else 2):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(fn(x + h * u, box, t) - fn(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), (name, which)


@pytest.mark.parametrize("name", ["mod_synth", "zbl_sic"])
def test_virial_is_the_strain_derivative_of_the_energy(refs, name):
    ref_o, drv, (x, box, t), ref, got = refs[name]
    assert tf.cut_margin(ref_o, x, box, t) >= 1e-3
    h = 1e-6
    for obj, w in ((drv, got["w"]), (ref_o, ref["w"])):
        for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            e = np.zeros((3, 3))
            e[a, b] = h
            ep = obj.energy(*tsn.strained(x, box, e), t)
            em = obj.energy(*tsn.strained(x, box, -e), t)
            assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)


def test_energy_loop_equals_compute(refs):
    for name in ("mod_trimer_h", "mod_cell8", "mod_synth", "zbl_trimer", "zbl_sic"):
        ref_o, _, case, ref, _ = refs[name]
        assert abs(ref_o.energy(*case) - ref["e"]) <= 1e-13 * max(abs(ref["e_att"]), abs(ref["e_rep"]))


def test_diamond_cohesive_energy(lib):
    """diamond at 5.429 A under the mod fixture: -4.630 eV per atom within 1e-3 eV, from the numpy loops, the driver and the closed form
    (four neighbours at a sqrt 3 / 4 < R - D, cos = -1/3, zeta = 3 g(-1/3) exp(0))"""
    p = tf.read_mod(MOD, ["Si"])[0]
    ref_o, drv = tf.TersoffMod(p), Driver(lib, "mod", MOD, ["Si"])
    x, box = tsn.diamond(2, 2, 2, 5.429)
    t = tsn.zeros(len(x))
    q = p[(0, 0, 0)]
    r = 5.429 * math.sqrt(3.0) / 4.0
    b = tf.bond_order_mod(q, 3.0 * tf.g_mod(q, -1.0 / 3.0)[0])[0]
    closed = 2.0 * (q["A"] * math.exp(-q["lambda1"] * r) - b * q["B"] * math.exp(-q["lambda2"] * r))
    assert abs(closed / tf.EV_TO_KCALMOL + 4.630) < 1e-3
    for o in (ref_o.compute(x, box, t), drv(x, box, t)):
        assert abs(o["e"] / len(x) / closed - 1.0) < 1e-12 and o["npairs"] == 4 * len(x) and o["nzeta"] == 12 * len(x)
        assert np.abs(o["f"]).max() < 1e-9 * abs(closed)


@pytest.mark.parametrize("pair", [("mod_a", "modc_a"), ("mod_scaled", "modc_scaled")])
def test_c0_shifts_the_energy_by_half_c0_sum_fc(refs, pair):
    """E(mod/c) - E(mod) = 1/2 c0 sum over the ordered pairs of fC(r_ij), in the part without b; the part with b and the forces inside
    R - D do not move.  The scaled cell has 384 pairs inside the switching region, where fC < 1 and the c0 term has a force"""
    c0 = tf.read_mod(MODC, ["Si"])[0][(0, 0, 0)]["c0"]
    assert c0 == -0.0251 * tf.EV_TO_KCALMOL
    for k in (3, 4):          # numpy, driver
        a, b = refs[pair[0]][k], refs[pair[1]][k]
        assert abs((b["e_rep"] - a["e_rep"]) - 0.5 * c0 * a["fcsum"]) <= 1e-13 * abs(a["e_rep"])
        assert b["e_att"] == a["e_att"] and b["fcsum"] == a["fcsum"]
        moved = np.abs(b["f"] - a["f"]).max()
        assert (moved == 0.0) if pair[0] == "mod_a" else (moved > 1e-6 * np.abs(a["f"]).max())
    assert refs[pair[0]][3]["fcsum"] < refs[pair[0]][3]["npairs"] or pair[0] == "mod_a"


def test_zbl_limits(lib, files):
    """A_F = 60 / A and r_C = 0.1 A: F = 1 to the bit from 1.26 A on, and ZBL equals plain Tersoff to 1e-12 (jittered SiC, shortest pair
    1.6 A).  r_C = 5 A: F = 0 to the bit below 3.8 A, and the energy is the pure ZBL pair energy of the pairs inside R + D"""
    x, box, t = tsn.case_sic(19)
    plain = tsn.Tersoff(tsn.read_tersoff(SIC, ["Si", "C"])[0]).compute(x, box, t)
    for obj in (zbl_ref(files["late"], ["Si", "C"]).compute, Driver(lib, "zbl", files["late"], ["Si", "C"])):
        o = obj(x, box, t)
        assert o["npairs"] == plain["npairs"] and o["nzeta"] == plain["nzeta"]
        assert np.abs(o["f"] - plain["f"]).max() <= 1e-12 * np.abs(plain["f"]).max()
        assert abs(o["e_rep"] - plain["e_rep"]) <= 1e-12 * abs(plain["e_att"]) and abs(o["e_att"] - plain["e_att"]) <= 1e-12 * abs(plain["e_att"])
        assert np.abs(o["w"] - plain["w"]).max() <= 1e-12 * np.abs(plain["w"]).max()
    early = zbl_ref(files["early"], ["Si", "C"])
    pure = tf.zbl_pair_energy(early, x, box, t)
    for obj in (early.compute, Driver(lib, "zbl", files["early"], ["Si", "C"])):
        o = obj(x, box, t)
        assert o["e_att"] == 0.0 and abs(o["e_rep"] - pure) <= 1e-13 * pure and pure > 0.0


# ---- 2. ts_core.h on the host against the reference ----
@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    ref_o, drv, case, ref, got = refs[name]
    _same(got, ref)
    if ref["npairs"]:
        assert abs(ref["f"].sum(axis=0)).max() < 1e-10 * np.abs(ref["f"]).max()
    if name in ("mod_dimer_cut", "zbl_dimer_cut", "mod_single", "zbl_single"):
        assert ref["npairs"] == 0
        if "dimer" in name:
            assert case[0][1, 0] - case[0][0, 0] == lib_cut(drv)
    if name == "mod_dimer_shell":
        assert 0.0 < ref["fcsum"] < 2.0
    if name == "mod_trimer_small":          # zeta below ca4: b = 1 and no force from zeta
        q = ref_o.p[(0, 0, 0)]
        assert 0.0 < got["t"][0] < tf.mod_switch(q)[1] and got["nzeta"] == 2          # (the pair of the short arm, first in list order)
    if name == "mod_trimer_big":            # zeta beyond ca1
        assert got["t"].max() > tf.mod_switch(ref_o.p[(0, 0, 0)])[0]
    if name == "mod_clamp":
        assert got["t"].max() > 1e20
    if name == "zbl_sic_cs":
        _same(got, refs["zbl_sic"][3], tol=1e-13)
    if name == "zbl_trimer":                # Z_i != Z_j, both arms near r_C
        assert len(set(case[2])) == 2 and ref["npairs"] == 6


def lib_cut(drv):
    return drv.L.tfh_cutmax(drv.h)


def test_functions_of_the_mod_form(refs):
    """fC: 1 and 0 at the ends of the shell, its derivative its own central difference, first AND second derivative zero at both ends (the
    reason for the form); g at cos = h is c1 to the bit with dg = 0, elsewhere the numpy value to 1e-14 and dg its central difference
    (c4 = 0 in the entry Y X Y of the synthetic file takes the branch without the exponential); b against the exact expression across
    both switch points"""
    ref_o, drv = refs["mod_a"][0], refs["mod_a"][1]
    q = ref_o.p[(0, 0, 0)]
    fc = lambda r: drv.fn("tfh_fc", 0, 0, r)
    assert list(fc(2.0)) == [1.0, 0.0] and fc(2.7)[0] == 1.0 and abs(fc(2.7)[1]) < 1e-15
    assert abs(fc(3.3 - 1e-9)[0]) < 1e-30 + 1e-16 and abs(fc(3.3 - 1e-9)[1]) < 1e-12
    for r in np.linspace(2.7, 3.3, 61)[1:-1]:
        v, d = fc(r)
        assert abs(v - tf.fc_mod(q, r)[0]) <= 1e-14 and abs(d - tf.fc_mod(q, r)[1]) <= 1e-13
        num = (fc(r + 1e-6)[0] - fc(r - 1e-6)[0]) / 2e-6
        assert abs(num - d) < 1e-8
    assert abs(fc(2.7 + 1e-4)[1]) < 1e-5 and abs(fc(3.3 - 1e-4)[1]) < 1e-5          # f' ~ delta^2 at the lower end, ~ delta^3 at the upper
    g, dg = drv.fn("tfh_g", 0, 0, 0, q["h"])
    assert g == q["c1"] and dg == 0.0
    for name, (i, j, k) in (("mod_a", (0, 0, 0)), ("mod_synth", (0, 0, 0)), ("mod_synth", (1, 0, 1)), ("mod_synth", (1, 1, 1))):
        o, d = refs[name][0], refs[name][1]
        p = o.p[(i, j, k)]
        for c in np.linspace(-1.0, 1.0, 201):
            g, dg = d.fn("tfh_g", i, j, k, c)
            assert abs(g - tf.g_mod(p, c)[0]) <= 1e-14 * g and abs(dg - tf.g_mod(p, c)[1]) <= 1e-13 * max(abs(dg), g)
            num = (d.fn("tfh_g", i, j, k, c + 1e-6)[0] - d.fn("tfh_g", i, j, k, c - 1e-6)[0]) / 2e-6
            assert abs(num - dg) <= 1e-6 * max(abs(dg), g)
    assert refs["mod_synth"][0].p[(1, 0, 1)]["c4"] == 0.0
    seen = 0
    for name, (i, j) in (("mod_a", (0, 0)), ("mod_synth", (0, 0)), ("mod_synth", (0, 1)), ("mod_synth", (1, 0)), ("mod_synth", (1, 1))):
        o, d = refs[name][0], refs[name][1]
        p = o.p[(i, j, j)]
        out = np.zeros(4)
        d.L.tfh_bond_order(d.h, i, j, 1.0, out.ctypes.data_as(C.c_void_p))
        ca1, ca4 = out[2], out[3]
        assert abs(ca1 / tf.mod_switch(p)[0] - 1.0) < 1e-12 and ca1 > 1.0 > ca4 > 0.0
        sweep = [s * k for s in (ca1, ca4) for k in (0.5, 0.999999, 1.000001, 2.0)] + list(np.logspace(-12, 12, 49)) + list(refs[name][4]["t"])
        for tval in sweep:
            zeta = tval / p["beta_ters"]
            d.L.tfh_bond_order(d.h, i, j, zeta, out.ctypes.data_as(C.c_void_p))
            assert abs(out[0] - tf.bond_order_mod_exact(p, zeta)) <= 1e-12 * out[0], (name, tval)
            nb, ndb = tf.bond_order_mod(p, zeta)
            assert abs(out[0] - nb) <= 1e-14 * nb and abs(out[1] - ndb) <= 1e-13 * abs(ndb)
            if ca4 < tval < ca1:
                hz = 1e-6 * zeta
                num = (tf.bond_order_mod_exact(p, zeta + hz) - tf.bond_order_mod_exact(p, zeta - hz)) / (2 * hz)
                assert abs(num - out[1]) <= 1e-6 * abs(num) + 1e-9 * out[0] / zeta
            seen += 1
    assert seen > 300


def test_functions_of_the_zbl_form(refs):
    """F = 1/2 at r_C to the bit, F and V_ZBL against numpy, their derivatives their own central differences; Z_i != Z_j"""
    ref_o, drv = refs["zbl_sic"][0], refs["zbl_sic"][1]
    assert drv.fn("tfh_zbl", 0, 0, 0.95, nout=4)[0] == 0.5
    for i, j in ((0, 0), (0, 1), (1, 0), (1, 1)):
        p = ref_o.p[(i, j, j)]
        for r in (0.1, 0.3, 0.7, 0.95, 1.2, 2.0, 2.9):
            F, dF, v, dv = drv.fn("tfh_zbl", i, j, r, nout=4)
            assert abs(F - tf.fermi(p, r)[0]) <= 1e-14 * F and abs(dF - tf.fermi(p, r)[1]) <= 1e-13 * abs(dF) + 1e-300
            assert abs(v - tf.v_zbl(p, r)[0]) <= 1e-14 * v and abs(dv - tf.v_zbl(p, r)[1]) <= 1e-13 * abs(dv)
            lo, hi = drv.fn("tfh_zbl", i, j, r - 1e-6, nout=4), drv.fn("tfh_zbl", i, j, r + 1e-6, nout=4)
            assert abs((hi[0] - lo[0]) / 2e-6 - dF) <= 1e-6 * max(abs(dF), F) and abs((hi[2] - lo[2]) / 2e-6 - dv) <= 1e-6 * abs(dv)
    assert ref_o.p[(0, 1, 1)]["Z_i"] == 14 and ref_o.p[(0, 1, 1)]["Z_j"] == 6
    # past the clamp of the exponent F is 0: r_C - r > 69.0776 / A_F = 4.93 A cannot happen below r_C = 0.95 A, so through a scaled file
    assert tf.fermi(dict(ZBLexpscale=100.0, ZBLcut=0.95), 0.2) == (0.0, 0.0)


def test_energy_unit(lib):
    """energy_unit 1 takes A, B (and c0) as written and, for ZBL, K / 0.043365121: mod energies scale by 23.060549 as a whole; for ZBL the
    Tersoff part does and the Coulomb part by 23.060549 * 0.043365121 (1.0000249...), seen on the dimer at 0.3 A where F = 1e-4"""
    x, box, t = tsn.case_a()
    e0, e1 = Driver(lib, "mod", MODC, ["Si"])(x, box, t), Driver(lib, "mod", MODC, ["Si"], energy_unit=1)(x, box, t)
    assert abs(e0["e"] / e1["e"] / tf.EV_TO_KCALMOL - 1.0) < 1e-14 and abs(e0["f"] / e1["f"] / tf.EV_TO_KCALMOL - 1.0).max() < 1e-12
    d = tsn.case_dimer(0.3)
    z0, z1 = Driver(lib, "zbl", ZBL, ["Si"])(*d), Driver(lib, "zbl", ZBL, ["Si"], energy_unit=1)(*d)
    ref1 = tf.TersoffZbl(tf.read_zbl(ZBL, ["Si"], energy_unit=1)[0]).compute(*d)
    assert abs(z1["e_rep"] - ref1["e_rep"]) <= 1e-12 * ref1["e_rep"]
    ref0 = tf.TersoffZbl(tf.read_zbl(ZBL, ["Si"], energy_unit=0)[0]).compute(*d)
    assert abs(z0["e_rep"] - ref0["e_rep"]) <= 1e-12 * ref0["e_rep"]
    ratio = z0["e_rep"] / z1["e_rep"]          # (mostly Coulomb: 23.060549 * 0.043365121 = 1.0000235, the rest of the way to 1.00008 is F fC fR)
    assert 1.00002 < ratio < 1.0002 and abs(ref0["e_rep"] / ref1["e_rep"] - ratio) < 1e-12


def test_wrong_builds_are_caught(lib, refs, files):
    """the wrong builds of the module docstring pass and fail where it says"""
    def fails(drv, name):
        try:
            _same(drv(*refs[name][2]), refs[name][3])
        except AssertionError:
            return True
        return False
    # 1: the plain fC for the pair
    w1 = Driver(lib, "mod", MOD, ["Si"], wrong=1)
    assert not fails(w1, "mod_dimer_inner") and not fails(w1, "mod_a")
    assert fails(w1, "mod_dimer_shell") and fails(w1, "mod_scaled") and fails(w1, "mod_gas")
    # 2: eta and 1/(2n) exchanged
    w2, w2s = Driver(lib, "mod", MOD, ["Si"], wrong=2), Driver(lib, "mod", files["synth"], ["X", "Y"], wrong=2)
    assert not fails(w2, "mod_dimer_inner") and not fails(w2, "mod_dimer_shell")
    assert fails(w2s, "mod_synth") and fails(w2, "mod_a")
    # 3: F left off fA
    w3 = Driver(lib, "zbl", ZBL, ["Si", "C"], wrong=3)
    bad, ref = w3(*refs["zbl_trimer"][2]), refs["zbl_trimer"][3]
    assert fails(w3, "zbl_trimer") and abs(bad["e_att"] / ref["e_att"] - 1.0) > 0.1
    # 4: F left off the zeta prefactor: the energy is right, the forces are not
    w4 = Driver(lib, "zbl", ZBL, ["Si", "C"], wrong=4)
    bad = w4(*refs["zbl_trimer"][2])
    es = max(abs(ref["e_rep"]), abs(ref["e_att"]))
    assert abs(bad["e_rep"] - ref["e_rep"]) <= 1e-12 * es and abs(bad["e_att"] - ref["e_att"]) <= 1e-12 * es
    assert np.abs(bad["f"] - ref["f"]).max() > 1e-3 * np.abs(ref["f"]).max() and fails(w4, "zbl_trimer")
    assert not fails(w4, "zbl_dimer_rc")          # (no third atom: no zeta)
    # 5: c0 multiplied by b
    w5, w5c = Driver(lib, "mod", MOD, ["Si"], wrong=5), Driver(lib, "mod", MODC, ["Si"], wrong=5)
    assert not fails(w5, "mod_a") and not fails(w5, "mod_scaled")
    c0 = refs["modc_a"][0].p[(0, 0, 0)]["c0"]
    a, b = w5(*refs["mod_a"][2]), w5c(*refs["mod_a"][2])
    assert abs((b["e_rep"] - a["e_rep"]) - 0.5 * c0 * a["fcsum"]) > 0.1 * abs(0.5 * c0 * a["fcsum"])
    assert fails(w5c, "modc_a")
