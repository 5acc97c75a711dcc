"""The born/coul/long arithmetic of the product (scema_amd/csrc/ionic/bl_core.h, the functions the HIP kernels of md_born_long.hip run, with
the table of host/born_long_params.cpp), compiled for the host as the stand-alone program tests/born_long_host_driver.cpp and held against
the independent numpy restatement tests/born_long_numpy.py: energies, forces and virial to 1e-12 relative (the virial on the scale of its
parts), the numpy forces against central differences of the numpy energy, the virial against the strain derivative of the total energy at
fixed g_ewald and fixed integer triples on neutral and non-neutral cells, the sum against a converged one of the same code, the Madelung
constant, and the k-space set-up of the product (scema_md_born_long_kvectors, a pure host function) against numpy's own copy of the rule.
No GPU needed: this is where every derivative is pinned; the `-m gpu` tests then compare the kernels' output with the same reference.  No
LAMMPS exists here to compare with: parity with `pair_style born/coul/long` + `kspace_style ewald` is unpinned.

Accuracy.  rms force error against the sum at accuracy 1e-12 (its own larger g), bound accuracy * K e^2/A^2: on 8 and 64 rock-salt ions
jittered by sigma = 0.15 A (seed 1) the test prints the fraction of the bound it finds.  Madelung constant of the perfect lattice at
accuracy 1e-5: within 3e-5 of 1.7475646.

Wrong builds of the driver (-DBLH_WRONG=k, switches of the driver, not of the product), each with the check that fails:
  1  the -g/sqrt(pi) term missing ...... the energy of every case and the Madelung value; forces and virial pass (the term has neither)
  2  the half-space factor 1 for 2 ..... energy, forces and virial of every case with a reciprocal part, the Madelung value
  3  the sign of the reciprocal force .. the forces alone: energy and virial pass
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import born_long_numpy as bl
import hostdrv
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NACL = os.path.join(ROOT, "tests", "golden", "NaCl.born_long")
MGO = os.path.join(ROOT, "tests", "golden", "MgO.buck_long")


def driver_exe(wrong=0, flags=(), tag=""):
    return hostdrv.build(f"born_long_host_driver_{wrong}{tag}", ["tests/born_long_host_driver.cpp", "scema_amd/csrc/host/born_long_params.cpp"], shared=False,
                         defines=(f"BLH_WRONG={wrong}",), flags=flags)


def _run(exe, path, x, box, types, q, g, triples, energy_unit=0):
    text = f"{len(x)}\n" + " ".join(repr(float(b)) for b in box) + f"\n{float(g)!r} {len(triples)}\n"
    text += "".join(f"{int(n[0])} {int(n[1])} {int(n[2])}\n" for n in triples)
    text += "".join(f"{int(t)} {float(c)!r} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for t, c, p in zip(types, q, x))
    out = subprocess.run([exe, path, str(energy_unit)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = out[0].split()
    f = np.array([[float(v) for v in line.split()] for line in out[2:2 + len(x)]])
    eb, ec = float(head[0]), float(head[1])
    return dict(e_born=eb, e_coul=ec, e=eb + ec, npairs=int(head[2]), ncoul=int(head[3]), w=np.array([float(v) for v in out[1].split()]), f=f)


def _mgo(case):
    x, box, t, q = case
    return x, box, t, 1.2 * q


def _inputs():
    """name -> (file, case): every static input of the CPU tests"""
    j64 = bl.case_jitter(2, 1)
    return {
        "single": (NACL, bl.case_single()),
        "two": (NACL, bl.case_two()),
        "cell8": (NACL, bl.rocksalt(1, 1, 1)),
        "cell8j": (NACL, bl.case_jitter(1, 1)),
        "cell64": (NACL, bl.rocksalt(2, 2, 2)),
        "jitter64": (NACL, j64),
        "c63": (NACL, bl.case_without(j64, [37])),
        "c65": (NACL, bl.case_with_extra(j64)),
        "slab48": (NACL, bl.case_jitter((1, 2, 3), 3)),
        "triclinic": (NACL, bl.case_triclinic()),
        "mgo": (MGO, _mgo(bl.case_jitter(2, 17, sigma=0.1, a=4.3))),
    }


NAMES = sorted(_inputs())


@pytest.fixture(scope="module")
def refs():
    """per input: (numpy object, file, case, numpy result, driver result, (g, triples) of the PRODUCT's set-up), each computed once"""
    exe = driver_exe()
    out = {}
    for name, (path, case) in _inputs().items():
        ref = bl.BornLong(bl.read_born_long(path))
        x, box, t, q = case
        kv = capi.born_long_kvectors(path, box, len(x), float(np.sum(q * q)))
        g, tr = kv["g_ewald"], kv["triples"]
        out[name] = (ref, path, case, ref.compute(x, box, t, q, g, tr), _run(exe, path, x, box, t, q, g, tr), (g, tr))
    return out


# what differs beyond 1e-12 of the largest force component, energy term (reciprocal and self terms among them) and virial part of ref, or,
# forces and virial, of `scale` (the perfect cell, whose forces cancel, is measured on its jittered twin)
mismatch = functools.partial(hostdrv.mismatch, counters=("npairs", "ncoul"), energies=("e_born", "e_coul"), tol=1e-12,
                             energy_scale=("e_born", "e_coul", "e_recip", "e_self"), virial_parts=("w_born", "w_real", "w_recip"))


def _scale(refs, name):
    return refs[{"cell8": "cell8j", "cell64": "jitter64"}.get(name, name)][3]


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    ref_bl, _, case, ref, got, (g, tr) = refs[name]
    assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and np.isfinite(got["e"])
    scale = _scale(refs, name)
    assert mismatch(got, ref, scale=scale) == [], mismatch(got, ref, scale=scale)
    fs = max(np.abs(scale["f"]).max(), ref_bl.K * 1e-12)
    assert abs(ref["f"].sum(axis=0)).max() <= 1e-10 * fs and abs(got["f"].sum(axis=0)).max() <= 1e-10 * fs      # no net force
    if name == "single":      # self, background and the ion's own images: no force
        assert ref["npairs"] == 0 and ref["e_born"] == 0.0 and ref["e_bg"] < 0.0 and ref["e_recip"] > 0.0
        assert np.abs(got["f"]).max() <= 1e-12 * ref_bl.K and np.abs(ref["f"]).max() <= 1e-12 * ref_bl.K
    if name in ("c63", "c65", "single"):
        assert abs(np.sum(case[3])) == 1.0 and ref["e_bg"] < 0.0
    if name == "cell8":
        assert ref["nk"] == 16 and ref["maxrow"] > 150
    if name == "slab48":
        assert len(case[0]) == 48 and len(set(np.abs(tr).max(axis=0))) == 3      # kmax differs per dimension
    if name == "mgo":
        assert ref_bl.p["style"] == "buck" and ref_bl.p["solver"] == "pppm" and ref_bl.accuracy == 1e-4 and not ref_bl.p["D"].any()
        assert ref_bl.p["cut_lj"][0, 1] == 7.0 and ref_bl.rc == 9.0


@pytest.mark.parametrize("name", ["jitter64", "c63", "c65", "triclinic", "mgo", "two"])
def test_numpy_forces_are_the_gradient_of_its_energy(refs, name):
    """central differences of the numpy energy at fixed g and triples, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h
    ~ 1e-7 kcal/mol/A.  Neither term is shifted at its cutoff, so every input keeps more than h from every cutoff"""
    ref_bl, _, (x, box, t, q), ref, _, (g, tr) = refs[name]
    assert ref_bl.margin(x, box, t) >= 1e-4
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(3):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(ref_bl.compute(x + h * u, box, t, q, g, tr)["e"] - ref_bl.compute(x - h * u, box, t, q, g, tr)["e"]) / (2 * h)
        assert abs(num - np.sum(ref["f"] * u)) < 1e-6 * np.abs(ref["f"]).max(), name


@pytest.mark.parametrize("name", ["jitter64", "c63", "c65", "mgo", "triclinic"])
def test_numpy_virial_is_the_strain_derivative_of_its_energy(refs, name):
    """W_ab = -dE/d eps_ab with E the total energy at fixed g and fixed integer triples (the k-vectors move with the box): the background
    term of a cell that is not neutral is in, the -g/sqrt(pi) term has no derivative"""
    ref_bl, _, (x, box, t, q), ref, _, (g, tr) = refs[name]
    assert ref_bl.margin(x, box, t) >= 1e-4
    h = 1e-6
    ws = max(np.abs(ref[k]).max() for k in ("w_born", "w_real", "w_recip"))
    for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        e = np.zeros((3, 3))
        e[a, b] = h
        xp, bp = bl.strained(x, box, e)
        xm, bm = bl.strained(x, box, -e)
        ep, em = ref_bl.compute(xp, bp, t, q, g, tr)["e"], ref_bl.compute(xm, bm, t, q, g, tr)["e"]
        assert abs(-(ep - em) / (2 * h) - ref["w"][k]) < 1e-5 * ws, (name, k)
    if name in ("c63", "c65"):      # the background term is a visible part of the diagonal
        assert abs(ref["e_bg"]) > 1e-3 * ws


def test_invariance_under_translation(refs):
    ref_bl, path, (x, box, t, q), ref, got, (g, tr) = refs["jitter64"]
    shift = np.array([3.21, -7.7, 0.113])
    ref2, got2 = ref_bl.compute(x + shift, box, t, q, g, tr), _run(driver_exe(), path, x + shift, box, t, q, g, tr)
    for a, b in ((ref2, ref), (got2, got)):
        assert mismatch(a, b, tol=1e-11, scale=ref) == []


@pytest.mark.parametrize("cells,accuracy", [(1, 1e-5), (2, 1e-5), (1, 1e-4), (2, 1e-4)])
def test_force_error_against_the_converged_sum(refs, cells, accuracy):
    """rms force error of the sum at that accuracy against the same code at accuracy 1e-12 (its own larger g): at most accuracy * K"""
    ref_bl = refs["cell8"][0]
    x, box, t, q = bl.case_jitter(cells, 1)
    a, b = bl.BornLong(ref_bl.p, accuracy=accuracy), bl.BornLong(ref_bl.p, accuracy=1e-12)
    fa, fb = a.compute(x, box, t, q), b.compute(x, box, t, q)
    assert fb["g"] > fa["g"] and fb["nk"] > fa["nk"]
    rms = float(np.sqrt(np.mean(np.sum((fa["f"] - fb["f"]) ** 2, axis=1))))
    print(f"{len(x)} ions at accuracy {accuracy:g}: rms force error {rms / (accuracy * ref_bl.K):.2f} of the bound, nk {fa['nk']} against {fb['nk']}")
    assert rms <= accuracy * ref_bl.K


@pytest.mark.parametrize("name", ["cell8", "cell64"])
def test_madelung_constant_of_rock_salt(refs, name):
    ref_bl, _, (x, box, t, q), ref, got, _ = refs[name]
    for who, r in (("numpy", ref), ("driver", got)):
        m = -r["e_coul"] / (len(x) / 2.0) * (bl.A_NACL / 2.0) / ref_bl.K
        print(f"Madelung constant of rock salt, {len(x)} ions, accuracy 1e-5 ({who}): {m:.7f} (exact {bl.MADELUNG_NACL}), off by {abs(m - bl.MADELUNG_NACL):.1e}")
        assert abs(m - bl.MADELUNG_NACL) < 3e-5
    assert np.abs(ref["f"]).max() < 1e-9      # (every ion sits on a centre of symmetry)


@pytest.mark.parametrize("cells,accuracy,nk", [(1, 1e-5, 16), (2, 1e-5, 128), (4, 1e-5, 709), (2, 1e-4, 61)])
def test_k_vectors_of_the_product_are_those_of_the_rule(tmp_path, cells, accuracy, nk):
    """scema_md_born_long_kvectors against numpy's own copy of the rule at a = 5.64 A, rc = 10 A: the same set of triples, g to 1e-14"""
    path = NACL
    if accuracy != 1e-5:
        path = str(tmp_path / "NaCl_1e-4.born_long")
        open(path, "w").write(open(NACL).read().replace("kspace_style ewald 1.0e-5", f"kspace_style ewald {accuracy!r}"))
    x, box, t, q = bl.rocksalt(cells, cells, cells)
    kv = capi.born_long_kvectors(path, box, len(x), float(np.sum(q * q)))
    g, kmax, tr = bl.ewald_rule(box, len(x), float(np.sum(q * q)), 10.0, accuracy)
    print(f"{len(x)} ions at {accuracy:g}: nk {kv['nk']}, g {kv['g_ewald']:.6f}, kmax of the list {kv['kmax']}")
    assert kv["nk"] == len(tr) == nk and len(kv["triples"]) == nk
    assert abs(kv["g_ewald"] - g) <= 1e-14 * g
    assert set(map(tuple, kv["triples"])) == set(map(tuple, tr)) and len(set(map(tuple, tr))) == nk
    assert list(kv["kmax"]) == [int(v) for v in np.abs(tr).max(axis=0)]
    if cells == 1 and accuracy == 1e-5:
        assert abs(g - 0.308215) < 5e-7


def test_k_vectors_are_invariant_under_box_flips():
    """a flip of xy or xz by a box length leaves the lattice and the Cartesian k-vectors where they were: the product's set for the
    flipped box holds the same vectors (up to the choice of the half space), each triple moved by n2 += m n1 or n3 += m n1"""
    x, box, t, q = bl.case_jitter(2, 1, a=6.0)
    L = box[3] - box[0]
    box = box.copy()
    box[6], box[7], box[8] = 0.45 * L, -0.42 * L, 0.1 * L

    def cart(b):
        kv = capi.born_long_kvectors(NACL, b, len(x), float(len(x)))
        K = 2.0 * np.pi * kv["triples"] @ np.linalg.inv(bl.h_matrix(b)).T
        return kv, K

    kv0, K0 = cart(box)
    for idx, m in ((6, -1), (7, 1)):
        fb = box.copy()
        fb[idx] += m * L
        kv1, K1 = cart(fb)
        assert kv1["nk"] == kv0["nk"] > 50 and abs(kv1["g_ewald"] - kv0["g_ewald"]) <= 1e-15
        both = lambda K: set(tuple(np.round(s * k, 9)) for k in K for s in (1.0, -1.0))
        assert both(K0) == both(K1)
        # triple by triple: the vector of (n1, n2, n3) in the old basis is that of the moved triple in the new one
        moved = kv0["triples"].copy()
        moved[:, 1 if idx == 6 else 2] += m * moved[:, 0]
        Km = 2.0 * np.pi * moved @ np.linalg.inv(bl.h_matrix(fb)).T
        assert np.abs(Km - K0).max() <= 1e-12 * np.abs(K0).max()
        assert not np.array_equal(np.sort(kv0["triples"], axis=0), np.sort(kv1["triples"], axis=0))


def test_both_energy_units_describe_one_potential(refs, tmp_path):
    """the fixture's numbers converted to kcal/mol by hand under `units real` give the same energies and forces, up to the rounding of K
    (3e-8 relative, in the Coulomb terms alone), as for born/coul/dsf"""
    _, _, (x, box, t, q), ref, got, (g, tr) = refs["jitter64"]
    lines = []
    for raw in open(NACL):
        w = raw.split("#")[0].split()
        if w and w[0] == "units":
            lines.append("units real\n")
        elif w and w[0] == "pair_coeff":
            v = [float(s) for s in w[3:]]
            for k in (0, 3, 4):
                v[k] *= bl.EV_TO_KCALMOL
            lines.append(" ".join(w[:3] + [repr(s) for s in v]) + "\n")
        else:
            lines.append(raw)
    p = tmp_path / "NaCl_real.born_long"
    p.write_text("".join(lines))
    ref_real = bl.BornLong(bl.read_born_long(str(p)))
    assert ref_real.p["unit"] == 1 and ref_real.K == bl.K_KCALMOL
    got_real = _run(driver_exe(), str(p), x, box, t, q, g, tr, energy_unit=1)
    assert mismatch(got_real, ref_real.compute(x, box, t, q, g, tr)) == []
    assert abs(got_real["e_born"] - got["e_born"]) <= 1e-12 * abs(got["e_born"])
    assert abs(got_real["e_coul"] - got["e_coul"]) <= 1e-7 * abs(got["e_coul"]) and mismatch(got_real, got, tol=1e-7, scale=ref) == []
    r = subprocess.run([driver_exe(), NACL, "1"], input="", capture_output=True, text=True)
    assert r.returncode == 1 and "line 4: units metal contradicts energy unit 1" in r.stderr


def test_the_pair_function_of_the_library_is_the_numpy_one(refs):
    """scema_md_born_long_eval (bl_pair through the C ABI) against numpy at a few distances and both sides of both cutoffs"""
    ref_bl, g = refs["mgo"][0], 0.31
    r = np.array([1.5, 2.1, 6.999999, 7.0, 8.5, 8.999999, 9.0, 9.5])
    eb, ec, fb, fc = capi.born_long_eval(MGO, g, 0, 1, 1.2, -1.2, r)
    wb, dwb = ref_bl.born(0, 1, r)
    wc, dwc = ref_bl.real(g, -1.44, r)
    assert np.abs(eb - wb).max() <= 1e-13 * np.abs(wb).max() and np.abs(ec - wc).max() <= 1e-13 * np.abs(wc).max()
    assert np.abs(fb * r + dwb).max() <= 1e-13 * np.abs(dwb).max() and np.abs(fc * r + dwc).max() <= 1e-13 * np.abs(dwc).max()
    assert eb[3] == 0.0 and eb[2] != 0.0 and ec[6] == 0.0 and ec[5] != 0.0 and fc[7] == 0.0


WRONG = {1: ["energy"], 2: ["forces", "energy", "virial"], 3: ["forces"]}


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_builds_are_caught(refs, wrong):
    exe = driver_exe(wrong)
    for name in ("jitter64", "c63", "mgo"):
        _, path, (x, box, t, q), ref, _, (g, tr) = refs[name]
        bad = mismatch(_run(exe, path, x, box, t, q, g, tr), ref)
        print(f"wrong build {wrong} on {name}: {bad}")
        assert bad == WRONG[wrong]
    ref_bl, path, (x, box, t, q), ref, _, (g, tr) = refs["cell8"]
    m = -_run(exe, path, x, box, t, q, g, tr)["e_coul"] / 4.0 * (bl.A_NACL / 2.0) / ref_bl.K
    print(f"wrong build {wrong}: Madelung value {m:.6f}")
    if wrong == 3:      # (the perfect cell has no force to get wrong)
        assert abs(m - bl.MADELUNG_NACL) < 3e-5
    else:      # (outside the bound of test_madelung_constant_of_rock_salt; the reciprocal part of this cell's energy is small: 8e-5 for build 2)
        assert abs(m - bl.MADELUNG_NACL) > 3e-5
