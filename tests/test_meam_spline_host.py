"""The spline-MEAM arithmetic on the CPU: tests/meam_spline_numpy.py (the independent FP64 restatement) pinned by closed forms, central
differences and symmetries, and scema_amd/csrc/meam_spline/ms_core.h -- the code the kernels of md_meam_spline.hip run -- compiled with g++
as a stand-alone program (tests/meam_spline_host_driver.cpp) held against it on every shape of the GPU list.  No GPU needed.

Budgets: numpy against the driver, the static budgets of the GPU tests (1e-10 of the largest force component, 1e-9 of the largest energy
term and virial component); forces against central differences of the numpy energy with h = 1e-5 A to 1e-6 of the largest force, the
virial against the strain derivative with h = 1e-6 to 1e-5 of its largest component (step and tolerance of tests/test_adp_host.py).
"""
import os
import subprocess

import numpy as np
import pytest

import hostdrv
import meam_spline_numpy as mn
from scema_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TI = os.path.join(ROOT, "tests", "golden", "Ti.meam.spline")
TIO = os.path.join(ROOT, "tests", "golden", "TiO.meam.spline")


def driver_exe(flags=(), tag=""):
    return hostdrv.build("meam_spline_host_driver" + tag, ["tests/meam_spline_host_driver.cpp", "scema_amd/csrc/host/meam_spline_params.cpp"], shared=False,
                         flags=flags)


def run_driver(exe, path, elements, x, box, types, energy_unit=0):
    text = f"{len(x)}\n" + " ".join(repr(float(b)) for b in box) + "\n"
    text += "".join(f"{int(t)} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for t, p in zip(types, x))
    out = subprocess.run([exe, path, str(energy_unit)] + list(elements), input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = out[0].split()
    w9 = np.array([float(v) for v in out[1].split()]).reshape(3, 3)
    f = np.array([[float(v) for v in line.split()] for line in out[2:2 + len(x)]])
    rho = np.array([float(v) for v in out[2 + len(x):2 + 2 * len(x)]])
    return dict(e_pair=float(head[0]), e_embed=float(head[1]), e=float(head[0]) + float(head[1]), npairs=int(head[2]), ntriplets=int(head[3]),
                maxin=int(head[4]), w33=w9, w=np.array([w9[0, 0], w9[1, 1], w9[2, 2], w9[0, 1], w9[0, 2], w9[1, 2]]), f=f, rho=rho)


def shapes():
    """name -> (file, elements, case): every shape of the GPU list (tests/test_gpu_meam_spline.py)"""
    one, two = (TI, ["Ti"]), (TIO, ["Ti", "O"])
    out = {}
    for r in (2.9, 4.0, 5.2, mn.TI_CUT - 0.05, mn.TI_CUT, mn.TI_CUT + 1e-9, mn.TI_KNOT):
        out[f"dimer {r!r}"] = (*one, mn.case_dimer(r))
    for (a, b) in ((0, 0), (0, 1), (1, 1)):
        for r in (2.5, 3.2, 4.5, 4.8):
            out[f"dimer {a}{b} {r}"] = (*two, mn.case_dimer(r, a, b))
    for r2 in (mn.TI_CUT_F - 1e-6, mn.TI_CUT_F, 2.9):
        out[f"trimer {r2!r}"] = (*one, mn.case_trimer(2.6, r2))
    out["collinear"] = (*one, mn.case_collinear())
    out["near-degenerate"] = (*one, mn.case_near_degenerate())
    out["trimer TiO"] = (*two, mn.case_trimer(2.4, 2.7, 95.0, (1, 0, 1)))
    out["compressed"] = (*one, mn.case_bcc(2, 2, 2, 2.8, 0.03, 2))
    for m in (15, 16, 17, 31, 32):
        out[f"cluster {m}"] = (*one, mn.case_cluster(m))
    out["cluster 33"] = (*one, mn.case_cluster(33))
    out["shell 40"] = (*one, mn.case_cluster(6, outer=40))
    out["cell"] = (*one, mn.case_bcc(1, 1, 2, 3.3))
    out["cell jittered"] = (*one, mn.case_bcc(1, 1, 2, 3.3, 0.05))
    out["triclinic"] = (*one, mn.case_triclinic())
    for n in (63, 64, 65):
        out[f"count {n}"] = (*one, mn.case_count(n))
    out["ordered TiO"] = (*two, mn.case_bcc(2, 2, 2, 3.3, 0.06, 3, "ordered"))
    out["random TiO"] = (*two, mn.case_bcc(2, 2, 2, 3.3, 0.06, 4, "random"))
    x, box, t = mn.case_bcc(2, 2, 2, 3.3, 0.06, 4, "random")
    out["random TiO, O Ti"] = (TIO, ["O", "Ti"], (x, box, 1 - t))
    out["random TiO, Ti Ti O"] = (TIO, ["Ti", "Ti", "O"], (x, box, np.where(t == 1, 2, np.arange(len(t)) % 2)))
    out["block 1025"] = (*one, mn.case_block(1025, a=3.8))
    return out


NAMES = sorted(shapes())


@pytest.fixture(scope="module")
def refs():
    """per shape: (numpy object, numpy result, driver result), each computed once"""
    exe = driver_exe()
    out = {}
    for name, (path, el, case) in shapes().items():
        splines, type_map = mn.read_meam_spline(path, el)
        ref = mn.MeamSpline(splines)
        x, box, t = case
        mapped = (x, box, np.asarray(type_map)[t])       # numpy takes elements, the driver LAMMPS types and the pair_coeff list
        out[name] = (ref, ref.compute(*mapped), run_driver(exe, path, el, *case), mapped)
    return out


# ---- the spline, closed forms ----
def _cubic_file(tmp_path, knots, name):
    """an old-format file whose five functions are the cubic p(x) = 0.3 - 1.1 x + 0.7 x^2 - 0.2 x^3 sampled at `knots` with its end slopes
    (phi, rho and f must end with 0 / slope 0: they get (x_last - x)^3 instead, a cubic all the same)"""
    p = lambda x: 0.3 - 1.1 * x + 0.7 * x ** 2 - 0.2 * x ** 3
    dp = lambda x: -1.1 + 1.4 * x - 0.6 * x ** 2
    q = lambda x: (knots[-1] - x) ** 3
    dq = lambda x: -3.0 * (knots[-1] - x) ** 2
    lines = ["# cubic"]
    for val, der in ((q, dq), (q, dq), (p, dp), (q, dq), (p, dp)):
        lines += [str(len(knots)), f"{float(der(knots[0])) + 0.0!r} {float(der(knots[-1])) + 0.0!r}", "skipped"] + [f"{float(x)!r} {float(val(x)) + 0.0!r} 0" for x in knots]
    path = tmp_path / name
    path.write_text("\n".join(lines) + "\n")
    return str(path), p, dp, q, dq


@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
def test_a_clamped_spline_through_a_cubic_is_the_cubic(tmp_path, kind):
    knots = np.linspace(0.5, 3.0, 11) if kind == "uniform" else np.array([0.5, 0.6, 0.9, 1.0, 1.7, 1.75, 2.2, 2.9, 3.0])
    path, p, dp, q, dq = _cubic_file(tmp_path, knots, kind + ".meam.spline")
    tab = capi.meam_spline_read_params(path, ["X"], energy_unit=1)
    assert [f["uniform"] for f in tab["fn"]] == [int(kind == "uniform")] * 5
    xs = np.linspace(knots[0], knots[-1], 401)
    for fn, (val, der) in ((2, (p, dp)), (0, (q, dq))):
        y, dy = capi.meam_spline_eval(path, ["X"], fn, xs, energy_unit=1)
        sp = mn.Spline(knots, val(knots), der(knots[0]), der(knots[-1]))
        ref = np.array([sp(t) for t in xs])
        scale = np.abs(val(xs)).max()
        for got_y, got_d in ((y, dy), (ref[:, 0], ref[:, 1])):      # the library and the numpy restatement alike
            assert np.abs(got_y - val(xs)).max() <= 1e-13 * scale and np.abs(got_d - der(xs)).max() <= 1e-12 * np.abs(der(xs)).max()
        # exactly at a knot the value is y, bit for bit
        yk, _ = capi.meam_spline_eval(path, ["X"], fn, knots, energy_unit=1)
        assert np.array_equal(yk, tab["fn"][fn]["y"]) and np.array_equal(np.array([sp(t)[0] for t in knots]), sp.y)
        # beyond either end: the linear continuation
        out = np.array([knots[0] - 0.7, knots[0] - 1e-9, knots[-1] + 1e-9, knots[-1] + 2.5])
        yo, do = capi.meam_spline_eval(path, ["X"], fn, out, energy_unit=1)
        want = np.where(out < knots[0], val(knots[0]) + der(knots[0]) * (out - knots[0]), val(knots[-1]) + der(knots[-1]) * (out - knots[-1]))
        wand = np.where(out < knots[0], der(knots[0]), der(knots[-1]))
        assert np.abs(yo - want).max() <= 1e-14 * scale and np.array_equal(do, wand + 0.0)
        assert np.abs(np.array([sp(t)[0] for t in out]) - want).max() <= 1e-14 * scale


def test_grid_and_search_agree_bit_for_bit():
    """every uniform function of both fixtures, on a dense set that holds every knot and the points a rounding next to each"""
    seen = 0
    for path, el in ((TI, ["Ti"]), (TIO, ["Ti", "O"])):
        tab = capi.meam_spline_read_params(path, el)
        for k, fn in enumerate(tab["fn"]):
            if not fn["uniform"]:
                continue
            seen += 1
            x = fn["x"]
            xs = np.concatenate([np.linspace(x[0] - 0.5, x[-1] + 0.5, 2001), x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)])
            a, b = capi.meam_spline_eval(path, el, k, xs), capi.meam_spline_eval(path, el, k, xs, search=True)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert seen >= 5


# ---- the triplet sum, closed form ----
def _constant_g_file(tmp_path, cs):
    """TiO.meam.spline with every g replaced by a constant (two knots, slopes 0): c per pair of elements"""
    lines = open(TIO).read().split("\n")
    starts = [k for k, s in enumerate(lines) if s.strip() == "spline3eq"]
    out = lines[:starts[9]]
    for c in cs:
        out += ["spline3eq", "2", "0 0", f"-1 {c!r} 0", f"1 {c!r} 0"]
    path = tmp_path / "constg.meam.spline"
    path.write_text("\n".join(out) + "\n")
    return str(path)


@pytest.mark.parametrize("elements", [("Ti",), ("Ti", "O")])
def test_the_triplet_sum_with_a_constant_g(tmp_path, elements):
    """g = c: the triplet part of rho_i is c ((sum f)^2 - sum f^2) / 2; with two elements and c per pair, the same identity per pair of
    element classes.  Held on the numpy restatement and on the driver (its densities)."""
    cs = (0.7, -0.4, 1.3)
    path = _constant_g_file(tmp_path, cs)
    el = list(elements)
    x, box, t = mn.case_bcc(2, 2, 2, 3.0, 0.1, 7, "random" if len(el) == 2 else None)
    ref = mn.MeamSpline(mn.read_meam_spline(path, el)[0])
    got = ref.compute(x, box, t)
    drv = run_driver(driver_exe(), path, el, x, box, t)
    I, J, D, R, n = ref.ordered_pairs(x, box, t)
    want = np.zeros(n)
    for i in range(n):
        sel = I == i
        tj, r = t[J[sel]], R[sel]
        want[i] = sum(ref.s["rho"][a](q)[0] for a, q in zip(tj, r) if q < ref.cut_rho[a])
        S = [sum(ref.s["f"][a](q)[0] for b, q in zip(tj, r) if b == a and q < ref.cut_f[a]) for a in range(ref.ne)]
        S2 = [sum(ref.s["f"][a](q)[0] ** 2 for b, q in zip(tj, r) if b == a and q < ref.cut_f[a]) for a in range(ref.ne)]
        want[i] += cs[0] * (S[0] ** 2 - S2[0]) / 2.0
        if ref.ne == 2:
            want[i] += cs[1] * S[0] * S[1] + cs[2] * (S[1] ** 2 - S2[1]) / 2.0
    assert got["ntriplets"] > 100 and np.abs(want).max() > 1.0
    assert np.abs(got["rho"] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(drv["rho"] - want).max() <= 1e-12 * np.abs(want).max()


# ---- numpy against the driver ----
@pytest.mark.parametrize("name", NAMES)
def test_numpy_against_the_driver(refs, name):
    ref_obj, ref, got, case = refs[name]
    assert (got["npairs"], got["ntriplets"], got["maxin"]) == (ref["npairs"], ref["ntriplets"], ref["maxin"])
    if ref["npairs"] == 0:
        assert got["e"] == 0.0 and not got["f"].any() and not got["w"].any() and ref["e"] == 0.0 and not ref["f"].any()
        return
    fs, ws, es = np.abs(ref["f"]).max(), np.abs(ref["w"]).max(), max(abs(ref["e_pair"]), abs(ref["e_embed"]))
    if name in ("cell",):       # the perfect cell: forces vanish by symmetry; measured on the scale of its jittered twin
        fs = np.abs(refs["cell jittered"][1]["f"]).max()
    assert np.abs(got["f"] - ref["f"]).max() <= 1e-10 * fs
    assert abs(got["e_pair"] - ref["e_pair"]) <= 1e-9 * es and abs(got["e_embed"] - ref["e_embed"]) <= 1e-9 * es
    assert np.abs(got["w"] - ref["w"]).max() <= 1e-9 * ws
    assert np.abs(got["rho"] - ref["rho"]).max() <= 1e-12 * max(np.abs(ref["rho"]).max(), 1e-3)
    assert abs(ref_obj.energy(*case) - ref["e"]) <= 1e-12 * es


def test_what_the_shapes_reach(refs):
    """the conditions the shapes were chosen for, on the reference alone"""
    U = refs["cell"][0].s["U"][0]
    assert refs["compressed"][1]["rho"].min() > U.x[-1]                       # beyond U's last knot
    far = refs[f"dimer {mn.TI_KNOT!r}"][1]["rho"]
    assert (far > U.x[0]).all() and (far < U.x[1]).all() and (far > 0.0).all()   # below U's first interior knot
    assert refs[f"dimer {mn.TI_CUT!r}"][1]["npairs"] == 0 and refs[f"dimer {mn.TI_CUT + 1e-9!r}"][1]["npairs"] == 0
    assert refs[f"dimer {mn.TI_CUT - 0.05!r}"][1]["npairs"] == 2 and refs["dimer 5.2"][1]["rho"].max() == 0.0 and refs["dimer 5.2"][1]["e_pair"] != 0.0
    assert refs[f"trimer {mn.TI_CUT_F!r}"][1]["ntriplets"] == 0 and refs[f"trimer {mn.TI_CUT_F - 1e-6!r}"][1]["ntriplets"] == 1
    for m in (15, 16, 17, 31, 32, 33):
        assert refs[f"cluster {m}"][1]["maxin"] == m
    for order in ("O Ti", "Ti Ti O"):      # the same crystal under another pair_coeff list: the same forces
        assert np.abs(refs["random TiO, " + order][1]["f"] - refs["random TiO"][1]["f"]).max() <= 1e-12 * np.abs(refs["random TiO"][1]["f"]).max()
    assert refs["shell 40"][1]["maxin"] <= 32 and refs["shell 40"][1]["npairs"] > 2 * 40
    x, box, _ = refs["collinear"][3]
    assert np.dot(x[1] - x[0], x[2] - x[0]) / (np.linalg.norm(x[1] - x[0]) * np.linalg.norm(x[2] - x[0])) == -1.0


# ---- finite differences, symmetries ----
FD_NAMES = ["cell jittered", "triclinic", "random TiO", "cluster 17", "near-degenerate", "trimer 2.9", "compressed"]


@pytest.mark.parametrize("name", FD_NAMES)
def test_forces_are_the_gradient_of_the_energy(refs, name):
    ref_obj, ref, _, (x, box, t) = refs[name]
    h, f = 1e-5, ref["f"]
    rng = np.random.default_rng(11)
    for which in range(3):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(ref_obj.energy(x + h * u, box, t) - ref_obj.energy(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * np.abs(f).max(), (name, which)
    for c in range(3):
        e = np.zeros_like(x)
        e[1, c] = h
        num = -(ref_obj.energy(x + e, box, t) - ref_obj.energy(x - e, box, t)) / (2 * h)
        assert abs(num - f[1, c]) < 1e-6 * np.abs(f).max(), (name, c)


@pytest.mark.parametrize("name", ["cell jittered", "triclinic", "random TiO"])
def test_the_virial_is_the_strain_derivative(refs, name):
    ref_obj, ref, _, (x, box, t) = refs[name]
    h, w = 1e-6, ref["w"]
    for k, (a, b) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        eps = np.zeros((3, 3))
        eps[a, b] = h
        ep, em = ref_obj.energy(*mn.strained(x, box, eps), t), ref_obj.energy(*mn.strained(x, box, -eps), t)
        assert abs(-(ep - em) / (2 * h) - w[k]) < 1e-5 * np.abs(w).max(), (k, w)      # W_ab = -dE/d eps_ab


@pytest.mark.parametrize("name", ["cluster 17", "random TiO", "triclinic"])
def test_symmetries(refs, name):
    """no net force, a symmetric virial, invariance under translation and (free clusters) rotation"""
    ref_obj, ref, _, (x, box, t) = refs[name]
    fs = np.abs(ref["f"]).max()
    assert np.abs(ref["f"].sum(axis=0)).max() <= 1e-10 * fs
    assert np.abs(ref["w33"] - ref["w33"].T).max() <= 1e-10 * np.abs(ref["w33"]).max()
    moved = ref_obj.compute(x + np.array([0.37, -1.21, 2.05]), box, t)
    assert abs(moved["e"] - ref["e"]) <= 1e-11 * abs(ref["e_embed"]) and np.abs(moved["f"] - ref["f"]).max() <= 1e-10 * fs
    if name == "cluster 17":
        a = 0.7
        Q = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, np.cos(0.4), -np.sin(0.4)],
                                                                                                                [0.0, np.sin(0.4), np.cos(0.4)]])
        turned = ref_obj.compute((x - 15.0) @ Q.T + 15.0, box, t)
        assert abs(turned["e"] - ref["e"]) <= 1e-11 * abs(ref["e_embed"]) and np.abs(turned["f"] - ref["f"] @ Q.T).max() <= 1e-10 * fs


def test_energy_units():
    x, box, t = mn.case_count(63)
    a = mn.MeamSpline(mn.read_meam_spline(TI, ["Ti"], 0)[0]).compute(x, box, t)
    b = mn.MeamSpline(mn.read_meam_spline(TI, ["Ti"], 1)[0]).compute(x, box, t)
    exe = driver_exe()
    da, db = run_driver(exe, TI, ["Ti"], x, box, t, 0), run_driver(exe, TI, ["Ti"], x, box, t, 1)
    for p, q in ((a, b), (da, db)):
        assert abs(p["e"] / q["e"] / mn.EV_TO_KCALMOL - 1.0) < 1e-12 and np.abs(p["f"] / q["f"] / mn.EV_TO_KCALMOL - 1.0).max() < 1e-9
