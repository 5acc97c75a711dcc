"""The Vashishta arithmetic of the product (scema_amd/csrc/vashishta/vs_core.h, the functions the HIP kernel of md_vashishta.hip runs, with
the tables of host/vashishta_params.cpp), compiled for the host as the stand-alone program tests/vashishta_host_driver.cpp and held
against the independent numpy restatement tests/vashishta_numpy.py: energies, forces and virial to 1e-12 relative, the numpy forces
against central differences of the numpy energy, the cohesive energy of zincblende SiC, the pair term at its cutoff.  No GPU needed: this
is where every derivative is pinned; the `-m gpu` tests then compare the kernel's output with the same helper.  No LAMMPS exists here to
compare with: parity with `pair_style vashishta` is unpinned.

Cohesive energy: with the numbers of tests/golden/SiC.vashishta zincblende SiC at a = 4.3581 A has -6.34014 eV per atom, the 6.34 eV of
Vashishta et al. (2007); a slip in the form or in a number of the fixture shows there.

Dimers "next to rc" stand 0.05 A inside it: there E2' ~ U''(rc) 0.05 A while its two terms U'(r), U'(rc) are each ~ U''(rc) 7 A, so the
rounding of the difference is 1e-16 x 150 of the result, inside 1e-12; at 1e-6 A it would be 1e-16 x 7e6 and say nothing about the code.

Wrong builds of the driver (-DVSH_WRONG=k, switches of the driver, not of the product), each with the case that fails:
  1  the shift terms left out ...................... dimer Si-C between r0 and rc (energy and force), every lattice
  2  r0, gamma of an arm from entry i j k .......... the synthetic file (its i j k entries write 0 there); tests/golden/SiC.vashishta
                                                     passes: its live triplets are the entries i j j themselves
  3  Zi Zj without its sign ........................ dimer Si-C, the 8-atom cell
  4  the pair energy in full at both ends .......... every case with a pair (energy only: forces and virial are not doubled)
  5  1 + C dc^2 missing from the derivative ........ the trimer (C = 5), jittered lattices; the perfect 8-atom cell passes (dc = 0)
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import hostdrv
import vashishta_numpy as vn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIC = os.path.join(ROOT, "tests", "golden", "SiC.vashishta")


def driver_exe(wrong=0):
    return hostdrv.build(f"vashishta_host_driver_{wrong}", ["tests/vashishta_host_driver.cpp", "scema_amd/csrc/host/vashishta_params.cpp"], shared=False,
                         defines=(f"VSH_WRONG={wrong}",))


def _run(exe, path, elements, x, box, types, energy_unit=0):
    text = f"{len(x)}\n" + " ".join(repr(float(b)) for b in box) + "\n"
    text += "".join(f"{int(t)} {float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for t, p in zip(types, x))
    out = subprocess.run([exe, path, str(energy_unit)] + list(elements), input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    head = out[0].split()
    f = np.array([[float(v) for v in line.split()] for line in out[2:2 + len(x)]])
    e2, e3 = float(head[0]), float(head[1])
    return dict(e2=e2, e3=e3, e=e2 + e3, npairs=int(head[2]), ntriplets=int(head[3]), maxin=int(head[4]), w=np.array([float(v) for v in out[1].split()]), f=f)


@pytest.fixture(scope="module")
def synth_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("vashishta") / "synth.vashishta"
    p.write_text(vn.SYNTH)
    return str(p)


SI, C_ = 0, 1
PAIRS = {"SiSi": (SI, SI), "CC": (C_, C_), "SiC": (SI, C_)}


def _inputs(synth_file):
    """name -> (file, elements, case): every static input of the CPU tests"""
    out = {}
    for pn, (a, b) in PAIRS.items():
        for rn, r in (("inside_r0", 2.0), ("between", 4.0), ("next_to_rc", vn.RC_SIC - 0.05)):
            out[f"dimer_{pn}_{rn}"] = (SIC, ["Si", "C"], vn.case_dimer(a, b, r))
    out["trimer_r0"] = (SIC, ["Si", "C"], vn.case_trimer())
    out["trimer"] = (SIC, ["Si", "C"], vn.case_trimer(r1=2.1))
    out["cell8"] = (SIC, ["Si", "C"], vn.case_cell8())
    out["cell8j"] = (SIC, ["Si", "C"], vn.case_cell8_jittered())
    out["jitter64"] = (SIC, ["Si", "C"], vn.case_jitter(2, 1))
    out["jitter216"] = (SIC, ["Si", "C"], vn.case_jitter(3, 2))
    out["synth"] = (synth_file, ["X", "Y"], vn.case_synth())
    return out


@pytest.fixture(scope="module")
def refs(synth_file):
    """per input: (numpy object, file, elements, case, numpy result, driver result), each computed once"""
    exe = driver_exe()
    out = {}
    for name, (path, el, case) in _inputs(synth_file).items():
        p, _, K = vn.read_vashishta(path, el)
        ref = vn.Vashishta(p, K)
        out[name] = (ref, path, el, case, ref.compute(*case), _run(exe, path, el, *case))
    return out


# what differs beyond 1e-12 of the largest force component, energy term and virial component of ref, or, forces and virial, of `scale` (the
# perfect cell, whose forces and virial cancel, is measured on its jittered twin)
mismatch = functools.partial(hostdrv.mismatch, counters=("npairs", "ntriplets", "maxin"), energies=("e2", "e3"), tol=1e-12)


NAMES = [f"dimer_{p}_{r}" for p in PAIRS for r in ("inside_r0", "between", "next_to_rc")] + ["trimer_r0", "trimer", "cell8", "cell8j", "jitter64", "jitter216", "synth"]


@pytest.mark.parametrize("name", NAMES)
def test_static_cases_match_numpy(refs, name):
    _, _, _, case, ref, got = refs[name]
    assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and np.isfinite(got["e"])
    scale = refs["cell8j"][4] if name == "cell8" else ref
    assert mismatch(got, ref, scale=scale) == [], mismatch(got, ref, scale=scale)
    assert abs(ref["f"].sum(axis=0)).max() <= 1e-10 * max(np.abs(scale["f"]).max(), 1e-300)
    if name in ("cell8", "cell8j"):
        assert (ref["maxin"], ref["npairs"], ref["ntriplets"], ref["maxrc"]) == (4, 8 * 158, 8 * 6, 158)
    if name.startswith("dimer"):
        assert ref["npairs"] == 2 and ref["ntriplets"] == 0
    if name == "trimer_r0":      # the arm at r0 - 1e-6: exp(-1e6) = 0 times a derivative of -1e12, finite
        assert ref["ntriplets"] == 1 and ref["maxin"] == 2 and got["e3"] == 0.0
    if name == "trimer":
        assert ref["e3"] > 0.0
    if name == "synth":
        assert ref["ntriplets"] > 64 and ref["e3"] > 0.0


def test_cohesive_energy_of_silicon_carbide(refs):
    ref = refs["cell8"][4]
    ecoh = ref["e"] / 8.0 / vn.EV_TO_KCALMOL
    print(f"zincblende SiC at {vn.A_SIC} A: {ecoh:.6f} eV per atom")
    assert abs(ecoh - (-6.34014)) < 5e-6
    assert np.abs(ref["f"]).max() < 1e-10      # (every atom sits on a centre of tetrahedral symmetry)


@pytest.mark.parametrize("name", ["jitter64", "jitter216", "synth", "trimer"])
def test_numpy_forces_are_the_gradient_of_its_energy(refs, name):
    """central differences of the numpy energy, h = 1e-5 A: truncation h^2 f'''/6 ~ 1e-10 f, rounding 1e-16 E / h ~ 1e-8 kcal/mol/A; every
    input keeps 1e-3 A from every rc and r0, so no pair changes sides within h"""
    ref_vs, _, _, (x, box, t), ref, _ = refs[name]
    assert ref_vs.margin(x, box, t) >= 1e-3
    assert abs(ref_vs.energy(x, box, t) - ref["e"]) <= 1e-13 * max(abs(ref["e2"]), abs(ref["e3"]))
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(3):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(ref_vs.energy(x + h * u, box, t) - ref_vs.energy(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(ref["f"] * u)) < 1e-6 * np.abs(ref["f"]).max(), name


def test_numpy_virial_is_the_strain_derivative_of_its_energy(refs):
    ref_vs, _, _, (x, box, t), ref, _ = refs["synth"]
    h = 1e-6
    for k, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
        e = np.zeros((3, 3))
        e[a, b] = h
        ep = ref_vs.energy(*vn.strained(x, box, e), t)
        em = ref_vs.energy(*vn.strained(x, box, -e), t)
        assert abs(-(ep - em) / (2 * h) - ref["w"][k]) < 1e-5 * np.abs(ref["w"]).max(), k      # W_ab = sum d_a f_b = -dE/d eps_ab


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_pair_term_vanishes_at_its_cutoff(refs, pair):
    """E2 and its force go to 0 at rc (1 - 1e-12); at and beyond rc they are exactly 0 and the pair is not counted (numpy and driver)"""
    ref_vs = refs["cell8"][0]
    a, b = PAIRS[pair]
    exe = driver_exe()
    e, de = ref_vs.e2(a, b, np.array([vn.RC_SIC * (1.0 - 1e-12)]))
    scale = abs(ref_vs.e2(a, b, np.array([4.0]))[0][0])
    assert abs(e[0]) <= 1e-12 * scale and abs(de[0]) <= 1e-9 * scale
    for r in (vn.RC_SIC, vn.RC_SIC + 1e-9, vn.RC_SIC + 1.0):
        case = vn.case_dimer(a, b, r)
        for got in (ref_vs.compute(*case), _run(exe, SIC, ["Si", "C"], *case)):
            assert got["npairs"] == 0 and got["e2"] == 0.0 and got["e3"] == 0.0 and not got["f"].any() and not got["w"].any()
    case = vn.case_dimer(a, b, vn.RC_SIC * (1.0 - 1e-12))
    for got in (ref_vs.compute(*case), _run(exe, SIC, ["Si", "C"], *case)):
        assert got["npairs"] == 2 and abs(got["e2"]) <= 1e-12 * scale and np.abs(got["f"]).max() <= 1e-9 * scale


def test_both_energy_units(refs, tmp_path):
    """energy_unit 1 takes H, D, W and B as written and K = 332.06371: the fixture read that way is another potential (the Coulomb term
    keeps its size, the others are 23 times weaker), and driver and numpy agree on it as they do on the metal reading"""
    _, _, _, case, ref, _ = refs["jitter64"]
    p, _, K = vn.read_vashishta(SIC, ["Si", "C"], energy_unit=1)
    assert K == vn.K_KCALMOL and p[(0, 1, 1)]["H"] == 447.09026
    got = _run(driver_exe(), SIC, ["Si", "C"], *case, energy_unit=1)
    assert mismatch(got, vn.Vashishta(p, K).compute(*case)) == []
    assert abs(got["e"] - ref["e"]) > 1e-2 * abs(ref["e"])


WRONG = {1: ("dimer_SiC_between", ["forces", "energy", "virial"]), 2: ("synth", None), 3: ("dimer_SiC_between", None),
         4: ("dimer_SiSi_between", ["energy"]), 5: ("trimer", None)}
PASSES = {2: "jitter64", 5: "cell8"}      # what a wrong build still passes: why the case named above is needed


@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_wrong_builds_are_caught(refs, wrong):
    exe = driver_exe(wrong)
    name, what = WRONG[wrong]
    _, path, el, case, ref, _ = refs[name]
    bad = mismatch(_run(exe, path, el, *case), ref)
    print(f"wrong build {wrong} on {name}: {bad}")
    assert bad and (what is None or bad == what)
    if wrong in PASSES:
        _, path, el, case, ref, _ = refs[PASSES[wrong]]
        assert mismatch(_run(exe, path, el, *case), ref, scale=refs["cell8j"][4] if PASSES[wrong] == "cell8" else None) == []
