"""The numpy references of the Tersoff and embedded-atom stages (tests/tersoff_numpy.py, tests/eam_numpy.py) and the host-compiled cores
(tests/tersoff_host_driver.cpp, tests/eam_host_driver.cpp) on the inputs of tests/test_gpu_tersoff_edges.py and tests/test_gpu_eam_edges.py,
where they do what no earlier case asked of them: lists of 15 to 32 entries, entries beyond the pair's own cutoff that serve as third atoms
only, boxes narrower than one cutoff (an atom pairs with its own image, j and k of a zeta term are two images of one atom), tilted cells two
images deep, files of four elements read under a permuted, a thinned and a many-to-one element list, atoms above and below rhomax in one
cell.  No GPU needed; the pattern is that of tests/test_sw_edges_host.py.

  * the counts the GPU tests rely on, pinned in COUNTS (Tersoff: most entries kept, ordered pairs, ordered (j, k); EAM: most neighbours,
    ordered pairs, atoms above rhomax);
  * supercell identity: the cell repeated 3 x 3 x 3 is the same crystal -- E / 27, W / 27 and the forces on the first n atoms equal the
    single cell's to 1e-12.  For Tersoff the supercell is wider than two cutoffs: no atom meets an image of itself and the minimum image
    suffices; for the embedded-atom cells (cutoff 5.5 A) it is 9.9 A wide and more: one image deep where the cell is two, no self-image;
  * forces against central differences of the reference's own energy, h = 1e-5 A, at the tolerance of tests/test_tersoff_host.py (not
    under the clamped file, where the force is not the gradient of the energy, as tests/tersoff_numpy.py says);
  * the host-compiled cores against the references at 1e-12;
  * a fourth wrong build of the Tersoff driver, the neighbour list cut at the pair's own R + D instead of cutin: it passes every earlier
    input, case_synth among them (none has an entry with R + D of the pair <= r < cutin), and fails on the shell case, which has 60.
"""
import numpy as np
import pytest

import eam_numpy as en
import tersoff_numpy as tsn
import test_eam_host as eh
import test_tersoff_host as th

SIC, CUAG = th.SIC, eh.CUAG

# Tersoff: (most entries kept in a list, ordered pairs, ordered (j, k))
TS_COUNTS = {"crowded15": (15, 92, 530), "crowded16": (16, 108, 680), "crowded17": (17, 116, 752), "crowded31": (31, 324, 3426),
             "crowded32": (32, 346, 3780), "crowded33": (33, 378, 4338), "crowded33_far": (7, 194, 968),
             "shell": (16, 624, 4984), "shell_clamp": (16, 624, 4984),
             "N1": (6, 6, 30), "N2": (14, 28, 364), "N3": (7, 26, 144), "N4": (8, 30, 198), "N5": (8, 28, 174), "N6": (7, 22, 97), "N7": (5, 14, 52),
             "count1024": (4, 3880, 11170)}
THIRD_ONLY = {"synth": 0, "shell": 60, "shell_clamp": 60}
# embedded atom: (most neighbours of an atom, ordered pairs, atoms above rhomax)
EAM_COUNTS = {"four": (54, 1644, 0), "four_perm": (54, 1644, 0), "four_sub": (54, 1644, 0), "four_dup": (54, 1644, 0), "partly": (57, 1764, 11),
              "count15": (9, 106, 0), "count16": (9, 120, 0), "count17": (9, 128, 0), "count64": (23, 1092, 0),
              "tilted+": (60, 240, 0), "tilted-": (60, 240, 0), "hot": (32, 234, 0)}
COUNTS = {"tersoff": TS_COUNTS, "eam": EAM_COUNTS}
CROWDED_FAR = 3.4          # the radius of the shell that leaves the centre of case_crowded without a neighbour


# ---------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("row_edges")
    (d / "synth.tersoff").write_text(tsn.SYNTH)
    (d / "clamp.tersoff").write_text(tsn.SYNTH_CLAMP)
    en.write_johnson(str(d / "four.eam.alloy"), en.FOUR)
    en.write_johnson(str(d / "CuLow.eam.alloy"), ["Cu"], rhomax_over_rhoe=1.1)
    return {k: str(d / v) for k, v in (("synth", "synth.tersoff"), ("clamp", "clamp.tersoff"), ("four", "four.eam.alloy"), ("low", "CuLow.eam.alloy"))}


def ts_inputs(files):
    """name -> (file, elements, case) of every new static Tersoff input"""
    out = {f"crowded{k}": (SIC, ["Si"], tsn.case_crowded(k)) for k in (15, 16, 17, 31, 32)}
    out["crowded33_far"] = (SIC, ["Si"], tsn.case_crowded(33, CROWDED_FAR))
    out["shell"] = (files["synth"], ["X", "Y"], tsn.case_shell())
    out["shell_clamp"] = (files["clamp"], ["X", "Y"], tsn.case_shell())
    for name in ("N1", "N2", "N3", "N4", "N5", "N7"):
        out[name] = (SIC, ["Si"], tsn.narrow(name))
    out["N6"] = (files["synth"], ["X", "Y"], tsn.narrow("N6"))
    out["count1024"] = (SIC, ["Si"], tsn.case_count(1024))
    return out


# the element lists under which the four-element cell is read: the file's order; a permutation (types renamed with it: the same crystal);
# Cu and Ag alone, which skips X1 in the middle of the file; three LAMMPS types on two elements
FOUR_PERM = ["X2", "Cu", "X1", "Ag"]


def four_variants():
    x, box, t = en.case_four(4)
    perm_t = np.array([FOUR_PERM.index(en.FOUR[v]) for v in t])
    return {"four": (en.FOUR, (x, box, t)), "four_perm": (FOUR_PERM, (x, box, perm_t)),
            "four_sub": (["Cu", "Ag"], (x, box, t % 2)), "four_dup": (["Cu", "Ag", "Cu"], en.case_four(3))}


def eam_inputs(files):
    """name -> (file, elements, case) of every new static embedded-atom input"""
    out = {k: (files["four"], el, case) for k, (el, case) in four_variants().items()}
    out["partly"] = (files["low"], ["Cu"], en.case_partly_above())
    for n in (15, 16, 17, 64):
        out[f"count{n}"] = (CUAG, ["Cu"], en.case_count(n))
    out["tilted+"] = (CUAG, ["Cu"], en.case_cell4_tilted(+1))
    out["tilted-"] = (CUAG, ["Cu"], en.case_cell4_tilted(-1))
    out["hot"] = (CUAG, ["Cu"], en.case_hot_gas())
    return out


@pytest.fixture(scope="module")
def ts_refs(files):
    """per input: (numpy object, case, numpy result), each computed once"""
    out = {}
    for name, (path, el, case) in ts_inputs(files).items():
        ref = tsn.Tersoff(tsn.read_tersoff(path, el)[0])
        out[name] = (ref, case, ref.compute(*case))
    return out


@pytest.fixture(scope="module")
def eam_refs(files):
    out = {}
    for name, (path, el, case) in eam_inputs(files).items():
        tab, tmap = en.read_setfl(path, el)
        ref = en.EAM(tab)
        x, box, t = case
        mapped = (x, box, np.array(tmap)[t])          # the reference indexes its tables by element, the type map applied here
        out[name] = (ref, mapped, ref.compute(*mapped))
    return out


TS_NAMES = sorted(ts_inputs({"synth": "", "clamp": ""}))
EAM_NAMES = ["four", "four_perm", "four_sub", "four_dup", "partly", "count15", "count16", "count17", "count64", "tilted+", "tilted-", "hot"]


# ---------------------------------------------------------------- counts and conditions
def test_pinned_counts_tersoff(ts_refs, files):
    for name, (ref, case, out) in ts_refs.items():
        assert (out["maxin"], out["npairs"], out["nzeta"]) == TS_COUNTS[name], name
        assert out["maxin"] <= 32
    si = ts_refs["N1"][0]
    c33 = si.compute(*tsn.case_crowded(33))
    assert (c33["maxin"], c33["npairs"], c33["nzeta"]) == TS_COUNTS["crowded33"]
    assert len(si.neighbours(*tsn.case_crowded(33, CROWDED_FAR))[0]) == 0          # the centre has no neighbour
    for k in (15, 16, 17, 31, 32, 33):
        x = tsn.case_crowded(k)[0]
        assert (np.linalg.norm(x[1:] - x[0], axis=1) < tsn.SI_CUT).sum() == k
    # entries at or beyond the pair's own R + D that are third atoms only: none in case_synth, 60 in the shell case
    synth = tsn.Tersoff(tsn.read_tersoff(files["synth"], ["X", "Y"])[0])
    assert tsn.third_only(synth, *tsn.case_synth()) == THIRD_ONLY["synth"]
    for name in ("shell", "shell_clamp"):
        assert tsn.third_only(ts_refs[name][0], *ts_refs[name][1]) == THIRD_ONLY[name] >= 30
    assert len(set(ts_refs["shell"][1][2])) == 2 and len(set(ts_refs["N6"][1][2])) == 2


def test_pinned_counts_eam(eam_refs):
    for name, (ref, case, out) in eam_refs.items():
        assert (out["maxin"], out["npairs"], out["nabove"]) == EAM_COUNTS[name], (name, out["maxin"], out["npairs"], out["nabove"])
    n = len(eam_refs["partly"][1][0])
    assert 0 < EAM_COUNTS["partly"][2] < n
    rho = eam_refs["partly"][2]["rho"] / eam_refs["partly"][0].rhomax
    assert np.abs(rho - 1.0).min() > 1e-3          # no atom sits on rhomax: the count does not hang on rounding
    assert sorted(set(eam_refs["four"][1][2])) == [0, 1, 2, 3] and sorted(set(eam_refs["four_dup"][1][2])) == [0, 1]
    # the permuted list names the same crystal: the same numbers
    eh.same(eam_refs["four_perm"][2], eam_refs["four"][2], tol=1e-13)


def test_conditions_on_the_boxes():
    """the Tersoff boxes: at least one width below the cutoff of 3.0 A (an atom within reach of its own image), every width at or above
    the 2.0 A below which the engine refuses; tilts of both signs.  The embedded-atom cells: every width between 3.25 A and the list
    radius 6.5 A (two images deep), |xy| = 0.45 lx; the hot gas 3.4 A wide"""
    for name in ("N1", "N2", "N3", "N4", "N5", "N6", "N7"):
        w = tsn.widths(tsn.narrow(name)[1])
        assert 2.0 <= w.min() < tsn.SI_CUT, (name, w)
    assert np.allclose(tsn.widths(tsn.narrow("N4")[1]), [2.68, 4.65, 5.6], atol=0.01) and tsn.narrow("N4")[1][6] == 1.3
    assert np.allclose(tsn.widths(tsn.narrow("N5")[1]), [2.79, 4.65, 5.6], atol=0.01) and tsn.narrow("N5")[1][6] == -1.3
    with pytest.raises(AssertionError):
        tsn.check_box(np.array([0.0, 0.0, 0.0, 1.99, 3.3, 3.4, 0.0, 0.0, 0.0]))
    for sign in (+1, -1):
        box = en.case_cell4_tilted(sign)[1]
        w = en.check_box(box)
        assert (w > 3.25).all() and (w < 6.5).all() and abs(box[6] - sign * 0.45 * (box[3] - box[0])) < 1e-12
    assert abs(en.widths(en.case_hot_gas()[1]).min() - 3.4) < 1e-12
    for gen in (lambda: tsn.narrow("N2"), lambda: tsn.narrow("N5"), tsn.case_shell, en.case_hot_gas, en.case_four, en.case_partly_above):
        a, b = gen(), gen()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])          # deterministic


# ---------------------------------------------------------------- supercell identity
@pytest.mark.parametrize("name", ["N1", "N2", "N3", "N4", "N5", "N6", "N7"])
def test_supercell_identity_tersoff(ts_refs, name):
    ref, (x, box, t), one = ts_refs[name]
    xs, bs, ts = tsn.supercell(x, box, t)
    assert (tsn.widths(bs) >= 2 * ref.cutmax).all()      # no atom of the supercell is within the cutoff of an image of itself
    big = ref.compute(xs, bs, ts)
    n = len(x)
    assert big["npairs"] == 27 * one["npairs"] and big["nzeta"] == 27 * one["nzeta"] and big["maxin"] == one["maxin"]
    es = max(abs(one["e_rep"]), abs(one["e_att"]))
    de = max(abs(big["e_rep"] / 27 - one["e_rep"]), abs(big["e_att"] / 27 - one["e_att"])) / es
    dw = np.abs(big["w"] / 27 - one["w"]).max() / np.abs(one["w"]).max()
    # (N1: the net force on the one atom is zero by symmetry; the scale is the largest single pair term)
    fs = max(np.abs(one["f"]).max(), tsn.fterm(ref, x, box, t) if name == "N1" else 0.0)
    df = np.abs(big["f"][:n] - one["f"]).max() / fs
    print(f"tersoff supercell {name}: energy {de:.1e}, forces {df:.1e}, virial {dw:.1e}")
    assert de <= 1e-12 and df <= 1e-12 and dw <= 1e-12


@pytest.mark.parametrize("name", ["tilted+", "tilted-", "hot"])
def test_supercell_identity_eam(eam_refs, name):
    ref, (x, box, t), one = eam_refs[name]
    xs, bs, ts = tsn.supercell(x, box, t)
    assert (en.widths(bs) > ref.cutoff).all() and en.widths(box).min() < ref.cutoff      # self-images in the cell, none in the supercell
    big = ref.compute(xs, bs, ts)
    n = len(x)
    assert big["npairs"] == 27 * one["npairs"] and big["maxin"] == one["maxin"] and big["nabove"] == 27 * one["nabove"]
    es = max(abs(one["e_pair"]), abs(one["e_embed"]))
    de = max(abs(big["e_pair"] / 27 - one["e_pair"]), abs(big["e_embed"] / 27 - one["e_embed"])) / es
    dw = np.abs(big["w"] / 27 - one["w"]).max() / np.abs(one["w"]).max()
    df = np.abs(big["f"][:n] - one["f"]).max() / np.abs(one["f"]).max()
    print(f"eam supercell {name}: energy {de:.1e}, forces {df:.1e}, virial {dw:.1e}")
    assert de <= 1e-12 and df <= 1e-12 and dw <= 1e-12


# ---------------------------------------------------------------- central differences
def _central(energy, f, x, box, t, scale, nvec):
    rng = np.random.default_rng(3)
    h = 1e-5
    for _ in range(nvec):
        u = rng.normal(size=x.shape)
        u /= np.linalg.norm(u)
        num = -(energy(x + h * u, box, t) - energy(x - h * u, box, t)) / (2 * h)
        assert abs(num - np.sum(f * u)) < 1e-6 * scale


@pytest.mark.parametrize("name", ["crowded17", "crowded32", "shell", "N1", "N2", "N3", "N4", "N5", "N6", "N7"])
def test_forces_are_the_gradient_of_the_energy_tersoff(ts_refs, name):
    """as tests/test_tersoff_host.py: truncation h^2 f''' / 6 ~ 1e-10 f, rounding 1e-16 E / h.  Moving an atom moves its images with it: in
    N1 every direction is a rigid translation, so the energy must not change and the force is zero"""
    ref, (x, box, t), one = ts_refs[name]
    scale = max(np.abs(one["f"]).max(), tsn.fterm(ref, x, box, t) if name == "N1" else 0.0)
    _central(ref.energy, one["f"], x, box, t, scale, 2 if name in ("shell", "crowded32") else 4)
    if name == "N1":
        assert np.abs(one["f"]).max() < 1e-12 * scale


@pytest.mark.parametrize("name", ["four", "four_dup", "partly", "tilted+", "tilted-", "hot"])
def test_forces_are_the_gradient_of_the_energy_eam(eam_refs, name):
    ref, (x, box, t), one = eam_refs[name]
    _central(ref.energy, one["f"], x, box, t, np.abs(one["f"]).max(), 2)


# ---------------------------------------------------------------- the host-compiled cores
@pytest.fixture(scope="module")
def ts_lib():
    return th.driver_lib()


@pytest.fixture(scope="module")
def eam_lib():
    return eh.driver_lib()


@pytest.mark.parametrize("name", TS_NAMES)
def test_host_compiled_tersoff_core(ts_lib, ts_refs, files, name):
    """ts_core.h in the loop structure of k_ts_force -- the list inside cutin, pass 1, pass 2 -- against the reference at 1e-12"""
    path, el, case = ts_inputs(files)[name]
    ref, _, want = ts_refs[name]
    got = th.Driver(ts_lib, path, el)(*case)
    assert got["maxin"] == want["maxin"]
    if name == "N1":      # zero net force: compare on the scale of the terms
        assert np.abs(got["f"]).max() <= 1e-12 * tsn.fterm(ref, *case)
        got["f"] = want["f"]
    th.same(got, want)
    if name == "shell_clamp":          # both clamps and the large-zeta end of b are reached here too
        assert got["t"].max() > 1e20


@pytest.mark.parametrize("name", EAM_NAMES)
def test_host_compiled_eam_core(eam_lib, eam_refs, files, name):
    """eam_core.h with the product's reader -- which applies the element list itself: the LAMMPS types go in unmapped -- at 1e-12"""
    path, el, case = eam_inputs(files)[name]
    got = eh.Driver(eam_lib, path, el)(*case)
    assert got["maxin"] == eam_refs[name][2]["maxin"]
    eh.same(got, eam_refs[name][2])


def test_list_cut_at_the_pair_cutoff_is_caught(ts_lib, ts_refs, files):
    """wrong build 4 of tests/tersoff_host_driver.cpp: the neighbour list cut at the pair's own R + D instead of cutin.  Every earlier input
    passes -- no entry of theirs lies between the two, case_synth's bonds end at 2.8 A and its next shell starts at 3.84 A -- and the shell
    case fails under both synthetic files, in the count of (j, k) and in the forces.  The three older wrong builds fail where they did
    (tests/test_tersoff_host.py::test_wrong_builds_are_caught) and on the shell case as well, whose i j k entries carry their own R, D"""
    def fails(got, want):
        try:
            th.same(got, want)
        except AssertionError:
            return True
        return False
    old = th.inputs((files["synth"], files["clamp"]))
    for name in th.NAMES:
        path, el, case = old[name]
        want = tsn.Tersoff(tsn.read_tersoff(path, el)[0]).compute(*case)
        assert not fails(th.Driver(ts_lib, path, el, wrong=4)(*case), want), name
    for name in ("shell", "shell_clamp"):
        path, el, case = ts_inputs(files)[name]
        want = ts_refs[name][2]
        bad = th.Driver(ts_lib, path, el, wrong=4)(*case)
        assert bad["npairs"] == want["npairs"] and bad["nzeta"] < want["nzeta"]          # the pairs are all there, third atoms are missing
        if name == "shell":          # (under the clamped file exp(40 (r_ij - r_ik)) of a third atom 1.2 A beyond the bond is 2e-21: the count alone differs)
            assert np.abs(bad["f"] - want["f"]).max() > 1e-2 * np.abs(want["f"]).max() and abs(bad["e_att"] - want["e_att"]) > 1e-4 * abs(want["e_att"])
        assert fails(bad, want)
        for wrong in (1, 2, 3):
            assert fails(th.Driver(ts_lib, path, el, wrong=wrong)(*case), want), (name, wrong)
        assert not fails(th.Driver(ts_lib, path, el)(*case), want)


# ---------------------------------------------------------------- dynamics: the reference's own reordering noise
def hot_velocities(n, temp, seed, mass):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3)) * np.sqrt(tsn.BOLTZ * temp / mass / tsn.MVV2E)
    return v - v.mean(axis=0)


NVE_STEPS = 40


def nve_case(kind):
    """(positions, box, types, masses, velocities) of the three runs with rebuilds: 300 K, seed 42"""
    if kind == "hot":
        x, box, t = en.case_hot_gas()
        return x, box, t, (en.CU_MASS,), hot_velocities(len(x), 300.0, 42, en.CU_MASS)
    x, box, t = tsn.narrow(kind)
    return x, box, t, (tsn.SI_MASS,), hot_velocities(len(x), 300.0, 42, tsn.SI_MASS)


def moved_and_outside(x0, xr, box):
    s = (xr - box[:3]) @ np.linalg.inv(tsn.h_matrix(box))
    return np.linalg.norm(xr - x0, axis=1).max(), int(((s < 0.0) | (s >= 1.0)).any(axis=1).sum())


@pytest.mark.parametrize("kind", ["N3", "N7", "hot"])
def test_reordering_noise_of_the_reference_trajectories(ts_refs, eam_refs, kind):
    """the runs of the GPU tests on the reference alone: the largest move passes half the skin of 1 A, so the rows are rebuilt in mid-run;
    N7 and the copper gas end with an atom outside the box.  The same run with the atoms permuted differs by the reference's own
    rounding, amplified by the trajectory: it must stay 100 times below the budgets of 1e-9 A and 1e-11 A/fs"""
    ref = eam_refs["hot"][0] if kind == "hot" else ts_refs[kind][0]
    x, box, t, masses, v = nve_case(kind)
    xr, vr = ref.nve(x, v, box, t, masses, 1.0, NVE_STEPS)
    moved, outside = moved_and_outside(x, xr, box)
    perm = np.random.default_rng(5).permutation(len(x))
    xp, vp = ref.nve(x[perm], v[perm], box, np.asarray(t)[perm], masses, 1.0, NVE_STEPS)
    nx, nv = np.abs(xp - xr[perm]).max(), np.abs(vp - vr[perm]).max()
    print(f"reference nve {kind}, {NVE_STEPS} steps: largest move {moved:.3f} A, {outside} atom(s) outside, reordering noise {nx:.1e} A, {nv:.1e} A/fs")
    assert moved > 0.5 and (outside >= 1 or kind == "N3")
    assert nx <= 1e-11 and nv <= 1e-13
