"""The Tersoff kernel (k_ts_force, md_tersoff.hip) where tests/test_gpu_tersoff.py does not take it, against the numpy reference
tests/tersoff_numpy.py, which tests/test_row_edges_host.py licenses on these inputs (supercell identity, central differences, pinned counts,
the host-compiled core):

  1  lists of 15, 16, 17, 31 and 32 entries: the second 16-lane chunk of rowf_filter, the second trip of pass 1, pass 2 over up to 992
     ordered (j, k); the refusal of 33, which leaves the engine and the batch path usable
  2  entries at or beyond the pair's own R + D that serve as third atoms only (fC = 0 in the list): 60 of them in the shell case -- the case
     that catches a list cut at the pair's own cutoff (tests/test_row_edges_host.py::test_list_cut_at_the_pair_cutoff_is_caught)
  3  boxes narrower than one cutoff: an atom's pair with its own image, (j, k) that are two images of one atom (two adds into one slot of
     the LDS table), a partner index equal to the central atom's; boxes tilted with either sign of xy; the refusal below 2.0 A
  4  1 024 atoms, the largest replica on the LDS force table
  5  the state a sheared run leaves behind after a box flip
  6  dynamics with rebuilds in mid-run and an atom that leaves the box, against the numpy stepper
  7  one launch that mixes image search, minimum image, the global-atomics kernel and a two-element table

Budgets are the standing ones of tests/test_gpu_tersoff.py: static parity 1e-10 of the largest force component (or force term), energy
term and virial component, NVE 1e-9 A and 1e-11 A/fs, sampled pressure 1e-10, a batch against each member alone 1e-9.  Each static check
prints its errors and the longest row against the row capacity.
"""
import numpy as np
import pytest

import rowkit as rk
import tersoff_numpy as tsn
from scema_amd import capi
from test_gpu_tersoff import MASS, SIC, TERSOFF, no_pairs, ref_si, sheared, synth_files  # noqa: F401  (fixtures)
from test_row_edges_host import CROWDED_FAR, NVE_STEPS, THIRD_ONLY, TS_COUNTS, moved_and_outside, nve_case

pytestmark = pytest.mark.gpu

TWO = dict(elements=("X", "Y"), masses=(28.0, 20.0))


_engine, _nts_and_rates = rk.engine, rk.nts_and_rates
_static = rk.static_of(TERSOFF, SIC, ("Si",), MASS)


_check_static = rk.checker(TERSOFF, "tersoff static", tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)      # the static budget of tests/test_gpu_tersoff.py


def _counts(ref):
    return ref["maxin"], ref["npairs"], ref["nzeta"]


def _check_terms(got, ref, fterm, what):
    """the static check where the net force is zero by symmetry: the force error on the scale of the largest single pair term"""
    assert got["npairs"] == ref["npairs"] and got["nzeta"] == ref["nzeta"] and got["maxrow"] <= got["rowcap"]
    es = max(abs(ref["e_rep"]), abs(ref["e_att"]))
    de = max(abs(got["e_rep"] - ref["e_rep"]), abs(got["e_att"] - ref["e_att"]))
    df, dw = np.abs(got["f"] - ref["f"]).max(), np.abs(got["w"] - ref["w"]).max()
    print(f"{what}: force err {df / fterm:.2e} of the largest pair term, energy err {de / es:.2e}, virial err {dw / np.abs(ref['w']).max():.2e}, "
          f"pairs {got['npairs']}, (j, k) {got['nzeta']}, rows {got['maxrow']}/{got['rowcap']}")
    assert df <= 1e-10 * fterm and de <= 1e-10 * es and dw <= 1e-10 * np.abs(ref["w"]).max()


# ---- 1. list lengths ----
@pytest.mark.parametrize("k", [15, 16, 17, 31, 32])
def test_static_parity_list_lengths(ref_si, k):
    x, box, t = tsn.case_crowded(k)
    ref = ref_si.compute(x, box, t)
    assert _counts(ref) == TS_COUNTS[f"crowded{k}"] and ref["maxin"] == k
    _check_static(_static(x, box, t), ref, what=f"tersoff static {k} neighbours")


def test_thirty_three_neighbours_are_refused_and_the_engine_goes_on(ref_si):
    x, box, t = tsn.case_crowded(33)
    assert _counts(ref_si.compute(x, box, t)) == TS_COUNTS["crowded33"]
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        with pytest.raises(capi.EngineError, match="more than 32 neighbours"):
            e.tersoff_compute("si", 1)
        # the same atoms with the shell beyond the cutoff: the centre has no neighbour, the engine is as good as new
        x2, _, _ = tsn.case_crowded(33, CROWDED_FAR)
        e.set_state(3, "si", 1, box, x2, np.zeros_like(x2))
        ref = ref_si.compute(x2, box, t)
        assert _counts(ref) == TS_COUNTS["crowded33_far"]
        _check_static(e.tersoff_compute("si", 1, qp=3), ref, what="tersoff static after a refusal")
    finally:
        e.close()


def test_crowded_update_is_refused_and_leaves_no_state():
    x, box, t = tsn.case_crowded(33)
    L = box[3:6] - box[:3]
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=rk.velocities(np.zeros(len(x), int), MASS, 300.0, 4)))
        sim = capi.make_sim(0, "si", 1, np.array([5e-4 * L[0], 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, dt=1.0, most_recent=capi.QP_NONE)
        with pytest.raises(capi.EngineError, match="more than 32 neighbours"):
            e.strain_batch([sim])
        assert not e.has_state(0, "si", 1)
    finally:
        e.close()


# ---- 2. third atoms only ----
@pytest.mark.parametrize("which", ["synth", "clamp"])
def test_static_parity_third_atom_only(synth_files, which):
    ref_ts = tsn.Tersoff(tsn.read_tersoff(synth_files[which], TWO["elements"])[0])
    x, box, t = tsn.case_shell()
    name = "shell" if which == "synth" else "shell_clamp"
    n3 = tsn.third_only(ref_ts, x, box, t)
    assert n3 == THIRD_ONLY[name] >= 30
    ref = ref_ts.compute(x, box, t)
    assert _counts(ref) == TS_COUNTS[name] and len(set(t)) == 2
    print(f"tersoff shell case ({which}): {n3} entries with R + D of the pair <= r < cutin")
    _check_static(_static(x, box, t, path=synth_files[which], **TWO), ref, what=f"tersoff static shell ({which})")


# ---- 3. narrow and tilted boxes ----
@pytest.mark.parametrize("name", ["N1", "N2", "N3", "N4", "N5", "N6", "N7"])
def test_static_parity_narrow_and_tilted(ref_si, synth_files, name):
    x, box, t = tsn.narrow(name)
    if name == "N6":
        ref_ts = tsn.Tersoff(tsn.read_tersoff(synth_files["synth"], TWO["elements"])[0])
        got = _static(x, box, t, path=synth_files["synth"], **TWO)
    else:
        ref_ts, got = ref_si, _static(x, box, t)
    ref = ref_ts.compute(x, box, t)
    assert _counts(ref) == TS_COUNTS[name]
    if name == "N1":      # one atom and its images: the net force is zero by symmetry, the pair terms set the rounding
        _check_terms(got, ref, tsn.fterm(ref_ts, x, box, t), "tersoff static N1")
    else:
        _check_static(got, ref, what=f"tersoff static {name}")


def test_box_below_half_a_list_radius_is_refused(ref_si):
    """1.99 A against (cutoff + skin) / 2 = 2.0 A: three images deep, which the row entries cannot code; the engine then evaluates N2"""
    thin = np.array([0.0, 0.0, 0.0, 1.99, 3.3, 3.4, 0.0, 0.0, 0.0])
    assert tsn.widths(thin).min() < tsn.SI_RLIST / 2.0 == 2.0
    x, box, t = tsn.narrow("N2")
    e = _engine()
    try:
        e.tersoff_configure("thin", SIC)
        e.tersoff_configure("si", SIC)
        e.register_replica("thin", 1, capi.bare_system(tsn.zeros(1), np.array([[1.0, 1.0, 1.0]]), thin))
        e.register_replica("si", 1, capi.bare_system(t, x, box))
        with pytest.raises(capi.EngineError, match="box width"):
            e.tersoff_compute("thin", 1)
        _check_static(e.tersoff_compute("si", 1), ref_si.compute(x, box, t), what="tersoff static N2 after a refusal")
    finally:
        e.close()


# ---- 4. the largest replica on the LDS force table ----
def test_static_parity_1024_atoms(ref_si):
    x, box, t = tsn.case_count(1024)
    ref = ref_si.compute(x, box, t)
    assert _counts(ref) == TS_COUNTS["count1024"]
    _check_static(_static(x, box, t), ref, what="tersoff static n = 1024")


# ---- 5. a flipped state ----
def test_static_parity_of_a_flipped_state(ref_si, sheared):
    """the last simulation of the sheared set of tests/test_gpu_tersoff.py alone: its box, written with xy = +0.4 lx, passes lx / 2 and
    flips; the forces on the state it leaves, in the box it leaves, against numpy"""
    fresh, sims = sheared[0], sheared[1]
    sim = sims[-1]
    e = fresh()
    try:
        e.strain_batch([sim])
        flips = e.profile()["box_flips"]
        box, x, _ = e.get_state(sim.qp_id, "si", 1)
        print(f"tersoff flipped state: {flips} flip(s), xy {2.0 * tsn.A_SI:.3f} -> {box[6]:.3f} A of lx {box[3] - box[0]:.3f} A")
        assert flips >= 1 and abs(box[6]) <= 0.5 * (box[3] - box[0]) and box[6] < 0.0
        _check_static(e.tersoff_compute("si", 1, qp=sim.qp_id), ref_si.compute(x, box, tsn.zeros(len(x))), what="tersoff static flipped state")
    finally:
        e.close()


# ---- 6. dynamics with rebuilds ----
@pytest.mark.parametrize("name", ["N3", "N7"])
def test_nve_with_rebuilds_in_a_narrow_box(ref_si, name):
    """the four-atom gas in 2.9 x 5.0 x 5.6 A and the three-atom gas in 2.45 x 4.4 x 5.2 A at 300 K, 40 steps: the gases start off
    equilibrium, an atom moves 1.11 A (0.81 A) -- past half the skin, so the rows are rebuilt in mid-run -- and in the second one ends
    outside the box.  The reference's own reordering noise on these runs is below 1e-15 A and 1e-16 A/fs
    (tests/test_row_edges_host.py::test_reordering_noise_of_the_reference_trajectories).  Then one sampled step FROM the reference's end state"""
    x, box, t, masses, v = nve_case(name)
    xr, vr = ref_si.nve(x, v, box, t, masses, 1.0, NVE_STEPS)
    moved, outside = moved_and_outside(x, xr, box)
    assert moved > 0.5 and (outside >= 1 or name == "N3"), (moved, outside)          # (else the test checks nothing new)
    e = _engine()
    try:
        e.tersoff_configure("si", SIC)
        e.register_replica("si", 1, capi.bare_system(t, x, box, v=v))
        e.set_state(0, "si", 1, box, x, v)
        e.debug_run("si", 1, NVE_STEPS, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        builds = e.profile()["neigh_builds"]
        _, xg, vg = e.get_state(0, "si", 1)
        dx = np.abs(tsn.minimage_diff(xg, xr, box)).max()
        print(f"tersoff nve {name}, {NVE_STEPS} steps: {builds} builds, largest move {moved:.2f} A, {outside} atom(s) outside; position difference "
              f"{dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert builds >= 2
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        e.set_state(1, "si", 1, box, xr, vr)
        p = e.debug_run("si", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref_si.nve(xr, vr, box, t, masses, 1.0, 1)
        want = ref_si.pressure_atm(x1, v1, box, t, masses)
        print(f"tersoff sampled pressure {name} (atm): max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


# ---- 7. a launch mixed in kind ----
@pytest.fixture(scope="module")
def mixed(synth_files):
    """Eight simulations (the smallest batch that runs as two parts), two each of N3 (image search, two deep), case (a) (minimum image),
    case_count(1025) (beyond the LDS force table: the launch takes the global-atomics kernel for everyone) and the shell case under the
    two-element file; each material under its own id; 10 straining steps, nss 10; and each one's stress alone in a fresh engine"""
    mats = {"n3": (tsn.narrow("N3"), SIC, ("Si",), MASS), "sia": (tsn.case_a(), SIC, ("Si",), MASS),
            "big": (tsn.case_count(1025), SIC, ("Si",), MASS), "two": (tsn.case_shell(), synth_files["synth"], TWO["elements"], TWO["masses"])}
    vel = {m: rk.velocities(np.zeros(len(c[0][0]), int), MASS, 300.0, 50 + k) for k, (m, c) in enumerate(sorted(mats.items()))}
    sims = []
    for q, m in enumerate(["n3", "sia", "big", "two", "two", "big", "sia", "n3"]):      # (both parts hold every kind)
        L = mats[m][0][1][3:6] - mats[m][0][1][:3]
        ezz = 4e-4 + 5e-5 * q          # norm below 1e-3 = 10 steps of dt 1 at the rate 1e-4
        sims.append((q, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))
        assert _nts_and_rates(sims[-1][2], mats[m][0][1], 1.0, 1e-4)[0] == 10

    def fresh(only=None):
        e = _engine()
        for m, ((x, box, t), path, el, masses) in mats.items():
            if only is None or m == only:
                e.tersoff_configure(m, path, el)
                e.register_replica(m, 1, capi.bare_system(t, x, box, v=vel[m], masses=masses))
        return e

    mk = lambda q, m, s: capi.make_sim(q, m, 1, s, nss=10, dt=1.0, temperature=300.0, strain_rate=1e-4, most_recent=capi.QP_NONE)
    alone = []
    for q, m, s in sims:
        e = fresh(m)
        alone.append(np.array(e.strain_batch([mk(q, m, s)])[0].stress[:]))
        e.close()
    return fresh, [mk(*s) for s in sims], np.array(alone)


def _mixed_batch(mixed, split):
    fresh, sims, alone = mixed
    e = fresh()
    try:
        e.batch_split(split)
        out = np.array([list(o.stress) for o in e.strain_batch(sims)])
        err = np.abs(out - alone).max(axis=1) / np.abs(alone).max(axis=1)
        builds = e.profile()["neigh_builds"]
        print(f"tersoff mixed batch of 8 (split {split}): {builds} builds, rel err per simulation {' '.join('%.1e' % v for v in err)}")
        assert np.isfinite(out).all() and err.max() <= 1e-9
        return builds
    finally:
        e.close()


@pytest.mark.parametrize("split", [0, 1])
def test_mixed_launch_equals_each_alone(mixed, split):
    """The batch against the SAME code in another launch shape: admissible only because test_static_parity_narrow_and_tilted (N3),
    test_static_parity_third_atom_only (the shell case), tests/test_gpu_tersoff.py::test_atom_count_edges (1 025) and its static case (a)
    pin each member's alone path against numpy."""
    _mixed_batch(mixed, split)


def test_mixed_launch_overflows_and_retries(mixed, monkeypatch):
    """the same batch from row capacities forced low (the overflow test hook): every member overflows, the batch regrows and retries"""
    normal = _mixed_batch(mixed, 1)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    assert _mixed_batch(mixed, 1) >= normal + 8          # (the attempt that overflowed built every member's rows once, too)
