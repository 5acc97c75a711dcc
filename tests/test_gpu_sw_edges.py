"""The Stillinger-Weber kernels (md_rows.hip, md_sw.hip) where tests/test_gpu_sw.py does not take them, against the numpy reference tests/sw_numpy.py, which
tests/test_sw_edges_host.py licenses on these inputs (supercell identity, central differences, pinned counts):

  1  boxes narrower than one list radius: the image search two boxes deep, an atom's pair with its own image (sw_owns with j == i), triplets
     whose two arms are images of one atom; boxes tilted to 0.45 lx in both branches of the row build; the refusal below half a list radius
  2  the state a sheared run leaves behind after a box flip
  3  atom counts next to the tile sizes of the row build (8 rows a wave, 64 a workgroup, 512 staged) and the force kernel (16 groups, the
     LDS force table up to 1 024 atoms); one atom; two atoms
  4  exactly 32 neighbours inside the cutoff (496 triplets around one atom), and the refusal of 33
  5  dynamics with a rebuild in mid-run and atoms that leave the box, against the numpy stepper
  6  one launch that mixes image search, minimum image, the global-atomics force kernel and a two-element table

Budgets are the standing ones of tests/test_gpu_sw.py: static parity 1e-10 of the largest force component (or force term) and energy term,
NVE 1e-9 A and 1e-11 A/fs, sampled pressure 1e-10, a batch against each member alone 1e-9.  The engine does not report the image depth of a
row build; the conditions on the boxes (tests/test_sw_edges_host.py::test_conditions_on_the_boxes) fix it, and each static check prints the
longest row against the row capacity.
"""
import numpy as np
import pytest

import rowkit as rk
import sw_numpy as swn
from scema_amd import capi
from test_gpu_sw import MASS, SI_SW, SW, no_pairs, ref_sw, sheared_cell  # noqa: F401  (ref_sw: a fixture)
from test_sw_edges_host import COUNTS, largest_force_term

pytestmark = pytest.mark.gpu

TWO = dict(elements=("Si", "X"), masses=(swn.SI_MASS, 20.0))


_engine, _nts_and_rates = rk.engine, rk.nts_and_rates
_static = rk.static_of(SW, SI_SW, ("Si",), MASS)


# (fterm=: size of the largest single force term, for configurations near equilibrium, where the terms cancel in the sum)
_check_static = rk.checker(SW, "sw static", tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, no_pairs=no_pairs)


@pytest.fixture(scope="module")
def two_sw(tmp_path_factory):
    p = tmp_path_factory.mktemp("sw_edges") / "two.sw"
    p.write_text(swn.TWO_ELEMENT_SW)
    return str(p), swn.SW(swn.read_sw(str(p), ["Si", "X"])[0])


# ---- 1. static parity, narrow and tilted ----
@pytest.mark.parametrize("name", ["N1", "N2", "N3", "N4", "N5", "T2", "T3"])
def test_static_parity_narrow_and_tilted(ref_sw, two_sw, name):
    x, box, t = swn.tilted(int(name[1])) if name[0] == "T" else swn.narrow(name)
    swn.check_box(box)
    if name == "N5":
        ref = two_sw[1].compute(x, box, t)
        got = _static(x, box, t, path=two_sw[0], **TWO)
    else:
        ref = ref_sw.compute(x, box, t)
        got = _static(x, box, t)
    assert (ref["npairs"], ref["ntriplets"], ref["maxin"]) == COUNTS[name][:3] and ref["maxin"] <= 32
    # (N4: one atom and its images; the net force is zero by symmetry, the pair terms set the rounding)
    _check_static(got, ref, fterm=largest_force_term(ref_sw, x, box, t) if name == "N4" else 0.0)


def test_box_below_half_a_list_radius_is_refused(ref_sw):
    """2.38 A against (cutoff + skin) / 2 = 2.386 A: three images deep, which the row entries cannot code; the engine then evaluates N1"""
    thin = np.array([0.0, 0.0, 0.0, 2.38, 3.3, 3.4, 0.0, 0.0, 0.0])
    assert swn.widths(thin).min() < swn.SI_RLIST / 2.0 < 2.39
    x, box, t = swn.narrow("N1")
    e = _engine()
    try:
        e.sw_configure("thin", SI_SW)
        e.sw_configure("si", SI_SW)
        e.register_replica("thin", 1, capi.sw_system(np.zeros(1, int), np.array([[1.1, 2.3, 0.7]]), thin))
        e.register_replica("si", 1, capi.sw_system(t, x, box))
        with pytest.raises(capi.EngineError, match="box width"):
            e.sw_compute("thin", 1)
        _check_static(e.sw_compute("si", 1), ref_sw.compute(x, box, t))
    finally:
        e.close()


# ---- 2. a flipped state ----
def test_static_parity_of_a_flipped_state(ref_sw):
    """the last simulation of the sheared set of tests/test_gpu_sw.py alone: its box passes xy = lx / 2 and flips; the forces on the state it
    leaves, in the box it leaves, against numpy"""
    fresh, sims, mk, box0 = rk.sheared_set(SW, sheared_cell())
    q, s = sims[-1]
    e = fresh()
    try:
        e.strain_batch([mk(q, s)])
        flips = e.profile()["box_flips"]
        box, x, _ = e.get_state(q, "si", 1)
        print(f"sw flipped state: {flips} flip(s), xy {box0[6]:.3f} -> {box[6]:.3f} A of lx {box[3] - box[0]:.3f} A")
        assert flips >= 1 and abs(box[6]) <= 0.5 * (box[3] - box[0]) and box[6] < 0.0 < box0[6]
        _check_static(e.sw_compute("si", 1, qp=q), ref_sw.compute(x, box, np.zeros(len(x), int)))
    finally:
        e.close()


# ---- 3. atom counts ----
TRUNCATED = {7: (7, 10), 9: (10, 18), 63: (101, 283), 65: (106, 301), 511: (1421, 7200), 513: (1426, 7225), 1024: (3087, 16591), 1025: (3092, 16631)}


@pytest.mark.parametrize("n", sorted(TRUNCATED))
def test_atom_count_edges(ref_sw, n):
    x, box, t = swn.truncated(n)
    ref = ref_sw.compute(x, box, t)
    assert (ref["npairs"], ref["ntriplets"]) == TRUNCATED[n] and ref["maxin"] <= 32
    _check_static(_static(x, box, t), ref)


def test_one_atom_and_two_atoms(ref_sw):
    one = ref_sw.compute(*swn.lone(1))
    assert one["npairs"] == 0 and one["ntriplets"] == 0
    _check_static(_static(*swn.lone(1)), one)          # (exactly zero, all of it)
    two = ref_sw.compute(*swn.lone(2))
    assert two["npairs"] == 1 and two["ntriplets"] == 0
    got = _static(*swn.lone(2))
    _check_static(got, two)
    assert got["e3"] == 0.0


# ---- 4. the 32-neighbour limit ----
def test_thirty_two_neighbours(ref_sw):
    x, box, t = swn.cluster(32)
    ref = ref_sw.compute(x, box, t)
    assert (ref["maxin"], ref["npairs"], ref["ntriplets"]) == (32, 151, 1506)
    _check_static(_static(x, box, t), ref)


def test_thirty_three_neighbours_are_refused(ref_sw):
    x, box, t = swn.cluster(33)
    assert ref_sw.compute(x, box, t)["maxin"] == 33
    e = _engine()
    try:
        e.sw_configure("si", SI_SW)
        e.register_replica("si", 1, capi.sw_system(t, x, box))
        with pytest.raises(capi.EngineError, match="more than 32 neighbours"):
            e.sw_compute("si", 1)
        # the same atoms with the shell beyond the cutoff: the centre has no neighbour, the engine is as good as new
        x2, _, _ = swn.cluster(33, 3.9)
        e.set_state(3, "si", 1, box, x2, np.zeros_like(x2))
        ref = ref_sw.compute(x2, box, t)
        assert ref["maxin"] <= 32 and ref["npairs"] == 115
        _check_static(e.sw_compute("si", 1, qp=3), ref)
    finally:
        e.close()


def test_crowded_update_is_refused_and_leaves_no_state(ref_sw):
    x, box, t = swn.case_a_compressed()
    assert ref_sw.compute(x, box, t)["maxin"] == 33
    L = box[3:6] - box[:3]
    e = _engine()
    try:
        e.sw_configure("si", SI_SW)
        e.register_replica("si", 1, capi.sw_system(t, x, box, v=rk.velocities(np.zeros(len(x), int), MASS, 300.0, 4)))
        sim = capi.make_sim(0, "si", 1, np.array([5e-4 * L[0], 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, dt=1.0, most_recent=capi.QP_NONE)
        with pytest.raises(capi.EngineError, match="more than 32 neighbours"):
            e.strain_batch([sim])
        assert not e.has_state(0, "si", 1)
    finally:
        e.close()


# ---- 5. dynamics with rebuilds ----
def test_nve_with_rebuilds_in_a_narrow_box(ref_sw):
    """N1 at 300 K, 20 steps: the gas starts off equilibrium, an atom moves 0.64 A -- past half the skin, so the rows are rebuilt in
    mid-run, two images deep -- and one ends outside the box.  The reference's own reordering noise on such a run is 9e-16 A and 8e-17 A/fs
    (atoms permuted), far below the budgets.  Then one sampled step FROM the reference's end state, an atom outside the box and all."""
    x, box, t = swn.narrow("N1")
    v = rk.velocities(np.zeros(len(x), int), MASS, 300.0, 42)
    xr, vr = ref_sw.nve(x, v, box, t, MASS, 1.0, 20)
    s = (xr - box[:3]) @ np.linalg.inv(swn.h_matrix(box))
    moved = np.linalg.norm(xr - x, axis=1).max()
    outside = int(((s < 0.0) | (s >= 1.0)).any(axis=1).sum())
    assert moved > 0.5 and outside >= 1, (moved, outside)          # (else the test checks nothing new)
    e = _engine()
    try:
        e.sw_configure("si", SI_SW)
        e.register_replica("si", 1, capi.sw_system(t, x, box, v=v))
        e.set_state(0, "si", 1, box, x, v)
        e.debug_run("si", 1, 20, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        builds = e.profile()["neigh_builds"]
        _, xg, vg = e.get_state(0, "si", 1)
        dx = np.abs(swn.minimage_diff(xg, xr, box)).max()
        print(f"sw nve N1, 20 steps: {builds} builds, largest move {moved:.2f} A, {outside} atom(s) outside; position difference {dx:.2e} A, "
              f"velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert builds >= 2
        assert dx < 1e-9 and np.abs(vg - vr).max() < 1e-11
        e.set_state(1, "si", 1, box, xr, vr)
        p = e.debug_run("si", 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref_sw.nve(xr, vr, box, t, MASS, 1.0, 1)
        want = ref_sw.pressure_atm(x1, v1, box, t, MASS)
        print(f"sw sampled pressure N1 (atm): max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
    finally:
        e.close()


# ---- 6. a launch mixed in kind ----
@pytest.fixture(scope="module")
def mixed(two_sw):
    """Eight simulations (the smallest batch that runs as two parts), two each of N1 (image search, two deep), case (a) (minimum image),
    truncated(1025) (beyond the LDS force table: the launch takes the global-atomics force kernel for everyone) and case (e) under the
    two-element file; each material under its own id; 10 straining steps, nss 10; and each one's stress alone in a fresh engine"""
    mats = {"n1": (swn.narrow("N1"), SI_SW, ("Si",), MASS), "sia": (swn.case_a(), SI_SW, ("Si",), MASS),
            "big": (swn.truncated(1025), SI_SW, ("Si",), MASS), "two": (swn.case_e(), two_sw[0], TWO["elements"], TWO["masses"])}
    vel = {m: rk.velocities(np.zeros(len(c[0][0]), int), MASS, 300.0, 50 + k) for k, (m, c) in enumerate(sorted(mats.items()))}
    sims = []
    for q, m in enumerate(["n1", "sia", "big", "two", "two", "big", "sia", "n1"]):      # (both parts hold every kind but one)
        L = mats[m][0][1][3:6] - mats[m][0][1][:3]
        ezz = 4e-4 + 5e-5 * q          # norm below 1e-3 = 10 steps of dt 1 at the rate 1e-4
        sims.append((q, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))
        assert _nts_and_rates(sims[-1][2], mats[m][0][1], 1.0, 1e-4)[0] == 10

    def fresh(only=None):
        e = _engine()
        for m, ((x, box, t), path, el, masses) in mats.items():
            if only is None or m == only:
                e.sw_configure(m, path, el)
                e.register_replica(m, 1, capi.sw_system(t, x, box, v=vel[m], masses=masses))
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
        print(f"sw mixed batch of 8 (split {split}): {builds} builds, rel err per simulation {' '.join('%.1e' % v for v in err)}")
        assert np.isfinite(out).all() and err.max() <= 1e-9
        return builds
    finally:
        e.close()


@pytest.mark.parametrize("split", [0, 1])
def test_mixed_launch_equals_each_alone(mixed, split):
    """The batch against the SAME code in another launch shape: admissible only because test_static_parity_narrow_and_tilted (N1),
    test_atom_count_edges (1 025) and the static cases of tests/test_gpu_sw.py (a, e) pin each member's alone path against numpy."""
    _mixed_batch(mixed, split)


def test_mixed_launch_overflows_and_retries(mixed, monkeypatch):
    """the same batch from row capacities forced low (the overflow test hook): every member overflows, the batch regrows and retries"""
    normal = _mixed_batch(mixed, 1)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    assert _mixed_batch(mixed, 1) >= normal + 8          # (the attempt that overflowed built every member's rows once, too)
