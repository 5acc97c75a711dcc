"""The kit of the row-stage GPU tests (tests/test_gpu_{sw,tersoff,tersoff_forms,eam,adp,vashishta,edip,meam_spline,born_dsf,born_long}.py
and the files that extend them): a descriptor per stage (Pot), the helpers every one of those files needs, and the scenarios they share,
as functions that a test calls with its own case, descriptor and literal budgets.

Nothing here knows a budget: every tolerance is a required argument, so each stays a literal in the test file, next to the docstring that
justifies it.  Nothing here is a test, a fixture or a hook; the module is imported like the numpy restatements (tests/ is on the path).
"""
import math
import os
import re
import shutil
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import pytest

import sw_numpy as swn
from scema_amd import capi

ATM_TO_PA = 1.01325e5


@dataclass(frozen=True)
class Pot:
    """one row stage as the tests see it"""
    label: str                  # in printed lines: "eam", "born/dsf"
    configure: str              # capi.Engine method: "eam_configure"
    compute: str                # capi.Engine method: "eam_compute"
    kind: str                   # in messages: "EAM" of `no EAM potential`
    energies: tuple             # the two energy terms compared: ("e_pair", "e_embed")
    counters: tuple             # compared exactly: ("npairs", "nabove")
    counts: str = ""            # the counters of a printed static line, a format over the counters, `got` and `ref`
    ionic: bool = False         # the replica carries charges (capi.ionic_system) and configure takes no element list
    energy_scale: tuple = ()    # keys of the reference whose largest sets the energy scale, where they are not `energies`


class Setup(NamedTuple):
    """one material with one replica: what a scenario configures and registers"""
    matid: str
    path: str
    elements: tuple             # None: the method's default (and always for an ionic stage)
    masses: tuple               # None: the default of capi.bare_system
    case: tuple                 # (x, box, t) or, ionic, (x, box, t, q)
    v: np.ndarray = None


def engine(**kw):
    return capi.Engine(capi.default_params(**kw))


def configure(pot, e, matid, path, elements=None, **kw):
    if pot.ionic or elements is None:
        getattr(e, pot.configure)(matid, path, **kw)
    else:
        getattr(e, pot.configure)(matid, path, elements, **kw)


def compute(pot, e, matid, replica=1, qp=capi.QP_NONE):
    return getattr(e, pot.compute)(matid, replica, qp)


def system(pot, case, masses=None, v=None):
    if pot.ionic:
        x, box, t, q = case
        return capi.ionic_system(t, q, x, box, masses, v=v)
    x, box, t = case
    return capi.bare_system(t, x, box, v=v) if masses is None else capi.bare_system(t, x, box, v=v, masses=masses)


def registered(pot, s, configure_it=True, v=True):
    """a fresh engine with the material of `s` configured (or not) and its replica registered, with or without the velocities"""
    e = engine()
    if configure_it:
        configure(pot, e, s.matid, s.path, s.elements)
    e.register_replica(s.matid, 1, system(pot, s.case, s.masses, s.v if v else None))
    return e


def static(pot, x, box, t, path, elements, masses, q=None, **conf):
    """the static hook on one replica in a fresh engine"""
    e = engine()
    try:
        configure(pot, e, "m", path, elements, **conf)
        e.register_replica("m", 1, system(pot, (x, box, t) if q is None else (x, box, t, q), masses))
        return compute(pot, e, "m", 1)
    finally:
        e.close()


def static_of(pot, path, elements, masses):
    """static() bound to one stage and its fixture: f(x, box, t[, q], path=.., elements=.., masses=.., **conf)"""
    def bound(*case, path=path, elements=elements, masses=masses, **conf):
        return static(pot, *case[:3], path, elements, masses, q=case[3] if len(case) > 3 else None, **conf)
    return bound


def assert_not_attached(pot, e, matid, replica=1):
    """the static hook on a material that holds another potential or none is refused by name: `no <kind> potential`"""
    with pytest.raises(capi.EngineError, match=f"no {re.escape(pot.kind)} potential"):
        compute(pot, e, matid, replica)


def nts_and_rates(strain, box, dt, rate):
    """the straining steps and the six rates that strain_batch derives for one simulation (nts_rule, rounded as the script prints them)"""
    lb = box[3:6] - box[:3]
    eps = np.array([strain[0] / lb[0], strain[1] / lb[1], strain[2] / lb[2], strain[3] / lb[2], strain[4] / lb[1], strain[5] / lb[0]])
    nrm = math.sqrt(eps[0] ** 2 + eps[1] ** 2 + eps[2] ** 2 + 2.0 * (eps[3] ** 2 + eps[4] ** 2 + eps[5] ** 2))
    nts = max(int(math.ceil(nrm / rate / dt / 10.0) * 10), 10)
    return nts, np.array([float("%.6e" % (eps[k] / (nts * dt))) for k in range(6)])


def velocities(types, masses, temp, seed):
    """Maxwell-Boltzmann velocities with no net momentum.  Atoms of one mass: one scale, the mean velocity removed; several masses: a
    scale per atom, the velocity of the centre of mass removed.  The stream is default_rng(seed).normal(size=(n, 3)) either way"""
    rng = np.random.default_rng(seed)
    m = np.asarray(masses, float)[np.asarray(types)]
    if (m == m[0]).all():
        v = rng.normal(size=(len(m), 3)) * math.sqrt(swn.BOLTZ * temp / float(m[0]) / swn.MVV2E)
        return v - v.mean(axis=0)
    m = m[:, None]
    v = rng.normal(size=(len(m), 3)) * np.sqrt(swn.BOLTZ * temp / m / swn.MVV2E)
    return v - (m * v).sum(axis=0) / m.sum()


def all_exactly_zero(got, ref, pot, what, head="no pairs", ref_keys=("e",)):
    """the usual body of a `no_pairs` function: no term at all, so every number is exactly zero and there is no scale to divide by"""
    assert all(ref[k] == 0.0 for k in ref_keys) and not ref["f"].any() and not ref["w"].any()
    assert all(got[k] == 0.0 for k in pot.energies) and (got["f"] == 0.0).all() and (got["w"] == 0.0).all()
    print(f"{what}: {head}, all exactly zero, rows {got['maxrow']}/{got['rowcap']}")


def check_static(got, ref, pot, *, tol_f, tol_e, tol_w, what, scale=None, no_pairs=None, fs=None, ws=None, fterm=0.0, tail=""):
    """one static evaluation against the reference: the counters exactly, rows within their capacity, finite numbers, then forces, the
    two energy terms and the virial within tol_* of their largest.  scale: another reference whose sizes are the yardstick (a perfect cell
    measured on its jittered twin); fs, ws: a force or virial scale given outright; fterm: the size of the largest single force term, a floor of
    the force scale where the terms cancel in the sum; no_pairs(got, ref, scale, what) -> bool: the stage's
    own branch for an input without a term, which asserts and prints what holds there and returns True when it took the case"""
    scale = scale or ref
    assert tuple(got[k] for k in pot.counters) == tuple(ref[k] for k in pot.counters), [(k, got[k], ref[k]) for k in pot.counters]
    assert got["maxrow"] <= got["rowcap"]
    assert np.isfinite(got["f"]).all() and np.isfinite(got["w"]).all() and all(math.isfinite(got[k]) for k in pot.energies)
    if no_pairs is not None and no_pairs(got, ref, scale, what):
        return
    fs = max(np.abs(scale["f"]).max(), fterm) if fs is None else fs
    ws = np.abs(scale["w"]).max() if ws is None else ws
    es = max(abs(scale[k]) for k in (pot.energy_scale or pot.energies))
    df = np.abs(got["f"] - ref["f"]).max()
    de = max(abs(got[k] - ref[k]) for k in pot.energies)
    dw = np.abs(got["w"] - ref["w"]).max()
    counts = pot.counts.format(got=got, ref=ref, **{k: got[k] for k in pot.counters})
    print(f"{what}: force err {df / fs:.2e}, energy err {de / es:.2e}, virial err {dw / ws:.2e}, {counts + ', ' if counts else ''}"
          f"rows {got['maxrow']}/{got['rowcap']}{tail}")
    assert df <= tol_f * fs and de <= tol_e * es and dw <= tol_w * ws


def checker(pot, what=None, **budgets):
    """check_static() bound to one stage, its budgets and its no_pairs branch: f(got, ref, what, scale=.., ..)"""
    def bound(got, ref, what=what, **kw):
        check_static(got, ref, pot, what=what, **budgets, **kw)
    return bound


# ---- the shared scenarios ----
def nve_and_sampled_pressure(pot, ref, s, *, steps, tol_x, tol_v, tol_p):
    """`steps` steps of NVE against the numpy velocity-Verlet stepper; then one step with sampling: the sampled tensor is
    (sum m v v + W) / V of the state after the step, in atm"""
    x, box, t = s.case
    e = registered(pot, s)
    try:
        e.set_state(0, s.matid, 1, box, x, s.v)
        e.debug_run(s.matid, 1, steps, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, s.matid, 1)
        xr, vr = ref.nve(x, s.v, box, t, s.masses, 1.0, steps)
        dx = np.abs(swn.minimage_diff(xg, xr, box)).max()
        print(f"{pot.label} nve {steps} steps: max position difference {dx:.2e} A, velocity {np.abs(vg - vr).max():.2e} A/fs")
        assert dx < tol_x and np.abs(vg - vr).max() < tol_v
        e.set_state(1, s.matid, 1, box, x, s.v)
        p = e.debug_run(s.matid, 1, 1, 1.0, 300.0, qp=1, nvt=False, use_shake=False, sample=True)
        x1, v1 = ref.nve(x, s.v, box, t, s.masses, 1.0, 1)
        want = ref.pressure_atm(x1, v1, box, t, s.masses)
        print(f"{pot.label} sampled pressure (atm): {p}, max rel err {np.abs(p - want).max() / np.abs(want).max():.2e}")
        assert np.abs(p - want).max() <= tol_p * np.abs(want).max()
    finally:
        e.close()


def by_debug_runs(e, matid, qp, strain, box, dt=1.0, temp=300.0, rate=1e-4, nss=10):
    """what strain_batch does for one simulation, issued through the parity hooks: the straining run, then the sampling run.
    -> (stress in Pa, straining steps)"""
    nts, rates = nts_and_rates(strain, box, dt, rate)
    e.debug_run(matid, 1, nts, dt, temp, qp=qp, nvt=True, use_shake=False, rates=rates)
    return -e.debug_run(matid, 1, nss, dt, temp, qp=qp, nvt=True, use_shake=False, sample=True) * ATM_TO_PA, nts


UPDATE = dict(nss=10, dt=1.0, temperature=300.0, strain_rate=1e-4)


def strain_batch_vs_debug_runs(pot, s, strain, *, expect_nts, tol):
    """one update against the straining run and the sampling run issued through the parity hooks"""
    x, box = s.case[0], s.case[1]
    e, f = registered(pot, s), registered(pot, s)
    try:
        out = np.array(e.strain_batch([capi.make_sim(0, s.matid, 1, strain, most_recent=capi.QP_NONE, **UPDATE)])[0].stress[:])
        f.set_state(0, s.matid, 1, box, x, s.v)
        want, nts = by_debug_runs(f, s.matid, 0, strain, box)
        print(f"{pot.label} strain_batch vs debug runs ({nts} + 10 steps): {np.abs(out - want).max() / np.abs(want).max():.2e}")
        assert nts == expect_nts and np.abs(out - want).max() <= tol * np.abs(want).max()
        assert e.has_state(0, s.matid, 1)
    finally:
        e.close()
        f.close()


def strain_batch_and_a_second_update(pot, s, s1, s2, *, tol):
    """an update against its two runs; then a second update from the stored states: qp 0 continues from its own, qp 1 branches from
    qp 0's"""
    x, box = s.case[0], s.case[1]
    m = s.matid
    e, f = registered(pot, s), registered(pot, s)
    try:
        out1 = np.array(e.strain_batch([capi.make_sim(0, m, 1, s1, most_recent=capi.QP_NONE, **UPDATE)])[0].stress[:])
        f.set_state(0, m, 1, box, x, s.v)
        want1, nts = by_debug_runs(f, m, 0, s1, box)
        print(f"{pot.label} strain_batch vs debug runs ({nts} + 10 steps): {np.abs(out1 - want1).max() / np.abs(want1).max():.2e}")
        assert np.abs(out1 - want1).max() <= tol * np.abs(want1).max()
        assert e.has_state(0, m, 1) and not e.has_state(1, m, 1)
        out2 = e.strain_batch([capi.make_sim(0, m, 1, s2, most_recent=0, **UPDATE), capi.make_sim(1, m, 1, s2, most_recent=0, **UPDATE)])
        a, b = np.array(out2[0].stress[:]), np.array(out2[1].stress[:])
        b1, _, _ = f.get_state(0, m, 1)
        want2, _ = by_debug_runs(f, m, 0, s2, b1)
        print(f"{pot.label} second update: {np.abs(a - want2).max() / np.abs(want2).max():.2e}, branch {np.abs(b - want2).max() / np.abs(want2).max():.2e}")
        assert np.abs(a - want2).max() <= tol * np.abs(want2).max() and np.abs(b - want2).max() <= tol * np.abs(want2).max()
        assert e.has_state(1, m, 1) and np.abs(a - out1).max() > 1e-3 * np.abs(out1).max()
    finally:
        e.close()
        f.close()


class Batch(NamedTuple):
    fresh: object               # () -> an engine with every material configured and registered
    sims: list
    alone: np.ndarray           # each simulation's stress alone in a fresh engine
    mat_of: list                # the material of each simulation


def batch_vs_alone_fixture(pot, mats, n, seed, thermal_masses=None, pick=None):
    """n simulations over the materials of `mats` (matid -> (case, path, elements, masses)): by default the first material where q % 3,
    the second elsewhere; velocities of 300 K from the seeds 7, 8, .. in the sorted order of the names (thermal_masses: one mass tuple
    for every atom, where the stage draws them so); strains of 10 to 30 straining steps, a ragged batch"""
    names = list(mats)
    pick = pick or (lambda q: names[0] if q % 3 else names[1])
    vel = {}
    for k, (m, c) in enumerate(sorted(mats.items())):
        t = c[0][2]
        vel[m] = velocities(t, c[3], 300.0, 7 + k) if thermal_masses is None else velocities(np.zeros(len(t), int), thermal_masses, 300.0, 7 + k)
    rng = np.random.default_rng(seed)
    sims = []
    for q in range(n):
        m = pick(q)
        box = mats[m][0][1]
        L = box[3:6] - box[:3]
        ezz = rng.uniform(5e-4, 2.5e-3)
        sims.append((q, m, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0])))

    def fresh():
        e = engine()
        for m, (case, path, el, masses) in mats.items():
            configure(pot, e, m, path, el)
            e.register_replica(m, 1, system(pot, case, masses, vel[m]))
        return e

    mk = lambda q, m, s: capi.make_sim(q, m, 1, s, most_recent=capi.QP_NONE, **UPDATE)
    alone = []
    for q, m, s in sims:
        e = fresh()
        alone.append(np.array(e.strain_batch([mk(q, m, s)])[0].stress[:]))
        e.close()
    return Batch(fresh, [mk(*s) for s in sims], np.array(alone), [m for _, m, _ in sims])


def assert_batch_vs_alone(pot, batch, split, *, what, tol, bitwise_forces=False):
    """the stresses of the batch, whole (split 0) or as part batches on two streams (split 1), against each simulation alone;
    bitwise_forces: and the forces on every end state, evaluated in the engine that ran the batch (its slots hold rows and records of
    other simulations) and in a fresh engine handed the same state, equal bit for bit"""
    e = batch.fresh()
    g = batch.fresh() if bitwise_forces else None
    try:
        e.batch_split(split)
        out = np.array([list(o.stress) for o in e.strain_batch(batch.sims)])
        err = np.abs(out - batch.alone).max(axis=1) / np.abs(batch.alone).max(axis=1)
        print(f"{what} (split {split}): max rel err {err.max():.2e}")
        assert np.isfinite(out).all() and err.max() <= tol
        if bitwise_forces:
            for q, m in enumerate(batch.mat_of):
                box, x, v = e.get_state(q, m, 1)
                g.set_state(q, m, 1, box, x, v)
                a, b = compute(pot, e, m, 1, qp=q), compute(pot, g, m, 1, qp=q)
                assert np.abs(a["f"]).max() > 0.0 and np.array_equal(a["f"], b["f"]), q
    finally:
        e.close()
        if g is not None:
            g.close()


def sheared_set(pot, s, rate=3.4e-3):
    """Eight simulations of the cell of `s`, which is written with xy = 0.4 lx, each sheared by 0.105 to 0.14 lx in xy, so that every one
    crosses +lx / 2 and flips once: (() -> engine with the replica registered, [(qp, strain)], (qp, strain) -> simulation, the box)"""
    box = s.case[1]
    lx, ly, lz = box[3:6] - box[:3]
    # (the tilt xy moves by strain[3] * ly / lz: nts_rule and fix deform's xy rate)
    sims = [(q, np.array([0.0, 0.0, 0.0, d * lx * lz / ly, 0.0, 0.0])) for q, d in enumerate(np.linspace(0.105, 0.14, 8))]
    mk = lambda q, st: capi.make_sim(q, s.matid, 1, st, nss=10, dt=1.0, temperature=300.0, strain_rate=rate, most_recent=capi.QP_NONE)
    return (lambda: registered(pot, s)), sims, mk, box


def sheared_fixture(pot, s):
    """the sheared set, and each one's stress, flips and final box when it runs alone in a fresh engine"""
    fresh, sims, mk, _ = sheared_set(pot, s)
    alone, flips, boxes = [], 0, []
    for q, st in sims:
        e = fresh()
        alone.append(np.array(e.strain_batch([mk(q, st)])[0].stress[:]))
        flips += e.profile()["box_flips"]
        boxes.append(e.get_state(q, s.matid, 1)[0])
        e.close()
    return fresh, [mk(*st) for st in sims], np.array(alone), flips, boxes


def assert_flips_in_split_batch(sheared, matid, split, *, what, tol):
    """eight is the smallest batch that runs as two parts: same stresses as each simulation alone, as many flips, every box back inside
    |xy| <= lx / 2"""
    fresh, sims, alone, flips, boxes = sheared
    assert flips >= 8
    e = fresh()
    try:
        e.batch_split(split)
        out = np.array([list(o.stress) for o in e.strain_batch(sims)])
        err = np.abs(out - alone).max(axis=1) / np.abs(alone).max(axis=1)
        print(f"{what}: max rel err {err.max():.2e}, box flips {e.profile()['box_flips']} (alone: {flips})")
        assert err.max() <= tol
        assert e.profile()["box_flips"] == flips
        for q in range(8):
            b = e.get_state(q, matid, 1)[0]
            assert abs(b[6]) <= 0.5 * (b[3] - b[0]) and abs(boxes[q][6]) <= 0.5 * (boxes[q][3] - boxes[q][0])
    finally:
        e.close()


def self_configuring_sim(matid, strain, folder, **kw):
    """a simulation whose scripts folder may configure its material"""
    return capi.make_sim(0, matid, 1, strain, nss=10, dt=1.0, most_recent=capi.QP_NONE, force_field="opls", scripts_folder=str(folder), **kw)


def dimer_update(pot, s, scripts, configure, strain_x, compute_qp=None):
    """one update of the few-atom replica of `s` with its potential configured beforehand or left to the scripts folder: with two terms
    to a sum (or one wave doing all the adding) its bits do not depend on the order of the atomic sums, and two runs of the same
    configuration agree bit for bit.  -> (stress, (box, x, v) of the end state[, the static hook at compute_qp])"""
    e = registered(pot, s, configure_it=configure)
    try:
        sim = self_configuring_sim(s.matid, np.array([strain_x, 0.0, 0.0, 0.0, 0.0, 0.0]), scripts, temperature=300.0, strain_rate=1e-4)
        out = np.array(e.strain_batch([sim])[0].stress[:])
        state = e.get_state(0, s.matid, 1)
        return (out, state) if compute_qp is None else (out, state, compute(pot, e, s.matid, 1, qp=compute_qp))
    finally:
        e.close()


def assert_malformed_pair_coeff_lines(pot, s, tmp_path, ext, good_line_tail, *, match_head="", match_tail="", lines=4, strain_x=None,
                                      missing_file=False):
    """a script whose pair_coeff line names the file of `s` wrongly -- types instead of * *, no ${locs}, no element, a subfolder (the
    first `lines` of these) -- is refused with the line number and the expected form; missing_file: and a well-formed line that names a
    file the folder lacks gets the reader's message"""
    name = os.path.basename(s.path)
    box = s.case[1]
    strain = np.array([1e-3 * (box[3] - box[0]) if strain_x is None else strain_x, 0, 0, 0, 0, 0])
    good = "pair_coeff * * ${locs}/" + name + " " + good_line_tail
    bad = [f"pair_coeff 1 1 ${{locs}}/{name} {good_line_tail}", f"pair_coeff * * {name} {good_line_tail}", f"pair_coeff * * ${{locs}}/{name}",
           f"pair_coeff * * ${{locs}}/sub/{name} {good_line_tail}"][:lines]
    expected = match_head + r"in\.strain\.lammps line 1: expected `pair_coeff \* \* \$\{locs\}/<name>" + re.escape(ext) + match_tail
    folders = [(f"bad{k}", line, True, expected) for k, line in enumerate(bad)]
    if missing_file:
        folders.append(("miss", good, False, f"{name}: cannot open"))
    for sub, line, with_file, match in folders:
        d = tmp_path / sub
        d.mkdir()
        if with_file:
            shutil.copy(s.path, d / name)
        (d / "in.strain.lammps").write_text(line + "\n")
        e = registered(pot, s, configure_it=False, v=False)
        try:
            with pytest.raises(capi.EngineError, match=match):
                e.strain_batch([self_configuring_sim(s.matid, strain, d)])
        finally:
            e.close()
