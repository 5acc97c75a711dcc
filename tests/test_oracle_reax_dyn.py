"""The ReaxFF oracle's second half (BASELINE config 5): oracle/reax_torch.py -- the energy of
oracle/reax_oracle.c as one differentiable expression, forces and virial by reverse-mode differentiation -- and
oracle/reax_md.py -- the dynamics of oracle/md_oracle.c (velocity Verlet, Nose-Hoover chain, fix deform, pressure average)
around those forces and `fix qeq/reax`.

PARITY UNPINNED (no LAMMPS, no USER-REAXC).  Pinned here: the two energy implementations agree part by part; the reverse-mode
forces and virial equal the central differences of the C energy; charges equal rxo_qeq's; the dynamics conserve what they must;
a whole evaluation is reproducible and continues from its stored state."""
import os

import numpy as np
import pytest
import torch

from oracle import pyreax as pr
from oracle import reax_md, reax_torch as rt
from test_oracle_reax import FFIELD, case_ethane, case_glycine_like
from test_reax_host import case_mixture, case_pe_cell

MVV2E = 48.88821291 ** 2
BOLTZ = 0.0019872067
MASS = dict(H=1.008, C=12.011, N=14.007, O=15.999)
ELEMENTS = ["H", "C", "N", "O"]                       # pair_coeff * * ffield.reax.2 H C N O (in.strain.lammps:11)


@pytest.fixture(scope="module")
def ff():
    f = pr.ForceField(FFIELD)
    yield f
    f.close()


@pytest.fixture(scope="module")
def R():
    return rt.ReaxEnergy(FFIELD)


def _same_energy(ff, R, t, x, box, q):
    e, parts = ff.energy(t, x, box=box, q=q)
    tot, pt = R.energy(t, torch.tensor(np.asarray(x, float)), box, None if q is None else torch.tensor(q))
    for k in pr.PARTS:
        assert abs(float(pt[k].detach()) - parts[k]) < 1e-10 * (1.0 + abs(parts[k])), (k, float(pt[k].detach()), parts[k])
    assert abs(float(tot) - e) < 1e-10 * (1.0 + abs(e))


def test_energy_equals_the_c_oracle_part_by_part(ff, R):
    t, x = case_glycine_like(ff)
    q = np.linspace(-0.3, 0.3, len(t)); q -= q.mean()
    _same_energy(ff, R, t, x, None, q)
    t, x = case_ethane(ff, 0.3)
    _same_energy(ff, R, t, x, None, None)
    sym, x, box = case_pe_cell(ff, tilt=(0.7, -0.4, 0.5))
    t = ff.types(sym)
    q, _ = ff.qeq(t, x, box)
    _same_energy(ff, R, t, x, box, q)
    sym, x, box = case_mixture()
    t = ff.types(sym)
    q, _ = ff.qeq(t, x, box)
    _same_energy(ff, R, t, x, box, q)


def test_reverse_mode_forces_equal_central_differences(ff, R):
    t, x = case_glycine_like(ff)
    q = np.linspace(-0.3, 0.3, len(t)); q -= q.mean()
    f, _, _ = R.forces(t, x, None, q)
    fd = ff.forces(t, x, None, q, h=1e-5)
    assert np.abs(f - fd).max() < 1e-7 * np.abs(fd).max()
    assert np.abs(f.sum(0)).max() < 1e-9 * np.abs(f).max()


def test_forces_and_virial_in_a_condensed_triclinic_cell(ff, R):
    """all 4 320 force components along random directions, and the virial against the strain derivative of the C energy"""
    sym, x, box = case_pe_cell(ff, tilt=(0.7, -0.4, 0.5))
    t = ff.types(sym)
    q, _ = ff.qeq(t, x, box)
    f, w, e, _ = R.forces(t, x, box, q, virial=True)
    rng = np.random.default_rng(3)
    for _ in range(4):
        d = rng.standard_normal(x.shape); d /= np.linalg.norm(d)
        h = 1e-4
        de = (ff.energy(t, x + h * d, box=box, q=q)[0] - ff.energy(t, x - h * d, box=box, q=q)[0]) / (2 * h)
        assert abs(de + (f * d).sum()) < 2e-6 * (1.0 + abs(de))
    wfd = np.zeros(6)
    pr.lib().rxo_forces_fd(ff.h, len(t), pr._p(np.ascontiguousarray(t, dtype=np.int32)), pr._p(np.ascontiguousarray(x)), pr._p(np.ascontiguousarray(box)),
                           pr._p(np.ascontiguousarray(q)), 1e-5, None, pr._p(wfd))
    assert np.abs(w - wfd).max() < 1e-6 * np.abs(wfd).max(), (w, wfd)


def test_charge_equilibration_equals_the_c_solver(ff, R):
    sym, x, box = case_mixture()
    t = ff.types(sym)
    qc, _ = ff.qeq(t, x, box, tol=1e-10, maxiter=500)
    H, dia = R.h_matrix(t, x, box)
    n = len(t)
    s, _ = R.cg(H, dia, -R.p.sbp["chi"][t], np.zeros(n), 1e-10, 500)
    tt, _ = R.cg(H, dia, -np.ones(n), np.zeros(n), 1e-10, 500)
    q = s - s.sum() / tt.sum() * tt
    assert np.abs(q - qc).max() < 1e-9 and abs(q.sum()) < 1e-10


def _thermal_velocities(sym, temperature, seed):
    m = np.array([MASS[s] for s in sym])
    v = np.random.default_rng(seed).standard_normal((len(sym), 3)) * np.sqrt(BOLTZ * temperature / (m[:, None] * MVV2E))
    return v - (m[:, None] * v).sum(0) / m.sum()


def _md(sym, x, box, v, **kw):
    lt = np.array([ELEMENTS.index(s) for s in sym])
    return reax_md.ReaxMD(FFIELD, ELEMENTS, lt, [MASS[e] for e in ELEMENTS], box, x, v, **kw)


def test_nve_and_nose_hoover_conserved_quantities(ff):
    """ethane in a large box (few pairs: fast): velocity Verlet keeps E, the thermostatted run keeps E + the chain's energy, to
    within a percent of the kinetic energy over 16 fs, and better with a shorter step.  Not to second order in the step, and it
    cannot be: the charges minimise the QEq functional with 14.4 eV A (fix_qeq_reax), the forces come from a Coulomb energy with
    332.06371 kcal A / mol (= 14.425 eV A; reaxc_nonbonded) at fixed charges, so (dE/dq - mu) dq/dt is not exactly zero -- USER-REAXC's
    own mismatch of constants, restated."""
    t, x = case_ethane(ff, 0.3)
    sym = [ff.names[k] for k in t]
    box = np.array([-20.0, -20, -20, 20, 20, 20, 0, 0, 0])
    v = _thermal_velocities(sym, 300.0, 5)
    drift = []
    for dt, nsteps in ((0.4, 40), (0.2, 80)):
        M = _md(sym, x, box, v, qeq_tol=1e-10, qeq_maxiter=500)
        _, tr = M.run(nsteps, dt, 300.0, nvt=False, trace=True)
        e = tr[:, 1] + tr[:, 2]
        drift.append(np.abs(e - e[0]).max())
        assert drift[-1] < 1.5e-2 * tr[:, 2].mean()
        assert np.abs(tr[:, 2] - tr[0, 2]).max() > 20.0 * drift[-1]        # while kinetic and potential energy trade much more than that
    assert drift[1] < 0.6 * drift[0]
    M = _md(sym, x, box, v, qeq_tol=1e-10, qeq_maxiter=500)
    _, tr = M.run(80, 0.2, 300.0, nvt=True, trace=True)
    cons = tr[:, 1] + tr[:, 2] + tr[:, 3]
    assert np.abs(cons - cons[0]).max() < 1.5e-2 * tr[:, 2].mean()
    assert np.abs(tr[:, 3]).max() > 2.0 * np.abs(cons - cons[0]).max()    # the chain did exchange energy


def test_a_strained_evaluation_is_reproducible_and_continues(ff):
    """STMDProblem::strain with md_force_field reax on the condensed mixture: straining steps by the nts rule, the box ends
    where fix deform should leave it, the stress is reproducible, and a second evaluation continues from the stored state"""
    sym, x, box = case_mixture(seed=10)
    v = _thermal_velocities(sym, 300.0, 2)
    lens = box[3:6] - box[:3]
    eps = np.array([0.004, -0.001, 0.0, 0.002, 0.0, -0.001])
    strain = eps * lens[[0, 1, 2, 2, 1, 0]]
    M = _md(sym, x, box, v)
    s1, nts = M.eval(strain, 0.25, 300.0, 1e-3, 10)
    nrm = np.sqrt((eps[:3] ** 2).sum() + 2.0 * (eps[3:] ** 2).sum())
    assert nts == max(10, int(np.ceil(nrm / 1e-3 / 0.25 / 10.0) * 10))
    b, _, _ = M.get_state()
    assert np.allclose((b[3:6] - b[:3]) / lens - 1.0, eps[:3], atol=2e-5)
    assert np.isfinite(s1).all() and np.abs(s1).max() > 1e5
    assert 2 <= M.qeq_iters / M.qeq_solves < 80
    M2 = _md(sym, x, box, v)
    s1b, _ = M2.eval(strain, 0.25, 300.0, 1e-3, 10)
    assert np.abs(s1 - s1b).max() < 1e-10 * np.abs(s1).max()
    s2, _ = M.eval(0.5 * strain, 0.25, 300.0, 1e-3, 10)
    assert np.isfinite(s2).all() and np.abs(s2 - s1).max() > 1e3


def test_committed_goldens_are_what_the_oracle_gives_now():
    """first evaluation of the mixture golden, regenerated (the full file takes minutes: tests/golden/make_golden_reax.py)"""
    import json
    path = os.path.join(os.path.dirname(__file__), "golden", "oracle_eval_reax.json")
    g = json.load(open(path))
    case = g["mixture"]
    sym, x, box, v = case["sym"], np.array(case["x"]), np.array(case["box"]), np.array(case["v"])
    M = _md(sym, x, box, v)
    ev = case["chains"][0]["evals"][0]
    s, nts = M.eval(np.array(ev["strain_len"]), g["params"]["dt"], g["params"]["temperature"], g["params"]["strain_rate"], g["params"]["nss"])
    assert nts == ev["nts"]
    assert np.abs(s - np.array(ev["stress"])).max() < 1e-9 * np.abs(s).max()
