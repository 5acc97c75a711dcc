"""k_bonded on its grouped stream (scema_md_bonded_grouping mode 1: dihedrals per central bond, 1-2 / 1-3 special pairs inside their bond /
angle term) against the per-term stream (mode 0) on the same states, and against the CPU oracle.  The parity hook always runs the
per-term stream, so every check goes through debug_run or an evaluated strain_batch.

Forces and the lumped virial of the production kernel are seen through one step of velocity Verlet without thermostat from a given
state: m (v1 - v0) / dt is the mean of the forces of the step's two evaluations (with fix shake on, the constraint forces too), and the
sampled pressure tensor holds the lumped virial.  `probe()` prints the mode-1-minus-mode-0 differences before it asserts.

Inputs: the 360-atom polyethylene crystal with OPLS-AA's 0 0 0.5 (120 groups of nine dihedrals, seven of them across the boundary of
its two tiles; 1 080 attached pairs, 1 080 weighted 1-4 pairs that stay terms), the 512-atom network (87 groups, 70 across tile
boundaries; 6 221 dihedrals that stay terms because the network lists them from both ends; 3 047 attached pairs) and the 1000-atom
network (six tiles, no group: attached pairs and left-over terms alone).  tests/test_bonded_groups_host.py asserts these features.
"""
import numpy as np
import pytest

from bonded_zoo import masses, probe
from test_oracle_topologies import KW, OWNERS, network_fixture, topo_stats, with_weights

pytestmark = pytest.mark.gpu

KS = dict(kspace_accuracy=1e-5, **KW)
RATES = np.array([1e-5, -2e-5, 3e-5, 1.5e-5, -0.5e-5, 2.5e-5])
# Two formulations of one sum: 1e-12 of the largest force and 1e-12 max(1, |virial|) at the most; ten times the measured difference
# (MEASURED below) where that is less.
CAP = 1e-12


def engine(**kw):
    from scema_amd import capi
    return capi.Engine(capi.default_params(**dict(KS, **kw)))


def oracle(d, **kw):
    from oracle import pyoracle as po
    return po.Oracle(d, po.default_params(**dict(KS, **kw)))


def relerr(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def strain_of(d, ezz=1.2e-3):
    lens = d["box"][3:6] - d["box"][:3]
    return np.array([-0.3 * ezz * lens[0], -0.3 * ezz * lens[1], ezz * lens[2], 5e-5 * lens[2], -3e-5 * lens[1], 2e-5 * lens[0]])


@pytest.fixture(scope="module")
def pe(small_pe):
    return with_weights(small_pe, (0.0, 0.0, 0.5), (0.0, 0.0, 0.5))


@pytest.fixture(scope="module")
def net4():
    return network_fixture()


@pytest.fixture(scope="module")
def net5():
    from scema_amd.systems import build_network
    return build_network(5, drop=0.0, seed=5, special_lj=(0.0, 0.0, 0.5), special_coul=(0.0, 0.0, 0.8333))


# Measured mode-1-minus-mode-0 differences on an MI355X, relative (force, pressure), per input: the largest over the states of the test
# below and over two runs (the order of the LDS atomics of either stream is not fixed, so a run differs from the next).  By state, force /
# pressure, first run | second run:
#   pe    static 7.4e-16 / 6.2e-16 | 1.0e-14 / 5.3e-15, after 20 steps 8.3e-16 / 2.7e-16 | 8.7e-16 / 2.7e-16,
#         SHAKE off 1.9e-15 / 6.3e-16 | 1.8e-15 / 6.3e-16, after 20 steps with SHAKE off 8.3e-16 / 4.1e-16 | 4.1e-16 / 2.7e-16
#   net4  static 1.4e-15 / 3.0e-16 | 5.0e-16 / 2.5e-16, after 20 steps 1.1e-15 / 1.2e-16 (both), SHAKE off 5.0e-16 / 3.0e-16 | 5.0e-16 / 2.5e-16
#   net5  static 6.5e-16 / 3.4e-16 (both), after 20 steps 1.6e-15 / 2.0e-16 | 8.0e-16 / 2.0e-16, SHAKE off 6.5e-16 / 3.4e-16 (both)
# (with fix shake on, the step's constraint iteration sits between the forces and the velocities that are compared: the largest figure).
# Mode 1 against the oracle's same step: forces 1.3e-14 / 2.6e-15 / 9.7e-15, pressure 3.7e-14 / 1.3e-14 / 5.8e-14; mixed batch, mode 1
# against mode 0: 1.6e-15 of the largest stress.
MEASURED = {"pe": (1.0e-14, 5.3e-15), "net4": (1.4e-15, 3.0e-16), "net5": (1.6e-15, 3.4e-16)}


@pytest.mark.parametrize("which", ["pe", "net4", "net5"])
def test_grouped_against_per_term_on_the_same_states(pe, net4, net5, which):
    """Forces and lumped virial of mode 1 against mode 0: on the initial state, on the state after 20 steps of NVT + SHAKE + deform,
    and with SHAKE off (the shaken bonds then run their harmonic part next to their attached pair); every replica's owners span at least
    two tiles, with groups across the boundary where the input has groups.  Bound: ten times MEASURED, at most 1e-12.
    Mode 1's one-step forces are also held against the oracle's same step at 1e-11 and the 20-step trajectory at the budgets of
    test_gpu_topologies.py."""
    d = {"pe": pe, "net4": net4, "net5": net5}[which]
    shake = which == "pe"                       # (the networks have no hydrogen: nothing to constrain)
    assert topo_stats(d)["rank"].max() // OWNERS >= 1
    mf, mp = MEASURED[which]
    bound_f, bound_p = min(CAP, 10.0 * mf), min(CAP, 10.0 * mp)
    eng = engine()
    eng.register_replica(which, 1, d)
    start = (d["box"], d["x"], d["v"])
    f1, p1 = probe(eng, which, d, start, shake, bound_f, bound_p, f"{which} static")
    # the oracle's same step
    o = oracle(d)
    po_, _ = o.run(1, 1.0, 300.0, nvt=False, use_shake=shake, sample=True)
    _, _, vo = o.get_state()
    fo = masses(d) * (vo - d["v"])
    print(f"{which} static: mode 1 against the oracle, forces {relerr(f1, fo):.3e}, pressure {relerr(p1, po_):.3e}")
    assert relerr(f1, fo) < 1e-11
    assert relerr(p1, po_) < 1e-8
    # 20 steps of NVT + SHAKE + deform in mode 1, against the oracle; then both modes on the state reached
    eng.bonded_grouping(1)
    eng.set_state(5, which, 1, *start)
    pavg = eng.debug_run(which, 1, 20, 1.0, 300.0, qp=5, nvt=True, use_shake=shake, rates=RATES, sample=True)
    box, x, v = eng.get_state(5, which, 1)
    o = oracle(d)
    pavg_o, _ = o.run(20, 1.0, 300.0, nvt=True, use_shake=shake, rates=RATES, sample=True)
    bo, xo, vo = o.get_state()
    assert np.abs(box - bo).max() < 1e-12
    assert np.abs(x - xo).max() < 1e-9
    assert relerr(v, vo) < 1e-8
    assert relerr(pavg, pavg_o) < 1e-8
    probe(eng, which, d, (box, x, v), shake, bound_f, bound_p, f"{which} after 20 steps")
    probe(eng, which, d, start, False, bound_f, bound_p, f"{which} SHAKE off")
    if shake:
        probe(eng, which, d, (box, x, v), False, bound_f, bound_p, f"{which} after 20 steps, SHAKE off")
    eng.close()


def test_mixed_batch_of_chain_and_network_in_one_launch(pe, net4):
    """One launch of the grouped kernel over the polyethylene replica and the network: evaluated stresses against the oracle at 1e-6,
    and against the same batch on the per-term stream."""
    from scema_amd import capi
    systems = {"pe": pe, "net4": net4}
    res = {}
    for mode in (0, 1):
        eng = engine()
        eng.bonded_grouping(mode)
        for k, d in systems.items():
            eng.register_replica(k, 1, d)
        out = eng.strain_batch([capi.make_sim(q, k, 1, strain_of(systems[k], 1e-3 + 2e-4 * q), nss=10, most_recent=capi.QP_NONE) for q, k in enumerate(systems)])
        assert all(o.stress_updated == 1 for o in out)
        res[mode] = np.array([list(o.stress) for o in out])
        eng.close()
    scale = np.abs(res[0]).max()
    print(f"mixed batch: mode 1 against mode 0, {np.abs(res[1] - res[0]).max() / scale:.3e} of the largest stress")
    assert np.abs(res[1] - res[0]).max() < 1e-9 * scale          # (20 steps of dynamics; the budget of test_mixed_launch_of_small_and_large_tiles)
    for q, k in enumerate(systems):
        exp, nts = oracle(systems[k]).eval(strain_of(systems[k], 1e-3 + 2e-4 * q), 2.0, 300.0, 1e-4, 10)
        assert nts == 10 and relerr(res[1][q], exp) < 1e-6, (k, relerr(res[1][q], exp))


def test_setter_takes_its_three_modes_and_refuses_others():
    from scema_amd import capi
    eng = engine()
    for mode in (0, 1, -1):
        eng.bonded_grouping(mode)
    for mode in (2, -2):
        with pytest.raises(capi.EngineError) as err:
            eng.bonded_grouping(mode)
        assert "scema_md_bonded_grouping" in str(err.value)
    eng.close()
