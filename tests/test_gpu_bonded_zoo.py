"""k_bonded's grouped stream (the production path; the parity hook never runs it) on the inputs of tests/bonded_zoo.py: small molecules
whose groups have every shape from one dihedral to nine, a field missing inside a group, dihedral types up to the edge of the four-bit
field and beyond, an atom with five bonds, rings of three, four and five, SHAKE clusters of two to four atoms, tiles with three and four
chunks of groups, with one, and with no term at all -- under special weights that differ at every level, so that the Lennard-Jones and
Coulomb force of a 1-2 pair inside its bond term and of a 1-3 pair inside its angle term are not zero.  tests/test_oracle_bonded_zoo.py
pins the oracle on these inputs and asserts that each of the six weighted contributions is at least 1e-3 of the largest force;
tests/test_bonded_groups_host.py asserts the cases (bonded_zoo.zoo_cases, also asserted here before anything is compared).

Everything but the first test goes through debug_run or strain_batch.  Forces are m (v1 - v0) / dt of one step without thermostat from
zero velocities (with fix shake on, the constraint forces too), the pressure is the sampled one: bonded_zoo.one_step.

MEASURED on an MI355X (printed by the tests; relative, force / pressure):
  one step of the zoo against the oracle, mode 1 (mode 0 within 1e-16 of the same figures), plain | permuted:
    W_A  SHAKE on 1.09e-13 / 3.8e-14 | 1.09e-13 / 4.1e-14    SHAKE off 2.2e-14 / 4.1e-14 | 2.2e-14 / 4.0e-14
    W_B  SHAKE on 7.4e-14 / 2.9e-14 | 7.4e-14 / 3.2e-14      SHAKE off 1.9e-14 / 4.8e-14 | 1.9e-14 / 4.7e-14
    W_C  SHAKE on 5.5e-14 / 9.5e-15 | 5.5e-14 / 8.0e-15      SHAKE off 1.8e-14 / 5.2e-14 | 1.7e-14 / 5.1e-14
  mode 1 against mode 0 on those states (largest |p| 5.6e3 .. 7.6e3), plain | permuted:
    W_A  SHAKE on 4.8e-16 / 6.0e-16 | 5.1e-15 / 4.8e-16      SHAKE off 3.2e-16 / 5.0e-16 | 4.8e-16 / 3.7e-16
    W_B  SHAKE on 9.9e-15 / 1.8e-16 | 2.1e-16 / 3.8e-16      SHAKE off 3.3e-16 / 5.7e-16 | 3.0e-16 / 1.1e-15
    W_C  SHAKE on 2.5e-16 / 4.9e-16 | 1.9e-16 / 6.1e-16      SHAKE off 1.6e-15 / 3.1e-16 | 1.9e-16 / 3.1e-16
  per kind of molecule under W_B, mode 1 against the oracle, of that kind's largest force, SHAKE on | off: butane 3.4e-14 | 1.8e-14,
    methanol_cx 8.5e-14 | 5.6e-14, methanol_xc 2.1e-13 | 8.5e-14, peroxide 2.0e-13 | 2.9e-14, propene 1.5e-13 | 1.1e-14,
    ring3 1.5e-13 | 1.6e-14, ring4 4.6e-14 | 1.8e-14, ring5 4.7e-14 | 5.8e-15, five_bonds 1.5e-14 | 1.2e-14, butane_hi 9.5e-14 | 1.3e-14,
    peroxide_twice 1.8e-13 | 3.6e-14, ion 1.6e-13 | 1.6e-13
  ua_chain: mode 1 against mode 0 2.4e-16 / 6.7e-17; against the oracle 4.2e-14 / 5.1e-15 (either mode)
  zoo under W_A after 20 steps against the oracle: box 0, x 4.6e-14 A, v 1.5e-13, pavg 3.4e-14; both streams there 5.2e-16 / 1.7e-15
  one launch: together against alone at most 2.1e-15 of the largest stress; mode 1 against the oracle 1.6e-14, 5.1e-14, 1.2e-14
"""
import functools

import numpy as np
import pytest

from bonded_zoo import KINDS, W_A, W_B, W_C, masses, one_step, probe, ua_chain, zoo, zoo_cases
from test_gpu_bonded_groups import CAP, RATES, engine, oracle, relerr, strain_of
from test_oracle_topologies import permuted, with_weights

pytestmark = pytest.mark.gpu

WEIGHTS = {"W_A": W_A, "W_B": W_B, "W_C": W_C}


@functools.lru_cache(maxsize=None)
def system(wname, layout):
    d = zoo(WEIGHTS[wname])
    if layout == "permuted":
        perm = np.random.default_rng(23).permutation(d["natoms"])
        assert (perm != np.arange(len(perm))).mean() > 0.9
        kind = [d["kind_of"][m] if m >= 0 else "ion" for m in np.asarray(d["mol"])[perm]]
        d = permuted(d, perm)
    else:
        kind = [d["kind_of"][m] if m >= 0 else "ion" for m in d["mol"]]
    d["kind_of_atom"] = np.array(kind)
    return d


@functools.lru_cache(maxsize=None)
def cases_hold():
    return zoo_cases(zoo(W_B), ua_chain(W_B))


def at_rest(d):
    return (d["box"], d["x"], np.zeros_like(d["v"]))


def oracle_step(d, state, use_shake):
    o = oracle(d)
    o.set_state(*state)
    p, _ = o.run(1, 1.0, 300.0, nvt=False, use_shake=use_shake, sample=True)
    _, _, v1 = o.get_state()
    return masses(d) * (v1 - state[2]), np.array(p)


@functools.lru_cache(maxsize=None)
def one_step_all(wname, use_shake, layout):
    """the one step of both streams and of the oracle from the zoo at rest: computed once, asserted on by the three tests below"""
    cases_hold()
    d = system(wname, layout)
    eng = engine()
    eng.register_replica("zoo", 1, d)
    out = {}
    for mode in (0, 1):
        eng.bonded_grouping(mode)
        out[mode] = one_step(eng, "zoo", d, at_rest(d), use_shake)
    eng.close()
    out["oracle"] = oracle_step(d, at_rest(d), use_shake)
    return out


CASES = [(w, s, l) for w in ("W_A", "W_B", "W_C") for s in (True, False) for l in ("plain", "permuted")]


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["W_A", "W_B"])
def test_parity_hook_on_the_zoo(wname):
    """The per-term stream through the parity hook, per part, at the budgets of test_gpu_topologies.static_parity: the baseline."""
    from test_gpu_topologies import static_parity
    cases_hold()
    eng = engine()
    static_parity(eng, "zoo", system(wname, "plain"), use_shake=False)
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,use_shake,layout", CASES)
def test_both_streams_against_the_oracle_s_same_step(wname, use_shake, layout):
    """Forces within 1e-11 of the largest force, pressure within 1e-8: the budgets of test_grouped_against_per_term_on_the_same_states."""
    r = one_step_all(wname, use_shake, layout)
    fo, po_ = r["oracle"]
    assert np.abs(fo).max() > 0.0
    for mode in (1, 0):
        f, p = r[mode]
        print(f"zoo {wname} shake={use_shake} {layout}: mode {mode} against the oracle, forces {relerr(f, fo):.3e}, pressure {relerr(p, po_):.3e}")
    for mode in (1, 0):
        f, p = r[mode]
        assert relerr(f, fo) < 1e-11, mode
        assert relerr(p, po_) < 1e-8, mode


# 3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname,use_shake,layout", CASES)
def test_grouped_against_per_term_stream(wname, use_shake, layout):
    """Two summation orders of one sum: CAP = 1e-12 of the largest force and of max(1, |p|)."""
    r = one_step_all(wname, use_shake, layout)
    (f0, p0), (f1, p1) = r[0], r[1]
    df, dp = np.abs(f1 - f0).max() / np.abs(f0).max(), np.abs(p1 - p0).max() / max(1.0, np.abs(p0).max())
    print(f"zoo {wname} shake={use_shake} {layout}: mode 1 against mode 0, forces {df:.3e}, pressure {dp:.3e} (largest |p| {np.abs(p0).max():.3e})")
    assert df <= CAP
    assert dp <= CAP


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_shake", [True, False])
def test_every_kind_of_molecule_on_its_own_scale(use_shake):
    """Mode 1 against the oracle under W_B, per kind of molecule: the largest force deviation over its atoms stays below 1e-10 of that
    kind's largest force, so that a term wrong on one small molecule cannot hide under the largest force of the box.  (The oracle itself
    is within 2e-14 of the autograd reference on every kind, test_oracle_bonded_zoo: no kind sits at an ill-conditioned geometry, and
    none needs the wider yardstick -- ten times the oracle's own deviation -- that the clamp test uses.)"""
    r = one_step_all("W_B", use_shake, "plain")
    kind = system("W_B", "plain")["kind_of_atom"]
    (f1, _), (fo, _) = r[1], r["oracle"]
    worst = {}
    for k in KINDS + ("ion",):
        sel = kind == k
        assert sel.sum() > 0 and np.abs(fo[sel]).max() > 0.0
        worst[k] = np.abs(f1[sel] - fo[sel]).max() / np.abs(fo[sel]).max()
        print(f"zoo W_B shake={use_shake}: {k}: largest force {np.abs(fo[sel]).max():.3e}, deviation {worst[k]:.3e} of it")
    assert max(worst.values()) < 1e-10, worst


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_three_and_four_chunks_of_groups_in_a_tile():
    """The united-atom chain: 192, 195 and 186 single-dihedral groups in its tiles, so waves 1 to 3 take a chunk of groups after their
    terms.  Mode 1 against mode 0 at CAP and against the oracle's same step at 1e-11 / 1e-8."""
    _, sc = cases_hold()
    assert sorted(-(-sc["groups_per_tile"] // 64)) == [3, 3, 4]
    d = ua_chain(W_B)
    eng = engine()
    eng.register_replica("chain", 1, d)
    f1, p1 = probe(eng, "chain", d, at_rest(d), False, CAP, CAP, "ua_chain")
    eng.bonded_grouping(0)
    f0, p0 = one_step(eng, "chain", d, at_rest(d), False)
    eng.close()
    fo, po_ = oracle_step(d, at_rest(d), False)
    print(f"ua_chain: against the oracle, forces {relerr(f1, fo):.3e} (mode 1) {relerr(f0, fo):.3e} (mode 0), pressure {relerr(p1, po_):.3e} {relerr(p0, po_):.3e}")
    assert relerr(f1, fo) < 1e-11 and relerr(f0, fo) < 1e-11
    assert relerr(p1, po_) < 1e-8 and relerr(p0, po_) < 1e-8


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_twenty_steps_of_dynamics_on_the_zoo():
    """NVT + SHAKE + deform under W_A in mode 1 against the oracle at the budgets of test_gpu_topologies.py, then both streams on the state
    reached."""
    cases_hold()
    d = system("W_A", "plain")
    eng = engine()
    eng.register_replica("zoo", 1, d)
    eng.bonded_grouping(1)
    eng.set_state(5, "zoo", 1, d["box"], d["x"], d["v"])
    pavg = eng.debug_run("zoo", 1, 20, 1.0, 300.0, qp=5, nvt=True, use_shake=True, rates=RATES, sample=True)
    box, x, v = eng.get_state(5, "zoo", 1)
    o = oracle(d)
    pavg_o, _ = o.run(20, 1.0, 300.0, nvt=True, use_shake=True, rates=RATES, sample=True)
    bo, xo, vo = o.get_state()
    print(f"zoo W_A after 20 steps: box {np.abs(box - bo).max():.3e}, x {np.abs(x - xo).max():.3e}, v {relerr(v, vo):.3e}, pavg {relerr(pavg, pavg_o):.3e}")
    assert np.abs(box - bo).max() < 1e-12
    assert np.abs(x - xo).max() < 1e-9
    assert relerr(v, vo) < 1e-8
    assert relerr(pavg, pavg_o) < 1e-8
    probe(eng, "zoo", d, (box, x, v), True, CAP, CAP, "zoo W_A after 20 steps")
    eng.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_zoo_chain_and_crystal_in_one_launch(small_pe):
    """One launch of k_bonded over the zoo, the chain and the polyethylene crystal: three sizes of the largest tile, tiles with three and
    four chunks of groups, with one and with none side by side.  In either mode every stress equals that simulation's evaluation alone
    within 1e-9 of the largest stress (tolerance and neigh_delay = 0 as in test_mixed_launch_of_small_and_large_tiles), and mode 1 matches
    the oracle's evaluation within 1e-6."""
    from scema_amd import capi
    from test_oracle_topologies import topo_stats
    cases_hold()
    kw = dict(kspace_accuracy=1e-4, neigh_delay=0)
    systems = {"zoo": system("W_B", "plain"), "chain": ua_chain(W_B), "pe": with_weights(small_pe, (0.0, 0.0, 0.5), (0.0, 0.0, 0.5))}
    touched = {k: topo_stats(d)["touched"].max() for k, d in systems.items()}
    assert len(set(touched.values())) == 3
    sim = lambda q, k: capi.make_sim(q, k, 1, strain_of(systems[k], 1e-3 + 2e-4 * q), nss=10, most_recent=capi.QP_NONE)

    def run(names, mode):
        eng = engine(**kw)
        eng.bonded_grouping(mode)
        for k in names.values():
            eng.register_replica(k, 1, systems[k])
        out = eng.strain_batch([sim(q, k) for q, k in names.items()])
        assert all(o.stress_updated == 1 for o in out)
        eng.close()
        return np.array([list(o.stress) for o in out])

    order = {q: k for q, k in enumerate(systems)}
    together = {mode: run(order, mode) for mode in (0, 1)}
    scale = np.abs(together[0]).max()
    for mode in (0, 1):
        for q, k in order.items():
            alone = run({q: k}, mode)[0]
            print(f"one launch, mode {mode}, {k}: together against alone {np.abs(together[mode][q] - alone).max() / scale:.3e} of the largest stress")
            assert np.abs(together[mode][q] - alone).max() < 1e-9 * scale, (mode, k)
    for q, k in order.items():
        exp, nts = oracle(systems[k], **kw).eval(strain_of(systems[k], 1e-3 + 2e-4 * q), 2.0, 300.0, 1e-4, 10)
        print(f"one launch, mode 1, {k}: against the oracle {relerr(together[1][q], exp):.3e}")
        assert nts == 10 and relerr(together[1][q], exp) < 1e-6, (k, relerr(together[1][q], exp))
