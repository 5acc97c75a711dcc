"""GPU parity on branched, scrambled topologies with fractional special weights: k_bonded, build_topo and the exclusion handling of
k_neigh_build on inputs that the polyethylene chains cannot produce (systems.build_network; helpers and the independent pin of the
oracle on these inputs in tests/test_oracle_topologies.py).  Every test first asserts that its input has the feature it is named
for, then compares with the CPU oracle on identical inputs.  Budgets as in test_gpu_parity.py: forces 1e-11 of the largest force,
per-part energies and virials 1e-10 max(1, |ref|), the same number of listed pairs, evaluated stresses 1e-6."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_topologies import (ANGLE_DEG, ANGLE_ILL, ANGLE_ILL_DEV, CHI, CHI_ILL, IMPROPER_ILL_DEV, KW, assert_clamp_cases, clamp_molecules,
                                    network_fixture, permuted, topo_stats, with_weights)

pytestmark = pytest.mark.gpu

KS = dict(kspace_accuracy=1e-5, **KW)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_LOCAL_ATOM = 60        # bytes of k_bonded's dynamic LDS per atom a tile touches (7 doubles + 1 int), tables not counted


def engine(**kw):
    from scema_amd import capi
    return capi.Engine(capi.default_params(**dict(KS, **kw)))


def oracle(d, **kw):
    from oracle import pyoracle as po
    return po.Oracle(d, po.default_params(**dict(KS, **kw)))


def relerr(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def static_parity(eng, name, d, use_shake=False, nparts=7):
    """debug_compute against oracle.compute(): pairs, forces, per-part energies and virials.  Returns the GPU result."""
    from scema_amd import capi
    eng.register_replica(name, 1, d)
    f, e, w, info = eng.debug_compute(name, 1, use_shake=use_shake)
    o = oracle(d)
    o.setup(use_shake=use_shake)
    fo, eo, wo = o.compute()
    assert info["npairs"] == o.npairs
    assert relerr(f, fo) < 1e-11, relerr(f, fo)
    for part in range(nparts):
        assert abs(e[part] - eo[part]) < 1e-10 * max(1.0, abs(eo[part])), (capi.PARTS[part], e[part], eo[part])
        assert np.abs(w[part] - wo[part]).max() < 1e-10 * max(1.0, np.abs(wo[part]).max()), capi.PARTS[part]
    return f, e, w, info, eo


def strain_of(d, ezz=1.2e-3):
    lens = d["box"][3:6] - d["box"][:3]
    return np.array([-0.3 * ezz * lens[0], -0.3 * ezz * lens[1], ezz * lens[2], 5e-5 * lens[2], -3e-5 * lens[1], 2e-5 * lens[0]])


@pytest.fixture(scope="module")
def net4():
    return network_fixture()


@pytest.fixture(scope="module")
def net5():
    from scema_amd.systems import build_network
    return build_network(5, drop=0.0, seed=5, special_lj=(0.0, 0.0, 0.5), special_coul=(0.0, 0.0, 0.8333))


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coul", [0.5, 0.8333])
def test_exactly_sixteen_partners(small_pe, coul):
    """The `e < na` boundary of k_neigh_build's 16 partner lanes per atom: polyethylene with weighted 1-4 pairs (OPLS-AA's 0 0 0.5, and
    lj differing from coul).  Static parts, then 20 steps of NVT + SHAKE + deform against the oracle."""
    d = with_weights(small_pe, (0.0, 0.0, 0.5), (0.0, 0.0, coul))
    partners = topo_stats(d)["partners"]
    typ = np.asarray(d["type"])
    assert set(partners[typ == 0]) == {16} and set(partners[typ == 1]) == {10}
    eng = engine()
    static_parity(eng, "pe", d, use_shake=True)
    rates = np.array([1e-5, -2e-5, 3e-5, 1.5e-5, -0.5e-5, 2.5e-5])
    eng.set_state(5, "pe", 1, d["box"], d["x"], d["v"])
    pavg = eng.debug_run("pe", 1, 20, 1.0, 300.0, qp=5, nvt=True, use_shake=True, rates=rates, sample=True)
    box, x, v = eng.get_state(5, "pe", 1)
    o = oracle(d)
    pavg_o, _ = o.run(20, 1.0, 300.0, nvt=True, use_shake=True, rates=rates, sample=True)
    bo, xo, vo = o.get_state()
    assert np.abs(box - bo).max() < 1e-12
    assert np.abs(x - xo).max() < 1e-9
    assert relerr(v, vo) < 1e-8
    assert relerr(pavg, pavg_o) < 1e-8
    eng.close()


# 2 ---------------------------------------------------------------------------------------------------------------------
_CHILD = ("import json, sys, numpy as np\n"
          "sys.path.insert(0, 'tests')\n"
          "from scema_amd import capi\n"
          "from test_oracle_topologies import network_fixture, KW\n"
          "d = network_fixture()\n"
          "e = capi.Engine(capi.default_params(kspace_accuracy=1e-5, **KW))\n"
          "e.register_replica('net', 1, d)\n"
          "f, en, w, info = e.debug_compute('net', 1, use_shake=False)\n"
          "print(json.dumps({'npairs': float(info['npairs']), 'f': np.asarray(f).ravel().tolist(), 'en': np.asarray(en)[:7].tolist()}))\n")


def test_more_than_sixteen_partners_on_every_list_build_path(net4):
    """Up to 40 partners per atom, from 0 on, in a tilted box: the partners beyond an atom's 16 lanes are struck out of the rows by the
    walk of the lists in memory.  Static parts against the oracle; then the same input through the whole-table walk, the three-kernel
    cell binning and the FP32 build (switches read once per process: child processes): the same pairs (the FP32 build may list
    the superset of its error band), forces and energies."""
    st = topo_stats(net4)
    p = st["partners"]
    assert p.max() >= 25 and (p == 16).any() and (p < 16).any() and (p > 16).sum() > len(p) // 2
    assert np.abs(net4["box"][6:9]).min() > 0.0 and net4["special_lj"][2] == 0.5 and net4["special_coul"][2] == 0.8333
    eng = engine()
    f, e, w, info, _ = static_parity(eng, "net", net4)
    eng.close()
    for name, env in (("whole_table", {"SCEMA_MD_QCAP16": "2"}), ("three_kernel_binning", {"SCEMA_MD_CELL_BUILD": "0"}),
                      ("fp32_build", {"SCEMA_MD_NEIGH_EXACT": "0"})):
        r = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **env))
        assert r.returncode == 0, name + r.stdout[-1500:] + r.stderr[-2500:]
        b = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        if name == "fp32_build":
            assert info["npairs"] <= b["npairs"] <= info["npairs"] * (1 + 1e-4), name
        else:
            assert b["npairs"] == info["npairs"], name
        assert relerr(np.array(b["f"]).reshape(-1, 3), f) < 1e-11, name
        assert np.all(np.abs(np.array(b["en"]) - e[:7]) < 1e-10 * np.maximum(1.0, np.abs(e[:7]))), name


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_terms_over_four_tiles_and_the_lds_opt_in(net5):
    """1000-atom network: dihedrals whose atoms lie in three and four tiles (evaluated by each, counted by one), tiles that touch
    several times their 192 owners and so need more than 48 KB of dynamic LDS.  Per-part parity through the parity hook, then one
    evaluation through the production path (lumped virial) against the oracle."""
    from scema_amd import capi
    st = topo_stats(net5)
    assert st["dihedral_spans"][2] + st["dihedral_spans"][3] >= 500 and st["dihedral_spans"][3] >= 100
    assert st["touched"].max() * LDS_PER_LOCAL_ATOM > 48 * 1024 and st["touched"].max() <= 1024
    eng = engine()
    static_parity(eng, "net5", net5)
    strain = strain_of(net5)
    out = eng.strain_batch([capi.make_sim(7, "net5", 1, strain, nss=10, most_recent=capi.QP_NONE)])
    exp, nts = oracle(net5).eval(strain, 2.0, 300.0, 1e-4, 10)
    assert out[0].stress_updated == 1 and nts == 10
    assert relerr(np.array(out[0].stress[:]), exp) < 1e-6
    eng.close()


# 4 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["network", "pe"])
def test_scrambled_atom_numbering(net4, small_pe, which):
    """build_topo ranks the atoms itself, 'whatever the numbering of the input': the same system under a random permutation of the atom
    indices (every term relabelled) against the oracle on the permuted input, and force by force against the unpermuted GPU run."""
    d = net4 if which == "network" else with_weights(small_pe, (0.0, 0.0, 0.5), (0.0, 0.0, 0.8333))
    perm = np.random.default_rng(17).permutation(d["natoms"])
    dp = permuted(d, perm)
    assert (perm != np.arange(len(perm))).mean() > 0.9
    assert np.abs(np.diff(dp["bonds"], axis=1)).mean() > d["natoms"] / 4       # bonded atoms are far apart in the input now (random: n / 3)
    eng = engine()
    f, e, w, info, _ = static_parity(eng, "plain", d)
    fp, ep, wp, info_p, _ = static_parity(eng, "scrambled", dp)
    assert info_p["npairs"] == info["npairs"]
    assert relerr(fp, f[perm]) < 1e-11
    assert np.all(np.abs(ep[:7] - e[:7]) < 1e-10 * np.maximum(1.0, np.abs(e[:7])))
    eng.close()


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_mixed_launch_of_small_and_large_tiles(small_pe, net4, net5):
    """One launch of k_bonded over replicas of three topologies lays out LDS by the launch's largest tile and coefficient table,
    not by the replica's own: every stress equals that replica's evaluation alone (tolerance and neigh_delay = 0 as in
    test_a_replica_does_not_know_its_batch)."""
    from scema_amd import capi
    systems = {"pe": small_pe, "net5": net5, "net4": net4}
    touched = {k: topo_stats(d)["touched"].max() for k, d in systems.items()}
    assert touched["pe"] < 300 < touched["net4"] < 600 < touched["net5"]
    ncoef = {k: 2 * len(d["bond_coeff"]) + 2 * len(d["angle_coeff"]) + 4 * len(d["dihedral_coeff"]) + 2 * len(d["improper_coeff"]) for k, d in systems.items()}
    assert ncoef["pe"] != ncoef["net5"]

    def run(names):
        eng = engine(kspace_accuracy=1e-4, neigh_delay=0)
        for k in names:
            eng.register_replica(k, 1, systems[k])
        out = eng.strain_batch([capi.make_sim(q, k, 1, strain_of(systems[k], 1e-3 + 2e-4 * q), nss=10, most_recent=capi.QP_NONE) for q, k in enumerate(names)])
        assert all(o.stress_updated == 1 for o in out)
        res = np.array([list(o.stress) for o in out])
        eng.close()
        return res

    names = ["pe", "net5", "net4"]
    together = run(names)
    scale = np.abs(together).max()
    for q, k in enumerate(names):
        eng = engine(kspace_accuracy=1e-4, neigh_delay=0)
        eng.register_replica(k, 1, systems[k])
        alone = np.array(eng.strain_batch([capi.make_sim(q, k, 1, strain_of(systems[k], 1e-3 + 2e-4 * q), nss=10, most_recent=capi.QP_NONE)])[0].stress[:])
        eng.close()
        assert np.abs(together[q] - alone).max() < 1e-9 * scale, (k, np.abs(together[q] - alone).max() / scale)


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_clamped_angles_and_impropers():
    """Linear angles (theta0 = 180 degrees) and planar impropers (chi0 = 0) inside, at the edge of and outside the sin clamp: the kernel's
    `s2 > 1e-6 ? rsq64(s2) : 1000` and `sn < 0.001` against the oracle.  Where acos is ill-conditioned the kernel's cosine differs
    from the oracle's by an ulp and the angle by ulp / sin: there the budget is ten times the oracle's own deviation from the
    extended-precision value (test_oracle_topologies.test_clamped_terms_against_extended_precision), elsewhere 1e-11 of the molecule's
    largest force.  Forces stay finite (and vanish) at exactly 180 degrees and exactly 0."""
    d, ranges = clamp_molecules()
    assert_clamp_cases(d)
    eng = engine()
    eng.register_replica("clamp", 1, d)
    f, e, w, info = eng.debug_compute("clamp", 1, use_shake=False)
    o = oracle(d)
    o.setup(use_shake=False)
    fo, eo, wo = o.compute()
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(e)) and np.all(np.isfinite(w))
    ill = ANGLE_ILL + CHI_ILL
    assert len(ranges) == len(ANGLE_DEG) + len(CHI) == len(ill)
    for m, (lo, hi) in enumerate(ranges):
        err = np.abs(f[lo:hi] - fo[lo:hi]).max()
        top = np.abs(fo[lo:hi]).max()
        print(f"molecule {m}: largest force {top:.3e}, deviation from the oracle {err:.3e}")
        if ill[m]:
            assert err <= 10 * (ANGLE_ILL_DEV if m < len(ANGLE_DEG) else IMPROPER_ILL_DEV), (m, err)
        else:
            assert top > 0.1 and err < 1e-11 * top, (m, err, top)
    for part in (3, 5):
        assert abs(e[part] - eo[part]) < 1e-10 * max(1.0, abs(eo[part]))
        assert np.abs(w[part] - wo[part]).max() < 1e-10 * max(1.0, np.abs(wo[part]).max())
    eng.close()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_a_tile_that_touches_more_than_1024_atoms_is_refused(small_pe):
    """The term descriptors hold 10-bit local atom indices: a topology one of whose tiles touches more atoms is refused at registration
    (an argument error on the host; nothing reaches the device), and the engine goes on to serve other replicas."""
    from scema_amd import capi
    from scema_amd.systems import build_network
    big = build_network(6, drop=0.0, seed=6, special_lj=(0.0, 0.0, 0.5), special_coul=(0.0, 0.0, 0.5))
    assert topo_stats(big)["touched"].max() > 1024
    eng = engine()
    with pytest.raises(capi.EngineError) as err:
        eng.register_replica("big", 1, big)
    msg = str(err.value)
    assert msg.startswith("rc=1:") and "bonded tile" in msg and "1024" in msg, msg       # SCEMA_MD_ERR_ARG
    static_parity(eng, "pe", small_pe, use_shake=True)
    eng.close()
