"""The CPU oracle on the inputs of tests/bonded_zoo.py (small molecules, rings, a five-bonded centre, ions; special weights that differ
at every level), pinned by the torch.float64 autograd reference of tests/test_oracle_topologies.py, which weights by bond-graph level and
shares no force or virial formula with the oracle; by central differences through the k-space correction of weighted 1-2 and 1-3 pairs;
and the check that each of the six weighted contributions is large enough for the budgets of tests/test_gpu_bonded_zoo.py to see it.
No GPU needed."""
import numpy as np
import pytest

from bonded_zoo import KINDS, W_B, W_C, _min_image, ua_chain, zoo, zoo_cases, zoo_stats
from oracle import pyoracle as po
from test_oracle_topologies import KW, reference_energy_force_virial, with_weights


def test_inputs_hold_the_cases_they_are_there_for():
    """shapes of the groups, the absent field, tile boundaries through molecules, the empty last tile, types 13 .. 16, hosts per level,
    at least 129 groups per tile of the chain (bonded_zoo.zoo_cases; the geometry guards are asserted by the builders themselves)"""
    for w in (W_B, W_C):
        z = zoo(w)
        lens = z["box"][3:6] - z["box"][:3]
        assert lens.min() > 2 * (KW["cut_lj"] + KW["skin"]) and np.abs(z["box"][6:9]).min() > 0.0
        mol, q = np.asarray(z["mol"]), np.asarray(z["charge"])
        for m in range(len(z["kind_of"])):
            assert abs(q[mol == m].sum()) < 1e-12 and np.abs(q[mol == m]).max() > 0.1       # neutral, and charged
        assert abs(q[mol < 0].sum()) < 1e-12 and (q[mol < 0] != 0.0).all()
        assert len({(e, s) for e, s in zip(np.diag(z["eps"]), np.diag(z["sigma"]))}) >= 3
    st, sc = zoo_cases(zoo(W_B), ua_chain(W_B))
    # W_C: level 2 is not special -- bonds host pairs, angles none
    hc = zoo_stats(zoo(W_C))["hosts"]
    assert hc[2] == 0 and hc[1] == st["hosts"][1] and hc[0] == st["hosts"][0]


@pytest.mark.parametrize("name", ["W_B", "W_C"])
def test_oracle_matches_the_autograd_reference_on_the_zoo(name):
    """Oracle against the torch.float64 restatement on the uncharged zoo (604 atoms), every level weighted differently.

    Measured deviations (x86-64), W_B | W_C: forces 7.4e-15 | 7.4e-15 of the largest force; per-part energies 2.0e-15 | 1.3e-15
    relative; total virial 1.06e-14 | 1.08e-14 of its largest component.  Asserted: ten times each, all below 1e-12.  Per kind of molecule the force deviation relative
    to that kind's largest force is printed: the yardstick of the per-molecule GPU test."""
    d = zoo({"W_B": W_B, "W_C": W_C}[name], charged=False)
    o = po.Oracle(d, po.default_params(kspace_accuracy=1e-5, **KW))
    o.setup(use_shake=False)
    f, e, w = o.compute()
    er, fr, wr, wr_t = reference_energy_force_virial(d, KW["cut_lj"])
    assert e[1] == 0.0 and e[6] == 0.0
    assert np.abs(wr[3:] - wr_t).max() < 1e-12 * np.abs(wr).max()
    eo = e[[0, 2, 3, 4, 5]]
    assert np.all(np.abs(er) > 0.1)                          # every part is really there
    dev_f = np.abs(f - fr).max() / np.abs(fr).max()
    dev_e = (np.abs(eo - er) / np.abs(er)).max()
    dev_w = np.abs(w.sum(0) - wr).max() / np.abs(wr).max()
    print(f"oracle vs autograd reference, {name}: forces {dev_f:.2e}, energies {dev_e:.2e}, virial {dev_w:.2e}")
    mol = np.asarray(d["mol"])
    for kind in KINDS:
        sel = np.isin(mol, [m for m, k in enumerate(d["kind_of"]) if k == kind])
        print(f"  {kind}: largest force {np.abs(fr[sel]).max():.3e}, deviation {np.abs(f[sel] - fr[sel]).max() / np.abs(fr[sel]).max():.2e} of it")
    bf, be, bw = BUDGET[name]
    assert max(bf, be, bw) <= 1e-12
    assert dev_f < bf
    assert dev_e < be
    assert dev_w < bw


BUDGET = {"W_B": (7.4e-14, 2.0e-14, 1.06e-13), "W_C": (7.4e-14, 1.3e-14, 1.08e-13)}   # ten times the measured deviations of the docstring above


FD_STEP = 1e-3


def fd_atoms(d):
    """one shaken H, a ring atom of each ring size, the five-bonded centre, an ion: of each the first none of whose pair distances lies
    within 3 FD_STEP of a cutoff (the truncated potentials jump there, and a stencil that reaches 2 FD_STEP must not cross the jump)"""
    mol, typ, x = np.asarray(d["mol"]), np.asarray(d["type"]), np.asarray(d["x"])
    deg = np.bincount(np.asarray(d["bonds"]).ravel(), minlength=d["natoms"])
    of_kind = lambda kind: np.isin(mol, [m for m, k in enumerate(d["kind_of"]) if k == kind])

    def first(mask):
        for i in np.flatnonzero(mask):
            r = np.linalg.norm(_min_image(x - x[i], d["box"]), axis=1)
            if min(np.abs(r - KW["cut_lj"]).min(), np.abs(r - KW["cut_coul"]).min()) > 3 * FD_STEP:
                return int(i)

    picks = [first((typ == 1) & of_kind("butane")), first(of_kind("ring3") & (deg == 4)), first(of_kind("ring4") & (deg == 4)),
             first(of_kind("ring5") & (deg == 3)), first(deg == 5), first(mol < 0)]
    assert None not in picks and typ[picks[0]] == 1 and deg[picks[5]] == 0
    return picks


def test_energy_force_consistency_on_the_charged_zoo():
    """Central differences of the oracle's total energy on the charged zoo under W_B (coul 0.3 0.7 0.8333): the k-space sum minus
    (1 - w) q q / r at levels 1 and 2 as well as 3, through six atoms in all three components.  The difference is the five-point central one,
    (-E(2h) + 8 E(h) - 8 E(-h) + E(-2h)) / 12h, at h = 1e-3.  Two errors decide h.  The Ewald energy of this system (-7e3 kcal/mol) comes
    back with a rounding noise of 3e-11 from one position to the next, which a difference turns into 2e-11 / h: 2e-6 at the h = 1e-5 of
    test_energy_force_consistency_per_term_charged_network, 2e-8 at 1e-3.  And the three-point difference truncates at h^2 / 6 times the third derivative of the force, where
    the weighted 1-2 Lennard-Jones term at 1.1 A has 13 14 15 f / r^3 for that: 1e-6 at h = 1e-4 already (both printed); the five-point
    one leaves h^4 / 30 times the fifth, below 1e-8.  Measured with it: at most 3e-8."""
    d = zoo(W_B)
    o = po.Oracle(d, po.default_params(kspace_accuracy=1e-6, kspace_pppm=0, **KW))
    o.setup(use_shake=False)
    f, e, w = o.compute()
    assert abs(e[1]) > 1.0 and abs(e[6]) > 1e-3
    box, x, v = o.get_state()
    h = FD_STEP

    def energy(i, k, step):
        xs = x.copy(); xs[i, k] += step
        o.set_state(box, xs, v)
        return o.compute()[1].sum()

    for i in fd_atoms(d):
        for k in range(3):
            e1, e2 = energy(i, k, h) - energy(i, k, -h), energy(i, k, 2 * h) - energy(i, k, -2 * h)
            fd2, fd = -e1 / (2 * h), -(8 * e1 - e2) / (12 * h)
            print(f"atom {i} component {k}: force {f[i, k]:.6e}, five-point difference off by {fd - f[i, k]:.2e}, three-point by {fd2 - f[i, k]:.2e}")
            assert abs(fd - f[i, k]) <= 1e-7 * max(1.0, abs(f[i, k])), (i, k, fd, f[i, k])
    assert np.abs(f.sum(0)).max() < 1e-9


def test_every_weighted_contribution_is_really_there():
    """The oracle's forces under W_B against W_B with one of its six weights set to zero: Lennard-Jones and Coulomb at levels 1, 2 and 3
    each move some force component by at least 1e-3 of the largest force -- a hundred million times the force budget of the GPU tests, so
    an error of any size in one of these paths shows there.  Measured, levels 1 / 2 / 3: lj 5.5e-1 / 5.7e-3 / 1.8e-3, coul 3.4e-1 / 1.8e-1 / 1.2e-1."""
    d = zoo(W_B)

    def forces(lj, coul):
        o = po.Oracle(with_weights(d, lj, coul), po.default_params(kspace_accuracy=1e-5, **KW))
        o.setup(use_shake=False)
        return o.compute()[0]

    f0 = forces(*W_B)
    top = np.abs(f0).max()
    for which in (0, 1):
        for lvl in range(3):
            w = [list(W_B[0]), list(W_B[1])]
            w[which][lvl] = 0.0
            part = np.abs(forces(*w) - f0).max() / top
            print(f"{('lj', 'coul')[which]} level {lvl + 1}: {part:.3e} of the largest force ({top:.3e})")
            assert part >= 1e-3, (which, lvl, part)
