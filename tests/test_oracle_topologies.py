"""The CPU oracle on branched topologies with fractional special weights (systems.build_network), pinned by a reference that
shares no hand-derived force or virial formula with it: the energy restated in torch.float64 (all-pairs minimum-image
Lennard-Jones weighted by bond-graph distance, harmonic bonds and angles, OPLS dihedrals, harmonic impropers), forces by
autograd, the virial as the derivative with respect to a homogeneous strain.  Plus finite differences through the fractional
k-space correction, and the clamps of the angle and improper terms against the same formulas in extended precision.

The helpers at the top are shared with tests/test_gpu_topologies.py."""
import numpy as np
import pytest

from oracle import pyoracle as po

KW = dict(cut_lj=5.0, cut_coul=4.0, skin=1.0)
OWNERS = 192          # owner atoms of a bonded tile (BT_OWNERS)


# ---------------------------------------------------------------------------------------------------------------------
# fixtures and topology bookkeeping
# ---------------------------------------------------------------------------------------------------------------------
def network_fixture(charge=0.2, special_coul=(0.0, 0.0, 0.8333)):
    """512-atom network, 15 % of the bonds dropped, tilted box, special_bonds lj 0 0 0.5 / coul as given."""
    from scema_amd.systems import build_network
    d = build_network(4, drop=0.15, seed=3, charge=charge, special_lj=(0.0, 0.0, 0.5), special_coul=special_coul)
    d["box"][6:9] = [0.5, -0.3, 0.4]
    return d


def with_weights(d, special_lj, special_coul):
    d = dict(d)
    d["special_lj"] = np.array(special_lj, float)
    d["special_coul"] = np.array(special_coul, float)
    return d


def bond_levels(d):
    """(n, n) matrix: 1, 2, 3 for atoms one, two, three bonds apart (the lowest level wins), 0 otherwise."""
    n = int(d["natoms"])
    a = np.zeros((n, n))                       # (path counts stay far below 2^53: exact in floating point)
    b = np.asarray(d["bonds"]).reshape(-1, 2)
    a[b[:, 0], b[:, 1]] = 1
    a[b[:, 1], b[:, 0]] = 1
    a2 = a @ a
    a3 = a2 @ a
    lvl = np.where(a > 0, 1, np.where(a2 > 0, 2, np.where(a3 > 0, 3, 0)))
    np.fill_diagonal(lvl, 0)
    return lvl


def topo_stats(d):
    """What the tests assert before they compare anything, restated from the documented layout of the bonded tiles: atoms ranked
    breadth-first (roots in index order, neighbours in bond-input order), OWNERS consecutive ranks per tile, every term and every
    special pair (a pair within three bonds whose weights are not both 1) given to each tile that owns one of its atoms.  Returns the
    partners per atom, the atoms each tile touches, and how many dihedrals span 1, 2, 3, 4 tiles."""
    n = int(d["natoms"])
    lvl = bond_levels(d)
    wl, wc = np.asarray(d["special_lj"]), np.asarray(d["special_coul"])
    special = np.zeros_like(lvl, bool)
    for k in range(3):
        if not (wl[k] == 1.0 and wc[k] == 1.0):
            special |= lvl == k + 1
    adj = [[] for _ in range(n)]
    for i, j in np.asarray(d["bonds"]).reshape(-1, 2):
        adj[i].append(int(j)); adj[j].append(int(i))
    rank = -np.ones(n, np.int64)
    nr = 0
    for root in range(n):
        if rank[root] >= 0:
            continue
        rank[root] = nr; nr += 1
        queue = [root]
        for h in queue:
            for c in adj[h]:
                if rank[c] < 0:
                    rank[c] = nr; nr += 1
                    queue.append(c)
    tile = rank // OWNERS
    touched = np.zeros((tile.max() + 1, n), bool)
    touched[tile, np.arange(n)] = True
    for rows in [np.asarray(d[key]) for key in ("bonds", "angles", "dihedrals", "impropers")] + [np.argwhere(np.triu(special))]:
        for c1 in range(rows.shape[1]):
            for c2 in range(rows.shape[1]):
                touched[tile[rows[:, c1]], rows[:, c2]] = True
    dt = np.sort(tile[np.asarray(d["dihedrals"]).reshape(-1, 4)], axis=1)
    spans = np.bincount(1 + (np.diff(dt, axis=1) != 0).sum(1), minlength=5)[1:5]
    return dict(partners=special.sum(1), touched=touched.sum(1), dihedral_spans=spans, rank=rank)


def permuted(d, perm):
    """The same system with atom k of the result being atom perm[k] of `d`; every term relabelled."""
    perm = np.asarray(perm)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    out = dict(d)
    for key in ("type", "charge", "x", "v"):
        out[key] = np.ascontiguousarray(np.asarray(d[key])[perm])
    if "mol" in d:
        out["mol"] = np.asarray(d["mol"])[perm]
    for key in ("bonds", "angles", "dihedrals", "impropers"):
        out[key] = inv[np.asarray(d[key])].astype(np.int32)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the independent reference
# ---------------------------------------------------------------------------------------------------------------------
def reference_energy_force_virial(d, cut_lj):
    """Per-part energies (lj, bond, angle, dihedral, improper), total forces and the total virial (xx, yy, zz, xy, xz, yz) of an
    uncharged system.  x' = (1 + eta) x, box' = (1 + eta) box; F = -dE/dx, W_ab = -dE/d eta_ab at eta = 0."""
    import torch
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    n = int(d["natoms"])
    box = np.asarray(d["box"], float)
    h = t64([[box[3] - box[0], 0, 0], [box[6], box[4] - box[1], 0], [box[7], box[8], box[5] - box[2]]])   # rows: cell vectors
    hinv = torch.linalg.inv(h)
    x = t64(d["x"]).requires_grad_(True)
    eta = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
    strain = torch.eye(3, dtype=torch.float64) + eta

    def sep(i, j):   # minimum-image r_i - r_j in the strained box (the image is chosen in the unstrained one)
        dv = x[i] - x[j]
        img = torch.round(dv @ hinv).detach()
        return (dv - img @ h) @ strain.T

    idx = lambda a: torch.tensor(np.asarray(a, np.int64))
    typ = np.asarray(d["type"])
    # Lennard-Jones over all pairs, weighted by bond-graph distance
    i, j = np.triu_indices(n, 1)
    lvl = bond_levels(d)[i, j]
    w = np.where(lvl > 0, np.asarray(d["special_lj"])[np.maximum(lvl, 1) - 1], 1.0)
    r2 = (sep(idx(i), idx(j)) ** 2).sum(1)
    s6 = (t64(np.asarray(d["sigma"])[typ[i], typ[j]]) ** 2 / r2) ** 3
    e_pair = t64(w) * 4.0 * t64(np.asarray(d["eps"])[typ[i], typ[j]]) * (s6 * s6 - s6)
    e_lj = e_pair[r2.detach() < cut_lj ** 2].sum()
    # harmonic bonds
    b = idx(d["bonds"]); cf = t64(d["bond_coeff"])[idx(d["bond_type"])]
    r = sep(b[:, 0], b[:, 1]).norm(dim=1)
    e_bond = (cf[:, 0] * (r - cf[:, 1]) ** 2).sum()
    # harmonic angles
    a = idx(d["angles"]); cf = t64(d["angle_coeff"])[idx(d["angle_type"])]
    d1, d2 = sep(a[:, 0], a[:, 1]), sep(a[:, 2], a[:, 1])
    theta = torch.atan2(torch.linalg.cross(d1, d2).norm(dim=1), (d1 * d2).sum(1))
    e_angle = (cf[:, 0] * (theta - cf[:, 1]) ** 2).sum()

    def torsion(t):   # IUPAC dihedral angle of atoms 1-2-3-4, signed, from atan2
        b1, b2, b3 = sep(t[:, 1], t[:, 0]), sep(t[:, 2], t[:, 1]), sep(t[:, 3], t[:, 2])
        n1, n2 = torch.linalg.cross(b1, b2), torch.linalg.cross(b2, b3)
        return torch.atan2((torch.linalg.cross(n1, n2) * b2).sum(1) / b2.norm(dim=1), (n1 * n2).sum(1))

    # OPLS dihedrals
    k = t64(d["dihedral_coeff"])[idx(d["dihedral_type"])]
    phi = torsion(idx(d["dihedrals"]))
    e_dih = 0.5 * (k[:, 0] * (1 + torch.cos(phi)) + k[:, 1] * (1 - torch.cos(2 * phi)) + k[:, 2] * (1 + torch.cos(3 * phi))
                   + k[:, 3] * (1 - torch.cos(4 * phi))).sum()
    # harmonic impropers: the unsigned angle between the planes (1, 2, 3) and (2, 3, 4)
    cf = t64(d["improper_coeff"])[idx(d["improper_type"])]
    chi = torsion(idx(d["impropers"])).abs()
    e_imp = (cf[:, 0] * (chi - cf[:, 1]) ** 2).sum()
    parts = [e_lj, e_bond, e_angle, e_dih, e_imp]
    gx, geta = torch.autograd.grad(sum(parts), [x, eta])
    g = -geta.numpy()
    # (the energy depends on distances only: the strain derivative is symmetric, asserted by the caller through xy = yx)
    return (np.array([float(p.detach()) for p in parts]), -gx.numpy(), np.array([g[0, 0], g[1, 1], g[2, 2], g[0, 1], g[0, 2], g[1, 2]]),
            np.array([g[1, 0], g[2, 0], g[2, 1]]))


@pytest.fixture(scope="module")
def uncharged():
    return network_fixture(charge=0.0)


def test_fixture_has_what_it_is_named_for(uncharged):
    st = topo_stats(uncharged)
    p = st["partners"]
    assert p.max() >= 25 and (p == 16).any() and (p < 16).any() and p.min() == 0
    assert (np.asarray(uncharged["dihedral_type"]) == 2).sum() > 100 and len(uncharged["impropers"]) > 100
    lens = uncharged["box"][3:6] - uncharged["box"][:3]
    assert lens.min() > 2 * (KW["cut_lj"] + KW["skin"])


def test_oracle_matches_the_autograd_reference(uncharged):
    """Oracle against the torch.float64 restatement on the uncharged 512-atom network (lj 0 0 0.5, 131 k pairs).

    Measured deviations (this fixture, x86-64): forces 3.8e-15 of the largest force; per-part energies 3.1e-15 relative;
    total virial 2.5e-15 of its largest component.  Asserted: ten times each (summation order over the pairs, nothing else)."""
    d = uncharged
    o = po.Oracle(d, po.default_params(kspace_accuracy=1e-5, **KW))
    o.setup(use_shake=False)
    f, e, w = o.compute()
    er, fr, wr, wr_t = reference_energy_force_virial(d, KW["cut_lj"])
    assert e[1] == 0.0 and e[6] == 0.0                       # uncharged: nothing but the five parts of the reference
    assert np.abs(wr[3:] - wr_t).max() < 1e-12 * np.abs(wr).max()
    eo = e[[0, 2, 3, 4, 5]]
    assert np.all(np.abs(er) > 1.0)                          # every part is really there
    dev_f = np.abs(f - fr).max() / np.abs(fr).max()
    dev_e = (np.abs(eo - er) / np.abs(er)).max()
    dev_w = np.abs(w.sum(0) - wr).max() / np.abs(wr).max()
    print(f"oracle vs autograd reference: forces {dev_f:.2e}, energies {dev_e:.2e}, virial {dev_w:.2e}")
    assert dev_f < 3.8e-14
    assert dev_e < 3.1e-14
    assert dev_w < 2.5e-14


def test_energy_force_consistency_per_term_charged_network():
    """test_oracle_physics.test_energy_force_consistency_per_term on the charged network with lj 0 0 0.5, coul 0 0 0.8333: central
    differences of the total energy through the weighted real-space term, i.e. the k-space sum minus (1 - 0.8333) q q / r."""
    d = network_fixture(charge=0.2)
    o = po.Oracle(d, po.default_params(kspace_accuracy=1e-6, kspace_pppm=0, **KW))
    o.setup(use_shake=False)
    f, e, w = o.compute()
    assert abs(e[1]) > 1.0 and abs(e[6]) > 1e-3
    box, x, v = o.get_state()
    h = 1e-5
    rng = np.random.default_rng(0)
    partners = topo_stats(d)["partners"]
    picks = list(rng.choice(o.n, 5, replace=False)) + [int(np.argmax(partners))]
    assert partners[picks].max() > 16
    for i in picks:
        for k in range(3):
            xp = x.copy(); xp[i, k] += h
            o.set_state(box, xp, v); _, ep, _ = o.compute()
            xm = x.copy(); xm[i, k] -= h
            o.set_state(box, xm, v); _, em, _ = o.compute()
            fd = -(ep.sum() - em.sum()) / (2 * h)
            assert abs(fd - f[i, k]) <= 1e-7 * max(1.0, abs(f[i, k])), (i, k, fd, f[i, k])
    assert np.abs(f.sum(0)).max() < 1e-9


# ---------------------------------------------------------------------------------------------------------------------
# the clamps of the angle and improper terms
# ---------------------------------------------------------------------------------------------------------------------
ANGLE_DEG = (180.0, 179.98, 179.0)           # theta0 = 180 degrees
CHI = (0.0, 5e-4, 2e-3, 0.1)                 # chi0 = 0
ANGLE_ILL = (True, True, False)              # where acos is ill-conditioned: |d theta| of the order of ulp(cos) / sin
CHI_ILL = (True, True, True, False)
# the oracle's own deviation from the extended-precision value over the ill-conditioned cases (kcal/mol/A, measured by
# test_clamped_terms_against_extended_precision): the yardstick of the GPU clamp test
ANGLE_ILL_DEV = 3.5e-12
IMPROPER_ILL_DEV = 9.5e-13


def clamp_molecules():
    """Three 3-atom molecules with one linear angle each (theta0 = 180 degrees; theta = ANGLE_DEG) and four 4-atom molecules with
    one planar improper each (chi0 = 0; chi = CHI), 7 A apart in a 28 A box, no charges, eps = 0 and no bond terms: nothing but the
    term under test acts.  The exactly linear and exactly planar molecules lie along the axes (so they are exact in binary), the
    others are turned into a general orientation.  Returns the system and the atom ranges of the molecules."""
    c, s = np.cos(0.7), np.sin(0.7)
    turn = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    x, angles, imps, ranges = [], [], [], []
    for m, deg in enumerate(ANGLE_DEG):
        th = np.deg2rad(deg)
        loc = np.array([[1.5, 0, 0], [0, 0, 0], [1.5 * np.cos(th), 1.5 * np.sin(th), 0]]) if deg != 180.0 else np.array([[1.5, 0, 0], [0, 0, 0], [-1.5, 0, 0]])
        if deg != 180.0:
            loc = loc @ turn.T
        base = len(x)
        x += list(loc + np.array([4.0 + 7.0 * m, 4.0, 4.0]))
        angles.append([base, base + 1, base + 2]); ranges.append((base, base + 3))
    for m, chi in enumerate(CHI):
        loc = np.array([[-0.5, 1.375, 0], [0, 0, 0], [1.5, 0, 0], [2.0, 1.375 * np.cos(chi), 1.375 * np.sin(chi)]])
        if chi != 0.0:
            loc = loc @ turn.T
        base = len(x)
        x += list(loc + np.array([4.0 + 7.0 * (m % 3), 11.0 + 7.0 * (m // 3), 11.0]))
        imps.append([base, base + 1, base + 2, base + 3]); ranges.append((base, base + 4))
    n = len(x)
    z = lambda *sh: np.zeros(sh, np.int32)
    d = dict(natoms=n, ntypes=1, type=z(n), charge=np.zeros(n), mass=np.array([12.011]), eps=np.zeros((1, 1)), sigma=np.ones((1, 1)),
             bonds=z(0, 2), bond_type=z(0), bond_coeff=np.zeros((0, 2)),
             angles=np.array(angles, np.int32), angle_type=z(len(angles)), angle_coeff=np.array([[60.0, np.pi]]),
             dihedrals=z(0, 4), dihedral_type=z(0), dihedral_coeff=np.zeros((0, 4)),
             impropers=np.array(imps, np.int32), improper_type=z(len(imps)), improper_coeff=np.array([[10.0, 0.0]]),
             special_lj=np.array([0.0, 0.0, 1.0]), special_coul=np.array([0.0, 0.0, 1.0]),
             box=np.array([0, 0, 0, 28.0, 28.0, 28.0, 0, 0, 0]), x=np.array(x), v=np.zeros((n, 3)))
    return d, ranges


def clamp_sines(d):
    """sin(theta) of every angle and sin(chi) of every improper of the system: where each molecule sits relative to the clamp at 0.001"""
    x = np.asarray(d["x"])
    unit = lambda v: v / np.linalg.norm(v)
    out = [np.linalg.norm(np.cross(unit(x[i] - x[j]), unit(x[k] - x[j]))) for i, j, k in d["angles"]]
    for i, j, k, l in d["impropers"]:
        n1, n2 = unit(np.cross(x[i] - x[j], x[j] - x[k])), unit(np.cross(x[l] - x[k], x[j] - x[k]))
        out.append(np.linalg.norm(np.cross(n1, n2)))
    return np.array(out)


def assert_clamp_cases(d):
    """the molecules are where their names say: exactly on the singularity, inside the clamp, outside it near and far"""
    sn = clamp_sines(d)
    assert sn[0] == 0.0 and 1e-4 < sn[1] < 1e-3 < 1e-2 < sn[2] < 2e-2
    assert sn[3] == 0.0 and 1e-4 < sn[4] < 1e-3 < sn[5] < 3e-3 and 0.09 < sn[6] < 0.11


def clamped_forces_extended(d):
    """The clamped LAMMPS formulas of angle_style harmonic and improper_style harmonic (sin clamped at 0.001) in numpy.longdouble,
    on the double-precision positions; no periodic images (the molecules sit inside the box).  Returns forces and the two energies."""
    L = np.longdouble
    x = np.asarray(d["x"]).astype(L)
    f = np.zeros_like(x)
    e_angle = e_imp = L(0)
    for (i1, i2, i3), t in zip(d["angles"], d["angle_type"]):
        K, th0 = L(d["angle_coeff"][t][0]), L(d["angle_coeff"][t][1])
        d1, d2 = x[i1] - x[i2], x[i3] - x[i2]
        rsq1, rsq2 = d1 @ d1, d2 @ d2
        r1, r2 = np.sqrt(rsq1), np.sqrt(rsq2)
        c = min(L(1), max(L(-1), (d1 @ d2) / (r1 * r2)))
        sn = max(np.sqrt(1 - c * c), L("0.001"))
        dth = np.arccos(c) - th0
        e_angle += K * dth * dth
        a = -2 * K * dth / sn
        f1 = a * c / rsq1 * d1 - a / (r1 * r2) * d2
        f3 = a * c / rsq2 * d2 - a / (r1 * r2) * d1
        f[i1] += f1; f[i3] += f3; f[i2] -= f1 + f3
    for at, t in zip(d["impropers"], d["improper_type"]):
        K, chi0 = L(d["improper_coeff"][t][0]), L(d["improper_coeff"][t][1])
        F, G, H = x[at[0]] - x[at[1]], x[at[1]] - x[at[2]], x[at[3]] - x[at[2]]
        A, B = np.cross(F, G), np.cross(H, G)
        a2, b2 = A @ A, B @ B
        iab = 1 / np.sqrt(a2 * b2)
        c = min(L(1), max(L(-1), (A @ B) * iab))
        sn = max(np.sqrt(1 - c * c), L("0.001"))
        dchi = np.arccos(c) - chi0
        e_imp += K * dchi * dchi
        dEdc = -2 * K * dchi / sn
        gA, gB = B * iab - c * A / a2, A * iab - c * B / b2
        dc = [np.cross(G, gA), None, None, np.cross(G, gB)]
        u = np.cross(gA, F) + np.cross(gB, H)
        dc[1], dc[2] = u - dc[0], -u - dc[3]
        for k in range(4):
            f[at[k]] -= dEdc * dc[k]
    return f, e_angle, e_imp


def test_clamped_terms_against_extended_precision():
    """Linear angles at theta0 = 180 degrees and planar impropers at chi0 = 0, inside, at the edge of and outside the sin clamp:
    the oracle against the same clamped formulas in 80-bit arithmetic.

    Where acos is well-conditioned (theta = 179 degrees, chi = 0.1) the oracle is held to 1e-11 of the molecule's largest force.
    Where it is not, an ulp of the cosine moves the angle by ulp / sin: measured deviation of the oracle's forces from the
    extended-precision ones, largest over the ill-conditioned molecules: angles 3.45e-12 kcal/mol/A (theta = 179.98 degrees, 2.5e-10 of
    that molecule's largest force), impropers 9.5e-13 (chi = 5e-4, 1.7e-10 of its largest force); 0 exactly for the linear and the
    planar molecule.  ANGLE_ILL_DEV / IMPROPER_ILL_DEV above record them, rounded up; the GPU test allows ten times as much."""
    assert np.finfo(np.longdouble).eps < 1e-18
    d, ranges = clamp_molecules()
    assert_clamp_cases(d)
    o = po.Oracle(d, po.default_params(kspace_accuracy=1e-5, **KW))
    o.setup(use_shake=False)
    f, e, w = o.compute()
    fx, ea, ei = clamped_forces_extended(d)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(w))
    assert abs(e[3] - float(ea)) < 1e-10 * max(1.0, float(ea)) and abs(e[5] - float(ei)) < 1e-10 * max(1.0, float(ei))
    ill = ANGLE_ILL + CHI_ILL
    dev = {"angle": 0.0, "improper": 0.0}
    for m, (lo, hi) in enumerate(ranges):
        kind = "angle" if m < len(ANGLE_DEG) else "improper"
        err = float(np.abs(f[lo:hi] - fx[lo:hi]).max())
        top = float(np.abs(fx[lo:hi]).max())
        print(f"{kind} molecule {m}: largest force {top:.3e}, oracle deviation {err:.3e}")
        if ill[m]:
            dev[kind] = max(dev[kind], err)
        else:
            assert top > 0.1 and err < 1e-11 * top, (m, err, top)
    print(f"ill-conditioned: angle {dev['angle']:.3e}, improper {dev['improper']:.3e}")
    # the exactly linear and the exactly planar molecule feel nothing
    assert np.abs(f[ranges[0][0]:ranges[0][1]]).max() < 1e-12 and np.abs(f[ranges[3][0]:ranges[3][1]]).max() < 1e-12
    assert dev["angle"] <= ANGLE_ILL_DEV and dev["improper"] <= IMPROPER_ILL_DEV
