"""Deterministic inputs for the grouped stream of k_bonded (scema_amd/csrc/md_bonded_groups.h), and the restatement in Python of what
build_topo makes of a topology: breadth-first ranks, special pairs, the dihedrals per central bond and the rule that decides which of
them become groups.  tests/test_bonded_groups_host.py, tests/test_oracle_bonded_zoo.py and tests/test_gpu_bonded_zoo.py share it.
Plain numpy, seeded, nothing read from disk; the systems are dicts in the format of scema_amd.systems.build_network.

zoo(weights)   41 small molecules on a lattice and 200 monatomic ions in a slab above them, 604 atoms in a tilted box of
               24.8 x 24.8 x 31.8 A.  Kinds (KINDS; four copies each, one more peroxide in front so that the tile boundaries at ranks 192
               and 384 fall inside a molecule): butane (CH3 ends; fix shake forms C + 3 H and C + 2 H clusters), methanol numbered C, X
               (the C-X bond is a (3, 1) group) and X, C (the same bond as (1, 3)), peroxide H-X-X-H ((1, 1)), propene ((2, 2), (2, 3) and
               an improper), a three-ring, a four-ring and a five-ring with substituents, a centre with five bonds next to an ordinary
               bond, a butane whose dihedrals have types 12..16 (type 14 in a group, 15 and 16 beyond the four-bit field: their bond keeps
               its terms), and a peroxide whose one dihedral is listed twice.
ua_chain()     one united-atom chain of 570 beads, a helix that winds 12.6 times through the periodic box: every interior bond is a
               (1, 1) group, 192 / 195 / 186 groups in its three tiles (three and four chunks of 64).

Lennard-Jones: five classes with sigma between 1.1 A (H) and 2.6 A and eps below 0.2 kcal/mol.  With W_B and W_C the 1-2 and 1-3
pairs carry a fraction of the full Lennard-Jones term at 0.96 .. 1.53 A and 1.6 .. 2.5 A.  At OPLS-AA's sigma of 3.5 A that is
(3.5 / 1.53)^12 = 2e4 times eps / r -- forces of 1e5 .. 1e6 kcal/mol/A, under which every other term would vanish in a relative budget.  With
sigma about 1.5 A the weighted 1-2 term is a few kcal/mol/A, the order of the bond and angle forces, and the weighted 1-3 term still
more than 1e-3 of the largest force (asserted by tests/test_oracle_bonded_zoo.py), so that an error in either shows."""
import collections

import numpy as np

from test_oracle_topologies import OWNERS, bond_levels

MAXTYPE = 15          # BTG_MAXTYPE: dihedral types a group's four-bit field holds
BOLTZ = 0.0019872067
MVV2E = 48.88821291 ** 2

W_A = ((0.0, 0.0, 0.5), (0.0, 0.0, 0.8333))
W_B = ((0.2, 0.6, 0.5), (0.3, 0.7, 0.8333))
W_C = ((0.2, 1.0, 0.5), (0.3, 1.0, 0.8333))


# ---------------------------------------------------------------------------------------------------------------------
# what build_topo makes of a topology, restated
# ---------------------------------------------------------------------------------------------------------------------
def bfs_rank(n, bonds):
    """breadth-first ranks as build_topo assigns them: roots in index order, neighbours in bond-input order"""
    adj = [[] for _ in range(n)]
    for i, j in bonds:
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
    return rank


def special_pairs(d):
    """pairs (i < j) within three bonds whose weights are not both 1, with their level"""
    lvl = bond_levels(d)
    wl, wc = np.asarray(d["special_lj"]), np.asarray(d["special_coul"])
    keep = np.zeros_like(lvl, bool)
    for k in range(3):
        if not (wl[k] == 1.0 and wc[k] == 1.0):
            keep |= lvl == k + 1
    ij = np.argwhere(np.triu(keep))
    return ij, lvl[ij[:, 0], ij[:, 1]]


def topology_of(d, owners=OWNERS):
    n = int(d["natoms"])
    bonds = np.asarray(d["bonds"]).reshape(-1, 2)
    pairs, levels = special_pairs(d)
    return dict(n=n, owners=owners, rank=bfs_rank(n, bonds), bonds=bonds, angles=np.asarray(d["angles"]).reshape(-1, 3),
                dihedrals=np.asarray(d["dihedrals"]).reshape(-1, 4), dihedral_type=np.asarray(d["dihedral_type"]).ravel(),
                pairs=pairs, levels=levels)


def sides(t):
    """per unordered central bond: the distinct end atoms on the side of the lower and of the higher central atom, and the (k, m) list"""
    out = collections.defaultdict(lambda: (set(), set(), []))
    for (a, b, c, d_), ty in zip(t["dihedrals"], t["dihedral_type"]):
        if b > c:
            a, b, c, d_ = d_, c, b, a
        s = out[(int(b), int(c))]
        s[0].add(int(a)); s[1].add(int(d_)); s[2].append((int(a), int(d_), int(ty)))
    return out


def stays_a_term(side):
    """the rule of group_dihedrals: all dihedrals of a central bond with more than three end atoms on a side, a (k, m) listed twice or a
    type the field does not hold stay terms"""
    ka, ma, km = side
    return len(ka) > 3 or len(ma) > 3 or len({(k, m) for k, m, _ in km}) < len(km) or any(ty >= MAXTYPE for _, _, ty in km)


def zoo_stats(d, owners=OWNERS):
    """What the tests assert before they compare anything, restated from the documented layout (md_bonded_groups.h): the set of
    (nk, nm) of the groups; the groups one of whose nk x nm fields is absent, as (c2, c3); per tile the groups it evaluates (a group goes
    to every tile that owns one of its atoms) and the dihedrals that stay terms there; per tile boundary b (between tiles b and b + 1)
    the groups with atoms on both sides; the special pairs per host: {1: on a bond, 2: on an angle, 0: none}.  Also the ranks."""
    t = topology_of(d, owners)
    tile = t["rank"] // owners
    ntile = int(tile.max()) + 1
    shapes, absent = set(), []
    groups_per_tile, left_per_tile = np.zeros(ntile, int), np.zeros(ntile, int)
    straddle = np.zeros(max(ntile - 1, 0), int)
    group_types = []
    for (c2, c3), side in sides(t).items():
        tiles_of = lambda atoms: sorted({int(tile[a]) for a in atoms})
        if stays_a_term(side):
            for k, m, _ in side[2]:
                for tl in tiles_of([k, c2, c3, m]):
                    left_per_tile[tl] += 1
            continue
        nk, nm = len(side[0]), len(side[1])
        shapes.add((nk, nm))
        if len(side[2]) < nk * nm:
            absent.append((c2, c3))
        tl = tiles_of([c2, c3] + list(side[0]) + list(side[1]))
        groups_per_tile[tl] += 1
        for b in range(len(straddle)):
            straddle[b] += tl[0] <= b < tl[-1]
        group_types.append(sorted(ty for _, _, ty in side[2]))
    outer = {(min(int(a), int(c)), max(int(a), int(c))) for a, _, c in t["angles"]}
    bonded = {(min(int(a), int(c)), max(int(a), int(c))) for a, c in t["bonds"]}
    hosts = {0: 0, 1: 0, 2: 0}
    for p in t["pairs"]:
        key = (int(p[0]), int(p[1]))
        hosts[1 if key in bonded else 2 if key in outer else 0] += 1
    return dict(shapes=shapes, absent=absent, groups_per_tile=groups_per_tile, straddle=straddle, left_per_tile=left_per_tile, hosts=hosts,
                group_types=group_types, rank=t["rank"], levels=t["levels"])


# ---------------------------------------------------------------------------------------------------------------------
# molecules
# ---------------------------------------------------------------------------------------------------------------------
C, H, X = 0, 1, 2                                  # atom types; 3, 4: the ions
R0 = {(C, C): 1.53, (C, H): 1.09, (C, X): 1.43, (X, X): 1.46, (H, X): 0.96}
BOND_TYPE = {(C, C): 0, (C, H): 1, (C, X): 2, (X, X): 3, (H, X): 4}
BOND_K = [250.0, 340.0, 300.0, 240.0, 450.0]
BOND_R = [R0[key] for key in sorted(BOND_TYPE, key=BOND_TYPE.get)]
# bond dipoles: the first atom of the key loses what the second gains.  Every molecule is neutral and has a polar bond.
DIPOLE = {(C, C): 0.0, (C, H): -0.12, (C, X): 0.2, (X, X): 0.0, (H, X): 0.35}


def _unit(v):
    return v / np.linalg.norm(v)


def _sprout(p, back, n, r, cone, phase, spread):
    """n positions at distance r from p whose bonds make the angle `cone` (degrees) with the unit vector `back`"""
    e1 = _unit(np.cross(back, [1.0, 0.0, 0.0]) if abs(back[0]) < 0.9 else np.cross(back, [0.0, 1.0, 0.0]))
    e2 = np.cross(back, e1)
    th = np.deg2rad(cone)
    return [p + r * (np.cos(th) * back + np.sin(th) * (np.cos(a) * e1 + np.sin(a) * e2)) for a in np.deg2rad(phase + spread * np.arange(n))]


def _tree(types, bonds):
    """atoms placed outward from atom 0: the first neighbour of the root along z, every other neighbour of an atom on a cone around the bond
    to its parent (tetrahedral; 100 degrees where four share it), staggered by depth"""
    n = len(types)
    adj = [[] for _ in range(n)]
    for i, j in bonds:
        adj[i].append(j); adj[j].append(i)
    r = lambda a, b: R0[tuple(sorted((types[a], types[b])))]
    pos = np.full((n, 3), np.nan)
    pos[0] = 0.0
    first = adj[0][0]
    pos[first] = [0.0, 0.0, r(0, first)]
    queue, depth, parent = [0, first], {0: 0, first: 1}, {0: first, first: 0}
    for a in queue:
        ch = [c for c in adj[a] if np.isnan(pos[c, 0])]
        if not ch:
            continue
        cone, spread = (109.5, 120.0) if len(ch) <= 3 else (100.0, 360.0 / len(ch))
        back = _unit(pos[parent[a]] - pos[a])
        for c, p in zip(ch, _sprout(pos[a], back, len(ch), 1.0, cone, 25.0 + 47.0 * depth[a], spread)):
            pos[c] = pos[a] + r(a, c) * (p - pos[a])
            parent[c] = a; depth[c] = depth[a] + 1
            queue.append(c)
    return pos


def _ring(nring, nsub, pucker):
    """regular polygon of C-C bonds in the xy plane (every other atom lifted by `pucker`), nsub substituents per ring atom outward"""
    rad = R0[(C, C)] / (2.0 * np.sin(np.pi / nring))
    types, bonds, pos = [C] * nring, [(i, (i + 1) % nring) for i in range(nring)], []
    for i in range(nring):
        a = 2.0 * np.pi * i / nring
        pos.append([rad * np.cos(a), rad * np.sin(a), pucker * (i % 2) * (i < nring - nring % 2)])
    for i in range(nring):
        a = 2.0 * np.pi * i / nring
        out = np.array([np.cos(a), np.sin(a), 0.0])
        sub = H if (nsub == 2 or i % 2 == 0) else X
        for s in range(nsub):
            tilt = np.deg2rad(55.0 * (1 - 2 * s) if nsub == 2 else 20.0 * (1 - 2 * (i % 2)))
            types.append(sub); bonds.append((i, len(types) - 1))
            pos.append(np.array(pos[i]) + R0[tuple(sorted((C, sub)))] * (np.cos(tilt) * out + np.array([0.0, 0.0, np.sin(tilt)])))
    return types, bonds, np.array(pos)


def _template(kind):
    """types, bonds, ideal positions, extra dihedrals (listed a second time) and a function (central bond, running index) -> dihedral type"""
    dtype = lambda bond, q: q % 13
    twice, improper = [], []
    if kind in ("butane", "butane_hi"):
        types = [C] * 4 + [H] * 10
        bonds = [(0, 1), (1, 2), (2, 3), (0, 4), (0, 5), (0, 6), (1, 7), (1, 8), (2, 9), (2, 10), (3, 11), (3, 12), (3, 13)]
        if kind == "butane_hi":
            # types 12, 13, 14 side by side in the nine fields of the central bond; 15 and 16 around (0, 1), whose dihedrals all stay terms
            dtype = lambda bond, q: {(1, 2): 12 + q % 3, (0, 1): 13 + q % 4}.get(bond, q % 13)
    elif kind == "methanol_cx":
        types, bonds = [C, X, H, H, H, H], [(0, 1), (0, 2), (0, 3), (0, 4), (1, 5)]
    elif kind == "methanol_xc":
        types, bonds = [X, C, H, H, H, H], [(0, 1), (0, 2), (1, 3), (1, 4), (1, 5)]
    elif kind in ("peroxide", "peroxide_twice"):
        types, bonds = [X, X, H, H], [(0, 1), (0, 2), (1, 3)]
        if kind == "peroxide_twice":
            twice = [((2, 0, 1, 3), 5)]
    elif kind == "propene":
        types = [C, C, C] + [H] * 6
        bonds = [(0, 1), (1, 2), (0, 3), (0, 4), (1, 5), (2, 6), (2, 7), (2, 8)]
        improper = [(1, 0, 2, 5)]
    elif kind == "five_bonds":
        # atom 0 with four X and the bond to atom 5; 5 - 6 is an ordinary C-C bond (a (3, 3) group: k = 0, H, H)
        types = [C, X, X, X, X, C, C] + [H] * 5
        bonds = [(0, 5), (0, 1), (0, 2), (0, 3), (0, 4), (5, 6), (5, 7), (5, 8), (6, 9), (6, 10), (6, 11)]
    elif kind in ("ring3", "ring4", "ring5"):
        types, bonds, pos = _ring(int(kind[4]), 1 if kind == "ring5" else 2, {"ring3": 0.0, "ring4": 0.25, "ring5": 0.3}[kind])
        return types, bonds, pos, twice, improper, dtype
    else:
        raise ValueError(kind)
    return types, bonds, _tree(types, bonds), twice, improper, dtype


KINDS = ("butane", "methanol_cx", "methanol_xc", "peroxide", "propene", "ring3", "ring4", "ring5", "five_bonds", "butane_hi", "peroxide_twice")
# the order of the molecules: four rounds of every kind, rotated so that another kind sits at each tile boundary
ORDER = ("peroxide",) + KINDS[3:] + KINDS[:3] + KINDS[5:] + KINDS[:5] + KINDS[1:] + KINDS[:1] + KINDS[8:] + KINDS[:8]


def _terms(n, bonds):
    """every angle and every proper dihedral of a bond graph; every second dihedral listed backwards"""
    adj = [[] for _ in range(n)]
    for i, j in bonds:
        adj[i].append(j); adj[j].append(i)
    angles = [(a, v, c) for v in range(n) for a in adj[v] for c in adj[v] if a < c]
    dih = []
    for j, k in bonds:
        for i in adj[j]:
            for l in adj[k]:
                if i != k and l != j and i != l:
                    dih.append(((i, j, k, l) if len(dih) % 2 else (l, k, j, i), (min(j, k), max(j, k))))
    return angles, dih


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q if np.linalg.det(q) > 0 else -q


def _min_image(dv, box):
    h = np.array([[box[3] - box[0], 0, 0], [box[6], box[4] - box[1], 0], [box[7], box[8], box[5] - box[2]]])
    return dv - np.round(dv @ np.linalg.inv(h)) @ h


def _assemble(types, charge, mol, mass, eps1, sig1, x, box, bonds, btype, bond_coeff, angles, dih, dtype, dihedral_coeff, imps, improper_coeff, weights, rng):
    """the dict; angle types from the ideal angles in buckets of five degrees (theta0 = the bucket's centre, K = 45), thermal velocities;
    and the geometry guards, from positions alone"""
    n = len(types)
    types = np.array(types, np.int32)
    sep = lambda i, j: _min_image(x[np.asarray(i)] - x[np.asarray(j)], box)
    angles = np.array(angles, np.int32).reshape(-1, 3)
    d1, d2 = sep(angles[:, 0], angles[:, 1]), sep(angles[:, 2], angles[:, 1])
    cs = (d1 * d2).sum(1) / np.linalg.norm(d1, axis=1) / np.linalg.norm(d2, axis=1)
    assert np.sqrt(1.0 - cs ** 2).min() > 0.05
    bucket = np.round(np.degrees(np.arccos(cs)) / 5.0).astype(int)
    used = sorted(set(bucket))
    atype = np.array([used.index(b) for b in bucket], np.int32)
    angle_coeff = np.array([[45.0, np.deg2rad(5.0 * b)] for b in used])
    dih = np.array(dih, np.int32).reshape(-1, 4)
    for rows in (dih, np.array(imps, np.int32).reshape(-1, 4)):
        f, g, hh = sep(rows[:, 0], rows[:, 1]), sep(rows[:, 1], rows[:, 2]), sep(rows[:, 3], rows[:, 2])
        na, nb = np.linalg.norm(np.cross(f, g), axis=1), np.linalg.norm(np.cross(hh, g), axis=1)
        ng = np.linalg.norm(g, axis=1)
        assert np.all(na > 0.2 * np.linalg.norm(f, axis=1) * ng) and np.all(nb > 0.2 * np.linalg.norm(hh, axis=1) * ng)   # no torsion near a singularity
    iu = np.triu_indices(n, 1)
    dist = np.linalg.norm(_min_image(x[iu[0]] - x[iu[1]], box), axis=1)
    assert dist.min() > 0.9, dist.min()
    mm = np.asarray(mass)[types]
    v = rng.normal(0.0, 1.0, (n, 3)) * np.sqrt(BOLTZ * 300.0 / (mm * MVV2E))[:, None]
    v -= (mm[:, None] * v).sum(0) / mm.sum()
    return dict(
        natoms=n, ntypes=len(mass), type=types, charge=np.array(charge, float), mol=np.array(mol, np.int32), mass=np.array(mass),
        eps=np.sqrt(np.outer(eps1, eps1)), sigma=np.sqrt(np.outer(sig1, sig1)),
        bonds=np.array(bonds, np.int32).reshape(-1, 2), bond_type=np.array(btype, np.int32), bond_coeff=np.array(bond_coeff),
        angles=angles, angle_type=atype, angle_coeff=angle_coeff,
        dihedrals=dih, dihedral_type=np.array(dtype, np.int32), dihedral_coeff=np.array(dihedral_coeff),
        impropers=np.array(imps, np.int32).reshape(-1, 4), improper_type=np.zeros(len(imps), np.int32), improper_coeff=np.array(improper_coeff),
        special_lj=np.array(weights[0], float), special_coul=np.array(weights[1], float),
        box=np.array(box, float), x=np.ascontiguousarray(x), v=np.ascontiguousarray(v))


NDTYPE = 17
DIHEDRAL_COEFF = [[0.6 + 0.07 * t, -(0.25 + 0.03 * t), 0.15 + 0.02 * t, -(0.08 + 0.01 * t)] for t in range(NDTYPE)]   # distinct, all four non-zero
SITE, ION_SITE, NION = 6.2, 3.1, 200


def zoo(weights=W_B, charged=True, seed=11):
    """see the module's docstring; `kind_of` (per molecule) and `mol` (per atom; the ions are molecule -1 .. kind "ion") say what is where"""
    rng = np.random.default_rng(seed)
    types, charge, mol, x, bonds, btype, angles, dih, dtype, imps, kind_of = [], [], [], [], [], [], [], [], [], [], []
    for m, kind in enumerate(ORDER):
        ty, bd, pos, twice, improper, type_of = _template(kind)
        n, base = len(ty), len(types)
        heavy = [i for i in range(n) if ty[i] != H]
        parent = {(i if ty[i] == H else j): (j if ty[i] == H else i) for i, j in bd if H in (ty[i], ty[j])}
        jit = np.zeros((n, 3))
        jit[heavy] = rng.normal(0.0, 0.015, (len(heavy), 3))
        for h, p in parent.items():
            jit[h] = jit[p]                        # a hydrogen moves with its heavy atom: the shaken bonds keep their exact r0
        site = np.array([m % 4, (m // 4) % 4, m // 16], float)
        pos = (pos - pos.mean(0) + jit) @ _rotation(rng).T + (site + 0.5) * SITE
        q = np.zeros(n)
        for i, j in bd:
            key = tuple(sorted((ty[i], ty[j])))
            lo, hi = (i, j) if ty[i] <= ty[j] else (j, i)
            q[lo] -= DIPOLE[key]; q[hi] += DIPOLE[key]
            bonds.append((base + i, base + j)); btype.append(BOND_TYPE[key])
        assert abs(q.sum()) < 1e-12 and np.abs(q).max() > 0.1
        ang, dh = _terms(n, bd)
        angles += [tuple(base + a for a in row) for row in ang]
        for qd, (row, bond) in enumerate(dh):
            dih.append(tuple(base + a for a in row)); dtype.append(type_of(bond, qd))
        for row, t in twice:
            dih.append(tuple(base + a for a in row)); dtype.append(t)
        imps += [tuple(base + a for a in row) for row in improper]
        types += ty; charge += list(q if charged else 0.0 * q); mol += [m] * n; x += list(pos); kind_of.append(kind)
    nmol_atoms = len(types)
    # the ions: a slab of four layers above the molecules, charges +- 0.5 in a checkerboard
    ztop = 3 * SITE
    for s in range(NION):
        i, j, k = s % 8, (s // 8) % 8, s // 64
        sign = 1 - 2 * ((i + j + k) % 2)
        types.append(3 if sign > 0 else 4); charge.append(0.5 * sign if charged else 0.0); mol.append(-1)
        x.append(np.array([(i + 0.5) * ION_SITE, (j + 0.5) * ION_SITE, ztop + 0.4 + (k + 0.5) * ION_SITE]) + rng.normal(0.0, 0.08, 3))
    assert abs(sum(charge)) < 1e-12
    box = [0.0, 0.0, 0.0, 4 * SITE, 4 * SITE, ztop + 0.4 + 4 * ION_SITE + 0.4, 0.5, -0.3, 0.4]
    d = _assemble(types, charge, mol, [12.011, 1.008, 15.999, 22.99, 35.45], [0.15, 0.03, 0.20, 0.05, 0.10], [1.7, 1.1, 1.6, 2.2, 2.6],
                  np.array(x), box, bonds, btype, [[k, r] for k, r in zip(BOND_K, BOND_R)],
                  angles, dih, dtype, DIHEDRAL_COEFF, imps, [[6.0, np.deg2rad(15.0)]], weights, rng)
    d["kind_of"], d["nmol_atoms"] = kind_of, nmol_atoms
    return d


def ua_chain(weights=W_B, n=570, seed=12):
    """see the module's docstring.  Bead s sits on a helix of radius 0.9 A, 100 degrees and 0.663 A along the axis per bead (bonds of 1.53 A),
    whose axis runs along (6.2, 1.55, 30) A, one passage of the box: thirteen passages, at least 6 A apart."""
    rng = np.random.default_rng(seed)
    lx, lz, rad, dphi = 24.8, 30.0, 0.9, np.deg2rad(100.0)
    rise = np.sqrt(1.53 ** 2 - (2.0 * rad * np.sin(0.5 * dphi)) ** 2)
    axis = _unit(np.array([0.25 * lx, 0.0625 * lx, lz]))
    e1 = _unit(np.cross(axis, [1.0, 0.0, 0.0]))
    e2 = np.cross(axis, e1)
    s = np.arange(n)[:, None]
    x = np.array([3.0, 3.0, 0.0]) + rise * s * axis + rad * (np.cos(dphi * s) * e1 + np.sin(dphi * s) * e2)
    x += rng.normal(0.0, 0.015, x.shape)
    box = [0.0, 0.0, 0.0, lx, lx, lz, 0.5, -0.3, 0.4]
    h = np.array([[lx, 0, 0], [box[6], lx, 0], [box[7], box[8], lz]])
    x -= np.floor(x @ np.linalg.inv(h)) @ h                       # wrapped into the box: the chain crosses its faces
    bonds = [(i, i + 1) for i in range(n - 1)]
    angles = [(i, i + 1, i + 2) for i in range(n - 2)]
    dih = [(i, i + 1, i + 2, i + 3) if i % 2 else (i + 3, i + 2, i + 1, i) for i in range(n - 3)]
    charge = [0.1 * (1 - 2 * (i % 2)) for i in range(n)]
    return _assemble([0] * n, charge, [0] * n, [14.027], [0.12], [1.7], x, box, bonds, [0] * len(bonds), [[250.0, 1.53]], angles, dih,
                     [i % 3 for i in range(len(dih))], DIHEDRAL_COEFF[:3], [], np.zeros((0, 2)), weights, rng)


def zoo_cases(z, chain):
    """what the zoo and the chain of tests/bonded_zoo.py are there for, from zoo_stats (shared with the oracle and GPU tests of the zoo)"""
    st = zoo_stats(z)
    assert z["natoms"] < 700 and len(st["groups_per_tile"]) == 4                     # three tiles with terms and one without
    # every shape of a group from one dihedral to nine, both ways round
    assert {(3, 3), (3, 1), (1, 3), (1, 1), (2, 2), (2, 3)} <= st["shapes"]
    # a zero field inside nk x nm: the three-rings' central bonds (the third ring atom on both sides), three per ring
    assert len(st["absent"]) == 3 * z["kind_of"].count("ring3")
    # groups and left-over dihedrals side by side in a tile; the boundaries at ranks 192 and 384 cut groups, of another kind of molecule each
    assert (st["groups_per_tile"][:3] > 0).all() and (st["left_per_tile"][:2] > 0).all() and (st["straddle"][:2] > 0).all()
    mol, rank = np.asarray(z["mol"]), st["rank"]
    cut = [{z["kind_of"][mol[int(np.flatnonzero(rank == r)[0])]] for r in (b - 1, b)} for b in (OWNERS, 2 * OWNERS)]
    assert all(len(c) == 1 for c in cut) and cut[0] != cut[1] and mol[rank == 2 * OWNERS] >= 0
    # the last tile: ions alone, no term and no group, and at least 193 charged atoms without bonds in all
    bonded = np.zeros(z["natoms"], bool)
    bonded[np.asarray(z["bonds"]).ravel()] = True
    assert (~bonded & (np.asarray(z["charge"]) != 0.0)).sum() >= 193 and not bonded[rank >= 3 * OWNERS].any()
    assert st["groups_per_tile"][3] == 0 and st["left_per_tile"][3] == 0
    # dihedral types 13 .. 16: 14 in a group next to 13 (all nine fields of that bond are set), 15 and 16 left as terms; 17 types in all
    assert len(z["dihedral_coeff"]) >= 17 and np.all(np.asarray(z["dihedral_coeff"]) != 0.0)
    assert len({tuple(row) for row in np.asarray(z["dihedral_coeff"])}) == len(z["dihedral_coeff"])
    assert any(len(ty) == 9 and 13 in ty and 14 in ty for ty in st["group_types"]) and max(max(ty) for ty in st["group_types"]) == 14
    assert {15, 16} <= set(int(ty) for ty in z["dihedral_type"])
    # mixed types in one group
    assert sum(len(set(ty)) > 1 for ty in st["group_types"]) > 50
    # hosts: every 1-2 pair on its bond, every 1-3 pair on an angle unless its atoms are bonded (three-rings), 1-4 pairs on none
    lv = st["levels"]
    assert st["hosts"] == {1: (lv == 1).sum(), 2: (lv == 2).sum(), 0: (lv == 3).sum()} and min(st["hosts"].values()) > 100
    assert st["hosts"][1] == len(z["bonds"])
    # SHAKE clusters of four, three and two atoms
    typ = np.asarray(z["type"])
    nh = np.bincount(np.asarray(z["bonds"])[typ[np.asarray(z["bonds"])[:, 1]] == 1][:, 0], minlength=z["natoms"])
    assert {1, 2, 3} <= set(nh) and nh.max() == 3 and (typ[np.asarray(z["bonds"])[:, 0]] != 1).all()
    # an atom with five bonds, whose dihedrals stay terms
    assert np.bincount(np.asarray(z["bonds"]).ravel()).max() == 5
    # the chain: three and four chunks of 64 groups per tile, every group a single dihedral
    sc = zoo_stats(chain)
    assert sc["shapes"] == {(1, 1)} and sc["groups_per_tile"].min() >= 129 and sc["left_per_tile"].sum() == 0
    assert sorted(-(-sc["groups_per_tile"] // 64)) == [3, 3, 4] and (sc["straddle"] > 0).all()
    return st, sc


# ---------------------------------------------------------------------------------------------------------------------
# the production kernel seen through one step (shared by tests/test_gpu_bonded_groups.py and tests/test_gpu_bonded_zoo.py)
# ---------------------------------------------------------------------------------------------------------------------
def masses(d):
    return np.asarray(d["mass"])[np.asarray(d["type"])][:, None]


def one_step(eng, name, d, state, use_shake):
    """m (v1 - v0) and the sampled pressure of one step without thermostat from `state`"""
    box, x, v = state
    eng.set_state(3, name, 1, box, x, v)
    p = eng.debug_run(name, 1, 1, 1.0, 300.0, qp=3, nvt=False, use_shake=use_shake, sample=True)
    _, _, v1 = eng.get_state(3, name, 1)
    return masses(d) * (v1 - v), np.array(p)


def probe(eng, name, d, state, use_shake, bound_f, bound_p, what):
    """mode 1 against mode 0 on one state; returns mode 1's (force, pressure)"""
    eng.bonded_grouping(0)
    f0, p0 = one_step(eng, name, d, state, use_shake)
    eng.bonded_grouping(1)
    f1, p1 = one_step(eng, name, d, state, use_shake)
    df, dp = np.abs(f1 - f0).max() / np.abs(f0).max(), np.abs(p1 - p0).max() / max(1.0, np.abs(p0).max())
    print(f"{what}: force difference {df:.3e} of the largest force, pressure difference {dp:.3e} of max(1, |p|) (largest |p| {np.abs(p0).max():.3e})")
    assert np.abs(f0).max() > 0.0 and df <= bound_f, (what, df)
    assert dp <= bound_p, (what, dp)
    return f1, p1
