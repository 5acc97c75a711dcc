"""Synthetic OPLS-AA replica generator (SURVEY.md §8(d) "PE-10k").

The reference ships no OPLS nanoscale input (materials `g0`/`epoxy80` are only named:
input_configurations/inputs_dogbone_cuboid.json:42), so benchmarks and parity tests use a
deterministic all-atom polyethylene crystal whose force-field *styles* are exactly the ones
`lammps_scripts_opls/in.set.lammps:36-57` selects (lj/cut/coul/long, harmonic bonds/angles,
OPLS dihedrals, SHAKE on X-H, special_bonds 0/0/1 from in.init.lammps:31).

All index arrays are 0-based; types are 0-based (C=0, H=1).
"""
from __future__ import annotations

import numpy as np

BOLTZ = 0.0019872067
MVV2E = 48.88821291 ** 2

# orthorhombic polyethylene cell (Angstrom)
PE_A, PE_B, PE_C = 7.40, 4.93, 2.534


def build_pe(nx: int = 6, ny: int = 9, nz: int = 16, temperature: float = 300.0, seed: int = 1234,
             jitter: float = 0.0, shake_project: bool = False) -> dict:
    """All-atom PE crystal, 12 atoms per cell, chains bonded through the periodic z boundary.

    6x9x16 -> 10 368 atoms, box 44.40 x 44.37 x 40.54 A (the PE-10k replica of SURVEY.md §8d).
    Returns a dict of numpy arrays describing topology, coefficients, box, positions, velocities.
    """
    rcc, rch = 1.529, 1.090
    half_c = 0.5 * PE_C
    dperp = np.sqrt(rcc ** 2 - half_c ** 2) * 0.5  # zig-zag amplitude
    hh = np.deg2rad(107.8) * 0.5
    chains = [((0.0, 0.0), np.deg2rad(45.0)), ((0.5 * PE_A, 0.5 * PE_B), np.deg2rad(-45.0))]

    nchain = 2 * nx * ny
    ncar = 2 * nz  # carbons per chain
    natoms = nchain * ncar * 3
    x = np.zeros((natoms, 3))
    typ = np.zeros(natoms, dtype=np.int32)
    q = np.zeros(natoms)
    mol = np.zeros(natoms, dtype=np.int32)

    def cidx(ch, k):  # carbon k of chain ch
        return (ch * ncar + (k % ncar)) * 3

    ch = 0
    for ix in range(nx):
        for iy in range(ny):
            for (cx, cy), phi in chains:
                u = np.array([np.cos(phi), np.sin(phi), 0.0])
                w = np.array([-np.sin(phi), np.cos(phi), 0.0])
                ax = np.array([ix * PE_A + cx + 0.25 * PE_A, iy * PE_B + cy + 0.25 * PE_B, 0.0])
                for k in range(ncar):
                    s = 1.0 if k % 2 == 0 else -1.0
                    pc = ax + s * dperp * u + np.array([0, 0, (k + 0.5) * half_c])
                    i = cidx(ch, k)
                    x[i] = pc
                    x[i + 1] = pc + rch * (s * np.cos(hh) * u + np.sin(hh) * w)
                    x[i + 2] = pc + rch * (s * np.cos(hh) * u - np.sin(hh) * w)
                    typ[i], typ[i + 1], typ[i + 2] = 0, 1, 1
                    q[i], q[i + 1], q[i + 2] = -0.12, 0.06, 0.06
                    mol[i:i + 3] = ch
                ch += 1

    bonds, btype, angles, atype, dihs, dtype = [], [], [], [], [], []
    for ch in range(nchain):
        for k in range(ncar):
            c0, c1 = cidx(ch, k), cidx(ch, k + 1)
            cm = cidx(ch, k - 1)
            c2 = cidx(ch, k + 2)
            bonds += [(c0, c1), (c0, c0 + 1), (c0, c0 + 2)]
            btype += [0, 1, 1]
            angles += [(cm, c0, c1), (cm, c0, c0 + 1), (cm, c0, c0 + 2), (c1, c0, c0 + 1), (c1, c0, c0 + 2),
                       (c0 + 1, c0, c0 + 2)]
            atype += [0, 1, 1, 1, 1, 2]
            # dihedrals about c0-c1
            for X, tx in ((cm, 'C'), (c0 + 1, 'H'), (c0 + 2, 'H')):
                for Y, ty in ((c2, 'C'), (c1 + 1, 'H'), (c1 + 2, 'H')):
                    if tx == 'C' and ty == 'C':
                        dihs.append((X, c0, c1, Y)); dtype.append(0)
                    elif tx == 'H' and ty == 'C':
                        dihs.append((X, c0, c1, Y)); dtype.append(1)
                    elif tx == 'C' and ty == 'H':
                        dihs.append((Y, c1, c0, X)); dtype.append(1)
                    else:
                        dihs.append((X, c0, c1, Y)); dtype.append(2)

    mass = np.array([12.011, 1.008])
    eps1 = np.array([0.066, 0.030])
    sig1 = np.array([3.50, 2.50])
    eps = np.sqrt(np.outer(eps1, eps1))   # geometric mixing (pair_modify default for this style)
    sigma = np.sqrt(np.outer(sig1, sig1))

    box = np.array([0.0, 0.0, 0.0, nx * PE_A, ny * PE_B, nz * PE_C, 0.0, 0.0, 0.0])

    rng = np.random.default_rng(seed)
    if jitter > 0.0:
        x = x + rng.normal(0.0, jitter, x.shape)
    m = mass[typ]
    v = rng.normal(0.0, 1.0, (natoms, 3)) * np.sqrt(BOLTZ * temperature / (m * MVV2E))[:, None]
    v -= (m[:, None] * v).sum(0) / m.sum()
    dof = 3 * natoms - 3
    if shake_project:
        # "... then SHAKE-projected": remove the relative velocity along every constrained X-H bond
        # (mass-weighted, a few sweeps because the two C-H bonds of a CH2 share the carbon), then scale to T with
        # the constrained number of degrees of freedom, so a fix-shake run starts at the requested temperature
        ch = [(a, b) for (a, b), t in zip(bonds, btype) if t == 1]
        ia = np.array([a for a, _ in ch]); ib = np.array([b for _, b in ch])
        dvec = x[ia] - x[ib]
        dvec /= np.linalg.norm(dvec, axis=1)[:, None]
        for _ in range(50):
            for sel in (slice(0, None, 2), slice(1, None, 2)):   # the two H of a carbon in separate half-sweeps
                a, b, dh = ia[sel], ib[sel], dvec[sel]
                rel = ((v[a] - v[b]) * dh).sum(1)
                ma, mb = m[a], m[b]
                v[a] -= (mb / (ma + mb) * rel)[:, None] * dh
                v[b] += (ma / (ma + mb) * rel)[:, None] * dh
        v -= (m[:, None] * v).sum(0) / m.sum()
        dof -= len(ch)
    tcur = (m[:, None] * v * v).sum() * MVV2E / (dof * BOLTZ)
    if tcur > 0:
        v *= np.sqrt(temperature / tcur)

    return dict(
        natoms=natoms, ntypes=2, type=typ, charge=q, mol=mol, mass=mass, eps=eps, sigma=sigma,
        bonds=np.array(bonds, dtype=np.int32).reshape(-1, 2), bond_type=np.array(btype, dtype=np.int32),
        bond_coeff=np.array([[268.0, 1.529], [340.0, 1.090]]),
        angles=np.array(angles, dtype=np.int32).reshape(-1, 3), angle_type=np.array(atype, dtype=np.int32),
        angle_coeff=np.array([[58.35, np.deg2rad(112.7)], [37.5, np.deg2rad(110.7)], [33.0, np.deg2rad(107.8)]]),
        dihedrals=np.array(dihs, dtype=np.int32).reshape(-1, 4), dihedral_type=np.array(dtype, dtype=np.int32),
        dihedral_coeff=np.array([[1.3, -0.05, 0.2, 0.0], [0.0, 0.0, 0.3, 0.0], [0.0, 0.0, 0.3, 0.0]]),
        impropers=np.zeros((0, 4), dtype=np.int32), improper_type=np.zeros(0, dtype=np.int32),
        improper_coeff=np.zeros((0, 2)),
        special_lj=np.array([0.0, 0.0, 1.0]), special_coul=np.array([0.0, 0.0, 1.0]),
        box=box, x=np.ascontiguousarray(x), v=np.ascontiguousarray(v),
    )


def build_ethane_oh(nx: int = 3, ny: int = 3, nz: int = 3, spacing: float = 5.2, seed: int = 5, temperature: float = 200.0) -> dict:
    """Small molecular liquid-like lattice for SHAKE coverage: on every lattice site one ethane (C2H6: two star clusters of
    4 atoms = C + 3 H) and one heavy-H diatomic (a cluster of 2), randomly oriented.  OPLS-style terms: bonds, angles,
    H-C-C-H dihedrals; types 0 = C, 1 = H, 2 = O-like heavy atom; charges neutral per molecule."""
    rng = np.random.default_rng(seed)
    rCC, rCH, rOH = 1.529, 1.09, 0.96
    tet = np.deg2rad(110.7)
    x, typ, q, bonds, btype, angles, atype, dihs, dtype_ = [], [], [], [], [], [], [], [], []
    def rot():
        a = rng.normal(size=(3, 3)); qm, _ = np.linalg.qr(a)
        return qm if np.linalg.det(qm) > 0 else -qm
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                c = (np.array([i, j, k], float) + 0.5) * spacing
                R = rot()
                base = len(x)
                loc = [np.array([0, 0, -rCC / 2]), np.array([0, 0, rCC / 2])]
                for side, sgn in ((0, -1.0), (1, 1.0)):
                    for m in range(3):
                        phi = 2 * np.pi * m / 3 + (np.pi / 3 if side else 0.0)
                        # H at the tetrahedral angle from the C-C axis
                        d = np.array([np.sin(np.pi - tet) * np.cos(phi), np.sin(np.pi - tet) * np.sin(phi), sgn * np.cos(np.pi - tet)])
                        loc.append(loc[side] + rCH * d)
                for v in loc:
                    x.append(c + R @ v)
                typ += [0, 0] + [1] * 6
                q += [-0.18, -0.18] + [0.06] * 6
                bonds.append([base, base + 1]); btype.append(0)
                for side in (0, 1):
                    hs = [base + 2 + 3 * side + m for m in range(3)]
                    for h in hs:
                        bonds.append([base + side, h]); btype.append(1)
                        angles.append([h, base + side, base + 1 - side]); atype.append(0)      # H-C-C
                    for a in range(3):
                        for b in range(a + 1, 3):
                            angles.append([hs[a], base + side, hs[b]]); atype.append(1)          # H-C-H
                for a in range(3):
                    for b in range(3):
                        dihs.append([base + 2 + a, base, base + 1, base + 5 + b]); dtype_.append(0)   # H-C-C-H
                # heavy-H diatomic on the body-centre position of the lattice (4.5 A from the ethane centres)
                R2 = rot()
                o = c + 0.5 * spacing * np.ones(3)
                b2 = len(x)
                x.append(o); x.append(o + R2 @ np.array([rOH, 0.0, 0.0]))
                typ += [2, 1]; q += [-0.4, 0.4]
                bonds.append([b2, b2 + 1]); btype.append(2)
    x = np.array(x); n = len(x)
    mass = np.array([12.011, 1.008, 15.999])
    eps1 = np.array([0.066, 0.030, 0.17]); sig1 = np.array([3.5, 2.5, 3.12])
    eps = np.sqrt(np.outer(eps1, eps1)); sig = np.sqrt(np.outer(sig1, sig1))
    L = np.array([nx, ny, nz], float) * spacing
    typ = np.array(typ, np.int32)
    v = rng.normal(size=(n, 3)) * np.sqrt(0.0019872067 * temperature / (mass[typ][:, None] * 48.88821291 ** 2))
    v -= (v * mass[typ][:, None]).sum(0) / mass[typ].sum()
    z = lambda *sh: np.zeros(sh, np.int32)
    return dict(natoms=n, ntypes=3, type=typ, charge=np.array(q), mass=mass, eps=eps, sigma=sig,
                bonds=np.array(bonds, np.int32), bond_type=np.array(btype, np.int32),
                bond_coeff=np.array([[268.0, rCC], [340.0, rCH], [553.0, rOH]]),
                angles=np.array(angles, np.int32), angle_type=np.array(atype, np.int32),
                angle_coeff=np.array([[37.5, tet], [33.0, np.deg2rad(107.8)]]),
                dihedrals=np.array(dihs, np.int32), dihedral_type=np.array(dtype_, np.int32), dihedral_coeff=np.array([[0.0, 0.0, 0.3, 0.0]]),
                impropers=z(0, 4), improper_type=z(0), improper_coeff=np.zeros((0, 2)),
                special_lj=np.array([0.0, 0.0, 1.0]), special_coul=np.array([0.0, 0.0, 1.0]),
                box=np.array([0, 0, 0, L[0], L[1], L[2], 0.3, -0.2, 0.25]), x=x, v=v)


def build_network(nc: int = 4, drop: float = 0.0, seed: int = 3, jitter: float = 0.04, charge: float = 0.2,
                  special_lj=(0.0, 0.0, 0.5), special_coul=(0.0, 0.0, 0.5), temperature: float = 300.0) -> dict:
    """Periodic tetrahedral network: a diamond-cubic lattice of nc^3 cells of 8 sites, every site bonded to its four nearest
    neighbours through the periodic box -- the branched counterpart of the PE chains (40 partners within three bonds per
    atom, terms that span up to four bonded tiles, tiles whose halo is several times their owners).  Two atom types, one
    per sublattice, charges +-`charge`.  Angles, OPLS dihedrals (two types by the sublattice of the second atom; every
    third listed in reversed atom order; every seventh listed a second time with a third type) and one improper per fully
    bonded site (two types) are derived from the surviving bond graph: `drop` removes that fraction of the bonds at random,
    and all four bonds of one site, so that the partner counts run from 0 to 40.

    Bond length 1.55 A (cell 3.58 A: the box holds 2 x 6 A from nc = 4 on).  sigma 1.50 / 1.45 A keeps every pair off the
    repulsive wall -- the 1-4 pairs (from 2.97 A) and also the two ends of a dropped bond, which face each other at 1.55 A with
    the full Lennard-Jones term (minimum at 1.66 A) -- so the system can be run, not only evaluated.  Angles are tetrahedral
    and the impropers sit at 35 degrees, far from the clamps of both terms for any jitter of a few hundredths of an Angstrom."""
    rb = 1.55
    a = 4.0 * rb / np.sqrt(3.0)
    fcc = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0]])                  # in quarters of the cell
    arms = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]])
    m = 4 * nc
    site = {}
    pos = []
    for ix in range(nc):
        for iy in range(nc):
            for iz in range(nc):
                for f in fcc:
                    for sub in (0, 1):
                        p = 4 * np.array([ix, iy, iz]) + f + sub * arms[0]
                        site[tuple(p % m)] = len(pos)
                        pos.append(p)
    pos = np.array(pos)
    natoms = len(pos)
    typ = (np.arange(natoms) % 2).astype(np.int32)
    rng = np.random.default_rng(seed)
    bonds = [(i, site[tuple((pos[i] + d) % m)]) for i in range(0, natoms, 2) for d in arms]
    btype = [k % 2 for i in range(0, natoms, 2) for k in range(4)]
    if drop > 0.0:
        lone = int(rng.integers(natoms))
        keep = [k and lone not in b for b, k in zip(bonds, rng.random(len(bonds)) >= drop)]
        bonds = [b for b, k in zip(bonds, keep) if k]
        btype = [t for t, k in zip(btype, keep) if k]
    nbr = [[] for _ in range(natoms)]
    for i, j in bonds:
        nbr[i].append(j); nbr[j].append(i)
    angles, atype, dihs, dtype, imps, itype = [], [], [], [], [], []
    for j in range(natoms):
        for p in range(len(nbr[j])):
            for q in range(p + 1, len(nbr[j])):
                angles.append((nbr[j][p], j, nbr[j][q])); atype.append(int(typ[j]))
        if len(nbr[j]) == 4:
            imps.append((j, nbr[j][0], nbr[j][1], nbr[j][2])); itype.append(int(typ[j]))
    for j, k in bonds:
        for i in nbr[j]:
            for l in nbr[k]:
                if i == k or l == j:
                    continue
                nd = len(dihs)
                dihs.append((i, j, k, l) if nd % 3 else (l, k, j, i)); dtype.append(int(typ[dihs[-1][1]]))
                if nd % 7 == 0:
                    dihs.append((i, j, k, l)); dtype.append(2)
    mass = np.array([12.011, 14.007])
    eps1 = np.array([0.15, 0.20])
    sig1 = np.array([1.50, 1.45])
    x = pos * (a / 4.0) + rng.normal(0.0, jitter, (natoms, 3))
    q = np.where(typ == 0, charge, -charge).astype(float)
    mm = mass[typ]
    v = rng.normal(0.0, 1.0, (natoms, 3)) * np.sqrt(BOLTZ * temperature / (mm * MVV2E))[:, None]
    v -= (mm[:, None] * v).sum(0) / mm.sum()
    tcur = (mm[:, None] * v * v).sum() * MVV2E / ((3 * natoms - 3) * BOLTZ)
    if tcur > 0:
        v *= np.sqrt(temperature / tcur)
    i32 = lambda rows, w: np.array(rows, dtype=np.int32).reshape(-1, w)
    return dict(
        natoms=natoms, ntypes=2, type=typ, charge=q, mol=np.zeros(natoms, dtype=np.int32), mass=mass,
        eps=np.sqrt(np.outer(eps1, eps1)), sigma=np.sqrt(np.outer(sig1, sig1)),
        bonds=i32(bonds, 2), bond_type=np.array(btype, dtype=np.int32),
        bond_coeff=np.array([[268.0, rb], [300.0, rb + 0.01]]),
        angles=i32(angles, 3), angle_type=np.array(atype, dtype=np.int32),
        angle_coeff=np.array([[58.35, np.deg2rad(109.5)], [50.0, np.deg2rad(112.0)]]),
        dihedrals=i32(dihs, 4), dihedral_type=np.array(dtype, dtype=np.int32),
        dihedral_coeff=np.array([[1.3, -0.05, 0.2, 0.1], [0.3, 0.2, 0.3, 0.0], [-0.4, 0.0, 0.15, -0.05]]),
        impropers=i32(imps, 4), improper_type=np.array(itype, dtype=np.int32),
        improper_coeff=np.array([[4.5, np.deg2rad(35.0)], [2.0, np.deg2rad(30.0)]]),
        special_lj=np.array(special_lj, dtype=float), special_coul=np.array(special_coul, dtype=float),
        box=np.array([0.0, 0.0, 0.0, nc * a, nc * a, nc * a, 0.0, 0.0, 0.0]), x=np.ascontiguousarray(x), v=np.ascontiguousarray(v),
    )


def build_pe10k(seed: int = 1234) -> dict:
    """The PE-10k benchmark replica of SURVEY.md 8(d): 10 368 atoms, 300 K with SHAKE-projected velocities."""
    return build_pe(6, 9, 16, 300.0, seed, shake_project=True)


def synthetic_strains(n_sims: int, box_lengths, seed: int = 2026, scale: float = 1.0, mode: str = "balanced") -> np.ndarray:
    """eps_zz ~ U(1.0e-3,1.8e-3), eps_xx=eps_yy=-0.3 eps_zz, shears ~ U(-1e-4,1e-4).

    Returns the Angstrom-valued MDSim.strain (raw order xx,yy,zz,xy,xz,yz), i.e. true strain times
    the box length the reference pairs with each component (stmd_sync.h:552-557):
    diag x own length, xy x Lz, yz x Lx, xz x Ly.
    """
    rng = np.random.default_rng(seed)
    lx, ly, lz = box_lengths
    out = np.zeros((n_sims, 6))
    for i in range(n_sims):
        if mode == "imbalanced":   # eps_zz log-uniform in [1e-3, 2e-2] -> nts from 10 to 100, ragged batch
            ezz = float(np.exp(rng.uniform(np.log(1.0e-3), np.log(2.0e-2))))
        else:
            ezz = rng.uniform(1.0e-3, 1.8e-3) * scale
        sh = rng.uniform(-1.0e-4, 1.0e-4, 3) * scale
        out[i] = [-0.3 * ezz * lx, -0.3 * ezz * ly, ezz * lz, sh[0] * lz, sh[1] * ly, sh[2] * lx]
    return out


def write_lammps_data(path: str, d: dict, title: str = "scema_amd synthetic replica") -> None:
    """Write the system as a LAMMPS data file of atom_style full (what `write_data` produces), so the same
    replica can be run through the reference's own scripts where LAMMPS is available, and read back by
    scema_md_load_lammps_data.  Pair coefficients are written per pair (PairIJ Coeffs)."""
    n = int(d["natoms"]); nt = int(d["ntypes"])
    box = [float(b) for b in np.asarray(d["box"], float)]   # plain floats: repr() must not say np.float64(..)
    with open(path, "w") as f:
        f.write(f"LAMMPS data file: {title}\n\n")
        f.write(f"{n} atoms\n{nt} atom types\n")
        f.write(f"{len(d['bond_type'])} bonds\n{len(d['bond_coeff'])} bond types\n")
        f.write(f"{len(d['angle_type'])} angles\n{len(d['angle_coeff'])} angle types\n")
        f.write(f"{len(d['dihedral_type'])} dihedrals\n{len(d['dihedral_coeff'])} dihedral types\n")
        f.write(f"{len(d['improper_type'])} impropers\n{len(d['improper_coeff'])} improper types\n\n")
        f.write(f"{box[0]!r} {box[3]!r} xlo xhi\n{box[1]!r} {box[4]!r} ylo yhi\n{box[2]!r} {box[5]!r} zlo zhi\n")
        f.write(f"{box[6]!r} {box[7]!r} {box[8]!r} xy xz yz\n\n")
        f.write("Masses\n\n")
        for t in range(nt):
            f.write(f"{t + 1} {float(d['mass'][t])!r}\n")
        f.write("\nPairIJ Coeffs # lj/cut/coul/long\n\n")
        for a in range(nt):
            for b in range(a, nt):
                f.write(f"{a + 1} {b + 1} {float(d['eps'][a][b])!r} {float(d['sigma'][a][b])!r}\n")
        if len(d["bond_coeff"]):
            f.write("\nBond Coeffs # harmonic\n\n")
            for t, (k, r0) in enumerate(d["bond_coeff"]):
                f.write(f"{t + 1} {float(k)!r} {float(r0)!r}\n")
        if len(d["angle_coeff"]):
            f.write("\nAngle Coeffs # harmonic\n\n")
            for t, (k, th) in enumerate(d["angle_coeff"]):
                f.write(f"{t + 1} {float(k)!r} {float(np.rad2deg(th))!r}\n")
        if len(d["dihedral_coeff"]):
            f.write("\nDihedral Coeffs # opls\n\n")
            for t, ks in enumerate(d["dihedral_coeff"]):
                f.write(f"{t + 1} " + " ".join(repr(float(k)) for k in ks) + "\n")
        if len(d["improper_coeff"]):
            f.write("\nImproper Coeffs # harmonic\n\n")
            for t, (k, chi) in enumerate(d["improper_coeff"]):
                f.write(f"{t + 1} {float(k)!r} {float(np.rad2deg(chi))!r}\n")
        f.write("\nAtoms # full\n\n")
        mol = d.get("mol", np.zeros(n, dtype=np.int32))
        for i in range(n):
            x = d["x"][i]
            f.write(f"{i + 1} {int(mol[i]) + 1} {int(d['type'][i]) + 1} {float(d['charge'][i])!r} {float(x[0])!r} {float(x[1])!r} {float(x[2])!r} 0 0 0\n")
        f.write("\nVelocities\n\n")
        for i in range(n):
            v = d["v"][i]
            f.write(f"{i + 1} {float(v[0])!r} {float(v[1])!r} {float(v[2])!r}\n")
        for name, key, tkey in (("Bonds", "bonds", "bond_type"), ("Angles", "angles", "angle_type"),
                                ("Dihedrals", "dihedrals", "dihedral_type"), ("Impropers", "impropers", "improper_type")):
            if len(d[tkey]):
                f.write(f"\n{name}\n\n")
                for m, (row, t) in enumerate(zip(d[key], d[tkey])):
                    f.write(f"{m + 1} {int(t) + 1} " + " ".join(str(int(a) + 1) for a in row) + "\n")


def read_replica_file(path: str) -> dict:
    """Read the engine's replica container (scema_md_write_replica_file) back into the dict form."""
    import struct
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:8] != b"SCEMAMD1":
        raise ValueError(f"{path}: not a replica container")
    h = struct.unpack_from("<10i", raw, 8)
    n, nt, nb, nbt, na, nat, nd, ndt, ni, nit = h
    off = 8 + 40

    def take(dtype, count, shape=None):
        nonlocal off
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=off).copy()
        off += a.nbytes
        return a if shape is None else a.reshape(shape)

    slj = take("<f8", 3); sc = take("<f8", 3); box = take("<f8", 9)
    d = dict(natoms=n, ntypes=nt, special_lj=slj, special_coul=sc, box=box)
    d["type"] = take("<i4", n); d["charge"] = take("<f8", n); d["mass"] = take("<f8", nt)
    d["eps"] = take("<f8", nt * nt, (nt, nt)); d["sigma"] = take("<f8", nt * nt, (nt, nt))
    d["bonds"] = take("<i4", 2 * nb, (nb, 2)); d["bond_type"] = take("<i4", nb); d["bond_coeff"] = take("<f8", 2 * nbt, (nbt, 2))
    d["angles"] = take("<i4", 3 * na, (na, 3)); d["angle_type"] = take("<i4", na); d["angle_coeff"] = take("<f8", 2 * nat, (nat, 2))
    d["dihedrals"] = take("<i4", 4 * nd, (nd, 4)); d["dihedral_type"] = take("<i4", nd); d["dihedral_coeff"] = take("<f8", 4 * ndt, (ndt, 4))
    d["impropers"] = take("<i4", 4 * ni, (ni, 4)); d["improper_type"] = take("<i4", ni); d["improper_coeff"] = take("<f8", 2 * nit, (nit, 2))
    d["x"] = take("<f8", 3 * n, (n, 3)); d["v"] = take("<f8", 3 * n, (n, 3))
    return d
