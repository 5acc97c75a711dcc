"""Embedded-atom method (pair_style eam/alloy on DYNAMO setfl tables) in plain numpy, FP64: the reference the EAM tests compare with
(tests/test_eam_*.py, tests/test_gpu_eam.py).

An independent restatement -- it shares no code with scema_amd/csrc/eam/eam_core.h or the library's reader:

  E     = sum_i F_{el(i)}(rho_i) + 1/2 sum_i sum_{j != i} phi_{el(i) el(j)}(r_ij)         over 0 < r^2 < cutoff^2
  rho_i = sum_{j != i} rho_{el(j)}(r_ij)

A function is tabulated as f[0..n-1] at x_k = k delta; knot k holds seven coefficients s0..s6 (spline() below says how), the lookup is
p = x / delta, k = min(int(p), n - 2) (for F also k >= 0), p = min(p - k, 1), value ((s3 p + s4) p + s5) p + s6, derivative
(s0 p + s1) p + s2.  Above rhomax = (Nrho - 1) drho the embedding energy continues with the slope of the clamped lookup.  The file stores
r phi: phi = z / r, phi' = z' / r - phi / r.  No LAMMPS exists to compare with: this file, the cubic-polynomial tables (which a spline of
this kind reproduces exactly away from its ends) and central differences of its own energy are what pins the arithmetic.

Neighbours are found by brute force over as many periodic images as the cutoff reaches.  The energy is a plain loop, computed first;
forces and virial W = sum d (x) f are analytic.  Units are LAMMPS `real`: kcal/mol, Angstrom, fs, g/mol.
"""
import itertools
import math

import numpy as np

from sw_numpy import (BOLTZ, FTM2V, KCALMOL_A3_TO_GPA, MVV2E, NKTV2P, gas, h_matrix, minimage_diff, strained, volume, widths)  # noqa: F401

EV_TO_KCALMOL = 23.060549


# ---- setfl files ----
def read_setfl(path, elements, energy_unit=0):
    """dict of the tables of the distinct names of `elements` (order of first appearance): nrho, drho, nr, dr, cutoff, masses, F[i],
    rho[i] (by source element), z[i][j] (r phi), F and z in kcal/mol; and the type map"""
    names = []
    for e in elements:
        if e not in names:
            names.append(e)
    lines = open(path).read().split("\n")[3:]
    w = " ".join(lines).split()
    nfile = int(w[0])
    fnames = w[1:1 + nfile]
    t = 1 + nfile
    nrho, drho, nr, dr, cutoff = int(w[t]), float(w[t + 1]), int(w[t + 2]), float(w[t + 3]), float(w[t + 4])
    t += 5
    scale = EV_TO_KCALMOL if energy_unit == 0 else 1.0
    F, rho, mass = {}, {}, {}
    for k in range(nfile):
        mass[fnames[k]] = float(w[t + 1])
        t += 4
        F[fnames[k]] = np.array([float(v) for v in w[t:t + nrho]]) * scale
        t += nrho
        rho[fnames[k]] = np.array([float(v) for v in w[t:t + nr]])
        t += nr
    z = {}
    for i in range(nfile):
        for j in range(i + 1):
            z[(fnames[i], fnames[j])] = z[(fnames[j], fnames[i])] = np.array([float(v) for v in w[t:t + nr]]) * scale
            t += nr
    ne = len(names)
    return dict(nrho=nrho, drho=drho, nr=nr, dr=dr, cutoff=cutoff, masses=[mass[a] for a in names], F=[F[a] for a in names],
                rho=[rho[a] for a in names], z=[[z[(a, b)] for b in names] for a in names], n=ne), [names.index(e) for e in elements]


def write_setfl(path, names, Z, masses, lattice, nrho, drho, nr, dr, cutoff, F, rho, z, header):
    """F[i], rho[i]: arrays per element in the order of `names`; z[(i, j)], i >= j: r phi.  Numbers at 17 significant digits, 5 per line"""
    out = list(header) + ["%d %s" % (len(names), " ".join(names)), "%d %.17g %d %.17g %.17g" % (nrho, drho, nr, dr, cutoff)]

    def block(a):
        a = list(a)
        return [" ".join("%.16e" % v for v in a[k:k + 5]) for k in range(0, len(a), 5)]
    for i in range(len(names)):
        out.append("%d %.17g %.17g %s" % (Z[i], masses[i], lattice[i], "fcc"))
        out += block(F[i]) + block(rho[i])
    for i in range(len(names)):
        for j in range(i + 1):
            out += block(z[(i, j)])
    assert len(header) == 3
    with open(path, "w") as fh:
        fh.write("\n".join(out) + "\n")


# ---- the splines ----
def spline(f, delta):
    """[n][7] coefficients s0..s6 of the knots of f"""
    f = np.asarray(f, float)
    n = len(f)
    s = np.zeros((n, 7))
    s[:, 6] = f
    s[0, 5] = f[1] - f[0]
    s[1, 5] = (f[2] - f[0]) / 2.0
    s[n - 2, 5] = (f[n - 1] - f[n - 3]) / 2.0
    s[n - 1, 5] = f[n - 1] - f[n - 2]
    for k in range(2, n - 2):
        s[k, 5] = ((f[k - 2] - f[k + 2]) + 8.0 * (f[k + 1] - f[k - 1])) / 12.0
    for k in range(n - 1):
        s[k, 4] = 3.0 * (f[k + 1] - f[k]) - 2.0 * s[k, 5] - s[k + 1, 5]
        s[k, 3] = s[k, 5] + s[k + 1, 5] - 2.0 * (f[k + 1] - f[k])
    s[:, 2] = s[:, 5] / delta
    s[:, 1] = 2.0 * s[:, 4] / delta
    s[:, 0] = 3.0 * s[:, 3] / delta
    return s


def lookup(s, delta, x, floor0=False):
    """value and derivative at x"""
    n = len(s)
    p = x / delta
    k = min(int(p), n - 2)
    if floor0:
        k = max(k, 0)
    p = min(p - k, 1.0)
    c = s[k]
    return ((c[3] * p + c[4]) * p + c[5]) * p + c[6], (c[0] * p + c[1]) * p + c[2]


class EAM:
    def __init__(self, tab):
        self.t = tab
        self.cutoff = tab["cutoff"]
        self.rhomax = (tab["nrho"] - 1) * tab["drho"]
        self.sF = [spline(f, tab["drho"]) for f in tab["F"]]
        self.srho = [spline(f, tab["dr"]) for f in tab["rho"]]
        self.sz = [[spline(f, tab["dr"]) for f in row] for row in tab["z"]]

    def neighbours(self, x, box):
        """per atom the list of (j, d, r) with 0 < r^2 < cutoff^2, d = x_j - x_i with the image's shift, sorted by (j, image)"""
        H = h_matrix(box)
        Hi = np.linalg.inv(H)
        n = len(x)
        d0 = x[None, :, :] - x[:, None, :]
        s = d0 @ Hi
        d0 = (s - np.rint(s)) @ H
        m = [int(math.floor(self.cutoff / w + 0.5)) + 1 for w in widths(box)]        # |s| <= 0.5 after the fold: images up to cutoff / w + 0.5 away
        found = [[] for _ in range(n)]
        c2 = self.cutoff * self.cutoff
        for sh in itertools.product(range(-m[0], m[0] + 1), range(-m[1], m[1] + 1), range(-m[2], m[2] + 1)):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ok = (r2 < c2) & (r2 > 0.0)
            for i, j in zip(*np.nonzero(ok)):
                found[i].append((int(j), sh, d[i, j].copy(), math.sqrt(r2[i, j])))
        return [[(j, d, r) for j, _, d, r in sorted(row, key=lambda q: (q[0], q[1]))] for row in found]

    def densities(self, nb, types):
        dr = self.t["dr"]
        return [sum(lookup(self.srho[types[j]], dr, r)[0] for j, _, r in row) for row in nb]

    def embed(self, ti, rho):
        e, fp = lookup(self.sF[ti], self.t["drho"], rho, floor0=True)
        if rho > self.rhomax:
            e += fp * (rho - self.rhomax)
        return e, fp

    def energy(self, x, box, types):
        """the energy alone"""
        x = np.asarray(x, float)
        nb = self.neighbours(x, box)
        e = 0.0
        for i, rho in enumerate(self.densities(nb, types)):
            e += self.embed(types[i], rho)[0]
            for j, _, r in nb[i]:
                e += 0.5 * lookup(self.sz[types[i]][types[j]], self.t["dr"], r)[0] / r
        return e

    def compute(self, x, box, types):
        """dict e_pair, e_embed, e, f [n,3], w (xx yy zz xy xz yz), w33, npairs (ordered pairs inside the cutoff), nabove (atoms with rho >
        rhomax), maxin (most neighbours of an atom inside the cutoff), rho"""
        x = np.asarray(x, float)
        n = len(x)
        dr = self.t["dr"]
        nb = self.neighbours(x, box)
        rho = self.densities(nb, types)
        emb = [self.embed(types[i], rho[i]) for i in range(n)]
        e_embed = sum(e for e, _ in emb)
        fp = [d for _, d in emb]
        e_pair = 0.0
        f = np.zeros((n, 3))
        w = np.zeros((3, 3))
        for i in range(n):
            ti = types[i]
            for j, d, r in nb[i]:
                tj = types[j]
                z, dz = lookup(self.sz[ti][tj], dr, r)
                phi = z / r
                dphi = dz / r - phi / r
                drho_j = lookup(self.srho[tj], dr, r)[1]
                drho_i = lookup(self.srho[ti], dr, r)[1]
                fpair = -(dphi + fp[i] * drho_j + fp[j] * drho_i) / r
                f[i] += -d * fpair                    # (x_i - x_j) fpair
                e_pair += 0.5 * phi
                w += 0.5 * fpair * np.outer(d, d)
        w6 = np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[0, 2], w[1, 2]])
        return dict(e_pair=e_pair, e_embed=e_embed, e=e_pair + e_embed, f=f, w=w6, w33=w, npairs=sum(len(r) for r in nb),
                    nabove=sum(1 for v in rho if v > self.rhomax), maxin=max(len(r) for r in nb), rho=np.array(rho))

    # ---- dynamics: velocity Verlet, NVE, units real (positions stay unwrapped)
    def nve(self, x, v, box, types, masses, dt, nsteps):
        x, v = np.array(x, float), np.array(v, float)
        m = np.asarray(masses, float)[np.asarray(types)][:, None]
        f = self.compute(x, box, types)["f"]
        for _ in range(nsteps):
            v += 0.5 * dt * FTM2V * f / m
            x += dt * v
            f = self.compute(x, box, types)["f"]
            v += 0.5 * dt * FTM2V * f / m
        return x, v

    def pressure_atm(self, x, v, box, types, masses):
        """(sum m v v + W) / V in atm, xx yy zz xy xz yz"""
        m = np.asarray(masses, float)[np.asarray(types)]
        kin = MVV2E * np.einsum("i,ij,ik->jk", m, v, v)
        t = (kin + self.compute(x, box, types)["w33"]) / volume(box) * NKTV2P
        return np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])


# ---- the analytic model behind tests/golden/CuAg.eam.alloy (tests/golden/make_eam_fixture.py) and the files written at test time ----
# Johnson's analytic nearest-neighbour EAM for fcc metals (R. A. Johnson, Phys. Rev. B 37, 3924 (1988); alloys: Phys. Rev. B 39, 12554
# (1989)):  rho(r) = fe exp(-beta (r / re - 1)),  phi(r) = phie exp(-gamma (r / re - 1)),
#           F(rho) = -Ec [1 - (alpha / beta) ln x] x^(alpha / beta) - 6 phie x^(gamma / beta),  x = rho / rhoe,
#           phi_ab  = 1/2 [fb / fa phi_aa + fa / fb phi_bb]
# with parameters in the range of his for copper and silver (Ec and phie in eV, re = a / sqrt 2), carried out to the file's cutoff and
# multiplied there by a switching function; rhoe is the density of the perfect lattice under that cutoff.  Physical accuracy is not claimed.
JOHNSON = {"Cu": dict(Z=29, mass=63.546, a=3.615, Ec=3.54, fe=0.30, phie=0.59, alpha=5.09, beta=5.85, gamma=8.00),
           "Ag": dict(Z=47, mass=107.8682, a=4.09, Ec=2.85, fe=0.17, phie=0.48, alpha=5.92, beta=5.96, gamma=8.26),
           # two invented elements for the four-element files of the edge tests (numbers of the same range, no metal meant)
           "X1": dict(Z=28, mass=58.7, a=3.52, Ec=4.45, fe=0.41, phie=0.74, alpha=4.98, beta=6.41, gamma=8.86),
           "X2": dict(Z=79, mass=197.0, a=4.08, Ec=3.93, fe=0.23, phie=0.65, alpha=6.37, beta=6.67, gamma=8.20)}
CUTOFF, SWITCH_ON = 5.5, 4.5
A_CU, A_AG = 3.615, 4.09
CU_MASS, AG_MASS = 63.546, 107.8682


def switch(r):
    """1 below SWITCH_ON, 1 - 3 t^2 + 2 t^3 on to the cutoff (value and slope zero there), 0 beyond"""
    t = np.clip((np.asarray(r, float) - SWITCH_ON) / (CUTOFF - SWITCH_ON), 0.0, 1.0)
    return 1.0 - 3.0 * t * t + 2.0 * t ** 3


def _rho(p, r):
    return p["fe"] * np.exp(-p["beta"] * (r / (p["a"] / math.sqrt(2.0)) - 1.0)) * switch(r)


def _phi(p, r):
    return p["phie"] * np.exp(-p["gamma"] * (r / (p["a"] / math.sqrt(2.0)) - 1.0)) * switch(r)


def _rhoe(p):
    pts = np.array(list(itertools.product(range(-4, 5), repeat=3)), float)
    basis = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
    r = np.linalg.norm((pts[:, None, :] + basis[None, :, :]).reshape(-1, 3) * p["a"], axis=1)
    r = r[(r > 0.0) & (r < CUTOFF)]
    return float(np.sum(_rho(p, r)))


def johnson_tables(names, nrho=500, nr=500, dr=0.0112, rhomax_over_rhoe=3.0):
    """the arguments of write_setfl after `lattice`, for the elements named: one drho for all of them, rhomax = rhomax_over_rhoe times
    the largest equilibrium density"""
    P = [JOHNSON[a] for a in names]
    drho = rhomax_over_rhoe * max(_rhoe(p) for p in P) / (nrho - 1)
    r = np.arange(nr) * dr
    F, rho, z = [], [], {}
    for p in P:
        x = np.arange(nrho) * drho / _rhoe(p)
        xs = np.where(x > 0.0, x, 1.0)
        F.append(np.where(x > 0.0, -p["Ec"] * (1.0 - p["alpha"] / p["beta"] * np.log(xs)) * xs ** (p["alpha"] / p["beta"]) - 6.0 * p["phie"] * xs ** (p["gamma"] / p["beta"]), 0.0))
        rho.append(_rho(p, r))
    for i, a in enumerate(P):
        for j, b in enumerate(P[:i + 1]):
            z[(i, j)] = r * (_phi(a, r) if i == j else 0.5 * (b["fe"] / a["fe"] * _phi(a, r) + a["fe"] / b["fe"] * _phi(b, r)))
    return nrho, drho, nr, dr, CUTOFF, F, rho, z


def write_johnson(path, names, header=None, **kw):
    P = [JOHNSON[a] for a in names]
    header = header or ["analytic EAM of the Johnson form, written by tests/eam_numpy.py at test time", "not from LAMMPS, not from the reference", "units metal"]
    write_setfl(path, names, [p["Z"] for p in P], [p["mass"] for p in P], [p["a"] for p in P], *johnson_tables(names, **kw), header)


# cubic polynomials in all three functions: a spline with five-point slopes reproduces a cubic exactly wherever it uses them
POLY = dict(F=(-1.5, 0.8, -0.11, 0.004), rho=(2.0, -0.6, 0.05, -0.002), z=(3.0, -1.1, 0.3, -0.02))


def poly(c, x):
    return ((c[3] * x + c[2]) * x + c[1]) * x + c[0]


def dpoly(c, x):
    return (3.0 * c[3] * x + 2.0 * c[2]) * x + c[1]


def write_poly(path, nrho=60, drho=0.25, nr=80, dr=0.07, cutoff=5.0):
    write_setfl(path, ["X"], [1], [10.0], [3.0], nrho, drho, nr, dr, cutoff, [poly(POLY["F"], np.arange(nrho) * drho)],
                [poly(POLY["rho"], np.arange(nr) * dr)], {(0, 0): poly(POLY["z"], np.arange(nr) * dr)},
                ["cubic polynomials in F, rho and r phi", "written by tests/eam_numpy.py at test time", "units metal"])


# ---- the static cases the CPU and GPU tests share ----
BIG_BOX = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])


def zeros(n):
    return np.zeros(n, int)


def fcc(nx, ny, nz, a):
    """positions of the fcc lattice, nx x ny x nz cubic cells of 4 atoms, and the orthogonal box"""
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0]], float) * 0.25
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0])


def case_single():
    return np.array([[14.0, 15.0, 16.0]]), BIG_BOX.copy(), zeros(1)


def case_dimer(r=2.5):
    """two atoms r apart along x; the first sits at x = 0, so r is the distance to the bit"""
    return np.array([[0.0, 10.0, 10.0], [r, 10.0, 10.0]]), BIG_BOX.copy(), zeros(2)


def case_cell4(width=A_CU, seed=41):
    """the 4-atom cubic cell of copper (jitter 0.05 A), scaled to that width: 3.615 A is narrower than the list radius 6.5 A, every
    atom meets images of itself and of the others two boxes away; 3.26 A is just above the width the engine refuses, (5.5 + 1) / 2"""
    x, box = fcc(1, 1, 1, A_CU)
    rng = np.random.default_rng(seed)
    x = (x + rng.uniform(-0.05, 0.05, x.shape)) * (width / A_CU)
    return x, box * (width / A_CU), zeros(4)


def case_jitter(nc, seed=11, a=A_CU):
    """nc^3 cells (32 atoms at nc = 2, 108 at 3, 256 at 4), jitter 0.1 A: some 54 neighbours inside the cutoff"""
    x, box = fcc(nc, nc, nc, a)
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, zeros(len(x))


def case_alloy(seed=13):
    """2 x 2 x 2 cells of a = 3.85 A, the two elements placed at random, jitter 0.1 A"""
    x, box, _ = case_jitter(2, seed, 3.85)
    return x, box, np.random.default_rng(seed + 1).integers(0, 2, len(x))


def case_gas(seed=1):
    """60 atoms at random in a 12 A box, no two closer than 2.0 A"""
    box = np.array([0.0, 0.0, 0.0, 12.0, 12.0, 12.0, 0.0, 0.0, 0.0])
    return gas(60, box, 2.0, seed), box, zeros(60)


def case_triclinic(seed=12):
    """3 x 2 x 3 cells (72 atoms), triclinic with all three tilts, atoms shifted so that several sit outside the box"""
    x, box = fcc(3, 2, 3, A_CU)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(seed)
    x = (x + rng.uniform(-0.1, 0.1, x.shape)) @ F.T
    box = box.copy()
    box[6], box[7], box[8] = 0.06 * 2 * A_CU, -0.05 * 3 * A_CU, 0.04 * 3 * A_CU
    x = x + np.array([0.9, -1.3, 0.4])
    H = h_matrix(box)
    x[::17] += H[0]
    x[5::23] -= H[2] + H[1]
    return x, box, zeros(len(x))


def case_count(n, seed=15):
    """the first n atoms of a jittered 7 x 7 x 7 copper block (1 372 atoms), in the block's box (vacuum where the others were)"""
    x, box = fcc(7, 7, 7, A_CU)
    rng = np.random.default_rng(seed)
    x = x + rng.uniform(-0.1, 0.1, x.shape)
    return x[:n].copy(), box, zeros(n)


# ---- inputs for the edges of the kernels (tests/test_row_edges_host.py, tests/test_gpu_eam_edges.py): generators only ----
FOUR = ["Cu", "X1", "Ag", "X2"]          # the element order of the four-element file: a kept subset (Cu, Ag) skips X1 in the middle
RLIST = CUTOFF + 1.0                     # + the default skin of eam_configure


def check_box(box):
    """each perpendicular width is at least RLIST / 2 (below it the engine refuses: it searches at most two images deep)"""
    w = widths(box)
    assert (w >= RLIST / 2.0).all(), w
    return w


def case_four(ntypes=4, seed=19):
    """2 x 2 x 2 cells of a = 3.85 A, jitter 0.1 A, `ntypes` LAMMPS types placed at random (each one present)"""
    x, box, _ = case_jitter(2, seed, 3.85)
    t = np.random.default_rng(seed + 1).integers(0, ntypes, len(x))
    assert len(set(int(v) for v in t)) == ntypes
    return x, box, t


def case_partly_above(amp=0.15):
    """the 32-atom jittered copper cell under the displacement u_x = -amp L / (2 pi) sin(2 pi x / L): compressed by amp along x around
    x = 0, stretched as much around x = L / 2.  Under a file with rhomax at 1.1 times the lattice's density some atoms lie above it, some below"""
    x, box, t = case_jitter(2)
    L = box[3] - box[0]
    x = x.copy()
    x[:, 0] -= amp * L / (2.0 * math.pi) * np.sin(2.0 * math.pi * x[:, 0] / L)
    return x, box, t


def case_cell4_tilted(sign=1):
    """case_cell4 sheared with its box to xy = sign * 0.45 lx: perpendicular widths 3.30 / 3.30 / 3.615 A, above the 3.25 A below which
    the engine refuses and below the list radius 6.5 A -- two images deep in a tilted cell"""
    x, box, t = case_cell4()
    F = np.array([[1.0, sign * 0.45, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    box = box.copy()
    box[6] = sign * 0.45 * (box[4] - box[1])
    check_box(box)
    return x @ F.T, box, t


HOT_BOX = np.array([0.0, 0.0, 0.0, 3.4, 7.0, 7.6, 0.0, 0.0, 0.0])


def case_hot_gas(n=8, dmin=1.65, seed=5):
    """a small copper gas in a box 3.4 A wide, no two atoms (or images) closer than dmin: far off equilibrium (the lattice's nearest
    neighbours are 2.556 A apart), so that the atoms move past half a skin within some tens of steps"""
    check_box(HOT_BOX)
    return gas(n, HOT_BOX, dmin, seed), HOT_BOX.copy(), zeros(n)
