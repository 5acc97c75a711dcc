"""Vashishta in plain numpy, FP64: the reference the Vashishta tests compare with (tests/test_vashishta_*.py, tests/test_gpu_vashishta.py).

An independent restatement -- it shares no code with scema_amd/csrc/vashishta/vs_core.h or the library's reader:

  U(r)  = H r^-eta + K Zi Zj exp(-r/lambda1)/r - D exp(-r/lambda4)/r^4 - W/r^6
  E2(r) = U(r) - U(rc) - (r - rc) U'(rc)                                                   r < rc, counted once per pair
  E3    = B dc^2/(1 + C dc^2) exp(g_ij/(r_ij - r0_ij) + g_ik/(r_ik - r0_ik)), dc = cos th - cos th0      r_ij < r0_ij, r_ik < r0_ik

with the pair quantities of (i, j) (H eta Zi Zj lambda1 D lambda4 W rc, and gamma r0 of an arm) from the file's entry `i j j` and B, C,
cos th0 of a triplet centred on i from entry `i j k` (LAMMPS pair_vashishta.cpp).  A lambda of 0 means exp(...) = 1.  Neighbours are
found by brute force: the fractional minimum image plus as many images around it as rc reaches (floor(rc / width + 1/2) per direction),
so the 8-atom cell, two images deep, is right.  `energy` sums the energy alone (half a pair's energy at each of its two ends) and is what the
central differences of tests/test_vashishta_host.py take; `compute` gathers every ordered pair and every triplet and sums energies,
analytic forces and the virial W = sum d (x) f.  Units are LAMMPS `real`: kcal/mol, Angstrom, fs, g/mol.
"""
import itertools

import numpy as np

from sw_numpy import BOLTZ, FTM2V, KCALMOL_A3_TO_GPA, MVV2E, NKTV2P, h_matrix, minimage_diff, strained, volume, widths  # noqa: F401

EV_TO_KCALMOL = 23.060549
K_EV, K_KCALMOL = 14.399645, 332.06371
FIELDS = ["H", "eta", "Zi", "Zj", "lambda1", "D", "lambda4", "W", "rc", "B", "gamma", "r0", "C", "costheta0"]
SI_MASS, C_MASS = 28.0855, 12.011
A_SIC = 4.3581
RC_SIC, R0_SIC = 7.35, 2.90


def read_vashishta(path, elements, energy_unit=0):
    """{(i, j, k): {field: value}} over the distinct names of `elements` (order of first appearance), the type map and K"""
    names = []
    for e in elements:
        if e not in names:
            names.append(e)
    words = []
    for line in open(path):
        words += line.split("#")[0].split()
    out = {}
    for t in range(0, len(words) - 16, 17):
        el, num = words[t:t + 3], [float(w) for w in words[t + 3:t + 17]]
        if all(e in names for e in el):
            d = dict(zip(FIELDS, num))
            if energy_unit == 0:
                for k in ("H", "D", "W", "B"):
                    d[k] *= EV_TO_KCALMOL
            out[tuple(names.index(e) for e in el)] = d
    return out, [names.index(e) for e in elements], (K_EV * EV_TO_KCALMOL if energy_unit == 0 else K_KCALMOL)


def _u(p, K, r):
    """U(r) and U'(r) of one pair entry; r: array"""
    e1 = np.exp(-r / p["lambda1"]) if p["lambda1"] > 0.0 else np.ones_like(r)
    e4 = np.exp(-r / p["lambda4"]) if p["lambda4"] > 0.0 else np.ones_like(r)
    i1 = 1.0 / p["lambda1"] if p["lambda1"] > 0.0 else 0.0
    i4 = 1.0 / p["lambda4"] if p["lambda4"] > 0.0 else 0.0
    q = K * p["Zi"] * p["Zj"]
    rep = p["H"] * r ** (-p["eta"]) if p["H"] != 0.0 else np.zeros_like(r)
    u = rep + q * e1 / r - p["D"] * e4 / r ** 4 - p["W"] / r ** 6
    du = -p["eta"] * rep / r - q * e1 * (i1 + 1.0 / r) / r + p["D"] * e4 * (i4 + 4.0 / r) / r ** 4 + 6.0 * p["W"] / r ** 7
    return u, du


class Vashishta:
    def __init__(self, params, K):
        self.p, self.K = params, K
        self.ne = 1 + max(k[0] for k in params)
        self.rc = np.array([[self.pair(a, b)["rc"] for b in range(self.ne)] for a in range(self.ne)])
        self.r0 = np.array([[self.pair(a, b)["r0"] for b in range(self.ne)] for a in range(self.ne)])
        self.cutmax = max(self.rc.max(), self.r0.max())

    def pair(self, ti, tj):
        return self.p[(ti, tj, tj)]

    def e2(self, ti, tj, r):
        """E2 and dE2/dr of the pair of elements at distances r < rc (array)"""
        p = self.pair(ti, tj)
        rc = np.array([p["rc"]])
        u, du = _u(p, self.K, np.asarray(r, float))
        uc, duc = _u(p, self.K, rc)
        return u - uc[0] - (r - rc[0]) * duc[0], du - duc[0]

    def ordered_pairs(self, x, box, types):
        """every ordered pair (i, j, image) with 0 < r < rc of its elements: arrays i, j, image number, d = x_j - x_i [.., 3], r;
        sorted by (i, j, image)"""
        x = np.asarray(x, float)
        types = np.asarray(types)
        H = h_matrix(box)
        n = len(x)
        s = (x[None, :, :] - x[:, None, :]) @ np.linalg.inv(H)
        d0 = (s - np.rint(s)) @ H
        depth = [int(np.floor(self.cutmax / w + 0.5)) for w in widths(box)]
        rcij = self.rc[types[:, None], types[None, :]]
        I, J, M, D = [], [], [], []
        for m, sh in enumerate(itertools.product(*[range(-k, k + 1) for k in depth])):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ok = (r2 < rcij ** 2) & (r2 > 0.0)
            ii, jj = np.nonzero(ok)
            keep = np.sqrt(r2[ii, jj]) < rcij[ii, jj]
            ii, jj = ii[keep], jj[keep]
            I.append(ii); J.append(jj); M.append(np.full(len(ii), m)); D.append(d[ii, jj])
        I, J, M, D = np.concatenate(I), np.concatenate(J), np.concatenate(M), np.concatenate(D)
        order = np.lexsort((M, J, I))
        I, J, M, D = I[order], J[order], M[order], D[order]
        return I, J, M, D, np.linalg.norm(D, axis=1), n

    def energy(self, x, box, types):
        """energy alone: half of every ordered pair, every triplet"""
        types = np.asarray(types)
        I, J, M, D, R, n = self.ordered_pairs(x, box, types)
        e = 0.0
        for a in range(self.ne):
            for b in range(self.ne):
                sel = (types[I] == a) & (types[J] == b)
                if sel.any():
                    e += 0.5 * float(np.sum(self.e2(a, b, R[sel])[0]))      # each pair stands in the list at both ends
        arm = R < self.r0[types[I], types[J]]
        Ia, Ja, Da, Ra = I[arm], J[arm], D[arm], R[arm]
        start = np.searchsorted(Ia, np.arange(n + 1))
        for i in range(n):
            lo, hi = start[i], start[i + 1]
            for a in range(lo, hi):
                for b in range(a + 1, hi):
                    q = self.p[(types[i], types[Ja[a]], types[Ja[b]])]
                    pa, pb = self.pair(types[i], types[Ja[a]]), self.pair(types[i], types[Ja[b]])
                    dc = np.dot(Da[a], Da[b]) / (Ra[a] * Ra[b]) - q["costheta0"]
                    e += q["B"] * dc * dc / (1.0 + q["C"] * dc * dc) * np.exp(pa["gamma"] / (Ra[a] - pa["r0"]) + pb["gamma"] / (Ra[b] - pb["r0"]))
        return e

    def compute(self, x, box, types):
        """dict e2, e3, e, f [n,3], w (xx yy zz xy xz yz), w33, npairs (ordered pairs inside rc), ntriplets (pairs (a, b) of the lists
        inside r0, whatever their B), maxin (most neighbours inside r0), maxrc (most inside rc)"""
        types = np.asarray(types)
        I, J, M, D, R, n = self.ordered_pairs(x, box, types)
        f = np.zeros((n, 3))
        w = np.zeros((3, 3))
        e2 = 0.0
        # ---- pair term: each end of a pair sums its own force; half of the energy and half of the virial at each end
        for a in range(self.ne):
            for b in range(self.ne):
                sel = (types[I] == a) & (types[J] == b)
                if not sel.any():
                    continue
                e, de = self.e2(a, b, R[sel])
                e2 += 0.5 * float(np.sum(e))
                g = (de / R[sel])[:, None] * D[sel]          # force on i: -dE/dx_i = +E' d / r
                np.add.at(f, I[sel], g)
                w += -0.5 * (D[sel].T @ g)                   # d (x) (force on j), force on j = -g
        # ---- triplets (a < b in the sorted list inside r0) around every atom
        arm = R < self.r0[types[I], types[J]]
        Ia, Ja, Da, Ra = I[arm], J[arm], D[arm], R[arm]
        start = np.searchsorted(Ia, np.arange(n + 1))
        ti_, tj_, tk_, d1, d2, p1, p2, p3 = [], [], [], [], [], [], [], []
        for i in range(n):
            lo, hi = start[i], start[i + 1]
            for a in range(lo, hi):
                for b in range(a + 1, hi):
                    ti_.append(i); tj_.append(Ja[a]); tk_.append(Ja[b]); d1.append(Da[a]); d2.append(Da[b])
                    p1.append(self.pair(types[i], types[Ja[a]])); p2.append(self.pair(types[i], types[Ja[b]]))
                    p3.append(self.p[(types[i], types[Ja[a]], types[Ja[b]])])
        e3 = 0.0
        if ti_:
            d1, d2 = np.array(d1), np.array(d2)
            r1, r2 = np.linalg.norm(d1, axis=1), np.linalg.norm(d2, axis=1)
            g1 = lambda k: np.array([q[k] for q in p1])
            g2 = lambda k: np.array([q[k] for q in p2])
            g3 = lambda k: np.array([q[k] for q in p3])
            c1, c2 = r1 - g1("r0"), r2 - g2("r0")
            E = np.exp(g1("gamma") / c1 + g2("gamma") / c2)
            cos = np.einsum("ij,ij->i", d1, d2) / (r1 * r2)
            dc = cos - g3("costheta0")
            B, Cc = g3("B"), g3("C")
            den = 1.0 + Cc * dc ** 2
            h = B * dc ** 2 / den * E
            e3 = float(np.sum(h))
            dh_dr1 = h * (-g1("gamma") / c1 ** 2)
            dh_dr2 = h * (-g2("gamma") / c2 ** 2)
            dh_dc = B * E * 2.0 * dc / den ** 2
            u1, u2 = d1 / r1[:, None], d2 / r2[:, None]
            gj = dh_dr1[:, None] * u1 + (dh_dc / r1)[:, None] * (u2 - cos[:, None] * u1)
            gk = dh_dr2[:, None] * u2 + (dh_dc / r2)[:, None] * (u1 - cos[:, None] * u2)
            np.add.at(f, np.array(tj_), -gj)
            np.add.at(f, np.array(tk_), -gk)
            np.add.at(f, np.array(ti_), gj + gk)
            w += -(d1.T @ gj) - (d2.T @ gk)
        w6 = np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[0, 2], w[1, 2]])
        nin = np.diff(start)
        return dict(e2=e2, e3=e3, e=e2 + e3, f=f, w=w6, w33=w, npairs=len(I), ntriplets=len(ti_), maxin=int(nin.max()) if n else 0,
                    maxrc=int(np.bincount(I, minlength=n).max()) if len(I) else 0)

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

    def margin(self, x, box, types):
        """smallest distance of any pair distance from rc and from r0 of its elements (the inputs of finite differences keep away from both)"""
        types = np.asarray(types)
        big = Vashishta({k: dict(v, rc=v["rc"] + 0.5 if k[1] == k[2] else v["rc"]) for k, v in self.p.items()}, self.K)
        I, J, _, _, R, _ = big.ordered_pairs(x, box, types)
        m = np.abs(R - self.rc[types[I], types[J]]).min()
        r0 = self.r0[types[I], types[J]]
        if (r0 > 0.0).any():
            m = min(m, np.abs(R - r0)[r0 > 0.0].min())
        return float(m)


# ---- inputs the CPU and GPU tests share: element 0 is Si, element 1 is C (elements ("Si", "C")) ----
BIG_BOX = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])


def zincblende(nx, ny, nz, a=A_SIC):
    """positions, orthogonal box and types of zincblende SiC: Si on the fcc sites, C a quarter of the body diagonal further"""
    fcc = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0]], float) * 0.25
    basis = np.vstack([fcc, fcc + 0.25])
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    t = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), len(cells))
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0]), t


def case_cell8(a=A_SIC):
    """the 8-atom cell: the box is narrower than rc + skin, the rows are built two images deep"""
    return zincblende(1, 1, 1, a)


def case_cell8_jittered(seed=4, jitter=0.02):
    """the 8-atom cell with a jitter that moves no pair across rc or r0: the counts of the perfect cell, but forces and a virial that do
    not cancel (the perfect cell sits at the potential's own minimum: forces of 1e-14, a virial 1e-4 of its terms)"""
    x, box, t = case_cell8()
    return x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape), box, t


def case_jitter(ncell, seed, jitter=0.05):
    """ncell^3 cells, uniform jitter"""
    x, box, t = zincblende(ncell, ncell, ncell)
    return x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape), box, t


def case_count(n, seed=5, jitter=0.05):
    """n atoms of a jittered lattice: 63 = 2 x 2 x 2 cells with a vacancy, 65 = 3 x 3 x 1 cells with seven, 1 000 = 5 x 5 x 5 cells,
    1 440 = 6 x 6 x 5 cells"""
    cells = {63: (2, 2, 2), 65: (3, 3, 1), 1000: (5, 5, 5), 1440: (6, 6, 5)}[n]
    x, box, t = zincblende(*cells)
    x = x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape)
    keep = np.ones(len(x), bool)
    keep[np.linspace(3, len(x) - 2, len(x) - n).astype(int)] = False
    assert keep.sum() == n
    return x[keep], box, t[keep]


def case_dimer(ti, tj, r):
    """two atoms r apart along x in the 30 A box; the first sits at x = 0 so that the distance is r to the bit"""
    x = np.array([[0.0, 10.0, 10.0], [r, 10.0, 10.0]])
    return x, BIG_BOX.copy(), np.array([ti, tj])


def case_trimer(r1=R0_SIC - 1e-6, r2=1.9, angle=100.0):
    """C - Si - C with the silicon atom in the middle: one arm r1 long along x (by default next to r0), the other r2 long at that angle"""
    a = np.radians(angle)
    x = np.array([[0.0, 10.0, 10.0], [r1, 10.0, 10.0], [r2 * np.cos(a), 10.0 + r2 * np.sin(a), 10.0]])
    return x, BIG_BOX.copy(), np.array([0, 1, 1])


def case_cluster(m, radius=2.5):
    """a silicon atom at the centre of m carbon atoms on a Fibonacci sphere of that radius, in the 30 A box: C-C has r0 = 0, so the centre's
    list inside r0 alone is long (m entries); all atoms lie inside rc of each other"""
    k = np.arange(m) + 0.5
    z = 1.0 - 2.0 * k / m
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    shell = radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    x = np.vstack([np.zeros((1, 3)), shell]) + 15.0
    return x, BIG_BOX.copy(), np.array([0] + [1] * m)


def case_triclinic(seed=12):
    """3 x 3 x 3 cells (216 atoms), all three tilts, jitter, atoms shifted so that several sit outside the box"""
    x, box, t = zincblende(3, 3, 3)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])
    x = (x + np.random.default_rng(seed).uniform(-0.05, 0.05, x.shape)) @ F.T
    L = 3 * A_SIC
    box[6], box[7], box[8] = 0.06 * L, -0.05 * L, 0.04 * L
    x = x + np.array([0.9, -1.3, 0.4])
    H = h_matrix(box)
    x[::17] += H[0]
    x[5::23] -= H[2] + H[1]
    return x, box, t


# a two-element file written at test time: every B != 0, another r0 and gamma per pair, a non-integer eta, one lambda1 = 0, C = 0 in one
# entry.  rc and r0 of X Y Y and Y X X agree, as the reader demands; the mixed entries are symmetric in the two arms (i j k = i k j), as
# those of every physical file are: which arm of a triplet is "j" follows the order of the neighbour list (in LAMMPS as here), and the
# rows of the device are not in the order of this file's lists wherever an atom has several images in range; units metal
SYNTH = """# synthetic two-element Vashishta file for the tests (no material)
X X X  30.0   7.5 0.9  0.9  4.5 10.0 2.8  5.0 6.0   6.0 0.9 2.7 4.0 -0.30
Y Y Y  200.0  7.0 -0.8 -0.8 0.0  2.0 3.0  0.0 5.5   4.0 0.7 2.4 0.0 -0.40
X Y Y  300.0  9.0 0.9  -0.8 5.0  6.0 3.2 40.0 6.5   8.0 1.1 2.9 5.0 -0.3333
Y X X  300.0  9.0 -0.8 0.9  5.0  6.0 3.2 40.0 6.5   7.0 1.0 2.9 3.0 -0.25
X X Y  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0   5.0 0.0 0.0 2.0 -0.35
X Y X  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0   5.0 0.0 0.0 2.0 -0.35
Y Y X  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0   3.0 0.0 0.0 1.0 -0.45
Y X Y  0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0 0.0   3.0 0.0 0.0 1.0 -0.45
"""


def case_synth(seed=34):
    """2 x 2 x 2 zincblende cells at 4.4 A, jitter 0.1 A, for the synthetic file (elements X, Y): with r0 from 2.4 to 2.9 A the like
    neighbours at 3.1 A stay outside, the unlike ones at 1.9 A inside; triplets of every kind need like arms too, so a quarter of the
    atoms changes its element"""
    x, box, t = zincblende(2, 2, 2, 4.4)
    rng = np.random.default_rng(seed)
    t = t.copy()
    t[rng.choice(len(t), len(t) // 4, replace=False)] ^= 1
    return x + rng.uniform(-0.1, 0.1, x.shape), box, t
