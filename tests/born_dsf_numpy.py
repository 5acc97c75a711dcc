"""born/coul/dsf in plain numpy, FP64: the reference the Born/DSF tests compare with (tests/test_born_dsf_*.py, tests/test_gpu_born_dsf.py).

An independent restatement -- it shares no code with scema_amd/csrc/ionic/bd_core.h or the library's reader: its own parser of the script
lines, math.erfc, neighbours by brute force over images.

  E_born = A exp((sigma - r)/rho) - C/r^6 + D/r^8                               r < cut_lj[ti][tj], not shifted, counted once per pair
  E_coul = K q_i q_j [ erfc(alpha r)/r - erfc(alpha rc)/rc + f_s (r - rc) ]     r < rc = cut_coul
  f_s    = erfc(alpha rc)/rc^2 + (2 alpha/sqrt(pi)) exp(-alpha^2 rc^2)/rc
  E_self = - K q_i^2 [ e_s/2 + alpha/sqrt(pi) ] per atom,  e_s = erfc(alpha rc)/rc + f_s rc

(Fennell and Gezelter, J. Chem. Phys. 124, 234104 (2006); LAMMPS `pair_style born/coul/dsf`, as remembered, unpinned.)  Forces are the
exact gradients; the self term has no force and no virial.  Neighbours: the fractional minimum image plus as many images around it as
the largest cutoff reaches (floor(cutmax / width + 1/2) per direction), so the 8-ion cell, two images deep, is right.  `energy` sums the
energy alone and is what the central differences take; `compute` gathers every ordered pair and sums energies, analytic forces and the
virial W = sum d (x) f.  Units are LAMMPS `real`: kcal/mol, Angstrom, fs, g/mol, charges in e.
"""
import itertools
import math

import numpy as np

from sw_numpy import BOLTZ, FTM2V, MVV2E, NKTV2P, h_matrix, minimage_diff, strained, volume, widths  # noqa: F401

EV_TO_KCALMOL = 23.060549
K_EV, K_KCALMOL = 14.399645, 332.06371
NA_MASS, CL_MASS, K_MASS = 22.98977, 35.453, 39.0983
A_NACL = 5.64
MADELUNG_NACL = 1.747565
MAXEL = 4
_erfc = np.vectorize(math.erfc, otypes=[float])


def read_born_dsf(path, energy_unit=None):
    """dict n, alpha, cut_coul, K, unit, and [n][n] arrays A (kcal/mol), rho, sigma, C, D, cut_lj of the script lines in `path`;
    energy_unit None: 1 iff the text says `units real`, else 0"""
    style, coeffs, unit = None, [], None
    for raw in open(path):
        w = raw.split("#")[0].split()
        if not w:
            continue
        if w[0] == "pair_style":
            assert style is None and w[1] == "born/coul/dsf", raw
            style = [float(v) for v in w[2:]]
        elif w[0] == "pair_coeff":
            coeffs.append((w[1], w[2], [float(v) for v in w[3:]]))
        elif w[0] == "units":
            unit = {"metal": 0, "real": 1}[w[1]]
    assert style is not None and len(style) in (2, 3)
    alpha, cut_lj = style[0], style[1]
    cut_coul = style[2] if len(style) == 3 else cut_lj
    if energy_unit is None:
        energy_unit = unit or 0
    named = [int(t) for a, b, _ in coeffs for t in (a, b) if t != "*"]
    n = max(named) if named else MAXEL
    conv = EV_TO_KCALMOL if energy_unit == 0 else 1.0
    p = {k: np.full((n, n), np.nan) for k in ("A", "rho", "sigma", "C", "D", "cut_lj")}
    for a, b, v in coeffs:
        for i in (range(1, n + 1) if a == "*" else [int(a)]):
            for j in (range(1, n + 1) if b == "*" else [int(b)]):
                if i > j:
                    continue
                for (u, w_) in ((i - 1, j - 1), (j - 1, i - 1)):
                    p["A"][u, w_], p["rho"][u, w_], p["sigma"][u, w_] = v[0] * conv, v[1], v[2]
                    p["C"][u, w_], p["D"][u, w_] = v[3] * conv, v[4] * conv
                    p["cut_lj"][u, w_] = v[5] if len(v) > 5 else cut_lj
    assert not np.isnan(p["A"]).any(), "a pair is never set"
    return dict(p, n=n, alpha=alpha, cut_coul=cut_coul, unit=energy_unit, K=K_EV * EV_TO_KCALMOL if energy_unit == 0 else K_KCALMOL)


class BornDsf:
    def __init__(self, p):
        self.p = p
        self.alpha, self.rc, self.K = p["alpha"], p["cut_coul"], p["K"]
        self.cutmax = max(self.rc, float(p["cut_lj"].max()))
        a, rc = self.alpha, self.rc
        self.f_s = math.erfc(a * rc) / rc ** 2 + 2.0 * a / math.sqrt(math.pi) * math.exp(-a * a * rc * rc) / rc
        self.e_s = math.erfc(a * rc) / rc + self.f_s * rc

    # ---- the two pair functions: energy and dE/dr at distances r (arrays), beyond the cutoff exactly 0
    def born(self, ti, tj, r):
        p = self.p
        A, rho, sg, C, D = (p[k][ti, tj] for k in ("A", "rho", "sigma", "C", "D"))
        r = np.asarray(r, float)
        rep = A * np.exp((sg - r) / rho)
        e = rep - C / r ** 6 + D / r ** 8
        de = -rep / rho + 6.0 * C / r ** 7 - 8.0 * D / r ** 9
        inside = r < p["cut_lj"][ti, tj]
        return np.where(inside, e, 0.0), np.where(inside, de, 0.0)

    def coul(self, qq, r):
        r = np.asarray(r, float)
        a = self.alpha
        ec = _erfc(a * r) if r.size else r
        e = self.K * qq * (ec / r - math.erfc(a * self.rc) / self.rc + self.f_s * (r - self.rc))
        de = -self.K * qq * (ec / r ** 2 + 2.0 * a / math.sqrt(math.pi) * np.exp(-a * a * r * r) / r - self.f_s)
        inside = r < self.rc
        return np.where(inside, e, 0.0), np.where(inside, de, 0.0)

    def self_energy(self, q):
        return float(-self.K * np.sum(np.asarray(q, float) ** 2) * (0.5 * self.e_s + self.alpha / math.sqrt(math.pi)))

    def ordered_pairs(self, x, box):
        """every ordered pair (i, j, image) with 0 < r < cutmax: arrays i, j, d = x_j - x_i [.., 3], r"""
        x = np.asarray(x, float)
        H = h_matrix(box)
        s = (x[None, :, :] - x[:, None, :]) @ np.linalg.inv(H)
        d0 = (s - np.rint(s)) @ H
        depth = [int(np.floor(self.cutmax / w + 0.5)) for w in widths(box)]
        I, J, D = [], [], []
        for sh in itertools.product(*[range(-k, k + 1) for k in depth]):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ii, jj = np.nonzero((r2 < self.cutmax ** 2) & (r2 > 0.0))
            I.append(ii); J.append(jj); D.append(d[ii, jj])
        I, J, D = np.concatenate(I), np.concatenate(J), np.concatenate(D)
        return I, J, D, np.sqrt(np.einsum("ij,ij->i", D, D))

    def _terms(self, x, box, types, q):
        types, q = np.asarray(types), np.asarray(q, float)
        I, J, D, R = self.ordered_pairs(x, box)
        eb, deb = np.zeros(len(R)), np.zeros(len(R))
        for a in range(self.p["n"]):
            for b in range(self.p["n"]):
                sel = (types[I] == a) & (types[J] == b)
                if sel.any():
                    eb[sel], deb[sel] = self.born(a, b, R[sel])
        ec, dec = self.coul(q[I] * q[J], R)
        return I, J, D, R, eb, deb, ec, dec

    def energy(self, x, box, types, q):
        """(Born, Coulomb with the self term): half of every ordered pair"""
        _, _, _, _, eb, _, ec, _ = self._terms(x, box, types, q)
        return 0.5 * float(eb.sum()), 0.5 * float(ec.sum()) + self.self_energy(q)

    def compute(self, x, box, types, q):
        """dict e_born, e_coul (with e_self), e_self, e, f [n,3], w (xx yy zz xy xz yz) and its parts w_born, w_coul, w33, npairs (ordered
        pairs inside cutmax), ncoul (ordered pairs inside cut_coul), maxrow (most partners of an atom inside cutmax)"""
        n = len(x)
        I, J, D, R, eb, deb, ec, dec = self._terms(x, box, types, q)
        f = np.zeros((n, 3))
        # force on i from the ordered pair (i, j): +dE/dr d / r (d points from i to j)
        g = ((deb + dec) / R)[:, None] * D if len(R) else np.zeros((0, 3))
        np.add.at(f, I, g)
        parts = []
        for de in (deb, dec):
            gg = (de / R)[:, None] * D if len(R) else np.zeros((0, 3))
            parts.append(-0.5 * np.einsum("ij,ik->jk", D, gg))      # half of d (x) (force on j) per ordered pair
        w33 = parts[0] + parts[1]
        vec = lambda m: np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])
        e_self = self.self_energy(q)
        e_born, e_coul = 0.5 * float(eb.sum()), 0.5 * float(ec.sum()) + e_self
        return dict(e_born=e_born, e_coul=e_coul, e_self=e_self, e=e_born + e_coul, f=f, w=vec(w33), w_born=vec(parts[0]), w_coul=vec(parts[1]), w33=w33,
                    npairs=len(R), ncoul=int((R < self.rc).sum()), maxrow=int(np.bincount(I, minlength=n).max()) if len(I) else 0)

    # ---- dynamics: velocity Verlet, NVE, units real (positions stay unwrapped)
    def nve(self, x, v, box, types, q, masses, dt, nsteps):
        x, v = np.array(x, float), np.array(v, float)
        m = np.asarray(masses, float)[np.asarray(types)][:, None]
        f = self.compute(x, box, types, q)["f"]
        for _ in range(nsteps):
            v += 0.5 * dt * FTM2V * f / m
            x += dt * v
            f = self.compute(x, box, types, q)["f"]
            v += 0.5 * dt * FTM2V * f / m
        return x, v

    def pressure_atm(self, x, v, box, types, q, masses):
        """(sum m v v + W) / V in atm, xx yy zz xy xz yz"""
        m = np.asarray(masses, float)[np.asarray(types)]
        kin = MVV2E * np.einsum("i,ij,ik->jk", m, v, v)
        t = (kin + self.compute(x, box, types, q)["w33"]) / volume(box) * NKTV2P
        return np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])

    def margin(self, x, box, types):
        """smallest distance of any pair distance from cut_coul and from cut_lj of its types (inputs of finite differences keep away)"""
        types = np.asarray(types)
        big = BornDsf(dict(self.p, cut_coul=self.cutmax + 0.5))
        I, J, _, R = big.ordered_pairs(x, box)
        return float(min(np.abs(R - self.rc).min(), np.abs(R - self.p["cut_lj"][types[I], types[J]]).min()))


# ---- inputs the CPU and GPU tests share: type 0 is Na (+1), type 1 is Cl (-1), type 2 (KNaCl) is K (+1) ----
BIG_BOX = np.array([0.0, 0.0, 0.0, 40.0, 40.0, 40.0, 0.0, 0.0, 0.0])


def rocksalt(nx, ny, nz, a=A_NACL):
    """positions, orthogonal box, types and charges of rock salt: Na on the fcc sites, Cl half a cell edge further"""
    fcc = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]], float) * 0.5
    basis = np.vstack([fcc, (fcc + np.array([0.5, 0.0, 0.0])) % 1.0])
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    t = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), len(cells))
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0]), t, np.where(t == 0, 1.0, -1.0)


def case_cell8(a=A_NACL, jitter=0.0, seed=4):
    """the 8-ion cell: narrower than the list radius of 11 A, so the rows are built two images deep and an ion meets its own images"""
    x, box, t, q = rocksalt(1, 1, 1, a)
    if jitter:
        x = x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape)
    return x, box, t, q


def case_jitter(ncell, seed, jitter=0.08, a=A_NACL):
    x, box, t, q = rocksalt(ncell, ncell, ncell, a)
    return x + np.random.default_rng(seed).uniform(-jitter, jitter, x.shape), box, t, q


def case_63(seed=5):
    """2 x 2 x 2 cells with one chlorine missing: a cell of net charge +1, and a short last group of 16 lanes' worth of atoms"""
    x, box, t, q = case_jitter(2, seed)
    keep = np.ones(len(x), bool)
    keep[37] = False
    assert t[37] == 1
    return x[keep], box, t[keep], q[keep]


def case_dimer(ti, tj, qi, qj, r):
    """two ions r apart along x in the 40 A box; the first sits at x = 0 so that the distance is r to the bit"""
    x = np.array([[0.0, 10.0, 10.0], [r, 10.0, 10.0]])
    return x, BIG_BOX.copy(), np.array([ti, tj]), np.array([qi, qj], float)


def case_single(q=1.0):
    return np.array([[3.0, 4.0, 5.0]]), BIG_BOX.copy(), np.array([0]), np.array([q])


def case_triclinic(seed=12):
    """2 x 2 x 2 cells (64 ions), all three tilts, jitter, ions shifted so that several sit outside the box"""
    x, box, t, q = rocksalt(2, 2, 2, 6.0)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])
    x = (x + np.random.default_rng(seed).uniform(-0.08, 0.08, x.shape)) @ F.T
    L = 12.0
    box[6], box[7], box[8] = 0.06 * L, -0.05 * L, 0.04 * L
    x = x + np.array([0.9, -1.3, 0.4])
    H = h_matrix(box)
    x[::7] += H[0]
    x[5::9] -= H[2] + H[1]
    return x, box, t, q


def case_gas(n=40, seed=8, L=26.0, dmin=2.4):
    """a ragged gas: n ions at random in a 26 A box, no two closer than 2.4 A: rows from none to many entries, alternating charges"""
    rng = np.random.default_rng(seed)
    x = []
    while len(x) < n:
        c = rng.uniform(0.0, L, 3) if len(x) % 3 else rng.uniform(8.0, 14.0, 3)      # (a third of them crowd one corner)
        if all(np.linalg.norm(minimage_diff(c, y, [0, 0, 0, L, L, L, 0, 0, 0])) >= dmin for y in x):
            x.append(c)
    t = np.arange(n) % 2
    return np.array(x), np.array([0.0, 0.0, 0.0, L, L, L, 0.0, 0.0, 0.0]), t, np.where(t == 0, 1.0, -1.0)


def case_knacl(seed=3):
    """2 x 2 x 2 cells at 6.0 A with every fourth cation a potassium (type 2): all six pairs of the three types, three Born cutoffs"""
    x, box, t, q = case_jitter(2, seed, a=6.0)
    t = t.copy()
    t[np.nonzero(t == 0)[0][::4]] = 2
    return x, box, t, q
