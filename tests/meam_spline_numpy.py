"""Spline MEAM (`pair_style meam/spline`) in plain numpy, FP64: the reference the tests compare with (tests/test_meam_spline_*.py,
tests/test_gpu_meam_spline.py).

An independent restatement -- it shares no code with scema_amd/csrc/meam_spline/ms_core.h or the library's reader:

  E     = sum_{i<j} phi_{ti tj}(r_ij) + sum_i [ U_ti(rho_i) - U_ti(0) ]
  rho_i = sum_j rho_tj(r_ij) + sum_{j<k} f_tj(r_ij) f_tk(r_ik) g_{tj tk}(cos theta_jik)

Every function is a clamped cubic spline through its knots with the two end slopes of the file; its second derivatives come from a dense
solve of the tridiagonal system (np.linalg.solve -- the library sweeps), its value from the piecewise cubic in Hermite-free "a, b" form
written out below, and outside the knots it continues linearly with its end slope.  phi, rho and f are zero at and beyond their last knot
(strict test r < last knot).  Neighbours are found by brute force: the fractional minimum image plus as many images around it as the
largest range reaches.  `energy` sums the energy alone in plain loops and is what the central differences of
tests/test_meam_spline_host.py take; `compute` sums energies, analytic forces and the virial W = sum d (x) f.  Units are LAMMPS `real`:
kcal/mol, Angstrom, fs, g/mol.

The file also states the analytic shapes of the two fixtures (tests/golden/make_meam_spline_fixture.py samples them) and the inputs
the CPU and GPU tests share.  The fixtures were written for this project: they come neither from LAMMPS nor from the reference, and are not
physically accurate.
"""
import itertools

import numpy as np

from sw_numpy import BOLTZ, FTM2V, KCALMOL_A3_TO_GPA, MVV2E, NKTV2P, h_matrix, minimage_diff, strained, volume, widths  # noqa: F401

EV_TO_KCALMOL = 23.060549
TI_MASS, O_MASS = 47.867, 15.999


# ---- one spline ----
class Spline:
    def __init__(self, x, y, d0, dn):
        self.x, self.y, self.d0, self.dn = np.asarray(x, float), np.asarray(y, float), float(d0), float(dn)
        n = len(self.x)
        assert n >= 2 and (np.diff(self.x) > 0.0).all()
        h = np.diff(self.x)
        A = np.zeros((n, n))
        b = np.zeros(n)
        A[0, 0], A[0, 1] = h[0] / 3.0, h[0] / 6.0
        b[0] = (self.y[1] - self.y[0]) / h[0] - self.d0
        for i in range(1, n - 1):
            A[i, i - 1], A[i, i], A[i, i + 1] = h[i - 1] / 6.0, (h[i - 1] + h[i]) / 3.0, h[i] / 6.0
            b[i] = (self.y[i + 1] - self.y[i]) / h[i] - (self.y[i] - self.y[i - 1]) / h[i - 1]
        A[n - 1, n - 2], A[n - 1, n - 1] = h[-1] / 6.0, h[-1] / 3.0
        b[n - 1] = self.dn - (self.y[-1] - self.y[-2]) / h[-1]
        self.m = np.linalg.solve(A, b)
        self.last = self.x[-1]

    def __call__(self, t):
        """(value, derivative) at the scalar t"""
        x, y, m = self.x, self.y, self.m
        if t < x[0]:
            return y[0] + self.d0 * (t - x[0]), self.d0
        if t > x[-1]:
            return y[-1] + self.dn * (t - x[-1]), self.dn
        k = min(max(int(np.searchsorted(x, t, side="right")) - 1, 0), len(x) - 2)
        h = x[k + 1] - x[k]
        a, b = (x[k + 1] - t) / h, (t - x[k]) / h
        v = a * y[k] + b * y[k + 1] + ((a ** 3 - a) * m[k] + (b ** 3 - b) * m[k + 1]) * h * h / 6.0
        d = (y[k + 1] - y[k]) / h - (3.0 * a * a - 1.0) / 6.0 * h * m[k] + (3.0 * b * b - 1.0) / 6.0 * h * m[k + 1]
        return v, d


# ---- the analytic shapes of the fixtures (eV, A): smooth functions sampled at 8 to 16 knots; phi, rho and f end with value 0 and slope 0
# through a cubed factor (rc - r)^3 ----
def shape_phi(amp, rz, rc):
    return lambda r: amp * (rc - r) ** 3 * (rz - r), lambda r: amp * (-3.0 * (rc - r) ** 2 * (rz - r) - (rc - r) ** 3)


def shape_rho(amp, rc):
    return lambda r: amp * (rc - r) ** 3, lambda r: -3.0 * amp * (rc - r) ** 2


def shape_u(a, b, s):
    return lambda p: -a * np.sqrt(p + s) + b * p * p, lambda p: -0.5 * a / np.sqrt(p + s) + 2.0 * b * p


def shape_f(amp, rc):
    return lambda r: amp * (rc - r) ** 3 * np.exp(-0.25 * r), lambda r: amp * np.exp(-0.25 * r) * (-3.0 * (rc - r) ** 2 - 0.25 * (rc - r) ** 3)


def shape_g(g0, g1, g2, g3):
    return lambda c: g0 + g1 * (c + 0.33) ** 2 + g2 * c ** 3 + g3 * c, lambda c: 2.0 * g1 * (c + 0.33) + 3.0 * g2 * c * c + g3


def _nonuniform(lo, hi, n, power):
    """n knots from lo to hi, denser towards lo"""
    x = lo + (hi - lo) * np.linspace(0.0, 1.0, n) ** power
    x[-1] = hi
    return x


G_KNOTS = np.array([-1.0, -0.8, -0.55, -0.25, 0.0, 0.3, 0.6, 0.85, 1.0])
# U: equidistant knots from -3 (below zero density) in steps of 4: the first interior knot, 1, lies above the density of a distant pair,
# the last, 33, below that of a compressed lattice
U_KNOTS = np.linspace(-3.0, 33.0, 10)

# (name, knots, shape); the old one-element format holds phi, rho, U, f, g in this order
TI_FUNCTIONS = [
    ("phi", _nonuniform(1.8, 5.5, 12, 1.4), shape_phi(0.02, 2.7, 5.5)),      # non-uniform
    ("rho", np.linspace(1.8, 5.0, 9), shape_rho(0.15, 5.0)),                 # uniform, h = 0.4
    ("U", U_KNOTS, shape_u(1.5, 0.002, 12.0)),                               # uniform, h = 4
    ("f", _nonuniform(1.8, 3.4, 8, 1.3), shape_f(6.0, 3.4)),                 # non-uniform, clearly shorter than phi
    ("g", G_KNOTS, shape_g(-0.1, 0.6, -0.25, 0.05)),                         # non-uniform on [-1, 1]
]
# the new format, elements Ti O: families phi (TiTi TiO OO), rho (Ti O), U (Ti O), f (Ti O), g (TiTi TiO OO), an amplitude of its own each
TIO_ELEMENTS = ("Ti", "O")
TIO_FUNCTIONS = [
    ("phi", _nonuniform(1.8, 5.5, 12, 1.4), shape_phi(0.02, 2.7, 5.5)),
    ("phi", _nonuniform(1.4, 5.0, 11, 1.3), shape_phi(0.031, 2.1, 5.0)),
    ("phi", np.linspace(1.2, 4.6, 16), shape_phi(0.043, 2.4, 4.6)),
    ("rho", np.linspace(1.8, 5.0, 9), shape_rho(0.15, 5.0)),
    ("rho", _nonuniform(1.2, 4.4, 10, 1.2), shape_rho(0.11, 4.4)),
    ("U", U_KNOTS, shape_u(1.5, 0.002, 12.0)),
    ("U", np.linspace(-3.0, 33.0, 13), shape_u(1.1, 0.0031, 9.0)),
    ("f", _nonuniform(1.8, 3.4, 8, 1.3), shape_f(6.0, 3.4)),
    ("f", np.linspace(1.2, 3.0, 10), shape_f(4.3, 3.0)),
    ("g", G_KNOTS, shape_g(-0.1, 0.6, -0.25, 0.05)),
    ("g", np.linspace(-1.0, 1.0, 11), shape_g(0.07, 0.45, 0.2, -0.11)),
    ("g", G_KNOTS, shape_g(-0.05, 0.8, -0.1, 0.17)),
]
TI_CUT, TI_CUT_RHO, TI_CUT_F = 5.5, 5.0, 3.4
TI_KNOT = float(np.linspace(1.8, 5.0, 9)[6])      # an interior knot of rho (4.2 A), as the file holds it


# ---- files ----
def read_meam_spline(path, elements, energy_unit=0):
    """(splines, type_map): splines = dict phi[(a, b)] (a <= b), rho[a], U[a], f[a], g[(a, b)] over the distinct elements named, in order
    of first appearance; phi and U in kcal/mol"""
    with open(path) as fh:
        lines = fh.read().split("\n")
    pos = 1
    head = lines[1].split()
    fresh = bool(head) and head[0] == "meam/spline"
    if fresh:
        file_el = head[2:]
        assert int(head[1]) == len(file_el)
        pos = 2
    else:
        file_el = [None]
    nf = len(file_el)
    npf = nf * (nf + 1) // 2

    def one(scale):
        nonlocal pos
        if fresh:
            assert lines[pos].split() == ["spline3eq"]
            pos += 1
        n = int(lines[pos].split()[0])
        d0, dn = (float(w) for w in lines[pos + 1].split())
        pos += 2 if fresh else 3
        tab = np.array([[float(w) for w in lines[pos + k].split()[:2]] for k in range(n)])
        pos += n
        return Spline(tab[:, 0], tab[:, 1] * scale, d0 * scale, dn * scale)

    es = EV_TO_KCALMOL if energy_unit == 0 else 1.0
    fam = [[one(es) for _ in range(npf)], [one(1.0) for _ in range(nf)], [one(es) for _ in range(nf)], [one(1.0) for _ in range(nf)],
           [one(1.0) for _ in range(npf)]]
    if fresh:
        kept = list(dict.fromkeys(elements))
        where = [file_el.index(e) for e in kept]
        type_map = [kept.index(e) for e in elements]
    else:
        where, type_map = [0], [0] * len(elements)
    tri = {}
    for a in range(nf):
        for b in range(a, nf):
            tri[(a, b)] = len(tri)
    pidx = lambda a, b: tri[(min(a, b), max(a, b))]
    out = dict(phi={}, rho={}, U={}, f={}, g={})
    for a, fa in enumerate(where):
        out["rho"][a], out["U"][a], out["f"][a] = fam[1][fa], fam[2][fa], fam[3][fa]
        for b, fb in enumerate(where):
            if b >= a:
                out["phi"][(a, b)], out["g"][(a, b)] = fam[0][pidx(fa, fb)], fam[4][pidx(fa, fb)]
    return out, type_map


class MeamSpline:
    def __init__(self, splines):
        self.s = splines
        self.ne = len(splines["rho"])
        self.cut_rho = np.array([splines["rho"][a].last for a in range(self.ne)])
        self.cut_f = np.array([splines["f"][a].last for a in range(self.ne)])
        self.cutmax = max(self.cut_rho.max(), self.cut_f.max(), max(p.last for p in splines["phi"].values()))

    def phi(self, a, b):
        return self.s["phi"][(min(a, b), max(a, b))]

    def g(self, a, b):
        return self.s["g"][(min(a, b), max(a, b))]

    def ordered_pairs(self, x, box, types):
        """every ordered pair (i, j, image) with 0 < r < cutmax: arrays i, j, d = x_j - x_i [.., 3], r; sorted by (i, j, image)"""
        x = np.asarray(x, float)
        H = h_matrix(box)
        n = len(x)
        s = (x[None, :, :] - x[:, None, :]) @ np.linalg.inv(H)
        d0 = (s - np.rint(s)) @ H
        tilt = 1 if (box[6] != 0.0 or box[7] != 0.0 or box[8] != 0.0) else 0
        depth = [int(np.floor(self.cutmax / w + 0.5)) + tilt for w in widths(box)]
        I, J, M, D = [], [], [], []
        for m, sh in enumerate(itertools.product(*[range(-k, k + 1) for k in depth])):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ii, jj = np.nonzero((r2 < self.cutmax ** 2 * (1.0 + 1e-12)) & (r2 > 0.0))
            keep = np.sqrt(r2[ii, jj]) < self.cutmax
            ii, jj = ii[keep], jj[keep]
            I.append(ii); J.append(jj); M.append(np.full(len(ii), m)); D.append(d[ii, jj])
        I, J, M, D = np.concatenate(I), np.concatenate(J), np.concatenate(M), np.concatenate(D)
        order = np.lexsort((M, J, I))
        I, J, D = I[order], J[order], D[order]
        return I, J, D, np.linalg.norm(D, axis=1), n

    def density(self, ti, tj, D, R):
        """rho of one atom of element ti from its neighbours (elements tj, vectors D, distances R)"""
        rho = 0.0
        arms = []
        for k in range(len(R)):
            if R[k] < self.cut_rho[tj[k]]:
                rho += self.s["rho"][tj[k]](R[k])[0]
            if R[k] < self.cut_f[tj[k]]:
                arms.append(k)
        for p in range(len(arms)):
            for q in range(p + 1, len(arms)):
                a, b = arms[p], arms[q]
                c = np.dot(D[a], D[b]) / (R[a] * R[b])
                rho += self.s["f"][tj[a]](R[a])[0] * self.s["f"][tj[b]](R[b])[0] * self.g(tj[a], tj[b])(c)[0]
        return rho, arms

    def energy(self, x, box, types):
        """energy alone, as plain loops over atoms, neighbours and pairs of neighbours"""
        types = np.asarray(types)
        I, J, D, R, n = self.ordered_pairs(x, box, types)
        start = np.searchsorted(I, np.arange(n + 1))
        e = 0.0
        for i in range(n):
            lo, hi = start[i], start[i + 1]
            tj = types[J[lo:hi]]
            for k in range(lo, hi):
                p = self.phi(types[i], types[J[k]])
                if R[k] < p.last:
                    e += 0.5 * p(R[k])[0]
            rho, _ = self.density(types[i], tj, D[lo:hi], R[lo:hi])
            U = self.s["U"][types[i]]
            e += U(rho)[0] - U(0.0)[0]
        return e

    def compute(self, x, box, types):
        """dict e_pair, e_embed, e, f [n,3], w (xx yy zz xy xz yz), w33, npairs (ordered pairs inside cutmax), ntriplets, maxin (most
        neighbours inside f's range), rho [n]"""
        types = np.asarray(types)
        I, J, D, R, n = self.ordered_pairs(x, box, types)
        start = np.searchsorted(I, np.arange(n + 1))
        f = np.zeros((n, 3))
        w = np.zeros((3, 3))
        rhos, up = np.zeros(n), np.zeros(n)
        e_pair = e_embed = 0.0
        ntrip = maxin = 0
        lists = []
        for i in range(n):
            lo, hi = start[i], start[i + 1]
            rho, arms = self.density(types[i], types[J[lo:hi]], D[lo:hi], R[lo:hi])
            U = self.s["U"][types[i]]
            u, du = U(rho)
            e_embed += u - U(0.0)[0]
            rhos[i], up[i] = rho, du
            lists.append(arms)
            maxin = max(maxin, len(arms))

        def push(i, j, d, g):
            """g = dE/d d of the vector d from i to j"""
            f[j] -= g
            f[i] += g
            nonlocal w
            w -= np.outer(d, g)

        for i in range(n):
            lo, hi = start[i], start[i + 1]
            ti = types[i]
            for k in range(lo, hi):
                tj, r, u = types[J[k]], R[k], D[k] / R[k]
                p = self.phi(ti, tj)
                if r < p.last:
                    v, dv = p(r)
                    e_pair += 0.5 * v
                    push(i, J[k], D[k], 0.5 * dv * u)
                if r < self.cut_rho[tj]:       # what j adds to the density at i
                    push(i, J[k], D[k], up[i] * self.s["rho"][tj](r)[1] * u)
            arms = lists[i]
            for p_ in range(len(arms)):
                for q_ in range(p_ + 1, len(arms)):
                    a, b = lo + arms[p_], lo + arms[q_]
                    ntrip += 1
                    ta, tb = types[J[a]], types[J[b]]
                    ua, ub = D[a] / R[a], D[b] / R[b]
                    c = float(np.dot(ua, ub))
                    fa, dfa = self.s["f"][ta](R[a])
                    fb, dfb = self.s["f"][tb](R[b])
                    g, dg = self.g(ta, tb)(c)
                    push(i, J[a], D[a], up[i] * (dfa * fb * g * ua + fa * fb * dg * (ub - c * ua) / R[a]))
                    push(i, J[b], D[b], up[i] * (fa * dfb * g * ub + fa * fb * dg * (ua - c * ub) / R[b]))
        w6 = np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[0, 2], w[1, 2]])
        return dict(e_pair=e_pair, e_embed=e_embed, e=e_pair + e_embed, f=f, w=w6, w33=w, npairs=len(I), ntriplets=ntrip, maxin=maxin, rho=rhos)

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


# ---- inputs the CPU and GPU tests share: element 0 is Ti, element 1 is O (elements ("Ti", "O")) ----
BIG_BOX = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])


def bcc(nx, ny, nz, a):
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = np.vstack([cells, cells + 0.5]) * a
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0])


def case_dimer(r, ti=0, tj=0):
    """two atoms r apart along x in the 30 A box; the first sits at x = 0 so that the distance is r to the bit"""
    return np.array([[0.0, 10.0, 10.0], [r, 10.0, 10.0]]), BIG_BOX.copy(), np.array([ti, tj])


def case_trimer(r1=2.6, r2=2.9, angle=100.0, t=(0, 0, 0)):
    """a bent trimer, the central atom first and at the origin of the arms: the arm r1 lies along x exactly"""
    a = np.radians(angle)
    x = np.array([[0.0, 10.0, 10.0], [r1, 10.0, 10.0], [r2 * np.cos(a), 10.0 + r2 * np.sin(a), 10.0]])
    return x, BIG_BOX.copy(), np.array(t)


def case_collinear(r1=2.5, r2=2.75):
    """i between j and k on the x axis: cos theta = -1 exactly (the products are exact: one coordinate)"""
    return np.array([[0.0, 10.0, 10.0], [r1, 10.0, 10.0], [-r2, 10.0, 10.0]]), BIG_BOX.copy(), np.zeros(3, int)


def case_near_degenerate(r1=2.3, r2=3.2, eps=1e-7):
    """both arms almost along x on the same side: cos theta -> 1, and may round past it"""
    return np.array([[0.0, 10.0, 10.0], [r1, 10.0, 10.0], [r2, 10.0 + eps, 10.0]]), BIG_BOX.copy(), np.zeros(3, int)


def fibonacci_sphere(m, radius):
    k = np.arange(m) + 0.5
    z = 1.0 - 2.0 * k / m
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)


def case_cluster(m, radius=3.2, outer=0, outer_radius=4.6):
    """an atom at the centre of m atoms on a Fibonacci sphere inside f's range (3.4 A), and of `outer` more on a sphere between f's range
    and cutmax: the centre's list holds m entries"""
    parts = [np.zeros((1, 3)), fibonacci_sphere(m, radius)] + ([fibonacci_sphere(outer, outer_radius)] if outer else [])
    x = np.vstack(parts) + 15.0
    return x, BIG_BOX.copy(), np.zeros(len(x), int)


def case_bcc(nx=1, ny=1, nz=2, a=3.2, jitter=0.0, seed=1, two_elements=None):
    """bcc titanium; with jitter > 0 Gaussian displacements.  two_elements "ordered": the body centres are oxygen (B2), "random": a random
    half"""
    x, box = bcc(nx, ny, nz, a)
    rng = np.random.default_rng(seed)
    if jitter:
        x = x + rng.normal(0.0, jitter, x.shape)
    t = np.zeros(len(x), int)
    if two_elements == "ordered":
        t[len(x) // 2:] = 1
    elif two_elements == "random":
        t = rng.integers(0, 2, len(x))
    return x, box, t


def case_count(n, a=3.3, jitter=0.08, seed=5):
    """n atoms of a jittered bcc block of 4 x 4 x 2 cells (64 sites) or 4 x 4 x 3 (96 sites, for 65) with vacancies"""
    x, box = bcc(4, 4, 2 if n <= 64 else 3, a)
    x = x + np.random.default_rng(seed).normal(0.0, jitter, x.shape)
    keep = np.ones(len(x), bool)
    if len(x) > n:
        keep[np.linspace(1, len(x) - 2, len(x) - n).astype(int)] = False
    assert keep.sum() == n
    return x[keep], box, np.zeros(n, int)


def case_block(n=1025, a=3.3, jitter=0.05, seed=8):
    """n atoms of a jittered bcc block of 8 x 8 x 9 cells (1 152 sites) with vacancies: past the LDS force table of 1 024"""
    x, box = bcc(8, 8, 9, a)
    x = x + np.random.default_rng(seed).normal(0.0, jitter, x.shape)
    keep = np.ones(len(x), bool)
    keep[np.linspace(3, len(x) - 2, len(x) - n).astype(int)] = False
    assert keep.sum() == n
    return x[keep], box, np.zeros(n, int)


def case_triclinic(seed=12, two_elements=None):
    """3 x 3 x 3 bcc cells (54 atoms) at 3.3 A, all three tilts, jitter, atoms shifted so that several sit outside the box"""
    x, box, t = case_bcc(3, 3, 3, 3.3, 0.08, seed, two_elements)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])
    x = x @ F.T
    L = box[3]
    box[6], box[7], box[8] = 0.06 * L, -0.05 * L, 0.04 * L
    x = x + np.array([0.9, -1.3, 0.4])
    H = h_matrix(box)
    x[::7] += H[0]
    x[5::9] -= H[2] + H[1]
    return x, box, t
