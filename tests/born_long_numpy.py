"""born/coul/long and buck/coul/long with an Ewald sum in plain numpy, FP64: the reference the Born/long tests compare with
(tests/test_born_long_*.py, tests/test_gpu_born_long.py).

An independent restatement -- it shares no code with scema_amd/csrc/ionic/bl_core.h, the library's reader or its k-space set-up: its own
parser of the script lines, math.erfc, neighbours by brute force over images, an explicit loop over k-vectors, and its own copy of the
g_ewald / kmax / sphere rule of `kspace_style ewald <accuracy>` (LAMMPS, as remembered, unpinned).

  E_born  = A exp((sigma - r)/rho) - C/r^6 + D/r^8                     r < cut_lj[ti][tj], not shifted, counted once per pair
  E_real  = K q_i q_j erfc(g r)/r                                      r < cut_coul, not shifted
  E_recip = (2 pi K/V) sum_{k != 0} exp(-k^2/4g^2)/k^2 |S(k)|^2        S(k) = sum_i q_i exp(i k.r_i); summed over half the space, doubled
  E_self  = -K g/sqrt(pi) sum q_i^2 - K pi (sum q_i)^2/(2 g^2 V)

Forces are the exact gradients; the virial is the strain derivative of the whole energy at fixed g and fixed integer triples.  The triples
belong to a box (`kbox`): k = 2 pi n . H(kbox)^-1; a run keeps them while the box deforms, so `compute` takes the box of the atoms for the
pairs and the volume and `kbox` -- by default the same -- for the k-vectors.  Units are LAMMPS `real`.
"""
import itertools
import math

import numpy as np

from sw_numpy import BOLTZ, FTM2V, MVV2E, NKTV2P, h_matrix, minimage_diff, strained, volume, widths  # noqa: F401

EV_TO_KCALMOL = 23.060549
K_EV, K_KCALMOL = 14.399645, 332.06371
NA_MASS, CL_MASS = 22.98977, 35.453
MG_MASS, O_MASS = 24.305, 15.9994
A_NACL = 5.64
MADELUNG_NACL = 1.7475646
MAXEL = 4
_erfc = np.vectorize(math.erfc, otypes=[float])


def read_born_long(path, energy_unit=None):
    """dict n, cut_coul, K, unit, accuracy, solver, style and [n][n] arrays A (kcal/mol), rho, sigma, C, D, cut_lj of the script lines in
    `path`; energy_unit None: 1 iff the text says `units real`, else 0"""
    style, name, coeffs, unit, ks = None, None, [], None, None
    for raw in open(path):
        w = raw.split("#")[0].split()
        if not w:
            continue
        if w[0] == "pair_style":
            assert style is None and w[1] in ("born/coul/long", "buck/coul/long"), raw
            name, style = w[1].split("/")[0], [float(v) for v in w[2:]]
        elif w[0] == "pair_coeff":
            coeffs.append((w[1], w[2], [float(v) for v in w[3:]]))
        elif w[0] == "units":
            unit = {"metal": 0, "real": 1}[w[1]]
        elif w[0] == "kspace_style":
            assert ks is None and w[1] in ("ewald", "pppm"), raw
            ks = (w[1], float(w[2]))
        assert w[0] != "kspace_modify", raw
    assert style is not None and len(style) in (1, 2) and ks is not None
    cut_lj = style[0]
    cut_coul = style[1] if len(style) == 2 else cut_lj
    if energy_unit is None:
        energy_unit = unit or 0
    named = [int(t) for a, b, _ in coeffs for t in (a, b) if t != "*"]
    n = max(named) if named else MAXEL
    conv = EV_TO_KCALMOL if energy_unit == 0 else 1.0
    p = {k: np.full((n, n), np.nan) for k in ("A", "rho", "sigma", "C", "D", "cut_lj")}
    for a, b, v in coeffs:
        if name == "buck":      # A rho C [cut]
            assert len(v) in (3, 4), v
            v = [v[0], v[1], 0.0, v[2], 0.0] + v[3:]
        else:
            assert len(v) in (5, 6), v
        for i in (range(1, n + 1) if a == "*" else [int(a)]):
            for j in (range(1, n + 1) if b == "*" else [int(b)]):
                if i > j:
                    continue
                for (u, w_) in ((i - 1, j - 1), (j - 1, i - 1)):
                    p["A"][u, w_], p["rho"][u, w_], p["sigma"][u, w_] = v[0] * conv, v[1], v[2]
                    p["C"][u, w_], p["D"][u, w_] = v[3] * conv, v[4] * conv
                    p["cut_lj"][u, w_] = v[5] if len(v) > 5 else cut_lj
    assert not np.isnan(p["A"]).any(), "a pair is never set"
    return dict(p, n=n, cut_coul=cut_coul, unit=energy_unit, K=K_EV * EV_TO_KCALMOL if energy_unit == 0 else K_KCALMOL, accuracy=ks[1], solver=ks[0],
                style=name)


def ewald_rule(box, natoms, qsqsum, rc, accuracy):
    """g_ewald, kmax per dimension of the search and the integer triples [nk, 3] of the half space inside the Cartesian sphere, for that
    box: the rule of `kspace_style ewald <accuracy>` with the relative accuracy (the absolute one is accuracy * K, K cancels)"""
    b = np.asarray(box, float)
    L = b[3:6] - b[:3]
    tt = accuracy * math.sqrt(natoms * rc * L[0] * L[1] * L[2]) / (2.0 * qsqsum)
    g = (1.35 - 0.15 * math.log(accuracy * K_KCALMOL)) / rc if tt >= 1.0 else math.sqrt(-math.log(tt)) / rc
    kmax = []
    for d in range(3):
        km = 1
        while 2.0 * qsqsum * g / L[d] * math.sqrt(1.0 / (math.pi * km * natoms)) * math.exp(-(math.pi * km / (g * L[d])) ** 2) > accuracy:
            km += 1
        kmax.append(km)
    gsqmx = max((2.0 * math.pi * kmax[d] / L[d]) ** 2 for d in range(3)) * 1.00001
    Hinv = np.linalg.inv(h_matrix(b))
    out = []
    for n1 in range(0, kmax[0] + 3):
        for n2 in range(-kmax[1] - 2, kmax[1] + 3):
            for n3 in range(-kmax[2] - 2, kmax[2] + 3):
                if n1 == 0 and (n2 < 0 or (n2 == 0 and n3 <= 0)):
                    continue
                k = 2.0 * math.pi * Hinv @ np.array([n1, n2, n3], float)
                if k @ k <= gsqmx:
                    out.append((n1, n2, n3))
    return g, kmax, np.array(out, int).reshape(-1, 3)


class BornLong:
    def __init__(self, p, accuracy=None):
        self.p = p
        self.rc, self.K = p["cut_coul"], p["K"]
        self.accuracy = p["accuracy"] if accuracy is None else accuracy
        self.cutmax = max(self.rc, float(p["cut_lj"].max()))

    def setup(self, box, q):
        """(g, triples) a run starting in that box uses"""
        q = np.asarray(q, float)
        g, _, tr = ewald_rule(box, len(q), float(np.sum(q * q)), self.rc, self.accuracy)
        return g, tr

    # ---- the pair functions: energy and dE/dr at distances r (arrays), beyond the cutoff exactly 0
    def born(self, ti, tj, r):
        p = self.p
        A, rho, sg, C, D = (p[k][ti, tj] for k in ("A", "rho", "sigma", "C", "D"))
        r = np.asarray(r, float)
        rep = A * np.exp((sg - r) / rho)
        e = rep - C / r ** 6 + D / r ** 8
        de = -rep / rho + 6.0 * C / r ** 7 - 8.0 * D / r ** 9
        inside = r < p["cut_lj"][ti, tj]
        return np.where(inside, e, 0.0), np.where(inside, de, 0.0)

    def real(self, g, qq, r):
        r = np.asarray(r, float)
        ec = _erfc(g * r) if r.size else r
        e = self.K * qq * ec / r
        de = -self.K * qq * (ec / r ** 2 + 2.0 * g / math.sqrt(math.pi) * np.exp(-g * g * r * r) / r)
        inside = r < self.rc
        return np.where(inside, e, 0.0), np.where(inside, de, 0.0)

    def ordered_pairs(self, x, box):
        """every ordered pair (i, j, image) with 0 < r < cutmax: arrays i, j, d = x_j - x_i [.., 3], r"""
        x = np.asarray(x, float)
        H = h_matrix(box)
        s = (x[None, :, :] - x[:, None, :]) @ np.linalg.inv(H)
        d0 = (s - np.rint(s)) @ H
        tilted = 1 if np.any(np.asarray(box)[6:9] != 0.0) else 0
        depth = [int(np.floor(self.cutmax / w + 0.5)) + tilted for w in widths(box)]
        I, J, D = [], [], []
        for sh in itertools.product(*[range(-k, k + 1) for k in depth]):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ii, jj = np.nonzero((r2 < self.cutmax ** 2) & (r2 > 0.0))
            I.append(ii); J.append(jj); D.append(d[ii, jj])
        I, J, D = np.concatenate(I), np.concatenate(J), np.concatenate(D)
        return I, J, D, np.sqrt(np.einsum("ij,ij->i", D, D))

    def recip(self, x, box, q, g, triples, kbox=None, half_factor=2.0):
        """(energy, forces [n, 3], virial 3 x 3) of the reciprocal sum, one k-vector after the other"""
        x, q = np.asarray(x, float), np.asarray(q, float)
        V = volume(box)
        Hinv = np.linalg.inv(h_matrix(box if kbox is None else kbox))
        e, f, w = 0.0, np.zeros((len(x), 3)), np.zeros((3, 3))
        for n in np.asarray(triples, float).reshape(-1, 3):
            k = 2.0 * math.pi * Hinv @ n
            k2 = float(k @ k)
            ph = x @ k
            c, s = np.cos(ph), np.sin(ph)
            sr, si = float(q @ c), float(q @ s)
            ck = half_factor * 2.0 * math.pi * self.K / V * math.exp(-k2 / (4.0 * g * g)) / k2
            ek = ck * (sr * sr + si * si)
            e += ek
            f += (-2.0 * ck * q * (si * c - sr * s))[:, None] * k[None, :]
            w += ek * (np.eye(3) - 2.0 * (1.0 / k2 + 0.25 / (g * g)) * np.outer(k, k))
        return e, f, w

    def self_terms(self, box, q, g):
        """(point self energy, background energy)"""
        q = np.asarray(q, float)
        return float(-self.K * g / math.sqrt(math.pi) * np.sum(q * q)), float(-self.K * math.pi * np.sum(q) ** 2 / (2.0 * g * g * volume(box)))

    def compute(self, x, box, types, q, g=None, triples=None, kbox=None):
        """dict e_born, e_coul (real + recip + self + background) and its parts e_real, e_recip, e_self, e_bg, e, f [n,3], w (xx yy zz xy xz
        yz) and its parts w_born, w_coul, w33, npairs (ordered pairs inside cutmax), ncoul (inside cut_coul), maxrow, g, nk"""
        types, q = np.asarray(types), np.asarray(q, float)
        if g is None:
            g, triples = self.setup(box, q)
        n = len(x)
        I, J, D, R = self.ordered_pairs(x, box)
        eb, deb = np.zeros(len(R)), np.zeros(len(R))
        for a in range(self.p["n"]):
            for b in range(self.p["n"]):
                sel = (types[I] == a) & (types[J] == b)
                if sel.any():
                    eb[sel], deb[sel] = self.born(a, b, R[sel])
        ec, dec = self.real(g, q[I] * q[J], R)
        f = np.zeros((n, 3))
        if len(R):
            np.add.at(f, I, ((deb + dec) / R)[:, None] * D)      # force on i from the ordered pair (i, j): +dE/dr d / r
        parts = []
        for de in (deb, dec):
            gg = (de / R)[:, None] * D if len(R) else np.zeros((0, 3))
            parts.append(-0.5 * np.einsum("ij,ik->jk", D, gg))
        er, fr, wr = self.recip(x, box, q, g, triples, kbox)
        e_self, e_bg = self.self_terms(box, q, g)
        w_coul = parts[1] + wr + e_bg * np.eye(3)
        w33 = parts[0] + w_coul
        vec = lambda m: np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])
        e_born, e_real = 0.5 * float(eb.sum()), 0.5 * float(ec.sum())
        e_coul = e_real + er + e_self + e_bg
        return dict(e_born=e_born, e_coul=e_coul, e_real=e_real, e_recip=er, e_self=e_self, e_bg=e_bg, e=e_born + e_coul, f=f + fr, f_recip=fr, w=vec(w33),
                    w_born=vec(parts[0]), w_coul=vec(w_coul), w_real=vec(parts[1]), w_recip=vec(wr), w33=w33, npairs=len(R), ncoul=int((R < self.rc).sum()),
                    maxrow=int(np.bincount(I, minlength=n).max()) if len(I) else 0, g=g, nk=len(triples))

    # ---- dynamics: velocity Verlet, units real (positions stay unwrapped); g and the triples are those of the start box
    def nve(self, x, v, box, types, q, masses, dt, nsteps, rates=None):
        """NVE; with rates (xx yy zz xy xz yz per fs, fix deform erate with remap x): the box moves linearly after every step and carries
        the positions along; the box is never flipped.  Returns x, v, and with rates the end box and the mean of the pressure (atm) sampled
        at every step before the box moves"""
        x, v = np.array(x, float), np.array(v, float)
        box0 = np.array(box, float)
        m = np.asarray(masses, float)[np.asarray(types)][:, None]
        g, tr = self.setup(box0, q)
        cur = box0.copy()
        c = self.compute(x, cur, types, q, g, tr, box0 if rates is None else cur)
        psum = np.zeros(6)
        for step in range(1, nsteps + 1):
            v += 0.5 * dt * FTM2V * c["f"] / m
            x += dt * v
            c = self.compute(x, cur, types, q, g, tr, cur)
            v += 0.5 * dt * FTM2V * c["f"] / m
            if rates is not None:
                kin = MVV2E * np.einsum("i,ij,ik->jk", m[:, 0], v, v)
                t = (kin + c["w33"]) / volume(cur) * NKTV2P
                psum += np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])
                L0, tt = box0[3:6] - box0[:3], step * dt
                nb = cur.copy()
                nb[:3] = box0[:3] - 0.5 * L0 * np.asarray(rates[:3]) * tt
                nb[3:6] = box0[3:6] + 0.5 * L0 * np.asarray(rates[:3]) * tt
                nb[6] = box0[6] + rates[3] * L0[1] * tt
                nb[7] = box0[7] + rates[4] * L0[2] * tt
                nb[8] = box0[8] + rates[5] * L0[2] * tt
                x = (x - cur[:3]) @ np.linalg.inv(h_matrix(cur)) @ h_matrix(nb) + nb[:3]
                cur = nb
        if rates is None:
            return x, v
        return x, v, cur, psum / nsteps

    def pressure_atm(self, x, v, box, types, q, masses, g=None, triples=None, kbox=None):
        """(sum m v v + W) / V in atm, xx yy zz xy xz yz"""
        m = np.asarray(masses, float)[np.asarray(types)]
        kin = MVV2E * np.einsum("i,ij,ik->jk", m, v, v)
        t = (kin + self.compute(x, box, types, q, g, triples, kbox)["w33"]) / volume(box) * NKTV2P
        return np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])

    def margin(self, x, box, types):
        """smallest distance of any pair distance from cut_coul and from cut_lj of its types (inputs of finite differences keep away)"""
        types = np.asarray(types)
        big = BornLong(dict(self.p, cut_coul=self.cutmax + 0.5))
        I, J, _, R = big.ordered_pairs(x, box)
        return float(min(np.abs(R - self.rc).min(), np.abs(R - self.p["cut_lj"][types[I], types[J]]).min()))


# ---- inputs the CPU and GPU tests share: type 0 is the cation, type 1 the anion ----
def rocksalt(nx, ny, nz, a=A_NACL, charge=1.0):
    """positions, orthogonal box, types and charges of rock salt: cations on the fcc sites, anions half a cell edge further"""
    fcc = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]], float) * 0.5
    basis = np.vstack([fcc, (fcc + np.array([0.5, 0.0, 0.0])) % 1.0])
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    t = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), len(cells))
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0]), t, np.where(t == 0, charge, -charge)


def case_jitter(cells, seed, sigma=0.15, a=A_NACL, charge=1.0):
    """rock salt of cells = (nx, ny, nz) or n for a cube, every coordinate moved by a normal deviate of that sigma"""
    cells = (cells,) * 3 if isinstance(cells, int) else cells
    x, box, t, q = rocksalt(*cells, a=a, charge=charge)
    return x + np.random.default_rng(seed).normal(0.0, sigma, x.shape), box, t, q


def case_without(case, drop):
    """the case with the atoms `drop` taken out (a cell that is not neutral)"""
    x, box, t, q = case
    keep = np.ones(len(x), bool)
    keep[list(drop)] = False
    return x[keep], box, t[keep], q[keep]


def case_with_extra(case, seed=2):
    """the case with one more cation at the most open spot among 4 000 random points (65 ions: not neutral, one past a staging width)"""
    x, box, t, q = case
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.0, 1.0, (4000, 3)) * (box[3:6] - box[:3])
    dmin = np.array([np.abs(np.linalg.norm(minimage_diff(np.tile(p, (len(x), 1)), x, box), axis=1)).min() for p in c])
    p = c[np.argmax(dmin)]
    return np.vstack([x, p]), box, np.append(t, 0), np.append(q, abs(q[0]))


def case_single(q=1.0, L=12.0):
    return np.array([[3.0, 4.0, 5.0]]), np.array([0.0, 0.0, 0.0, L, L, L, 0.0, 0.0, 0.0]), np.array([0]), np.array([q])


def case_two(L=6.0):
    """two ions +1 and -1 in a 6 A cube: the image search two boxes deep"""
    return np.array([[0.7, 1.1, 0.4], [3.4, 3.9, 2.9]]), np.array([0.0, 0.0, 0.0, L, L, L, 0.0, 0.0, 0.0]), np.array([0, 1]), np.array([1.0, -1.0])


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


def case_flip(seed=14):
    """2 x 2 x 2 cells (64 ions) at 6.0 A in a box tilted close to the flip in xy and in xz, and rates (per fs) that carry xy past half
    a box length after a few steps and xz a few steps later"""
    x, box, t, q = rocksalt(2, 2, 2, 6.0)
    L = 12.0
    txy, txz = 0.4975, 0.4955
    F = np.array([[1.0, txy, txz], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    x = (x + np.random.default_rng(seed).normal(0.0, 0.08, x.shape)) @ F.T
    box[6], box[7] = txy * L, txz * L
    rates = np.array([0.0, 0.0, 0.0, 5e-4, 5e-4, 0.0])
    return (x, box, t, q), rates
