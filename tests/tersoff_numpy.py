"""Tersoff in plain numpy, FP64: the reference the Tersoff tests compare with (tests/test_tersoff_*.py, tests/test_gpu_tersoff.py).

An independent restatement -- it shares no code with scema_amd/csrc/tersoff/ts_core.h or the library's reader:

  E       = 1/2 sum_i sum_{j != i} fC(r_ij) [ A exp(-lambda1 r_ij) - b_ij B exp(-lambda2 r_ij) ]
  fC      = 1 (r < R - D),  1/2 - 1/2 sin(pi/2 (r - R) / D) (R - D <= r < R + D),  0 (from R + D on)
  b_ij    = (1 + (beta zeta_ij)^n)^(-1/(2n))                      the exact expression at every zeta; zeta == 0 gives (b, b') = (1, 0)
  zeta_ij = sum_{k != i, j} fC(r_ik) g(cos theta_jik) exp[(lambda3 (r_ij - r_ik))^m]
  g(c)    = gamma (1 + c^2 x^2 / (d^2 (d^2 + x^2))),  x = cos - cos0       (the form without cancellation; g_textbook is the other one)

with n, beta, lambda2, B, lambda1, A and the pair's R, D from the file's entry `i j j`, and m, gamma, lambda3, c, d, cos0 and the R, D of
fC(r_ik) from entry `i j k` (LAMMPS pair_tersoff.cpp).  The exponent of zeta's exponential is clamped at +-69.0776 (1e30 above, 0 below);
lambda3 = 0 gives the factor 1.  No LAMMPS and no Tersoff file of the project this one was modelled on exist to compare with: this file,
central differences of its own energy (tests/test_tersoff_host.py) and the closed form of the diamond lattice are what pins the arithmetic.

Neighbours are found by brute force: the minimum image in fractional coordinates plus the 26 images around it.  The energy is a plain
loop over (i, j, k); forces and virial W = sum d (x) f are analytic.  Units are LAMMPS `real`: kcal/mol, Angstrom, fs, g/mol.
"""
import itertools
import math

import numpy as np

from sw_numpy import (BOLTZ, FTM2V, KCALMOL_A3_TO_GPA, MVV2E, NKTV2P, diamond, gas, h_matrix, minimage_diff, strained,  # noqa: F401
                      supercell, volume, widths)

EV_TO_KCALMOL = 23.060549
FIELDS = ["m", "gamma", "lambda3", "c", "d", "costheta0", "n", "beta", "lambda2", "B", "R", "D", "lambda1", "A"]
SI_MASS, C_MASS = 28.0855, 12.011
EXPMAX = 69.0776


def read_tersoff(path, elements, energy_unit=0):
    """{(i, j, k): {field: value}} over the distinct names of `elements` (order of first appearance), and the type map"""
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
                d["A"] *= EV_TO_KCALMOL
                d["B"] *= EV_TO_KCALMOL
            out[tuple(names.index(e) for e in el)] = d
    return out, [names.index(e) for e in elements]


def fc(p, r):
    """fC and its derivative under the R, D of entry p"""
    R, D = p["R"], p["D"]
    if r < R - D:
        return 1.0, 0.0
    if r < R + D:
        a = 0.5 * math.pi * (r - R) / D
        return 0.5 - 0.5 * math.sin(a), -0.25 * math.pi / D * math.cos(a)
    return 0.0, 0.0


def g_stable(p, cos):
    x = cos - p["costheta0"]
    c2, d2 = p["c"] ** 2, p["d"] ** 2
    return p["gamma"] * (1.0 + c2 * x * x / (d2 * (d2 + x * x))), p["gamma"] * 2.0 * c2 * x / (d2 + x * x) ** 2


def g_textbook(p, cos):
    x = cos - p["costheta0"]
    c2, d2 = p["c"] ** 2, p["d"] ** 2
    return p["gamma"] * (1.0 + c2 / d2 - c2 / (d2 + x * x))


def expo(p, dr):
    """exp[(lambda3 dr)^m], clamped, and its derivative with respect to dr"""
    if p["lambda3"] == 0.0:
        return 1.0, 0.0
    m = int(p["m"])
    arg = (p["lambda3"] * dr) ** m
    v = 1.0e30 if arg > EXPMAX else (0.0 if arg < -EXPMAX else math.exp(arg))
    return v, m * p["lambda3"] ** m * dr ** (m - 1) * v


def bond_order(p, zeta):
    """the exact b and db/dzeta"""
    if zeta == 0.0:
        return 1.0, 0.0
    n = p["n"]
    tn = (p["beta"] * zeta) ** n
    if tn == 0.0:
        return 1.0, 0.0
    return (1.0 + tn) ** (-0.5 / n), -0.5 * (1.0 + tn) ** (-0.5 / n - 1.0) * tn / zeta


class Tersoff:
    def __init__(self, params):
        self.p = params
        self.cutmax = max(d["R"] + d["D"] for d in params.values())

    def neighbours(self, x, box, types):
        """per atom the list of (j, image index, d, |d|) with |d| < cutmax, sorted by (j, image index)"""
        H = h_matrix(box)
        Hi = np.linalg.inv(H)
        n = len(x)
        d0 = x[None, :, :] - x[:, None, :]                    # d0[i, j] = x_j - x_i
        s = d0 @ Hi
        d0 = (s - np.rint(s)) @ H
        assert (widths(box) * 1.5 >= self.cutmax).all()        # (|s| <= 1.5 box vectors searched)
        found = [[] for _ in range(n)]
        for m, sh in enumerate(itertools.product((-1, 0, 1), repeat=3)):
            d = d0 + np.array(sh, float) @ H
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ok = r2 < self.cutmax ** 2
            if m == 13:
                ok &= ~np.eye(n, dtype=bool)
            for i, j in zip(*np.nonzero(ok)):
                found[i].append((int(j), m, d[i, j].copy(), math.sqrt(r2[i, j])))
        for row in found:
            row.sort(key=lambda t: (t[0], t[1]))
        return found

    def energy(self, x, box, types):
        """the energy alone: plain loops over (i, j, k)"""
        x = np.asarray(x, float)
        nb = self.neighbours(x, box, types)
        e = 0.0
        for i in range(len(x)):
            ti = types[i]
            for a, (j, _, dj, rj) in enumerate(nb[i]):
                pij = self.p[(ti, types[j], types[j])]
                if not rj < pij["R"] + pij["D"]:
                    continue
                zeta = 0.0
                for b_, (k, _, dk, rk) in enumerate(nb[i]):
                    q = self.p[(ti, types[j], types[k])]
                    if b_ == a or not rk < q["R"] + q["D"]:
                        continue
                    zeta += fc(q, rk)[0] * g_stable(q, float(dj @ dk) / (rj * rk))[0] * expo(q, rj - rk)[0]
                b = bond_order(pij, zeta)[0]
                e += 0.5 * fc(pij, rj)[0] * (pij["A"] * math.exp(-pij["lambda1"] * rj) - b * pij["B"] * math.exp(-pij["lambda2"] * rj))
        return e

    def compute(self, x, box, types):
        """dict e_rep, e_att, e, f [n,3], w (xx yy zz xy xz yz), w33, npairs (ordered pairs inside their cutoff), nzeta (ordered (j, k)
        evaluated), maxin (most neighbours inside the cutoffs under which they are used), nshell (unordered pairs with R - D <= r < R + D)"""
        x = np.asarray(x, float)
        n = len(x)
        nb = self.neighbours(x, box, types)
        f = np.zeros((n, 3))
        w = np.zeros((3, 3))
        e_rep = e_att = 0.0
        npairs = nzeta = maxin = nshell = 0
        for i in range(n):
            ti = types[i]
            used = 0
            for (k, _, dk, rk) in nb[i]:
                cuts = [self.p[(ti, types[k], types[k])]] + [self.p[(ti, tj, types[k])] for tj in set(int(t) for t in types)]
                used += 1 if rk < max(q["R"] + q["D"] for q in cuts) else 0
            maxin = max(maxin, used)
            for a, (j, _, dj, rj) in enumerate(nb[i]):
                pij = self.p[(ti, types[j], types[j])]
                if not rj < pij["R"] + pij["D"]:
                    continue
                npairs += 1
                nshell += 1 if rj >= pij["R"] - pij["D"] else 0
                uj = dj / rj
                terms = []
                zeta = 0.0
                for b_, (k, _, dk, rk) in enumerate(nb[i]):
                    q = self.p[(ti, types[j], types[k])]
                    if b_ == a or not rk < q["R"] + q["D"]:
                        continue
                    nzeta += 1
                    cos = float(dj @ dk) / (rj * rk)
                    fk, dfk = fc(q, rk)
                    gg, dg = g_stable(q, cos)
                    ex, dex = expo(q, rj - rk)
                    zeta += fk * gg * ex
                    uk = dk / rk
                    # gradients of the term with respect to x_j and x_k (x_i takes minus their sum)
                    gj = fk * gg * dex * uj + fk * dg * ex * (uk - cos * uj) / rj
                    gk = (dfk * gg * ex - fk * gg * dex) * uk + fk * dg * ex * (uj - cos * uk) / rk
                    terms.append((k, dk, gj, gk))
                b, db = bond_order(pij, zeta)
                fcj, dfcj = fc(pij, rj)
                fr = pij["A"] * math.exp(-pij["lambda1"] * rj)
                fa = -pij["B"] * math.exp(-pij["lambda2"] * rj)
                e_rep += 0.5 * fcj * fr
                e_att += 0.5 * fcj * b * fa
                dvdr = 0.5 * (dfcj * (fr + b * fa) + fcj * (-pij["lambda1"] * fr - b * pij["lambda2"] * fa))
                fj = -dvdr * uj
                f[j] += fj
                f[i] -= fj
                w += np.outer(dj, fj)
                pref = 0.5 * fcj * fa * db
                for k, dk, gj, gk in terms:
                    f[j] -= pref * gj
                    f[k] -= pref * gk
                    f[i] += pref * (gj + gk)
                    w -= pref * (np.outer(dj, gj) + np.outer(dk, gk))
        w6 = np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[0, 2], w[1, 2]])
        return dict(e_rep=e_rep, e_att=e_att, e=e_rep + e_att, f=f, w=w6, w33=w, npairs=npairs, nzeta=nzeta, maxin=maxin, nshell=nshell // 2)

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


def diamond_energy_per_atom(p, a):
    """closed form on the perfect diamond lattice (four neighbours at r = a sqrt 3 / 4 < R - D, cos = -1/3, lambda3 = 0)"""
    r = a * math.sqrt(3.0) / 4.0
    zeta = 3.0 * g_stable(p, -1.0 / 3.0)[0]
    b = (1.0 + (p["beta"] * zeta) ** p["n"]) ** (-0.5 / p["n"])
    return 2.0 * (p["A"] * math.exp(-p["lambda1"] * r) - b * p["B"] * math.exp(-p["lambda2"] * r))


# ---- the static cases the CPU and GPU tests share (tests/golden/SiC.tersoff) ----
A_SI, A_C, A_SIC = 5.432, 3.5656, 4.36
BIG_BOX = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])


def zeros(n):
    return np.zeros(n, int)


def case_single():
    return np.array([[14.0, 15.0, 16.0]]), BIG_BOX.copy(), zeros(1)


def case_dimer(r=2.3):
    """two atoms r apart along x; the first sits at x = 0, so r is the distance to the bit"""
    return np.array([[0.0, 10.0, 10.0], [r, 10.0, 10.0]]), BIG_BOX.copy(), zeros(2)


def case_trimer():
    """a bent trimer: arms of 2.3 and 2.5 A, 100 degrees apart"""
    t = math.radians(100.0)
    return np.array([[15.0, 15.0, 15.0], [17.3, 15.0, 15.0], [15.0 + 2.5 * math.cos(t), 15.0 + 2.5 * math.sin(t), 15.0]]), BIG_BOX.copy(), zeros(3)


def case_cell8():
    """the 8-atom cubic cell of silicon: the box is narrower than two list radii, each atom meets its own images' neighbours"""
    x, box = diamond(1, 1, 1, A_SI)
    rng = np.random.default_rng(41)
    return x + rng.uniform(-0.05, 0.05, x.shape), box, zeros(8)


def case_a(seed=11, a=A_SI):
    """2 x 2 x 2 cells (64 atoms), jitter 0.1 A"""
    x, box = diamond(2, 2, 2, a)
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, zeros(len(x))


def case_scaled(seed=11):
    """2 x 2 x 2 cells of 0.75 * 5.432 A (box 8.148 A), jitter 0.03 A: bonds of 1.76 A and the twelve second neighbours at 2.88 A, which
    the jitter (at most 0.104 A in a distance) keeps inside the switching shell 2.7 .. 3.0 A: 16 neighbours for every atom, 384 pairs
    in the shell"""
    x, box = diamond(2, 2, 2, 0.75 * A_SI)
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.03, 0.03, x.shape), box, zeros(len(x))


def case_gas(seed):
    """216 atoms at random in a 16.3 A box, no two closer than 2.0 A"""
    box = np.array([0.0, 0.0, 0.0, 16.3, 16.3, 16.3, 0.0, 0.0, 0.0])
    return gas(216, box, 2.0, seed), box, zeros(216)


def case_triclinic(seed=12):
    """3 x 2 x 4 cells (192 atoms), triclinic with all three tilts, atoms shifted so that several sit outside the box"""
    x, box = diamond(3, 2, 4, A_SI)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(seed)
    x = (x + rng.uniform(-0.1, 0.1, x.shape)) @ F.T
    box = box.copy()
    box[6], box[7], box[8] = 0.06 * 2 * A_SI, -0.05 * 4 * A_SI, 0.04 * 4 * A_SI
    x = x + np.array([0.9, -1.3, 0.4])
    H = h_matrix(box)
    x[::17] += H[0]
    x[5::23] -= H[2] + H[1]
    return x, box, zeros(len(x))


def case_sic(seed=13):
    """2 x 2 x 2 cells of zincblende SiC (64 atoms), a = 4.36 A, jitter 0.1 A: type 0 on one fcc sublattice, type 1 on the other"""
    x, box, _ = case_a(seed, A_SIC)
    return x, box, np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), 8)


def case_count(n, seed=15):
    """the first n atoms of a jittered 5 x 5 x 6 silicon block, in the block's box (vacuum where the others were)"""
    x, box = diamond(5, 5, 6, A_SI)
    rng = np.random.default_rng(seed)
    x = x + rng.uniform(-0.1, 0.1, x.shape)
    return x[:n].copy(), box, zeros(n)


def case_crowded(k=33, radius=2.6):
    """a centre atom and k atoms on a Fibonacci sphere of that radius around it (the generator of sw_numpy.cluster): k neighbours inside
    the silicon cutoff of 3.0 A"""
    m = np.arange(k) + 0.5
    z = 1.0 - 2.0 * m / k
    phi = m * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    shell = radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return np.vstack([np.zeros((1, 3)), shell]) + 15.0, BIG_BOX.copy(), zeros(k + 1)


# a synthetic two-element file: m = 1 and m = 3 with lambda3 = 1.3 and gamma = 0.7, so that the exponential factor and its derivative
# are exercised (the clamp is reached through SYNTH_CLAMP below); the entries i j k carry R, D that differ from those of the pair (i, k),
# so that a build which takes the cutoff of fC(r_ik) from the wrong entry fails
SYNTH = """# synthetic Tersoff file of the tests: element X with m = 3, Y with m = 1
X X X  3 0.7 1.3 4.8 2.1 -0.45  0.9  0.35 1.9 310.0  2.9 0.2 2.9 1500.0
Y Y Y  1 0.7 1.3 3.9 1.7 -0.30  1.1  0.22 2.1 280.0  2.7 0.2 3.1 1300.0
X Y Y  3 0.7 1.3 4.8 2.1 -0.45  0.9  0.35 2.0 295.0  2.8 0.2 3.0 1400.0
Y X X  1 0.7 1.3 3.9 1.7 -0.30  1.1  0.22 2.0 295.0  2.8 0.2 3.0 1400.0
X X Y  3 0.7 1.3 4.8 2.1 -0.45  0 0 0 0  2.6 0.3  0 0     # third atom Y around X: cut 2.9, the pair (X, Y) has 3.0
X Y X  3 0.7 1.3 4.8 2.1 -0.45  0 0 0 0  2.7 0.25 0 0     # third atom X around X: cut 2.95, the pair (X, X) has 3.1
Y Y X  1 0.7 1.3 3.9 1.7 -0.30  0 0 0 0  2.9 0.15 0 0     # third atom X around Y: cut 3.05, the pair (Y, X) has 3.0
Y X Y  1 0.7 1.3 3.9 1.7 -0.30  0 0 0 0  2.5 0.3  0 0     # third atom Y around Y: cut 2.8, the pair (Y, Y) has 2.9
"""
# the same with lambda3 = 40: (40 dr)^3 passes +-69.0776 at |dr| = 0.103 A (element X, m = 3: both clamps are reached in case_synth, and
# with them the large-zeta end of b); 40 dr would at 1.73 A (element Y, m = 1: not reached).  Where the factor is clamped the force is
# not the gradient of the energy, here as in LAMMPS: this file is for comparing two implementations, not for central differences
SYNTH_CLAMP = SYNTH.replace(" 0.7 1.3 ", " 0.7 40.0 ")


def case_synth(seed=17):
    """2 x 2 x 2 diamond cells of 5.432 A, the two elements placed at random (so that every entry i j k of the file is used), jitter
    0.15 A: bonds of 1.9 to 2.8 A, across the switching shells of the file"""
    x, box = diamond(2, 2, 2, A_SI)
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.15, 0.15, x.shape), box, rng.integers(0, 2, len(x))


# ---- inputs for the edges of the kernel (tests/test_row_edges_host.py, tests/test_gpu_tersoff_edges.py): generators only ----
SI_CUT = 3.0                     # R + D of silicon in tests/golden/SiC.tersoff
SI_RLIST = SI_CUT + 1.0          # + the default skin of tersoff_configure
SYNTH_CUT = 3.1                  # the largest R + D of SYNTH (the pair X X)


def check_box(box, cutmax=SI_CUT, rlist=SI_RLIST):
    """the conditions every input box of the edge tests meets: each perpendicular width is at least cutmax / 1.5 (Tersoff.neighbours
    searches the fractional minimum image +- 1, complete only above that width) and at least rlist / 2 (below it the engine refuses)"""
    w = widths(box)
    assert (w >= cutmax / 1.5).all() and (w >= rlist / 2.0).all(), w
    return w


def case_shell(seed=17):
    """2 x 2 x 2 diamond cells of 0.78 * 5.432 A (box 8.474 A), the two elements at random, jitter 0.06 A: bonds of 1.83 A and second
    neighbours around 3.0 A, where the pair cutoffs of SYNTH (2.9 to 3.1 A) and the cutoffs of its i j k entries (2.8 to 3.05 A) cross:
    entries at or beyond the pair's own R + D that still count as the third atom of another pair's zeta"""
    x, box = diamond(2, 2, 2, 0.78 * A_SI)
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.06, 0.06, x.shape), box, rng.integers(0, 2, len(x))


def third_only(ref, x, box, types):
    """the number of row entries (i, k) with R + D of the pair (i, k) <= r < the largest R + D under which k is used around i: the
    kernel's entries with fC = 0 that serve as third atoms only"""
    count = 0
    kinds = sorted(set(int(t) for t in types))
    for i, row in enumerate(ref.neighbours(x, box, types)):
        ti = types[i]
        for k, _, _, rk in row:
            own = ref.p[(ti, types[k], types[k])]
            cutin = max([own["R"] + own["D"]] + [ref.p[(ti, tj, types[k])]["R"] + ref.p[(ti, tj, types[k])]["D"] for tj in kinds])
            count += 1 if own["R"] + own["D"] <= rk < cutin else 0
    return count


NARROW_BOX = np.array([0.0, 0.0, 0.0, 2.45, 2.6, 2.75, 0.0, 0.0, 0.0])
SLAB_BOX = np.array([0.0, 0.0, 0.0, 2.9, 5.0, 5.6, 0.0, 0.0, 0.0])
ROD_BOX = np.array([0.0, 0.0, 0.0, 2.45, 4.4, 5.2, 0.0, 0.0, 0.0])


def narrow(name):
    """boxes narrower than one cutoff (3.0 A; the engine refuses below 2.0 A): an atom pairs with its own image, j and k of a zeta term
    may be two images of one atom, a partner's index may be the central atom's own
      N1  one atom in 2.45 x 2.6 x 2.75 A: every neighbour is its own image       N2  two atoms, gas(2, ., 1.9, 7), in the same box
      N3  four atoms, gas(4, ., 2.0, 3), in 2.9 x 5.0 x 5.6 A                      N4  gas(4, ., 2.0, 3) in that box tilted by xy 1.3, xz -1.2,
      N5  N4 with xy -1.3 (widths 2.79 / 4.65 / 5.6 A)                                 yz 2.2 (widths 2.68 / 4.65 / 5.6 A)
      N6  gas(4, ., 2.0, 3) in 2.85 x 5.0 x 5.6 A, types alternating (SYNTH): an atom's own image inside the Y Y shell 2.7 .. 2.9 A
      N7  three atoms, gas(3, ., 2.0, 5), in 2.45 x 4.4 x 5.2 A (dynamics)"""
    if name == "N1":
        x, box, t = np.array([[1.0, 1.0, 1.0]]), NARROW_BOX.copy(), zeros(1)
    elif name == "N2":
        x, box, t = gas(2, NARROW_BOX, 1.9, 7), NARROW_BOX.copy(), zeros(2)
    elif name in ("N3", "N4", "N5", "N6"):
        box = SLAB_BOX.copy()
        if name == "N6":
            box[3] = 2.85          # (not 2.9 A: an atom's own image would sit on the Y Y cutoff of SYNTH to the bit)
        if name in ("N4", "N5"):
            box[6], box[7], box[8] = (1.3 if name == "N4" else -1.3), -1.2, 2.2
        x = gas(4, box, 2.0, 3)          # (the same draws: in N4 the fractional coordinates of N3, in N5 its first candidates)
        t = np.arange(4) % 2 if name == "N6" else zeros(4)
    elif name == "N7":
        x, box, t = gas(3, ROD_BOX, 2.0, 5), ROD_BOX.copy(), zeros(3)
    else:
        raise KeyError(name)
    check_box(box, *((SYNTH_CUT, SYNTH_CUT + 1.0) if name == "N6" else ()))
    return x, box, t


def fterm(ref, x, box, types):
    """the largest pair force at b = 1 among the pairs of a configuration: the size of the terms that cancel in a symmetric one"""
    out = 0.0
    for i, row in enumerate(ref.neighbours(x, box, types)):
        for j, _, _, r in row:
            p = ref.p[(types[i], types[j], types[j])]
            fcv, dfc = fc(p, r)
            fr, fa = p["A"] * math.exp(-p["lambda1"] * r), -p["B"] * math.exp(-p["lambda2"] * r)
            out = max(out, abs(0.5 * (dfc * (fr + fa) + fcv * (-p["lambda1"] * fr - p["lambda2"] * fa))))
    return out
