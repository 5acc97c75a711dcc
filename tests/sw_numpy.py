"""Stillinger-Weber in plain numpy, FP64: the reference the SW tests compare with (tests/test_sw_*.py, tests/test_gpu_sw.py).

An independent restatement -- it shares no code with scema_amd/csrc/sw/sw_core.h or the library's reader:

  phi2(r)          = A eps (B (sigma/r)^p - (sigma/r)^q) exp(sigma / (r - a sigma))                          r < a sigma
  phi3(r1, r2, th) = lambda eps (cos th - cos th0)^2 exp(g1 s1 / (r1 - a1 s1) + g2 s2 / (r2 - a2 s2))       r1 < a1 s1, r2 < a2 s2

with the pair parameters of (i, j) from the file's entry `i j j` and lambda, eps, cos th0 of a triplet centred on i from entry `i j k`
(LAMMPS pair_sw.cpp).  Neighbours are found by minimum image in fractional coordinates plus the 26 images around it, so boxes down to one
cutoff wide are right.  Pairs and triplets are gathered by explicit loops; energies, analytic forces and the virial W = sum d (x) f follow.
Units are LAMMPS `real`: kcal/mol, Angstrom, fs, g/mol.

test_sw_host.py checks this file's forces against central differences of its own energy.
"""
import itertools

import numpy as np

EV_TO_KCALMOL = 23.060549
FTM2V = 1.0 / 48.88821291 / 48.88821291      # (kcal/mol/A) / (g/mol) -> A/fs^2
MVV2E = 48.88821291 * 48.88821291            # g/mol (A/fs)^2 -> kcal/mol
NKTV2P = 68568.415                           # kcal/mol/A^3 -> atm
BOLTZ = 0.0019872067
KCALMOL_A3_TO_GPA = 4184.0 / 6.02214076e23 / 1e-30 / 1e9
FIELDS = ["epsilon", "sigma", "a", "lambda", "gamma", "costheta0", "A", "B", "p", "q", "tol"]
SI_MASS = 28.0855


def read_sw(path, elements, energy_unit=0):
    """{(i, j, k): {field: value}} over the distinct names of `elements` (order of first appearance), and the type map"""
    names = []
    for e in elements:
        if e not in names:
            names.append(e)
    words = []
    for line in open(path):
        words += line.split("#")[0].split()
    out = {}
    for t in range(0, len(words) - 13, 14):
        el, num = words[t:t + 3], [float(w) for w in words[t + 3:t + 14]]
        if all(e in names for e in el):
            d = dict(zip(FIELDS, num))
            if energy_unit == 0:
                d["epsilon"] *= EV_TO_KCALMOL
            out[tuple(names.index(e) for e in el)] = d
    return out, [names.index(e) for e in elements]


def h_matrix(box):
    """rows = cell vectors a1, a2, a3 of a LAMMPS box (xlo ylo zlo xhi yhi zhi xy xz yz)"""
    b = np.asarray(box, float)
    return np.array([[b[3] - b[0], 0.0, 0.0], [b[6], b[4] - b[1], 0.0], [b[7], b[8], b[5] - b[2]]])


def volume(box):
    return float(abs(np.linalg.det(h_matrix(box))))


def diamond(nx, ny, nz, a):
    """positions of the diamond lattice, nx x ny x nz cubic cells of 8 atoms, and the orthogonal box"""
    basis = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0], [1, 1, 1], [1, 3, 3], [3, 1, 3], [3, 3, 1]], float) * 0.25
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0])


def strained(x, box, eps):
    """homogeneous strain x -> (1 + eps) x of positions and box (eps: symmetric 3 x 3; the box stays upper-triangular only for strains
    that keep a1 along x and a2 in the xy plane: normal strains and the tilts xy, xz, yz as eps[0,1], eps[0,2], eps[1,2] one-sided)"""
    F = np.eye(3) + np.asarray(eps, float)
    H = h_matrix(box) @ F.T
    assert abs(H[0, 1]) < 1e-14 and abs(H[0, 2]) < 1e-14 and abs(H[1, 2]) < 1e-14
    lo = F @ np.asarray(box[:3], float)
    nb = np.array([lo[0], lo[1], lo[2], lo[0] + H[0, 0], lo[1] + H[1, 1], lo[2] + H[2, 2], H[1, 0], H[2, 0], H[2, 1]])
    return x @ F.T, nb


class SW:
    def __init__(self, params):
        self.p = params
        self.cutmax = max(d["a"] * d["sigma"] for d in params.values())

    def pair(self, ti, tj):
        return self.p[(ti, tj, tj)]

    def neighbours(self, x, box, types):
        """per atom the list of (j, image index, d) with |d| < a sigma of the pair, sorted by (j, image index)"""
        H = h_matrix(box)
        Hi = np.linalg.inv(H)
        n = len(x)
        d0 = x[None, :, :] - x[:, None, :]                    # d0[i, j] = x_j - x_i
        s = d0 @ Hi
        d0 = (s - np.rint(s)) @ H
        shifts = [np.array(sh, float) @ H for sh in itertools.product((-1, 0, 1), repeat=3)]
        types = np.asarray(types)
        cut = np.array([[self.pair(a, b)["a"] * self.pair(a, b)["sigma"] for b in range(types.max() + 1)] for a in range(types.max() + 1)])
        cutij = cut[types[:, None], types[None, :]]
        found = [[] for _ in range(n)]
        for m, sh in enumerate(shifts):
            d = d0 + sh
            r2 = np.einsum("ijk,ijk->ij", d, d)
            ok = r2 < cutij ** 2
            if m == 13:
                ok &= ~np.eye(n, dtype=bool)
            for i, j in zip(*np.nonzero(ok)):
                if np.sqrt(r2[i, j]) < cutij[i, j]:
                    found[i].append((int(j), m, d[i, j].copy()))
        for row in found:
            row.sort(key=lambda t: (t[0], t[1]))
        return found

    def compute(self, x, box, types, forces=True):
        """dict e2, e3, f [n,3], w (xx yy zz xy xz yz), w33, npairs, ntriplets, maxin"""
        x = np.asarray(x, float)
        n = len(x)
        nb = self.neighbours(x, box, types)
        # ---- pairs, each once: the lower index owns it; an atom's pair with its own image under the upper image index
        pi, pj, pd, pp = [], [], [], []
        for i in range(n):
            for j, m, d in nb[i]:
                if j > i or (j == i and m > 13):
                    pi.append(i); pj.append(j); pd.append(d); pp.append(self.pair(types[i], types[j]))
        e2 = 0.0
        f = np.zeros((n, 3))
        w = np.zeros((3, 3))
        if pi:
            d = np.array(pd)
            r = np.linalg.norm(d, axis=1)
            g = lambda k: np.array([q[k] for q in pp])
            eps, sig, a, A, B, p, q = g("epsilon"), g("sigma"), g("a"), g("A"), g("B"), g("p"), g("q")
            ex = np.exp(sig / (r - a * sig))
            poly = B * sig ** p * r ** (-p) - sig ** q * r ** (-q)
            e2 = float(np.sum(A * eps * poly * ex))
            dpoly = -p * B * sig ** p * r ** (-p - 1) + q * sig ** q * r ** (-q - 1)
            dedr = A * eps * ex * (dpoly - poly * sig / (r - a * sig) ** 2)
            fj = (-dedr / r)[:, None] * d                      # force on j; on i the opposite
            np.add.at(f, np.array(pj), fj)
            np.add.at(f, np.array(pi), -fj)
            w += d.T @ fj
        # ---- triplets (j < k in the sorted list) around every atom
        ti_, tj_, tk_, d1, d2, p1, p2, p3 = [], [], [], [], [], [], [], []
        for i in range(n):
            row = nb[i]
            for a_ in range(len(row)):
                for b_ in range(a_ + 1, len(row)):
                    j, _, da = row[a_]
                    k, _, db = row[b_]
                    ti_.append(i); tj_.append(j); tk_.append(k); d1.append(da); d2.append(db)
                    p1.append(self.pair(types[i], types[j])); p2.append(self.pair(types[i], types[k])); p3.append(self.p[(types[i], types[j], types[k])])
        e3 = 0.0
        if ti_:
            d1, d2 = np.array(d1), np.array(d2)
            r1, r2 = np.linalg.norm(d1, axis=1), np.linalg.norm(d2, axis=1)
            g1 = lambda k: np.array([q[k] for q in p1])
            g2 = lambda k: np.array([q[k] for q in p2])
            g3 = lambda k: np.array([q[k] for q in p3])
            c1, c2 = r1 - g1("a") * g1("sigma"), r2 - g2("a") * g2("sigma")
            E = np.exp(g1("gamma") * g1("sigma") / c1 + g2("gamma") * g2("sigma") / c2)
            cos = np.einsum("ij,ij->i", d1, d2) / (r1 * r2)
            dc = cos - g3("costheta0")
            le = g3("lambda") * g3("epsilon")
            h = le * dc ** 2 * E
            e3 = float(np.sum(h))
            dh_dr1 = h * (-g1("gamma") * g1("sigma") / c1 ** 2)
            dh_dr2 = h * (-g2("gamma") * g2("sigma") / c2 ** 2)
            dh_dc = 2.0 * le * dc * E
            u1, u2 = d1 / r1[:, None], d2 / r2[:, None]
            gj = dh_dr1[:, None] * u1 + (dh_dc / r1)[:, None] * (u2 - cos[:, None] * u1)
            gk = dh_dr2[:, None] * u2 + (dh_dc / r2)[:, None] * (u1 - cos[:, None] * u2)
            np.add.at(f, np.array(tj_), -gj)
            np.add.at(f, np.array(tk_), -gk)
            np.add.at(f, np.array(ti_), gj + gk)
            w += -(d1.T @ gj) - (d2.T @ gk)
        w6 = np.array([w[0, 0], w[1, 1], w[2, 2], w[0, 1], w[0, 2], w[1, 2]])
        return dict(e2=e2, e3=e3, e=e2 + e3, f=f, w=w6, w33=w, npairs=len(pi), ntriplets=len(ti_), maxin=max(len(r) for r in nb))

    def energy(self, x, box, types):
        return self.compute(x, box, types)["e"]

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


def minimage_diff(xa, xb, box):
    """xa - xb folded to the minimum image of the box"""
    H = h_matrix(box)
    s = (np.asarray(xa) - np.asarray(xb)) @ np.linalg.inv(H)
    return (s - np.rint(s)) @ H


# ---- the static cases the CPU and GPU tests share (silicon: tests/golden/Si.sw, lattice constant of the SW minimum) ----
def si_lattice_constant(sigma=2.0951):
    return 4.0 * 2.0 ** (1.0 / 6.0) * sigma / np.sqrt(3.0)


def case_a(seed=11):
    """2 x 2 x 2 cells (64 atoms), jitter 0.1 A"""
    x, box = diamond(2, 2, 2, si_lattice_constant())
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, np.zeros(len(x), int)


def case_b(seed=12):
    """3 x 2 x 4 cells (192 atoms), triclinic with all three tilts, atoms shifted so that several sit outside the box"""
    a = si_lattice_constant()
    x, box = diamond(3, 2, 4, a)
    F = np.array([[1.0, 0.06, -0.05], [0.0, 1.0, 0.04], [0.0, 0.0, 1.0]])      # x' = F x: xy = 0.06 ly, xz = -0.05 lz, yz = 0.04 lz
    rng = np.random.default_rng(seed)
    x = (x + rng.uniform(-0.1, 0.1, x.shape)) @ F.T
    box = box.copy()
    box[6], box[7], box[8] = 0.06 * 2 * a, -0.05 * 4 * a, 0.04 * 4 * a
    x = x + np.array([0.9, -1.3, 0.4])          # atoms near the faces leave the box
    H = h_matrix(box)
    x[::17] += H[0]                              # and a few by a whole cell vector
    x[5::23] -= H[2] + H[1]
    return x, box, np.zeros(len(x), int)


def case_c(seed=11):
    """case (a) compressed 10 %: every atom has 16 neighbours inside the cutoff, 120 triplets"""
    x, box, t = case_a(seed)
    x, box = strained(x, box, -0.1 * np.eye(3))
    return x, box, t


def case_e(seed=13):
    """2 x 2 x 2 cells, two elements alternating on the lattice (the two fcc sublattices), jitter 0.1 A"""
    x, box, _ = case_a(seed)
    t = np.tile(np.array([0, 0, 0, 0, 1, 1, 1, 1]), 8)
    return x, box, t


def case_f(seed=14):
    """4 x 4 x 4 cells (512 atoms), jitter 0.1 A: eight tiles of the force kernel"""
    x, box = diamond(4, 4, 4, si_lattice_constant())
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, np.zeros(len(x), int)


def case_g(seed=15):
    """5 x 5 x 6 cells (1 200 atoms), jitter 0.1 A: beyond the force kernel's LDS table"""
    x, box = diamond(5, 5, 6, si_lattice_constant())
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, np.zeros(len(x), int)


def case_h(seed=16):
    """1 x 2 x 2 cells (32 atoms) in a box narrower than two list radii: the image search"""
    x, box = diamond(1, 2, 2, si_lattice_constant())
    rng = np.random.default_rng(seed)
    return x + rng.uniform(-0.1, 0.1, x.shape), box, np.zeros(len(x), int)


def case_d(delta, cut=1.8 * 2.0951):
    """four atoms in a large box: a pair along x at distance cut + delta (delta < 0: inside; the first atom sits at x = 0, so delta = 0 is
    the cutoff to the bit), a third atom in range of the first alone, so that the pair is also an arm of a triplet; the fourth far away"""
    box = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])
    x = np.array([[0.0, 10.0, 10.0], [cut + delta, 10.0, 10.0], [0.0, 12.1, 11.1], [22.0, 22.0, 22.0]])
    return x, box, np.zeros(4, int)


TWO_ELEMENT_SW = """# a two-element file for the tests: Si as tests/golden/Si.sw, X softer and shorter, mixed entries symmetric in the two arms
Si Si Si 2.1683 2.0951 1.80 21.0 1.20 -0.333333333333 7.049556277 0.6022245584 4.0 0.0 0.0
X  X  X  1.3000 1.9500 1.75 26.0 1.10 -0.25           6.5         0.58         4.5 0.5 0.0
Si X  X  1.7000 2.0200 1.78 23.0 1.15 -0.30           6.8         0.59         4.2 0.2 0.0   # pair parameters of (Si, X)
X  Si Si 1.7000 2.0200 1.78 23.5 1.15 -0.31           6.8         0.59         4.2 0.2 0.0   # pair parameters of (X, Si)
Si Si X  1.9000 0.0    0.0  22.0 0.0  -0.32           0.0         0.0          0.0 0.0 0.0
Si X  Si 1.9000 0.0    0.0  22.0 0.0  -0.32           0.0         0.0          0.0 0.0 0.0
X  X  Si 1.5000 0.0    0.0  24.0 0.0  -0.28           0.0         0.0          0.0 0.0 0.0
X  Si X  1.5000 0.0    0.0  24.0 0.0  -0.28           0.0         0.0          0.0 0.0 0.0
"""


# ---- inputs for the edges of the kernels (tests/test_sw_edges_host.py, tests/test_gpu_sw_edges.py): generators only ----
SI_CUT = 1.8 * 2.0951            # a sigma of tests/golden/Si.sw
SI_RLIST = SI_CUT + 1.0          # + the default skin of sw_configure


def widths(box):
    """perpendicular widths of the box between its three pairs of faces"""
    H = h_matrix(box)
    v = volume(box)
    return np.array([v / np.linalg.norm(np.cross(H[1], H[2])), v / np.linalg.norm(np.cross(H[2], H[0])), v / np.linalg.norm(np.cross(H[0], H[1]))])


def check_box(box, cutmax=SI_CUT, rlist=SI_RLIST):
    """the conditions every input box of the edge tests meets: each perpendicular width is at least cutmax / 1.5 (SW.neighbours searches the
    fractional minimum image +- 1: |s| <= 1.5 box vectors, complete only above that width) and at least rlist / 2 (below it the engine
    refuses: it searches at most two images deep)"""
    w = widths(box)
    assert (w >= cutmax / 1.5).all() and (w >= rlist / 2.0).all(), w
    return w


def gas(n, box, dmin, seed):
    """n atoms inserted at random (uniform in the cell, one after the other, a candidate rejected when it comes closer than dmin to an atom
    placed before, to one of that atom's periodic images, or to a periodic image of itself); deterministic in the seed"""
    box = np.asarray(box, float)
    H = h_matrix(box)
    shifts = np.array(list(itertools.product(range(-3, 4), repeat=3)), float) @ H
    own = shifts[np.einsum("ij,ij->i", shifts, shifts) > 0.0]
    assert np.linalg.norm(own, axis=1).min() >= dmin, "an atom's own image is closer than dmin in this box"
    assert (3.0 * widths(box) > dmin).all()          # (three images deep covers dmin)
    rng = np.random.default_rng(seed)
    x = np.zeros((0, 3))
    for _ in range(100000):
        if len(x) == n:
            break
        c = box[:3] + rng.uniform(size=3) @ H
        d = (x[:, None, :] - c[None, None, :]) + shifts[None, :, :]
        if d.size == 0 or np.sqrt(np.einsum("ijk,ijk->ij", d, d)).min() >= dmin:
            x = np.vstack([x, c])
    assert len(x) == n, "the box does not hold that many atoms at this distance"
    return x


def truncated(n, seed=15):
    """the first n atoms of a jittered diamond block large enough to hold them, in the block's box (vacuum where the others were): up to
    1 200 atoms the 5 x 5 x 6 block of case (g), with its jitter"""
    nz = 6
    while 5 * 5 * nz * 8 < n:
        nz += 1
    x, box = diamond(5, 5, nz, si_lattice_constant())
    rng = np.random.default_rng(seed)
    x = x + rng.uniform(-0.1, 0.1, x.shape)
    return x[:n].copy(), box, np.zeros(n, int)


BIG_BOX = np.array([0.0, 0.0, 0.0, 30.0, 30.0, 30.0, 0.0, 0.0, 0.0])


def cluster(k, radius=3.5):
    """a centre atom and k atoms on a Fibonacci sphere of that radius around it, in a 30 A box"""
    m = np.arange(k) + 0.5
    z = 1.0 - 2.0 * m / k
    phi = m * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    shell = radius * np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    x = np.vstack([np.zeros((1, 3)), shell]) + 15.0
    return x, BIG_BOX.copy(), np.zeros(k + 1, int)


def lone(n):
    """one atom, or two atoms 2.4 A apart along the body diagonal, in a 30 A box"""
    u = 2.4 / np.sqrt(3.0)
    x = np.array([[14.0, 15.0, 16.0], [14.0 + u, 15.0 + u, 16.0 + u]])[:n]
    return x, BIG_BOX.copy(), np.zeros(n, int)


def narrow(name):
    """boxes narrower than one list radius: the image search two boxes deep, atoms that are their own neighbours
      N1  24-atom gas, 3.2 x 11 x 12 A orthogonal            N2  5-atom gas, triclinic, lower corner off the origin, widths 8.02 / 2.92 / 3.40 A
      N3  4-atom gas, 2.6 x 2.7 x 12 A with xy = 0.4 A       N4  one atom in 3.2 x 3.3 x 3.4 A: every neighbour is its own image
      N5  N1's positions, types alternating (TWO_ELEMENT_SW)
    The seeds of N2 and N3 are chosen so that a pair inside the cutoff sits two box vectors from its wrapped partner (an atom next to one
    face, its partner next to the opposite one: rare among seeds).  N1 and N4 cannot have one: at 3.2 A and a distance of 2.1 A to the
    nearest image, the image two boxes away is beyond the cutoff (3.2^2 + 2.1^2 > 3.77^2); their second images fill the skin only."""
    if name in ("N1", "N5"):
        box = np.array([0.0, 0.0, 0.0, 3.2, 11.0, 12.0, 0.0, 0.0, 0.0])
        x = gas(24, box, 2.1, 101)
        t = np.zeros(24, int) if name == "N1" else np.arange(24) % 2
    elif name == "N2":
        box = np.array([0.5, -1.0, 2.0, 9.5, 2.0, 5.4, 1.1, -0.9, 0.8])
        x = gas(5, box, 2.1, 136)
        t = np.zeros(5, int)
    elif name == "N3":
        box = np.array([0.0, 0.0, 0.0, 2.6, 2.7, 12.0, 0.4, 0.0, 0.0])
        x = gas(4, box, 2.1, 106)
        t = np.zeros(4, int)
    elif name == "N4":
        box = np.array([0.0, 0.0, 0.0, 3.2, 3.3, 3.4, 0.0, 0.0, 0.0])
        x = np.array([[1.1, 2.3, 0.7]])
        t = np.zeros(1, int)
    else:
        raise KeyError(name)
    check_box(box)
    return x, box, t


def tilted(ncell, seed=17):
    """jittered diamond, ncell^3 cells of edge L / ncell, tilted by xy = 0.45 L, xz = -0.45 L, yz = 0.45 L: |xy| close to lx / 2, the box a
    sheared run passes through before it flips.  ncell 3: widths 12.77 / 14.86 / 16.29 A, above two list radii (minimum image); ncell 2:
    8.51 / 9.91 / 10.86 A (one image deep)"""
    a = si_lattice_constant()
    x, box = diamond(ncell, ncell, ncell, a)
    L = ncell * a
    F = np.array([[1.0, 0.45, -0.45], [0.0, 1.0, 0.45], [0.0, 0.0, 1.0]])
    rng = np.random.default_rng(seed)
    x = (x + rng.uniform(-0.1, 0.1, x.shape)) @ F.T
    box[6], box[7], box[8] = 0.45 * L, -0.45 * L, 0.45 * L
    check_box(box)
    return x, box, np.zeros(len(x), int)


def case_a_compressed(frac=0.31):
    """case (a) compressed by 31 %: 33 neighbours inside the cutoff, one more than the force kernel lists (28 at 25 %)"""
    x, box, t = case_a()
    x, box = strained(x, box, -frac * np.eye(3))
    return x, box, t


def supercell(x, box, types, m=3):
    """the cell repeated m x m x m along its own vectors, the original atoms first"""
    H = h_matrix(box)
    box = np.asarray(box, float)
    sh = np.array(list(itertools.product(range(m), repeat=3)), float) @ H
    xs = (sh[:, None, :] + np.asarray(x)[None, :, :]).reshape(-1, 3)
    lo = box[:3]
    nb = np.array([lo[0], lo[1], lo[2], lo[0] + m * H[0, 0], lo[1] + m * H[1, 1], lo[2] + m * H[2, 2], m * H[1, 0], m * H[2, 0], m * H[2, 1]])
    return xs, nb, np.tile(np.asarray(types), m ** 3)
