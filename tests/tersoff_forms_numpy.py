"""The Tersoff forms tersoff/mod, tersoff/mod/c and tersoff/zbl in plain numpy, FP64: the reference of tests/test_tersoff_forms_*.py and
tests/test_gpu_tersoff_forms.py.  An independent restatement: it shares no code with scema_amd/csrc/tersoff/ts_core.h or the library's
readers; from tests/tersoff_numpy.py it takes the neighbour search, the stepper and the generators of inputs, nothing of the arithmetic.

mod (c0 = 0: tersoff/mod)
  E       = 1/2 sum_i sum_{j != i} fC(r_ij) [ A exp(-lambda1 r_ij) + c0 - b_ij B exp(-lambda2 r_ij) ]
  fC      = 1 (r < R - D),  1/2 - 9/16 sin(pi/2 (r - R)/D) - 1/16 sin(3 pi/2 (r - R)/D) (up to R + D),  0 (from R + D on)
  zeta_ij = sum_k fC(r_ik) g(cos theta_jik) exp[(alpha (r_ij - r_ik))^beta]         exponent clamped at +-69.0776 (1e30 above, 0 below)
  g(c)    = c1 + [c2 (h - c)^2 / (c3 + (h - c)^2)] [1 + c4 exp(-c5 (h - c)^2)]
  b_ij    = (1 + t^eta)^(-1/(2n)), t = beta_ters zeta;  t > ca1: t^(-eta/(2n));  t < ca4: b = 1, b' = 0;  ca1 = (2n 1e-16)^(-1/eta) = 1/ca4
zbl (everything else as in plain Tersoff, tests/tersoff_numpy.py)
  pair    = 1/2 [ (1 - F) V_ZBL + F fC fR ] + 1/2 fC b F fA,   F = 1 / (1 + exp(-A_F (r - r_C))), 0 where the exponent passes 69.0776
  V_ZBL   = K Z_i Z_j phi(r/a) / r,  a = 0.8854 * 0.529 / (Z_i^0.23 + Z_j^0.23),  K = 1/(4 pi 0.00552635) eV A
with the pair's quantities from entry i j j and everything inside zeta from entry i j k.  The energy is a plain loop (Form.energy); forces
and virial are analytic (Form.compute) and held against central differences of that energy by tests/test_tersoff_forms_host.py.
Units are LAMMPS `real`: kcal/mol, Angstrom.
"""
import math

import numpy as np

import tersoff_numpy as tsn

EV_TO_KCALMOL = 23.060549
EXPMAX = 69.0776
MOD_FIELDS = ["beta", "alpha", "h", "eta", "beta_ters", "lambda2", "B", "R", "D", "lambda1", "A", "n", "c1", "c2", "c3", "c4", "c5", "c0"]
ZBL_FIELDS = tsn.FIELDS + ["Z_i", "Z_j", "ZBLcut", "ZBLexpscale"]
ZBL_K_EV = 1.0 / (4.0 * math.pi * 0.00552635)
ZBL_EV_REAL = 0.043365121
MOD_CUT = 3.3           # R + D of the silicon fixture


def _words(path):
    w = []
    for line in open(path):
        w += line.split("#")[0].split()
    return w


def _isnum(s):
    try:
        float(s)
        return True
    except ValueError:
        return False


def read_mod(path, elements, energy_unit=0):
    """{(i, j, k): {field: value}}, type map, columns per entry (17: mod, 18: mod/c -- the count of numbers after the first three names)"""
    names = list(dict.fromkeys(elements))
    w = _words(path)
    ncol = 0
    while 3 + ncol < len(w) and _isnum(w[3 + ncol]):
        ncol += 1
    assert ncol in (17, 18), ncol
    unit = EV_TO_KCALMOL if energy_unit == 0 else 1.0
    out = {}
    for t in range(0, len(w) - ncol - 2, ncol + 3):
        el, num = w[t:t + 3], [float(v) for v in w[t + 3:t + 3 + ncol]] + ([0.0] if ncol == 17 else [])
        if all(e in names for e in el):
            d = dict(zip(MOD_FIELDS, num))
            for k in ("A", "B", "c0"):
                d[k] *= unit
            out[tuple(names.index(e) for e in el)] = d
    return out, [names.index(e) for e in elements], ncol


def read_zbl(path, elements, energy_unit=0):
    names = list(dict.fromkeys(elements))
    w = _words(path)
    out = {}
    for t in range(0, len(w) - 20, 21):
        el, num = w[t:t + 3], [float(v) for v in w[t + 3:t + 21]]
        if all(e in names for e in el):
            d = dict(zip(ZBL_FIELDS, num))
            if energy_unit == 0:
                d["A"] *= EV_TO_KCALMOL
                d["B"] *= EV_TO_KCALMOL
            d["K"] = ZBL_K_EV * EV_TO_KCALMOL if energy_unit == 0 else ZBL_K_EV / ZBL_EV_REAL
            out[tuple(names.index(e) for e in el)] = d
    return out, [names.index(e) for e in elements]


# ---- the functions of the two forms, each (value, derivative) ----
def fc_mod(p, r):
    R, D = p["R"], p["D"]
    if r < R - D:
        return 1.0, 0.0
    if r < R + D:
        a = 0.5 * math.pi * (r - R) / D
        return (0.5 - 9.0 / 16.0 * math.sin(a) - 1.0 / 16.0 * math.sin(3.0 * a),
                -0.5 * math.pi / D * (9.0 / 16.0 * math.cos(a) + 3.0 / 16.0 * math.cos(3.0 * a)))
    return 0.0, 0.0


def g_mod(q, cos):
    x = q["h"] - cos
    u = x * x
    g1, dg1 = q["c2"] * u / (q["c3"] + u), q["c2"] * q["c3"] / (q["c3"] + u) ** 2          # d/du
    e = q["c4"] * math.exp(-q["c5"] * u)
    g2, dg2 = 1.0 + e, -q["c5"] * e
    return q["c1"] + g1 * g2, (dg1 * g2 + g1 * dg2) * (-2.0 * x)                          # du/dcos = -2 x


def expo_mod(q, dr):
    return tsn.expo({"lambda3": q["alpha"], "m": q["beta"]}, dr)


def mod_switch(p):
    ca1 = (2.0 * p["n"] * 1e-16) ** (-1.0 / p["eta"])
    return ca1, 1.0 / ca1


def bond_order_mod(p, zeta):
    t = p["beta_ters"] * zeta
    ca1, ca4 = mod_switch(p)
    q = p["eta"] / (2.0 * p["n"])
    if t > ca1:
        return t ** -q, -q * t ** -q / zeta
    if t < ca4:
        return 1.0, 0.0
    te = t ** p["eta"]
    return (1.0 + te) ** (-0.5 / p["n"]), -q * (1.0 + te) ** (-0.5 / p["n"] - 1.0) * te / zeta


def bond_order_mod_exact(p, zeta):
    te = (p["beta_ters"] * zeta) ** p["eta"]
    return (1.0 + te) ** (-0.5 / p["n"])


def fermi(p, r):
    arg = -p["ZBLexpscale"] * (r - p["ZBLcut"])
    if arg > EXPMAX:
        return 0.0, 0.0
    if arg < -EXPMAX:
        return 1.0, 0.0
    e = math.exp(arg)
    return 1.0 / (1.0 + e), p["ZBLexpscale"] * e / (1.0 + e) ** 2


PHI = ((0.1818, 3.2), (0.5099, 0.9423), (0.2802, 0.4029), (0.02817, 0.2016))


def v_zbl(p, r):
    a = 0.8854 * 0.529 / (p["Z_i"] ** 0.23 + p["Z_j"] ** 0.23)
    kzz = p["K"] * p["Z_i"] * p["Z_j"]
    phi = sum(c * math.exp(-s * r / a) for c, s in PHI)
    dphi = sum(-c * s / a * math.exp(-s * r / a) for c, s in PHI)
    return kzz * phi / r, kzz * (dphi / r - phi / (r * r))


class Form(tsn.Tersoff):
    """what the two forms share: the loops.  A subclass gives fc (pair and third atom), g, expo, bond_order and the pair term"""

    def pair(self, p, r, b):
        """(energy without b, energy with b, d/dr of each at fixed b, the fA that enters the zeta prefactor 1/2 fC fA b')"""
        raise NotImplementedError

    def zeta(self, nb_i, a, ti, types):
        j, _, dj, rj = nb_i[a]
        z = 0.0
        for b_, (k, _, dk, rk) in enumerate(nb_i):
            q = self.p[(ti, types[j], types[k])]
            if b_ == a or not rk < q["R"] + q["D"]:
                continue
            z += self.fc(q, rk)[0] * self.g(q, float(dj @ dk) / (rj * rk))[0] * self.expo(q, rj - rk)[0]
        return z

    def energy(self, x, box, types):
        x = np.asarray(x, float)
        nb = self.neighbours(x, box, types)
        e = 0.0
        for i in range(len(x)):
            for a, (j, _, dj, rj) in enumerate(nb[i]):
                pij = self.p[(types[i], types[j], types[j])]
                if not rj < pij["R"] + pij["D"]:
                    continue
                b = self.bond_order(pij, self.zeta(nb[i], a, types[i], types))[0]
                er, ea, _, _, _ = self.pair(pij, rj, b)
                e += er + ea
        return e

    def compute(self, x, box, types):
        """as tersoff_numpy.Tersoff.compute, plus fcsum = sum over ordered pairs of fC(r_ij) and rmargin = the least |r - (R + D)| over all
        neighbour entries and the cutoffs they are held against"""
        x = np.asarray(x, float)
        n = len(x)
        nb = self.neighbours(x, box, types)
        f, w = np.zeros((n, 3)), np.zeros((3, 3))
        e_rep = e_att = fcsum = 0.0
        npairs = nzeta = maxin = 0
        rmargin = np.inf
        kinds = sorted(set(int(t) for t in types))
        for i in range(n):
            ti = types[i]
            used = 0
            for (k, _, dk, rk) in nb[i]:
                cuts = [self.p[(ti, types[k], types[k])]] + [self.p[(ti, tj, types[k])] for tj in kinds]
                used += 1 if rk < max(q["R"] + q["D"] for q in cuts) else 0
                rmargin = min([rmargin] + [abs(rk - q["R"] - q["D"]) for q in cuts])
            maxin = max(maxin, used)
            for a, (j, _, dj, rj) in enumerate(nb[i]):
                pij = self.p[(ti, types[j], types[j])]
                if not rj < pij["R"] + pij["D"]:
                    continue
                npairs += 1
                uj = dj / rj
                terms, zeta = [], 0.0
                for b_, (k, _, dk, rk) in enumerate(nb[i]):
                    q = self.p[(ti, types[j], types[k])]
                    if b_ == a or not rk < q["R"] + q["D"]:
                        continue
                    nzeta += 1
                    cos = float(dj @ dk) / (rj * rk)
                    fk, dfk = self.fc(q, rk)
                    gg, dg = self.g(q, cos)
                    ex, dex = self.expo(q, rj - rk)
                    zeta += fk * gg * ex
                    uk = dk / rk
                    gj = fk * gg * dex * uj + fk * dg * ex * (uk - cos * uj) / rj
                    gk = (dfk * gg * ex - fk * gg * dex) * uk + fk * dg * ex * (uj - cos * uk) / rk
                    terms.append((k, dk, gj, gk))
                b, db = self.bond_order(pij, zeta)
                er, ea, der, dea, fa = self.pair(pij, rj, b)
                fcj = self.fc(pij, rj)[0]
                fcsum += fcj
                e_rep += er
                e_att += ea
                fj = -(der + dea) * uj
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
        return dict(e_rep=e_rep, e_att=e_att, e=e_rep + e_att, f=f, w=w6, w33=w, npairs=npairs, nzeta=nzeta, maxin=maxin, fcsum=fcsum,
                    rmargin=rmargin)


class TersoffMod(Form):
    fc = staticmethod(fc_mod)
    g = staticmethod(g_mod)
    expo = staticmethod(expo_mod)
    bond_order = staticmethod(bond_order_mod)

    def pair(self, p, r, b):
        fcv, dfc = fc_mod(p, r)
        fr, fa = p["A"] * math.exp(-p["lambda1"] * r), -p["B"] * math.exp(-p["lambda2"] * r)
        return (0.5 * fcv * (fr + p["c0"]), 0.5 * fcv * b * fa, 0.5 * (dfc * (fr + p["c0"]) - fcv * p["lambda1"] * fr),
                0.5 * b * (dfc - fcv * p["lambda2"]) * fa, fa)


class TersoffZbl(Form):
    fc = staticmethod(tsn.fc)
    g = staticmethod(tsn.g_stable)
    expo = staticmethod(tsn.expo)
    bond_order = staticmethod(tsn.bond_order)

    def pair(self, p, r, b):
        fcv, dfc = tsn.fc(p, r)
        F, dF = fermi(p, r)
        v, dv = v_zbl(p, r)
        fr, fa = p["A"] * math.exp(-p["lambda1"] * r), -p["B"] * math.exp(-p["lambda2"] * r)
        er = 0.5 * ((1.0 - F) * v + F * fcv * fr)
        der = 0.5 * (-dF * v + (1.0 - F) * dv + dF * fcv * fr + F * dfc * fr - F * fcv * p["lambda1"] * fr)
        ea = 0.5 * fcv * b * F * fa
        dea = 0.5 * b * (dfc * F + fcv * dF - fcv * F * p["lambda2"]) * fa
        return er, ea, der, dea, F * fa


def zbl_pair_energy(ref, x, box, types):
    """1/2 sum over the ordered pairs inside R + D of V_ZBL alone"""
    e = 0.0
    for i, row in enumerate(ref.neighbours(np.asarray(x, float), box, types)):
        for j, _, _, r in row:
            p = ref.p[(types[i], types[j], types[j])]
            if r < p["R"] + p["D"]:
                e += 0.5 * v_zbl(p, r)[0]
    return e


def cut_margin(ref, x, box, types):
    """the least |r - (R + D)| over every pair of atoms (images included) and every cutoff the pair can be held against: the pair's own and
    those of the entries i j k under which it serves as a third atom.  Pairs just OUTSIDE the largest cutoff count too"""
    kinds = sorted(set(int(t) for t in types))
    keep, out = ref.cutmax, np.inf
    ref.cutmax = keep + 0.05
    try:
        for i, row in enumerate(ref.neighbours(np.asarray(x, float), box, types)):
            for k, _, _, rk in row:
                cuts = [ref.p[(types[i], types[k], types[k])]] + [ref.p[(types[i], tj, types[k])] for tj in kinds]
                out = min([out] + [abs(rk - q["R"] - q["D"]) for q in cuts])
    finally:
        ref.cutmax = keep
    return out


# ---- the synthetic file of the tests (the three fixtures under tests/golden/ are written by tests/golden/make_tersoff_forms_fixture.py) ----
# two elements, eta != 1, beta = 3 (X) and 1 (Y), R, D that differ per triplet, c4 = 0 in one entry (Y X Y)
SYNTH_MOD = """# synthetic tersoff/mod/c file of the tests
# El El El  beta alpha h    eta beta_ters lambda2 B    R    D    lambda1 A      n    c1   c2   c3   c4   c5   c0
X X X       3    1.3   -0.40 0.8 1.0      1.9   310.0  2.9  0.2  2.9   1500.0   0.9  0.25 3.1  2.0  0.6  5.0  0.04
Y Y Y       1    1.1   -0.30 1.3 1.0      2.1   280.0  2.7  0.2  3.1   1300.0   1.1  0.15 2.2  1.5  0.9  8.0  -0.03
X Y Y       3    1.3   -0.40 0.9 1.0      2.0   295.0  2.8  0.2  3.0   1400.0   1.0  0.25 3.1  2.0  0.6  5.0  0.02
Y X X       1    1.1   -0.30 1.2 1.0      2.0   295.0  2.8  0.2  3.0   1400.0   0.95 0.15 2.2  1.5  0.9  8.0  0.01
X X Y       3    1.3   -0.40 0 1.0 0 0          2.6  0.3  0 0      0    0.25 3.1  2.0  0.6  5.0  0
X Y X       3    1.3   -0.40 0 1.0 0 0          2.7  0.25 0 0      0    0.20 2.8  2.0  0.6  5.0  0
Y Y X       1    1.1   -0.30 0 1.0 0 0          2.9  0.15 0 0      0    0.15 2.2  1.5  0.9  8.0  0
Y X Y       1    1.1   -0.30 0 1.0 0 0          2.5  0.3  0 0      0    0.15 2.2  1.5  0.0  8.0  0
"""
# the same with alpha = 40 for element X: (40 dr)^3 passes the clamp at |dr| = 0.103 A, zeta reaches 1e30 > ca1
SYNTH_MOD_CLAMP = SYNTH_MOD.replace("3    1.3   ", "3    40.0  ")
SYNTH_MOD_CUT = 3.1


# ---- inputs of the forms' tests (the generators of tests/tersoff_numpy.py under the mod cutoff of 3.3 A where their licence holds) ----
def case_h_trimer(h=-0.365, r1=2.3, r2=2.4):
    """a trimer whose angle at the first atom has cos theta = h as closely as the coordinates allow; arms r1 and r2"""
    s = math.sqrt(1.0 - h * h)
    return np.array([[8.0, 8.0, 8.0], [8.0 + r1, 8.0, 8.0], [8.0 + r2 * h, 8.0 + r2 * s, 8.0]]), tsn.BIG_BOX.copy(), tsn.zeros(3)


def case_arm_trimer(r1, r2, deg=100.0, types=None):
    """a bent trimer with arms r1, r2 at the first atom"""
    t = math.radians(deg)
    if types is not None:
        return np.array([[15.0, 15.0, 15.0], [15.0 + r1, 15.0, 15.0], [15.0 + r2 * math.cos(t), 15.0 + r2 * math.sin(t), 15.0]]), tsn.BIG_BOX.copy(), np.array(types)
    return np.array([[15.0, 15.0, 15.0], [15.0 + r1, 15.0, 15.0], [15.0 + r2 * math.cos(t), 15.0 + r2 * math.sin(t), 15.0]]), tsn.BIG_BOX.copy(), tsn.zeros(3)
