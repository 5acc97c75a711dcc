"""pair_style hybrid/overlay coul/long <cut_coul> eam/alloy with an Ewald sum in plain numpy, FP64: the reference the EAM/coul tests compare
with (tests/test_eam_coul_*.py, tests/test_gpu_eam_coul.py).

The restatement is a SUM of two restatements that exist: tests/eam_numpy.py (EAM) on the setfl file and its cutoff, and
tests/born_long_numpy.py (BornLong) with every Born constant zero, so that only its four Coulomb terms remain, on cut_coul.  Each keeps its
own neighbour search on its own cutoff, so either cutoff may be the larger one.  It shares no code with the library: its own parser of the
script lines below, the setfl parser of eam_numpy, the g_ewald / kmax / sphere rule of born_long_numpy.  It does not read the kernels' code.

  E = sum_i F(rho_i) + 1/2 sum phi(r)         (0 < r^2 < cutoff^2 of the setfl file)
    + E_real + E_recip + E_self               (born_long_numpy: K q_i q_j erfc(g r)/r inside cut_coul, the k sum, self and background)

Units are LAMMPS `real`.  The type of an atom indexes the element list of the script's eam/alloy line; its charge is the replica's.
"""
import itertools
import math
import os

import numpy as np

import born_long_numpy as bl
import eam_numpy as en
from sw_numpy import FTM2V, MVV2E, NKTV2P, h_matrix, minimage_diff, strained, volume  # noqa: F401

O_MASS, U_MASS = 15.9994, 238.02891
Q_O, Q_U = -1.1104, 2.2208
A_UO2 = 5.47


def read_eam_coul(path, energy_unit=None):
    """dict cut_coul, accuracy, solver, unit, K, setfl (resolved against the script's folder), elements of the script lines in `path`;
    energy_unit None: 1 iff the text says `units real`, else 0"""
    style, coul, eam, unit, ks = None, 0, None, None, None
    for raw in open(path):
        w = raw.split("#")[0].split()
        if not w:
            continue
        if w[0] == "pair_style":
            assert style is None and w[1] == "hybrid/overlay", raw
            rest = w[2:]
            k = rest.index("coul/long")
            style = float(rest[k + 1])
            assert sorted(rest[:k] + rest[k + 2:]) == ["eam/alloy"], raw
        elif w[0] == "pair_coeff":
            assert w[1:3] == ["*", "*"] and w[3] in ("coul/long", "eam/alloy"), raw
            if w[3] == "coul/long":
                assert len(w) == 4
                coul += 1
            else:
                assert eam is None and len(w) >= 6 and "NULL" not in w[5:]
                eam = (w[4], w[5:])
        elif w[0] == "units":
            unit = {"metal": 0, "real": 1}[w[1]]
        elif w[0] == "kspace_style":
            assert ks is None and w[1] in ("ewald", "pppm"), raw
            ks = (w[1], float(w[2]))
        assert w[0] != "kspace_modify", raw
    assert style is not None and style > 0.0 and coul == 1 and eam is not None and ks is not None and 0.0 < ks[1] < 1.0
    if energy_unit is None:
        energy_unit = unit or 0
    name = eam[0][len("${locs}/"):] if eam[0].startswith("${locs}/") else eam[0]
    setfl = name if os.path.isabs(name) else os.path.join(os.path.dirname(os.path.abspath(path)), name)
    return dict(cut_coul=style, accuracy=ks[1], solver=ks[0], unit=energy_unit, K=bl.K_EV * bl.EV_TO_KCALMOL if energy_unit == 0 else bl.K_KCALMOL,
                setfl=setfl, elements=list(eam[1]))


class EamCoul:
    def __init__(self, p, accuracy=None):
        self.p = p
        tab, tmap = en.read_setfl(p["setfl"], p["elements"], p["unit"])
        self.eam, self.tmap = en.EAM(tab), np.array(tmap, int)
        z, one = np.zeros((1, 1)), np.ones((1, 1))
        # (every Born constant zero and its cutoff zero: BornLong.born returns exactly 0 for every pair, cutmax is cut_coul)
        self.bl = bl.BornLong(dict(A=z, rho=one, sigma=z, C=z, D=z, cut_lj=z, n=1, cut_coul=p["cut_coul"], unit=p["unit"], K=p["K"],
                                   accuracy=p["accuracy"], solver=p["solver"], style="born"), accuracy)
        self.K, self.rc, self.cutoff = p["K"], p["cut_coul"], tab["cutoff"]
        self.cutmax = max(self.rc, self.cutoff)

    def setup(self, box, q):
        return self.bl.setup(box, q)

    def compute(self, x, box, types, q, g=None, triples=None, kbox=None):
        """dict e_eam, e_coul and the parts e_pair, e_embed, e_real, e_recip, e_self, e_bg; f [n,3]; w (xx yy zz xy xz yz), w33 and the parts
        w_eam, w_real, w_recip; npairs (ordered pairs inside the setfl cutoff), ncoul (inside cut_coul)"""
        types, q = np.asarray(types, int), np.asarray(q, float)
        a = self.eam.compute(np.asarray(x, float), box, self.tmap[types])
        b = self.bl.compute(x, box, np.zeros(len(types), int), q, g, triples, kbox)
        assert b["e_born"] == 0.0 and not b["w_born"].any()
        return dict(e_eam=a["e"], e_coul=b["e_coul"], e_pair=a["e_pair"], e_embed=a["e_embed"], e_real=b["e_real"], e_recip=b["e_recip"], e_self=b["e_self"],
                    e_bg=b["e_bg"], e=a["e"] + b["e_coul"], f=a["f"] + b["f"], f_eam=a["f"], f_coul=b["f"], w=a["w"] + b["w"], w33=a["w33"] + b["w33"],
                    w_eam=a["w"], w_coul=b["w_coul"], w_real=b["w_real"], w_recip=b["w_recip"], npairs=a["npairs"], ncoul=b["ncoul"], g=b["g"], nk=b["nk"])

    def nve(self, x, v, box, types, q, masses, dt, nsteps):
        """velocity Verlet, NVE; g and the triples are those of the start box"""
        x, v = np.array(x, float), np.array(v, float)
        m = np.asarray(masses, float)[np.asarray(types)][:, None]
        g, tr = self.setup(box, q)
        f = self.compute(x, box, types, q, g, tr)["f"]
        for _ in range(nsteps):
            v += 0.5 * dt * FTM2V * f / m
            x += dt * v
            f = self.compute(x, box, types, q, g, tr)["f"]
            v += 0.5 * dt * FTM2V * f / m
        return x, v

    def pressure_atm(self, x, v, box, types, q, masses, g=None, triples=None):
        """(sum m v v + W) / V in atm, xx yy zz xy xz yz"""
        m = np.asarray(masses, float)[np.asarray(types)]
        kin = MVV2E * np.einsum("i,ij,ik->jk", m, v, v)
        t = (kin + self.compute(x, box, types, q, g, triples)["w33"]) / volume(box) * NKTV2P
        return np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])


# ---- the analytic model behind tests/golden/UO2.eam.alloy (tests/golden/make_eam_coul_fixture.py) ----
# In the SHAPE of the many-body oxide models of Cooper, Rushton and Grimes (J. Phys.: Condens. Matter 26, 105401 (2014)):
#   phi_ab(r) = A exp(-r / rho) - C / r^6 + D [exp(-2 gamma (r - r0)) - 2 exp(-gamma (r - r0))]        Buckingham + Morse
#   rho_b(r)  = (n_b / r^8) 1/2 (1 + erf(20 (r - 1.5)))                                                the erf switch at short range
#   F_a(rho)  = -G_a sqrt(rho)
# Every function is evaluated at max(r, R_FLOOR) (no pole in a table) and multiplied by a switch that takes value and slope to 0 at the
# cutoff.  SYNTHETIC: the constants below are WRITTEN FROM MEMORY in the range of such models and pin nothing physical.
CRG = dict(pairs={("U", "U"): dict(A=18600.0, rho=0.2747, C=0.0, D=0.0, gamma=0.0, r0=0.0),
                  ("O", "U"): dict(A=448.779, rho=0.387758, C=0.0, D=0.66080, gamma=2.05815, r0=2.38051),
                  ("O", "O"): dict(A=830.283, rho=0.352856, C=3.884372, D=0.0, gamma=0.0, r0=0.0)},
           G=dict(U=1.806, O=0.690), n=dict(U=3450.995, O=106.856), Z=dict(U=92, O=8), mass=dict(U=U_MASS, O=O_MASS))
CUTOFF, SWITCH_ON, R_FLOOR = 7.0, 6.0, 0.6
NR, NRHO, DR, RHOMAX = 500, 500, 0.0142, 60.0
_erf = np.vectorize(math.erf, otypes=[float])


def switch(r):
    t = np.clip((np.asarray(r, float) - SWITCH_ON) / (CUTOFF - SWITCH_ON), 0.0, 1.0)
    return 1.0 - 3.0 * t * t + 2.0 * t ** 3


def crg_phi(a, b, r):
    p = CRG["pairs"][tuple(sorted((a, b)))]
    rr = np.maximum(np.asarray(r, float), R_FLOOR)
    morse = p["D"] * (np.exp(-2.0 * p["gamma"] * (rr - p["r0"])) - 2.0 * np.exp(-p["gamma"] * (rr - p["r0"])))
    return (p["A"] * np.exp(-rr / p["rho"]) - p["C"] / rr ** 6 + morse) * switch(r)


def crg_rho(b, r):
    rr = np.maximum(np.asarray(r, float), R_FLOOR)
    return CRG["n"][b] / rr ** 8 * 0.5 * (1.0 + _erf(20.0 * (rr - 1.5))) * switch(r)


def crg_tables(names):
    """the arguments of eam_numpy.write_setfl after `lattice`"""
    r, rho = np.arange(NR) * DR, np.arange(NRHO) * (RHOMAX / (NRHO - 1))
    F = [-CRG["G"][a] * np.sqrt(rho) for a in names]
    dens = [crg_rho(a, r) for a in names]
    z = {(i, j): r * crg_phi(names[i], names[j], r) for i in range(len(names)) for j in range(i + 1)}
    return NRHO, RHOMAX / (NRHO - 1), NR, DR, CUTOFF, F, dens, z


# ---- the static cases the CPU and GPU tests share: type 0 is O, type 1 is U (`pair_coeff * * eam/alloy UO2.eam.alloy O U`) ----
def fluorite(nx, ny, nz, a=A_UO2):
    """positions, orthogonal box, types and charges of the fluorite structure: U on the fcc sites, O on the eight tetrahedral sites"""
    fcc = np.array([[0, 0, 0], [0, 2, 2], [2, 0, 2], [2, 2, 0]], float) * 0.25
    tet = np.array(list(itertools.product((0.25, 0.75), repeat=3)))
    basis = np.vstack([fcc, tet])
    cells = np.array(list(itertools.product(range(nx), range(ny), range(nz))), float)
    x = (cells[:, None, :] + basis[None, :, :]).reshape(-1, 3) * a
    t = np.tile(np.array([1] * 4 + [0] * 8), len(cells))
    return x, np.array([0.0, 0.0, 0.0, nx * a, ny * a, nz * a, 0.0, 0.0, 0.0]), t, np.where(t == 1, Q_U, Q_O)


def case_rattled(cells, seed, sigma=0.1, tilt_xy=0.0):
    """fluorite of cells = (nx, ny, nz) or n for a cube, every coordinate moved by a normal deviate of that sigma; tilt_xy: the box and
    the lattice sheared by that fraction of lx in xy"""
    cells = (cells,) * 3 if isinstance(cells, int) else cells
    x, box, t, q = fluorite(*cells)
    x = x + np.random.default_rng(seed).normal(0.0, sigma, x.shape)
    if tilt_xy:
        ly = box[4] - box[1]
        box[6] = tilt_xy * (box[3] - box[0])
        x = x + np.outer(x[:, 1] / ly, [box[6], 0.0, 0.0])
    return x, box, t, q


def case_with_interstitial(case, n_extra=1, seed=2):
    """the case with n_extra more oxygen ions, each at the most open spot among 4 000 random points: a net charge, the background term"""
    x, box, t, q = case
    rng = np.random.default_rng(seed)
    H = h_matrix(box)
    for _ in range(n_extra):
        c = rng.uniform(0.0, 1.0, (4000, 3)) @ H + box[:3]
        dmin = np.array([np.linalg.norm(minimage_diff(np.tile(p, (len(x), 1)), x, box), axis=1).min() for p in c])
        x, t, q = np.vstack([x, c[np.argmax(dmin)]]), np.append(t, 0), np.append(q, Q_O)
    return x, box, t, q


def case_single(L=20.0):
    return np.array([[3.0, 4.0, 5.0]]), np.array([0.0, 0.0, 0.0, L, L, L, 0.0, 0.0, 0.0]), np.array([1]), np.array([Q_U])


def case_trimer(cut_a, cut_b, L=30.0, eps=0.05):
    """a neutral O-U-O trimer: one arm eps inside cut_a, the other eps outside cut_b (along x and along y: the two O are further apart
    than either cutoff)"""
    c = np.array([12.0, 12.0, 12.0])
    x = np.array([c, c + [cut_a - eps, 0.0, 0.0], c + [0.0, cut_b + eps, 0.0]])
    return x, np.array([0.0, 0.0, 0.0, L, L, L, 0.0, 0.0, 0.0]), np.array([1, 0, 0]), np.array([Q_U, Q_O, Q_O])
