"""The mesh reciprocal solver of the Born/long stage (PPPM: order-5 assignment, ik differentiation, the optimal influence function of
the step's box) in plain numpy, FP64: the reference the mesh tests compare with (tests/test_born_long_mesh_host.py,
tests/test_gpu_born_long_mesh.py).

An independent restatement -- it shares no code with scema_amd/csrc/ionic/blm_core.h or the engine's set-up: its own copy of the grid /
adjust_gewald rule of `kspace_style pppm <accuracy>` (LAMMPS' set_grid_global and adjust_gewald, as remembered, unpinned), the order-5
weights from the closed form of the cardinal B-spline (truncated powers, not the blending polynomials of the kernels), np.fft for the
transforms, the influence function with the alias range |m| <= 2 per dimension, and the energy, virial, self and background terms.  The
real-space part, the Born term and the cases are those of tests/born_long_numpy.py, which this class extends.

  rho(p)  = (NG/V) sum_i q_i W(p - n s_i)            s_i the fractional coordinates of the step's box, wrapped; p on the mesh n
  a(k)    = fft(rho)/NG,  k = 2 pi H^-1 m            m the signed mode index (the middle of an even dimension counts as -n/2)
  E_recip = (K V/2) sum_{k != 0} G(k) |a(k)|^2
  G(k)    = (4 pi/k^2) sum_b (k.k_b/k_b^2) exp(-k_b^2/4g^2) U^2(k_b) / (sum_b U^2(k_b))^2,   k_b = k + 2 pi H^-1 (n b), |b_d| <= 2
  E(p)    = NG ifft(-i k G a),   F_i = K q_i sum_p W(p - n s_i) E(p)
  W_recip = sum_k e_k [1 - 2 (1/k^2 + 1/4g^2) k k^T]

The mesh and g belong to a run (its start box) and stay; the mesh lives in the fractional coordinates of the box of each step, so `nve`
takes the box of each step, the flipped one after a flip.
"""
import math

import numpy as np

import born_long_numpy as bl
from born_long_numpy import *  # noqa: F401,F403  (the cases and constants the tests share)
from sw_numpy import FTM2V, MVV2E, NKTV2P, h_matrix, volume

ORDER = 5
ACONS5 = [1.0 / 23232.0, 7601.0 / 13628160.0, 143.0 / 69120.0, 517231.0 / 106536960.0, 106640677.0 / 11737571328.0]
MAXGRID, MAXDIM = 4194304, 4096


# ---- the set-up of `kspace_style pppm <accuracy>` ----
def _ik_error(h, prd, g, q2, natoms):
    s = sum(a * (h * g) ** (2.0 * m) for m, a in enumerate(ACONS5))
    return q2 * (h * g) ** 5.0 * math.sqrt(g * prd * math.sqrt(2.0 * math.pi) * s / natoms) / (prd * prd)


def _factorable(n):
    for f in (2, 3, 5):
        while n % f == 0:
            n //= f
    return n == 1


def mesh_rule(box, natoms, qsqsum, rc, accuracy, cap=MAXDIM):
    """(g_ewald after adjust_gewald, mesh (nx, ny, nz)) for that box: the initial estimate of g from the relative accuracy (K cancels), the
    grid search per dimension (the increment follows the evaluation, so it stops one past the first admissible grid), the triclinic
    rescaling, products of 2, 3 and 5, then Newton steps on real-space error minus k-space error"""
    b = np.asarray(box, float)
    prd = b[3:6] - b[:3]
    xy, xz, yz = b[6:9]
    acc, q2 = accuracy * bl.K_KCALMOL, qsqsum * bl.K_KCALMOL
    tt = acc * math.sqrt(natoms * rc * prd[0] * prd[1] * prd[2]) / (2.0 * q2)
    g = (1.35 - 0.15 * math.log(acc)) / rc if tt >= 1.0 else math.sqrt(-math.log(tt)) / rc
    n = []
    for d in range(3):
        h = 1.0 / g
        nd = int(prd[d] / h) + 1
        err = _ik_error(h, prd[d], g, q2, natoms)
        while err > acc and nd < cap:
            err = _ik_error(h, prd[d], g, q2, natoms)
            nd += 1
            h = prd[d] / nd
        n.append(nd)
    t = [n[0] / prd[0], n[1] / prd[1], n[2] / prd[2]]
    u = [prd[0] * t[0], xy * t[0] + prd[1] * t[1], xz * t[0] + yz * t[1] + prd[2] * t[2]]
    n = [max(int(v + 1e-9) + 1, 2) for v in u]
    for d in range(3):
        while not _factorable(n[d]):
            n[d] += 1
    hinv = [1.0 / prd[0], 1.0 / prd[1], 1.0 / prd[2], -yz / (prd[1] * prd[2]), (yz * xy - prd[1] * xz) / (prd[0] * prd[1] * prd[2]), -xy / (prd[0] * prd[1])]
    hs = [1.0 / (hinv[0] * n[0]), 1.0 / (hinv[5] * n[0] + hinv[1] * n[1]), 1.0 / (hinv[4] * n[0] + hinv[3] * n[1] + hinv[2] * n[2])]

    def f(gg):
        df_r = 2.0 * q2 * math.exp(-gg * gg * rc * rc) / math.sqrt(natoms * rc * prd[0] * prd[1] * prd[2])
        e = [_ik_error(hs[d], prd[d], gg, q2, natoms) for d in range(3)]
        return df_r - math.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2) / math.sqrt(3.0)

    for _ in range(10000):
        dx = 0.000001
        f1, f2 = f(g), f(g + dx)
        g -= f1 / ((f2 - f1) / dx)
        if abs(f(g)) < 0.00001:
            break
    return g, tuple(n)


def refused(grid):
    """what the mesh solver refuses: "cap" (a dimension reached the search cap), "points" (more than MAXGRID), or None"""
    if max(grid) >= MAXDIM:
        return "cap"
    return "points" if grid[0] * grid[1] * grid[2] > MAXGRID else None


# ---- assignment ----
def bspline5(t):
    """the centred cardinal B-spline of order 5 (degree 4, support |t| < 5/2) from its truncated-power form"""
    t = np.asarray(t, float)
    out = np.zeros_like(t)
    for k in range(ORDER + 1):
        out += (-1.0) ** k * math.comb(ORDER, k) * np.maximum(t + 0.5 * ORDER - k, 0.0) ** (ORDER - 1)
    return out / math.factorial(ORDER - 1)


def stencil(s, n):
    """for fractional coordinates s [N] in [0, 1) on n points: indices [N, 5] (wrapped) and weights [N, 5] of the nearest point +- 2"""
    u = s * n
    i0 = np.floor(u + 0.5).astype(int)
    j = i0[:, None] + np.arange(-2, 3)[None, :]
    return j % n, bspline5(u[:, None] - j)


def fractional(x, box):
    s = (np.asarray(x, float) - np.asarray(box, float)[:3]) @ np.linalg.inv(h_matrix(box))
    return s - np.floor(s)


def signed_modes(n):
    m = np.arange(n)
    return m - n * (2 * m // n)


class BornLongMesh(bl.BornLong):
    """BornLong with the reciprocal sum on the mesh: `setup` returns (g, mesh) and every `triples` argument takes the mesh"""

    def setup(self, box, q):
        q = np.asarray(q, float)
        return mesh_rule(box, len(q), float(np.sum(q * q)), self.rc, self.accuracy)

    def influence(self, box, g, grid):
        """G [nx, ny, nz] of the box, and the Cartesian k [nx, ny, nz, 3]"""
        B = 2.0 * math.pi * np.linalg.inv(h_matrix(box))          # k = B @ m
        p = np.stack(np.meshgrid(*[signed_modes(n) for n in grid], indexing="ij"), axis=-1).astype(float)
        k = p @ B.T
        k2 = np.einsum("...i,...i->...", k, k)
        num, den = np.zeros(grid), np.zeros(grid)
        sinc = lambda v: np.sinc(v / math.pi)
        U2 = [[sinc(math.pi * (signed_modes(n) + n * a) / n) ** (2 * ORDER) for a in range(-2, 3)] for n in grid]
        for a1 in range(-2, 3):
            for a2 in range(-2, 3):
                for a3 in range(-2, 3):
                    kb = (p + np.array([a1 * grid[0], a2 * grid[1], a3 * grid[2]], float)) @ B.T
                    kb2 = np.einsum("...i,...i->...", kb, kb)
                    w2 = U2[0][a1 + 2][:, None, None] * U2[1][a2 + 2][None, :, None] * U2[2][a3 + 2][None, None, :]
                    den += w2
                    with np.errstate(divide="ignore", invalid="ignore"):
                        num += np.where(kb2 > 0.0, np.einsum("...i,...i->...", k, kb) / kb2 * np.exp(-kb2 / (4.0 * g * g)) * w2, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.where(k2 > 0.0, 4.0 * math.pi / k2 * num / (den * den), 0.0)
        G[0, 0, 0] = 0.0
        return G, k

    def recip(self, x, box, q, g, grid, kbox=None, half_factor=2.0, field_sign=1.0):
        """(energy, forces [n, 3], virial 3 x 3) of the reciprocal sum on the mesh `grid` in the box of the atoms (kbox is not used: the
        mesh follows the box of the step)"""
        x, q = np.asarray(x, float), np.asarray(q, float)
        grid = tuple(int(v) for v in grid)
        V, NG = volume(box), grid[0] * grid[1] * grid[2]
        s = fractional(x, box)
        st = [stencil(s[:, d], grid[d]) for d in range(3)]
        rho = np.zeros(grid)
        idx = (st[0][0][:, :, None, None], st[1][0][:, None, :, None], st[2][0][:, None, None, :])
        wgt = st[0][1][:, :, None, None] * st[1][1][:, None, :, None] * st[2][1][:, None, None, :]
        np.add.at(rho, idx, q[:, None, None, None] * wgt * (NG / V))
        a = np.fft.fftn(rho) / NG
        G, k = self.influence(box, g, grid)
        k2 = np.einsum("...i,...i->...", k, k)
        ek = 0.5 * V * self.K * G * np.abs(a) ** 2
        e = float(ek.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            vt = np.where(k2 > 0.0, -2.0 * (1.0 / k2 + 0.25 / (g * g)), 0.0)
        w = float(ek.sum()) * np.eye(3) + np.einsum("xyz,xyzi,xyzj->ij", ek * vt, k, k)
        f = np.zeros((len(x), 3))
        for c in range(3):
            E = np.fft.ifftn(-1j * k[..., c] * G * a).real * NG
            f[:, c] = field_sign * self.K * q * np.sum(wgt * E[idx], axis=(1, 2, 3))
        return e, f, w

    def compute(self, x, box, types, q, g=None, triples=None, kbox=None):
        if g is None:
            g, triples = self.setup(box, q)
        out = bl.BornLong.compute(self, x, box, types, q, g, triples, kbox)
        out["nk"], out["mesh"] = 0, tuple(int(v) for v in triples)
        return out

    # ---- dynamics: velocity Verlet on the box of each step; fix deform with flips as LAMMPS' `flip yes` applies them
    def nve(self, x, v, box, types, q, masses, dt, nsteps, rates=None):
        """NVE; with rates (xx yy zz xy xz yz per fs, fix deform erate with remap x) the box moves linearly after every step and carries
        the positions along, and a tilt past half a box length flips after the step that took it there (xy, xz: the box of the next
        step is the flipped one; a yz flip is not supported).  Returns x, v, and with rates the end box, the mean of the pressure (atm)
        sampled at every step before the box moves, and the number of flips"""
        x, v = np.array(x, float), np.array(v, float)
        box0 = np.array(box, float)
        m = np.asarray(masses, float)[np.asarray(types)][:, None]
        g, grid = self.setup(box0, q)
        cur = box0.copy()
        c = self.compute(x, cur, types, q, g, grid)
        psum, shift, flips = np.zeros(6), np.zeros(3), 0
        for step in range(1, nsteps + 1):
            v += 0.5 * dt * FTM2V * c["f"] / m
            x += dt * v
            c = self.compute(x, cur, types, q, g, grid)
            v += 0.5 * dt * FTM2V * c["f"] / m
            if rates is not None:
                kin = MVV2E * np.einsum("i,ij,ik->jk", m[:, 0], v, v)
                t = (kin + c["w33"]) / volume(cur) * NKTV2P
                psum += np.array([t[0, 0], t[1, 1], t[2, 2], t[0, 1], t[0, 2], t[1, 2]])
                L0, tt = box0[3:6] - box0[:3], step * dt
                nb = cur.copy()
                nb[:3] = box0[:3] - 0.5 * L0 * np.asarray(rates[:3]) * tt
                nb[3:6] = box0[3:6] + 0.5 * L0 * np.asarray(rates[:3]) * tt
                nb[6] = box0[6] + rates[3] * L0[1] * tt + shift[0]
                nb[7] = box0[7] + rates[4] * L0[2] * tt + shift[1]
                nb[8] = box0[8] + rates[5] * L0[2] * tt + shift[2]
                x = (x - cur[:3]) @ np.linalg.inv(h_matrix(cur)) @ h_matrix(nb) + nb[:3]
                cur = nb
                if step < nsteps:          # (a flip that falls behind the last step is never applied)
                    lx, ly = cur[3] - cur[0], cur[4] - cur[1]
                    assert abs(cur[8]) <= 0.5 * ly, "a yz flip"
                    for k in (0, 1):
                        if abs(cur[6 + k]) > 0.5 * lx:
                            d = -math.copysign(lx, cur[6 + k])
                            cur[6 + k] += d
                            shift[k] += d
                            flips += 1
        if rates is None:
            return x, v
        return x, v, cur, psum / nsteps, flips

    def pressure_atm(self, x, v, box, types, q, masses, g=None, triples=None, kbox=None):
        return bl.BornLong.pressure_atm(self, x, v, box, types, q, masses, g, triples, kbox)


def case_needle(seed=3):
    """the jittered 1 x 1 x 16 cell, 128 ions: an Ewald index of 24"""
    return bl.case_jitter((1, 1, 16), seed)


def rms_force_error(f, f_ref, accuracy, K):
    """the rms force error over accuracy x K (LAMMPS' accuracy is an rms force error in units of the force between two unit charges 1 A apart)"""
    d = np.asarray(f) - np.asarray(f_ref)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1)))) / (accuracy * K)
