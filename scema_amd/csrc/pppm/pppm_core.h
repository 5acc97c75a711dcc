// pppm_core.h -- the arithmetic of PPPM (Hockney & Eastwood; order-5 charge assignment, ik differentiation, the optimal influence function
// with direct alias sums |m| <= 2 per dimension), once, for the two mesh solvers of the engine: the molecular path (md_pppm.hip) and the
// Ewald ionic stage on the row driver (md_born_long_mesh.hip, ionic/blm_core.h).  Compiled by hipcc for the kernels and by plain g++ for
// the host (tests/born_long_mesh_host_driver.cpp runs it with a plain DFT on the CPU and holds it against a numpy restatement).
//
//   rho(p)   = (NG/V) sum_i q_i W(p - u_i)                  u_i = n_d s_d, s the fractional coordinates of the step's box
//   rho~(k)  = sum_p rho(p) exp(-2 pi i m.p/n)              (unnormalised forward transform), a(k) = rho~(k)/NG
//   E_recip  = (K V/2) sum_{k != 0} G(k) |a(k)|^2           G the influence function (4 pi/k^2 times the alias quotient)
//   E(k)     = -i k G(k) a(k),  E(p) its unnormalised backward transform,  F_i = K q_i sum_p W(p - u_i) E(p)
//   virial   = e_k [delta_ab - 2 (1/k^2 + 1/4g^2) k_a k_b] per mode
//
// The box enters as its six inverse entries in the layout of BoxD::hinv (1/lx, 1/ly, 1/lz, the yz-, xz- and xy-term: box_derive of
// md_device.h, bl_hinv of ionic/bl_core.h) and as its volume.  What the two paths do differently stays with them:
//   * position -> fractional coordinate: pos_lamda (md_pppm.hip) multiplies by hinv, blm_frac (blm_core.h) divides and clamps;
//   * the self and background term: inline in pppm_mode of md_pppm.hip at idx == 0, bl_self of bl_core.h on the ionic side;
//   * the 64-bit fixed-point charge grid is the ionic path's alone (blm_core.h);
//   * every launch shape, LDS layout, tile and bin belongs to the kernels.
// hipcc contracts multiply-adds by expression shape after inlining: the expressions below are written as md_pppm.hip had them, whose
// bits more tests pin.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PPPM_HD __host__ __device__ __forceinline__
#define PPPM_UNROLL _Pragma("unroll")
#else
#define PPPM_HD inline
#define PPPM_UNROLL
#endif

#define PPPM_ORDER 5
#define PPPM_PI 3.14159265358979323846

// weights of the order-5 cardinal B-spline at the 5 grid points i-2 .. i+2 around u, i = floor(u + 1/2).  With dx = i - u in (-1/2, 1/2] the
// argument of weight k, t_k = 9/2 - k - dx, lies in the spline's piece 4 - k for every k, at the SAME local coordinate s = 1/2 - dx in [0, 1):
// the five weights are the five quartic blending polynomials of the uniform B-spline in s (they sum to 1) -- 18 multiply-adds instead of the
// recursion over indicator functions that the oracle walks (oracle: pppm_weights; 330 instructions per dimension, half of the spreading and of
// the interpolation kernel until round 5).  Same numbers to the last places (the two forms round differently: 1e-16).
static_assert(PPPM_ORDER == 5, "the blending polynomials below are those of order 5");
// the nearest grid point of u (0 <= u <= n gives 0 .. n): the centre of the stencil, and -- taken mod n -- what decides an atom's home tile
PPPM_HD int pppm_nearest(double u) { return (int)floor(u + 0.5); }
PPPM_HD void pppm_blend(double s, double (&w)[PPPM_ORDER]) {
  const double r = 1.0 - s;
  const double s2 = s * s, r2 = r * r;
  constexpr double q = 1.0 / 24.0;
  w[4] = q * (s2 * s2);
  w[0] = q * (r2 * r2);
  w[3] = fma(fma(fma(fma(-4.0 * q, s, 4.0 * q), s, 6.0 * q), s, 4.0 * q), s, q);
  w[2] = fma(fma(fma(fma(6.0 * q, s, -12.0 * q), s, -6.0 * q), s, 12.0 * q), s, 11.0 * q);
  w[1] = fma(fma(fma(fma(-4.0 * q, s, 12.0 * q), s, -6.0 * q), s, -12.0 * q), s, 11.0 * q);
}
PPPM_HD int pppm_weights(double u, double (&w)[PPPM_ORDER]) {
  const int i = pppm_nearest(u);
  pppm_blend(0.5 - ((double)i - u), w);
  return i;
}
// the same weights around a nearest point that was decided before (k_pppm_keys) and is known mod n: km == 0 stands for 0 or for n
PPPM_HD void pppm_weights_at(double u, int n, int km, double (&w)[PPPM_ORDER]) {
  const int i = (km == 0 && u >= 1.0) ? n : km;
  pppm_blend(0.5 - ((double)i - u), w);
}
PPPM_HD int pppm_mod(int a, int n) { const int r = a % n; return r < 0 ? r + n : r; }
// the periodic index of v in [-2, n + 2]; grids of fewer than 4 points wrap more than once
PPPM_HD int pppm_wrap1(int v, int n) {
  if (n < 4) return pppm_mod(v, n);
  return v < 0 ? v + n : (v >= n ? v - n : v);
}
// the five periodic grid indices i-2 .. i+2 of one dimension (0 <= i <= n)
PPPM_HD void pppm_wrap(int i, int n, int (&g)[PPPM_ORDER]) {
  PPPM_UNROLL
  for (int k = 0; k < PPPM_ORDER; k++) {
    const int v = i + k - 2;
    g[k] = v < 0 ? v + n : (v >= n ? v - n : v);
  }
  if (n < 4)
    PPPM_UNROLL
    for (int k = 0; k < PPPM_ORDER; k++) g[k] = pppm_mod(i + k - 2, n);
}

// the signed index of mode m along a dimension of n points
PPPM_HD int pppm_signed(int m, int n) { return m - n * (2 * m / n); }
// Cartesian k of an integer triple: k = 2 pi p . h^-1
PPPM_HD void pppm_kvec(const double (&hinv)[6], int p1, int p2, int p3, double &kx, double &ky, double &kz) {
  const double twopi = 2.0 * PPPM_PI;
  kx = twopi * (hinv[0] * p1); ky = twopi * (hinv[5] * p1 + hinv[1] * p2); kz = twopi * (hinv[4] * p1 + hinv[3] * p2 + hinv[2] * p3);
}
PPPM_HD double pppm_sinc_pow10(double x) {
  if (x == 0.0) return 1.0;
  const double s = sin(x) / x, s2 = s * s, s4 = s2 * s2;
  return s4 * s4 * s2;
}
// the optimal influence function (ik differentiation) of mode (m1, m2, m3) of the mesh nx x ny x nz at g_ewald g; 0 for k = 0
PPPM_HD double pppm_gf(const double (&hinv)[6], double g, int nx, int ny, int nz, int m1, int m2, int m3) {
  const int p1 = pppm_signed(m1, nx), p2 = pppm_signed(m2, ny), p3 = pppm_signed(m3, nz);
  if (p1 == 0 && p2 == 0 && p3 == 0) return 0.0;
  double kx, ky, kz;
  pppm_kvec(hinv, p1, p2, p3, kx, ky, kz);
  const double sqk = kx * kx + ky * ky + kz * kz, g2inv4 = 0.25 / (g * g);
  double wxs[5], wys[5], wzs[5];   // squared transform of the assignment function, per lattice index
  PPPM_UNROLL
  for (int a = 0; a < 5; a++) {
    wxs[a] = pppm_sinc_pow10(PPPM_PI * (double)(p1 + nx * (a - 2)) / nx);
    wys[a] = pppm_sinc_pow10(PPPM_PI * (double)(p2 + ny * (a - 2)) / ny);
    wzs[a] = pppm_sinc_pow10(PPPM_PI * (double)(p3 + nz * (a - 2)) / nz);
  }
  double num = 0.0, den = 0.0;
  for (int a3 = 0; a3 < 5; a3++)
    for (int a2 = 0; a2 < 5; a2++) {
      const int q2 = p2 + ny * (a2 - 2), q3 = p3 + nz * (a3 - 2);
      const double w23 = wys[a2] * wzs[a3];
      PPPM_UNROLL
      for (int a1 = 0; a1 < 5; a1++) {
        double qx, qy, qz;
        pppm_kvec(hinv, p1 + nx * (a1 - 2), q2, q3, qx, qy, qz);
        const double dot2 = qx * qx + qy * qy + qz * qz;
        const double w2 = wxs[a1] * w23;
        den += w2;
        num += (kx * qx + ky * qy + kz * qz) / dot2 * exp(-dot2 * g2inv4) * w2;
      }
    }
  return 4.0 * PPPM_PI / sqk * num / (den * den);
}

// One mode: with a(k) = (ar, ai), the transform of the charge grid over NG, the mode's influence function gf and its wave vector, its share
// of the energy (added to e) and of the virial (added to v: xx yy zz xy xz yz) in a box of volume vol with the Coulomb prefactor kc; the
// potential gf a(k) comes back in (pr, pi): its products with -i k are the field spectra.  (g by reference, and the potential written first,
// imaginary part before real: inlined into k_pppm_poisson and k_pppm_solve this leaves the load of g_ewald inside the branch and the two
// products in the order those kernels have had, instruction for instruction; no value depends on either.)
PPPM_HD void pppm_mode_term(double vol, double kc, const double &g, double kx, double ky, double kz, double ar, double ai, double gf, double (&v)[6], double &e,
                            double &pr, double &pi) {
  pi = gf * ai; pr = gf * ar;
  if (gf != 0.0) {
    const double sqk = kx * kx + ky * ky + kz * kz;
    const double eg = 0.5 * vol * kc * gf * (ar * ar + ai * ai);
    const double vterm = -2.0 * (1.0 / sqk + 0.25 / (g * g));
    e += eg;
    v[0] += eg * (1.0 + vterm * kx * kx); v[1] += eg * (1.0 + vterm * ky * ky); v[2] += eg * (1.0 + vterm * kz * kz);
    v[3] += eg * vterm * kx * ky; v[4] += eg * vterm * kx * kz; v[5] += eg * vterm * ky * kz;
  }
}
