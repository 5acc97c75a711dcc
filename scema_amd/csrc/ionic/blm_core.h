// blm_core.h -- the arithmetic of the mesh reciprocal solver of the Ewald ionic stage (md_born_long_mesh.hip): PPPM as the molecular path
// does it (md_pppm.hip; order-5 assignment, ik differentiation, the optimal influence function of the step's box with alias sums
// |m| <= 2 per dimension), restated on the row layout with the table's K.  Compiled by hipcc for the kernels and by plain g++ for the
// host (tests/born_long_mesh_host_driver.cpp runs it with a plain DFT on the CPU).  The blending weights, the wrap, the influence-function
// term and the per-mode energy / virial term are copies of those in md_pppm.hip, which stays as it is.
//
//   rho(p)   = (NG/V) sum_i q_i W(p - u_i)                  u_i = n_d s_d, s the fractional coordinates of the step's box
//   rho~(k)  = sum_p rho(p) exp(-2 pi i m.p/n)              (unnormalised forward transform), a(k) = rho~(k)/NG
//   E_recip  = (K V/2) sum_{k != 0} G(k) |a(k)|^2           G the influence function (4 pi/k^2 times the alias quotient)
//   E(k)     = -i k G(k) a(k),  E(p) its unnormalised backward transform,  F_i = K q_i sum_p W(p - u_i) E(p)
//   virial   = e_k [delta_ab - 2 (1/k^2 + 1/4g^2) k_a k_b] per mode; E_self and the background as in bl_core.h (bl_self)
//
// The charge grid is summed in 64-bit fixed point: integer addition commutes, so the grid does not depend on the order in which the
// atoms arrive.  The scale is 2^s with s = BLM_FIXED_BITS - e, 2^(e-1) <= M < 2^e, M = (sum |q_i|) NG/V: a grid point never exceeds M in
// magnitude (weights lie in [0, 1] and sum to 1 per atom), so every sum stays below 2^62, and one unit is 2^(e-62) < 2^-60 M.
#pragma once
#include "bl_core.h"

#define BLM_ORDER 5
#define BLM_MAXGRID 4194304   /* mesh points one replica may hold */
#define BLM_MAXDIM 4096       /* where the grid search of the set-up stops: a dimension that reaches it is refused */
#define BLM_FIXED_BITS 62

// the five quartic blending polynomials of the uniform order-5 B-spline at the local coordinate s in [0, 1): they sum to 1
BD_HD void blm_blend(double s, double *w) {
  const double r = 1.0 - s;
  const double s2 = s * s, r2 = r * r;
  const double q = 1.0 / 24.0;
  w[4] = q * (s2 * s2);
  w[0] = q * (r2 * r2);
  w[3] = fma(fma(fma(fma(-4.0 * q, s, 4.0 * q), s, 6.0 * q), s, 4.0 * q), s, q);
  w[2] = fma(fma(fma(fma(6.0 * q, s, -12.0 * q), s, -6.0 * q), s, 12.0 * q), s, 11.0 * q);
  w[1] = fma(fma(fma(fma(-4.0 * q, s, 12.0 * q), s, -6.0 * q), s, -12.0 * q), s, 11.0 * q);
}
// weights at the grid points i - 2 .. i + 2 around u, i = floor(u + 1/2), which is returned (0 <= u <= n gives 0 .. n)
BD_HD int blm_weights(double u, double *w) {
  const int i = (int)floor(u + 0.5);
  blm_blend(0.5 - ((double)i - u), w);
  return i;
}
// the periodic index of v in [-2, n + 2]; meshes of fewer than 4 points wrap more than once
BD_HD int blm_wrap(int v, int n) {
  if (n < 4) { const int r = v % n; return r < 0 ? r + n : r; }
  return v < 0 ? v + n : (v >= n ? v - n : v);
}
// fractional coordinates of a point in the box h = lx, ly, lz, yz, xz, xy with origin lo, wrapped into [0, 1)
BD_HD void blm_frac(const double *h, const double *lo, const double *x, double *t) {
  const double d[3] = {x[0] - lo[0], x[1] - lo[1], x[2] - lo[2]};
  double s[3];
  bl_frac(h, d, s);
  for (int k = 0; k < 3; k++) {
    t[k] = s[k] - floor(s[k]);
    if (!(t[k] >= 0.0 && t[k] < 1.0)) t[k] = 0.0;   // (a coordinate a rounding below 0 lands on 1; a non-finite one is a fault of the integrator's)
  }
}
// the binary exponent s of the fixed-point scale for a replica with sum |q| = qabs on a mesh of ng points in a box of volume vol
BD_HD int blm_fixed_shift(double qabs, int ng, double vol) {
  const double m = qabs * (double)ng / vol;
  if (!(m > 0.0) || !(m < 1e300)) return 0;
  return BLM_FIXED_BITS - (ilogb(m) + 1);
}
BD_HD long long blm_to_fixed(double v, int shift) { return llrint(ldexp(v, shift)); }
BD_HD double blm_from_fixed(long long v, int shift) { return ldexp((double)v, -shift); }

// the signed index of a mode along a dimension of n points
BD_HD int blm_signed(int m, int n) { return m - n * (2 * m / n); }

BD_HD double blm_sinc_pow10(double x) {
  if (x == 0.0) return 1.0;
  const double s = sin(x) / x, s2 = s * s, s4 = s2 * s2;
  return s4 * s4 * s2;
}
// the optimal influence function (ik differentiation) of mode (m1, m2, m3) of the mesh n in the box h at g_ewald g; 0 for k = 0
BD_HD double blm_gf(const double *h, double g, const int *n, int m1, int m2, int m3) {
  const int p1 = blm_signed(m1, n[0]), p2 = blm_signed(m2, n[1]), p3 = blm_signed(m3, n[2]);
  if (p1 == 0 && p2 == 0 && p3 == 0) return 0.0;
  const double pi = 3.14159265358979323846;
  double kv[3];
  bl_kvec(h, p1, p2, p3, kv);
  const double sqk = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2], g2inv4 = 0.25 / (g * g);
  double wxs[5], wys[5], wzs[5];   // squared transform of the assignment function, per lattice index
  for (int a = 0; a < 5; a++) {
    wxs[a] = blm_sinc_pow10(pi * (double)(p1 + n[0] * (a - 2)) / n[0]);
    wys[a] = blm_sinc_pow10(pi * (double)(p2 + n[1] * (a - 2)) / n[1]);
    wzs[a] = blm_sinc_pow10(pi * (double)(p3 + n[2] * (a - 2)) / n[2]);
  }
  double num = 0.0, den = 0.0;
  for (int a3 = 0; a3 < 5; a3++)
    for (int a2 = 0; a2 < 5; a2++) {
      const int q2 = p2 + n[1] * (a2 - 2), q3 = p3 + n[2] * (a3 - 2);
      const double w23 = wys[a2] * wzs[a3];
      for (int a1 = 0; a1 < 5; a1++) {
        double qv[3];
        bl_kvec(h, p1 + n[0] * (a1 - 2), q2, q3, qv);
        const double dot2 = qv[0] * qv[0] + qv[1] * qv[1] + qv[2] * qv[2];
        const double w2 = wxs[a1] * w23;
        den += w2;
        num += (kv[0] * qv[0] + kv[1] * qv[1] + kv[2] * qv[2]) / dot2 * exp(-dot2 * g2inv4) * w2;
      }
    }
  return 4.0 * pi / sqk * num / (den * den);
}

// One mode: with the unnormalised transform (re, im) of the charge grid and the mode's influence function gf, its wave vector kv, its
// share of the energy (added to *e) and of the virial (added to v: xx yy zz xy xz yz), and the potential gf a(k) in (pr, pi), whose
// products with -i k are the field spectra.  kc is the table's K.
BD_HD void blm_mode(const double *h, double g, double kc, const int *n, int m1, int m2, int m3, double re, double im, double gf, double *kv, double *v,
                    double *e, double *pr, double *pi) {
  bl_kvec(h, blm_signed(m1, n[0]), blm_signed(m2, n[1]), blm_signed(m3, n[2]), kv);
  const double scaleinv = 1.0 / ((double)n[0] * (double)n[1] * (double)n[2]);
  const double ar = re * scaleinv, ai = im * scaleinv;
  if (gf != 0.0) {
    const double vol = h[0] * h[1] * h[2];
    const double sqk = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    const double eg = 0.5 * vol * kc * gf * (ar * ar + ai * ai);
    const double vterm = -2.0 * (1.0 / sqk + 0.25 / (g * g));
    *e += eg;
    v[0] += eg * (1.0 + vterm * kv[0] * kv[0]); v[1] += eg * (1.0 + vterm * kv[1] * kv[1]); v[2] += eg * (1.0 + vterm * kv[2] * kv[2]);
    v[3] += eg * vterm * kv[0] * kv[1]; v[4] += eg * vterm * kv[0] * kv[2]; v[5] += eg * vterm * kv[1] * kv[2];
  }
  *pr = gf * ar; *pi = gf * ai;
}
