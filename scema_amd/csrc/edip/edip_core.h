// edip_core.h -- the arithmetic of the environment-dependent interatomic potential (Justo, Bazant, Kaxiras, Bulatov and Yip, Phys. Rev. B
// 58, 2539 (1998); `pair_style edip`, `pair_style edip/multi`): parameter tables in the layout the kernel uses, and every function of the
// form with its analytic derivatives, in closed form (pair_edip.cpp interpolates grids; nothing here does).  Compiled by hipcc for the
// kernel of md_edip.hip and by plain g++ for the host (host/edip_params.cpp fills the tables, tests/edip_host_driver.cpp pins the
// derivatives on the CPU), as sw/sw_core.h is.
//
//   f(r)    = 1 (r <= c),  exp(alpha / (1 - x^-3)) with x = (r - c)/(a - c) (c < r < a),  0 (r >= a)
//   Z_i     = sum_m f(r_im)                                           the coordination of the central atom
//   V2(r,Z) = A [ (B/r)^rho - exp(-beta Z^2) ] exp(sigma/(r - a))
//   g(r)    = exp(gamma/(r - a))                                      the arm of a triplet
//   Q(Z)    = Q0 exp(-mu Z),   tau(Z) = u1 + u2 (u3 exp(-u4 Z) - exp(-2 u4 Z))
//   h(l,Z)  = lambda [ (1 - exp(-Q (l + tau)^2)) + eta Q (l + tau)^2 ]
//   E       = sum_i [ sum_{j != i} V2(r_ij, Z_i) + sum_{j<k} g(r_ij) g(r_ik) h(cos theta_jik, Z_i) ]
//
// The pair sum runs over ORDERED pairs with no factor 1/2: V2(r_ij, Z_i) and V2(r_ji, Z_j) are two terms.  The pair quantities of (i, j)
// -- A B rho beta sigma a c alpha gamma -- are those of the file's entry `i j j`, the eight numbers of h those of entry `i j k`.  A pair
// at or beyond a contributes exactly nothing and must never reach an exponential (beyond a the exponents are positive and unbounded):
// the callers test `r < a` first, and edip_f tests its own two ends strictly.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EDIP_HD __host__ __device__ __forceinline__
#else
#define EDIP_HD inline
#endif

#define EDIP_MAXEL 4   /* elements kept (named by pair_coeff) */

typedef struct {
  double A, B, rho, beta, sigma;   // V2
  double a, c, alpha;              // the cutoff function f: outer end (the pair's cutoff), inner end, exponent
  double gamma;                    // the arm g
  double iw;                       // 1 / (a - c), computed by the reader
} EdipPairP;
typedef struct {
  double lambda, eta, q0, mu, u1, u2, u3, u4;
} EdipTripP;
typedef struct {
  int nelem, pad_;
  double cutmax;                                         // the largest a over the pairs kept
  EdipPairP pair[EDIP_MAXEL * EDIP_MAXEL];               // [i][j], from entry i j j
  EdipTripP trip[EDIP_MAXEL * EDIP_MAXEL * EDIP_MAXEL];  // [i][j][k]
} EdipTable;

// the cutoff function and its derivative at 0 < r < P.a.  alpha / (1 - x^-3) is written alpha x^3 / (x^3 - 1): no power of 1/x next to c.
// x^3 = 1 can come out of r < a by rounding; it is the outer end
EDIP_HD void edip_f(const EdipPairP &P, double r, double *f, double *df) {
  *f = 1.0; *df = 0.0;
  if (!(r > P.c)) return;
  const double x = (r - P.c) * P.iw, x3 = x * x * x, q = x3 - 1.0;
  if (!(q < 0.0)) { *f = 0.0; return; }
  *f = exp(P.alpha * x3 / q);
  *df = -3.0 * P.alpha * x * x / (q * q) * P.iw * *f;
}

// V2(r, Z) of a pair at r < P.a with its two partial derivatives
EDIP_HD void edip_v2(const EdipPairP &P, double r, double z, double *e, double *de_dr, double *de_dz) {
  const double q = r - P.a;   // < 0
  const double ex = exp(P.sigma / q);
  const double rep = P.A != 0.0 ? pow(P.B / r, P.rho) : 0.0;
  const double pz = exp(-P.beta * z * z);
  *e = P.A * (rep - pz) * ex;
  *de_dr = -P.A * P.rho * rep / r * ex - *e * P.sigma / (q * q);
  *de_dz = 2.0 * P.A * P.beta * z * pz * ex;
}

// the radial factor one arm of a triplet carries: g = exp(gamma / (r - a)) and da = g'/g, r < P.a
EDIP_HD void edip_arm(const EdipPairP &P, double r, double *g, double *da) {
  const double q = r - P.a;   // < 0
  *g = exp(P.gamma / q);
  *da = -P.gamma / (q * q);
}

// tau(Z)
EDIP_HD double edip_tau(const EdipTripP &T, double z) {
  const double e1 = exp(-T.u4 * z);
  return T.u1 + T.u2 * (T.u3 * e1 - e1 * e1);
}

// h(l, Z) with dh/dl and dh/dZ
EDIP_HD void edip_h(const EdipTripP &T, double l, double z, double *h, double *dh_dl, double *dh_dz) {
  const double e1 = exp(-T.u4 * z);
  const double tau = T.u1 + T.u2 * (T.u3 * e1 - e1 * e1);
  const double dtau = T.u2 * T.u4 * (2.0 * e1 * e1 - T.u3 * e1);
  const double Q = T.q0 * exp(-T.mu * z);
  const double s = l + tau, w = Q * s * s;
  const double ew = exp(-w);
  const double dw = T.lambda * (ew + T.eta);   // dh / d(Q s^2)
  *h = T.lambda * ((1.0 - ew) + T.eta * w);
  *dh_dl = dw * 2.0 * Q * s;
  *dh_dz = dw * (2.0 * Q * s * dtau - T.mu * w);
}

// three-body term of the triplet centred on i with arms d1 = x_j - x_i (length r1) and d2 = x_k - x_i (length r2), both inside their a,
// with the arms' factors from edip_arm and the centre's coordination z: energy, the forces on j and k at fixed z (the force on i is minus
// their sum), and dE/dz
EDIP_HD void edip_three(const EdipTripP &T, double z, const double *d1, double r1, double g1, double da1, const double *d2, double r2, double g2, double da2,
                        double *e, double *fj, double *fk, double *de_dz) {
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  double h, dh_dl, dh_dz;
  edip_h(T, c, z, &h, &dh_dl, &dh_dz);
  const double gg = g1 * g2;
  const double erad = gg * h, eang = gg * dh_dl;
  *e = erad;
  *de_dz = gg * dh_dz;
  // d cos / d d1 = d2 / (r1 r2) - cos d1 / r1^2
  const double a12 = eang * ir1 * ir2;
  const double s1 = erad * da1 * ir1 - eang * c * ir1 * ir1;
  const double s2 = erad * da2 * ir2 - eang * c * ir2 * ir2;
  for (int k = 0; k < 3; k++) {
    fj[k] = -(s1 * d1[k] + a12 * d2[k]);
    fk[k] = -(s2 * d2[k] + a12 * d1[k]);
  }
}
