// ts_core.h -- the Tersoff arithmetic (Tersoff, Phys. Rev. B 37, 6991 (1988) and 39, 5566 (1989); LAMMPS `pair_style tersoff`): parameter
// tables in the layout the kernels use, the cutoff function, the pair term at fixed bond order, the bond order and the gradient of its
// argument zeta.  Compiled by hipcc for the kernels of md_tersoff.hip and by plain g++ for the host (host/tersoff_params.cpp fills the
// tables, tests/tersoff_host_driver.cpp pins the derivatives on the CPU), as sw/sw_core.h is.
//
//   E       = 1/2 sum_i sum_{j != i} fC(r_ij) [ fR(r_ij) + b_ij fA(r_ij) ]
//   fR      = A exp(-lambda1 r)          fA = -B exp(-lambda2 r)
//   fC      = 1 (r < R - D),  1/2 - 1/2 sin(pi/2 (r - R) / D) (R - D <= r < R + D),  0 (from R + D on)
//   b_ij    = (1 + (beta zeta_ij)^n)^(-1/(2n))
//   zeta_ij = sum_{k != i, j} fC(r_ik) g(cos theta_jik) exp[(lambda3 (r_ij - r_ik))^m]
//   g(c)    = gamma (1 + c^2/d^2 - c^2/(d^2 + (c - cos0)^2))
//
// with n, beta, lambda2, B, lambda1, A and the pair's R, D taken from the file's entry `i j j`, and m, gamma, lambda3, c, d, cos0 AND the
// R, D of the fC(r_ik) inside zeta from its entry `i j k`, as pair_tersoff.cpp does.  V_ij != V_ji: every atom evaluates all of its own
// ordered pairs.  A pair at or beyond R + D contributes exactly zero and never reaches an exponential: the callers test `r < cut` first.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TS_HD __host__ __device__ __forceinline__
#else
#define TS_HD inline
#endif

#define TS_MAXEL 4           /* elements kept (named by pair_coeff) */
#define TS_EXPMAX 69.0776    /* the exponent of zeta's exponential is clamped: above it the factor is 1e30, below its negative 0 */

typedef struct {
  double biga, bigb;         // A, B (kcal/mol)
  double lam1, lam2;
  double beta, powern;
  double bigr, bigd;
  double cut;                // R + D
  double c1, c2, c3, c4;     // where b(zeta) switches to its leading terms (ts_bond_order)
} TsPairP;
typedef struct {
  double gamma, lam3;
  double c2, d2;             // c^2, d^2
  double cos0;
  double bigr, bigd;         // of the fC(r_ik) inside zeta
  double cut;                // R + D
  int m3;                    // 1: m == 3, 0: m == 1
  int pad_;
} TsTripP;
typedef struct {
  int nelem, pad_;
  double cutmax;                                   // the largest R + D of the entries kept
  double cutin[TS_MAXEL * TS_MAXEL];               // [i][k]: the largest R + D under which a neighbour k of i is used (its pair's, or as third atom)
  TsPairP pair[TS_MAXEL * TS_MAXEL];               // [i][j], from entry i j j
  TsTripP trip[TS_MAXEL * TS_MAXEL * TS_MAXEL];    // [i][j][k]
} TsTable;

// fC(r) and its derivative for r < R + D
TS_HD void ts_fc(double bigr, double bigd, double r, double *fc, double *dfc) {
  if (r < bigr - bigd) { *fc = 1.0; *dfc = 0.0; return; }
  const double a = 1.57079632679489662 * (r - bigr) / bigd;
  *fc = 0.5 * (1.0 - sin(a));
  *dfc = -0.785398163397448310 / bigd * cos(a);
}

// g(cos theta) and dg/dcos in the form without cancellation: gamma (1 + c^2 x^2 / (d^2 (d^2 + x^2))), x = cos - cos0.  (The textbook form
// subtracts c^2/d^2 and c^2/(d^2 + x^2), both near 3.8e7 for silicon, to get 1e4.)
TS_HD void ts_g(const TsTripP &Q, double c, double *g, double *dg) {
  const double x = c - Q.cos0, den = Q.d2 + x * x;
  *g = Q.gamma * (1.0 + Q.c2 * x * x / (Q.d2 * den));
  *dg = Q.gamma * 2.0 * Q.c2 * x / (den * den);
}

// exp[(lambda3 (r1 - r2))^m] and its derivative with respect to r1 (minus that with respect to r2), the exponent clamped at +-TS_EXPMAX;
// lambda3 = 0: the factor is 1 and no exponential is called
TS_HD void ts_ex(const TsTripP &Q, double dr, double *ex, double *dex) {
  if (Q.lam3 == 0.0) { *ex = 1.0; *dex = 0.0; return; }
  const double l = Q.lam3 * dr;
  const double arg = Q.m3 ? l * l * l : l;
  const double v = arg > TS_EXPMAX ? 1.0e30 : (arg < -TS_EXPMAX ? 0.0 : exp(arg));
  *ex = v;
  *dex = (Q.m3 ? 3.0 * Q.lam3 * l * l : Q.lam3) * v;
}

// b(zeta) and db/dzeta.  With t = beta zeta both switch to their leading terms at the ends: t < c4: 1 and 0; t < c3: 1 - t^n / (2n);
// t > c2, t > c1: the large-t forms; the exact expression in between.  For n < 1 the exact derivative is singular at zeta = 0.
TS_HD void ts_bond_order(const TsPairP &P, double zeta, double *b, double *db) {
  const double t = P.beta * zeta, n = P.powern;
  if (t > P.c1) {
    *b = 1.0 / sqrt(t);
    *db = -0.5 * P.beta * pow(t, -1.5);
  } else if (t > P.c2) {
    const double tn = pow(t, -n);
    *b = (1.0 - tn / (2.0 * n)) / sqrt(t);
    *db = -0.5 * P.beta * pow(t, -1.5) * (1.0 - (1.0 + 1.0 / (2.0 * n)) * tn);
  } else if (t < P.c4) {
    *b = 1.0;
    *db = 0.0;
  } else if (t < P.c3) {
    *b = 1.0 - pow(t, n) / (2.0 * n);
    *db = -0.5 * P.beta * pow(t, n - 1.0);
  } else {
    const double tn = pow(t, n);
    const double bo = pow(1.0 + tn, -1.0 / (2.0 * n));
    *b = bo;
    *db = -0.5 * bo * tn / ((1.0 + tn) * zeta);   // (1 + t^n)^(-1 - 1/(2n)) = b / (1 + t^n): no third pow
  }
}

// The pair term of the ordered pair (i, j) at distance r < P.cut and FIXED bond order b: the repulsive part 1/2 fC fR and the part that
// carries b, 1/2 fC b fA, each with fp so that (force on j) = fp d and (force on i) = -fp d, d = x_j - x_i; fa = fA(r) for the caller's
// zeta prefactor 1/2 fC fA b'
TS_HD void ts_pair(const TsPairP &P, double r, double fc, double dfc, double b, double *erep, double *eatt, double *fprep, double *fpatt, double *fa) {
  const double fr = P.biga * exp(-P.lam1 * r);
  const double fat = -P.bigb * exp(-P.lam2 * r);
  *erep = 0.5 * fc * fr;
  *eatt = 0.5 * fc * b * fat;
  *fprep = -0.5 * (dfc - fc * P.lam1) * fr / r;
  *fpatt = -0.5 * b * (dfc - fc * P.lam2) * fat / r;
  *fa = fat;
}

// one term of zeta_ij: the arms d1 = x_j - x_i (length r1) and d2 = x_k - x_i (length r2 < Q.cut), Q = entry i j k
TS_HD double ts_zeta_term(const TsTripP &Q, const double *d1, double r1, const double *d2, double r2) {
  double fc, dfc, g, dg, ex, dex;
  ts_fc(Q.bigr, Q.bigd, r2, &fc, &dfc);
  ts_g(Q, (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) / (r1 * r2), &g, &dg);
  ts_ex(Q, r1 - r2, &ex, &dex);
  return fc * g * ex;
}

// what the same term of zeta_ij adds to the forces, with pref = dE/dzeta_ij = 1/2 fC(r_ij) fA(r_ij) b'(zeta_ij): the forces on j and on k
// (the force on i is minus their sum)
TS_HD void ts_zeta_force(const TsTripP &Q, double pref, const double *d1, double r1, const double *d2, double r2, double *fj, double *fk) {
  double fc, dfc, g, dg, ex, dex;
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  ts_fc(Q.bigr, Q.bigd, r2, &fc, &dfc);
  ts_g(Q, c, &g, &dg);
  ts_ex(Q, r1 - r2, &ex, &dex);
  const double tr1 = pref * fc * g * dex;                     // d/dr1
  const double tr2 = pref * (dfc * g * ex - fc * g * dex);    // d/dr2
  const double tc = pref * fc * dg * ex;                      // d/dcos
  // d cos / d d1 = d2 / (r1 r2) - cos d1 / r1^2
  const double a12 = tc * ir1 * ir2;
  const double g1 = tr1 * ir1 - tc * c * ir1 * ir1;
  const double g2 = tr2 * ir2 - tc * c * ir2 * ir2;
  for (int k = 0; k < 3; k++) {
    fj[k] = -(g1 * d1[k] + a12 * d2[k]);
    fk[k] = -(g2 * d2[k] + a12 * d1[k]);
  }
}
