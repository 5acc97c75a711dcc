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
// (the forms tersoff/mod, tersoff/mod/c and tersoff/zbl stand at the end of the file, each with its own header; ts_zeta_term, ts_zeta_force
// and ts_ex serve every form through the type of the triplet entry they are given)
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

// fC of the ordered pair itself under the R, D of its entry i j j (every form has one: the kernel and the host drivers call this)
TS_HD void ts_pair_fc(const TsPairP &P, double r, double *fc, double *dfc) { ts_fc(P.bigr, P.bigd, r, fc, dfc); }
TS_HD double ts_pair_cut(const TsPairP &P) { return P.cut; }

// g(cos theta) and dg/dcos in the form without cancellation: gamma (1 + c^2 x^2 / (d^2 (d^2 + x^2))), x = cos - cos0.  (The textbook form
// subtracts c^2/d^2 and c^2/(d^2 + x^2), both near 3.8e7 for silicon, to get 1e4.)
TS_HD void ts_g(const TsTripP &Q, double c, double *g, double *dg) {
  const double x = c - Q.cos0, den = Q.d2 + x * x;
  *g = Q.gamma * (1.0 + Q.c2 * x * x / (Q.d2 * den));
  *dg = Q.gamma * 2.0 * Q.c2 * x / (den * den);
}

// exp[(lambda3 (r1 - r2))^m] and its derivative with respect to r1 (minus that with respect to r2), the exponent clamped at +-TS_EXPMAX;
// lambda3 = 0: the factor is 1 and no exponential is called
template <class Trip>
TS_HD void ts_ex(const Trip &Q, double dr, double *ex, double *dex) {
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

// fC(r_ik) under the R, D of a triplet entry: what ts_zeta_term and ts_zeta_force call, with ts_g and ts_ex, for the entry's own form
TS_HD void ts_trip_fc(const TsTripP &Q, double r, double *fc, double *dfc) { ts_fc(Q.bigr, Q.bigd, r, fc, dfc); }

// one term of zeta_ij: the arms d1 = x_j - x_i (length r1) and d2 = x_k - x_i (length r2 < Q.cut), Q = entry i j k (TsTripP, or the
// TsModTripP of tersoff/mod below: the form's fC and g come with the entry's type)
template <class Trip>
TS_HD double ts_zeta_term(const Trip &Q, const double *d1, double r1, const double *d2, double r2) {
  double fc, dfc, g, dg, ex, dex;
  ts_trip_fc(Q, r2, &fc, &dfc);
  ts_g(Q, (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) / (r1 * r2), &g, &dg);
  ts_ex(Q, r1 - r2, &ex, &dex);
  return fc * g * ex;
}

// what the same term of zeta_ij adds to the forces, with pref = dE/dzeta_ij = 1/2 fC(r_ij) fA(r_ij) b'(zeta_ij): the forces on j and on k
// (the force on i is minus their sum)
template <class Trip>
TS_HD void ts_zeta_force(const Trip &Q, double pref, const double *d1, double r1, const double *d2, double r2, double *fj, double *fk) {
  double fc, dfc, g, dg, ex, dex;
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  ts_trip_fc(Q, r2, &fc, &dfc);
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

// ---- tersoff/mod and tersoff/mod/c (Kumagai, Izumi, Hara, Sakai, Comp. Mater. Sci. 39, 457 (2007); LAMMPS `pair_style tersoff/mod`,
// `tersoff/mod/c`): one form, c0 = 0 gives tersoff/mod ----
//
//   E       = 1/2 sum_i sum_{j != i} fC(r_ij) [ fR(r_ij) + c0 + b_ij fA(r_ij) ]            fR, fA as above
//   fC      = 1 (r < R - D),  1/2 - 9/16 sin(pi/2 (r - R)/D) - 1/16 sin(3 pi/2 (r - R)/D) (up to R + D),  0 (from R + D on)
//   zeta_ij = sum_k fC(r_ik) g(cos theta_jik) exp[(alpha (r_ij - r_ik))^beta]             beta 1 or 3, the exponent clamped by ts_ex
//   g(c)    = c1 + [c2 (h - c)^2 / (c3 + (h - c)^2)] [1 + c4 exp(-c5 (h - c)^2)]
//   b_ij    = (1 + (beta_ters zeta)^eta)^(-1/(2n));  t = beta_ters zeta > ca1: t^(-eta/(2n));  t < ca4: 1 and b' = 0
//
// The entries are chosen as above: pair quantities (and c0) from i j j, everything inside zeta from i j k.  The c0 term carries no b: it
// belongs to the repulsive part.  g as written has no cancellation to avoid: with c2, c3, c4, c5 >= 0 its second term is a product of
// non-negative factors, x^2 / (c3 + x^2) is evaluated by one division, and c2/c3 is of order 1 for silicon (0.73 against the 3.8e7 that
// the plain form subtracts), so g_o = g(h) = c1 comes out to the bit and g near it keeps every digit of c1 + O(x^2).
typedef struct {
  double biga, bigb;
  double lam1, lam2;
  double beta, eta, powern;  // beta_ters (the reader admits 1 only), eta, n
  double bigr, bigd;
  double cut;                // R + D
  double ca1, ca4;           // where b(zeta) switches to its end forms
  double c0;                 // tersoff/mod/c; 0: tersoff/mod
} TsModPairP;
typedef struct {
  double lam3;               // alpha
  double h;
  double c1, c2, c3, c4, c5;
  double bigr, bigd;         // of the fC(r_ik) inside zeta
  double cut;                // R + D
  int m3;                    // 1: beta == 3, 0: beta == 1
  int pad_;
} TsModTripP;
typedef struct {
  int nelem, pad_;
  double cutmax;
  double cutin[TS_MAXEL * TS_MAXEL];
  TsModPairP pair[TS_MAXEL * TS_MAXEL];
  TsModTripP trip[TS_MAXEL * TS_MAXEL * TS_MAXEL];
} TsModTable;

// fC of the mod form and its derivative for r < R + D: both vanish at R + D, and so does the second derivative (the reason for the form).
// The three terms cancel there with an absolute rounding of 1e-16: within some 3e-5 A of R + D the value may come out as -5e-17 where 2e-17
// is meant.  A zeta that is negative by that much has t < ca4 and takes the end form b = 1 of ts_bond_order, never a power.
TS_HD void ts_fc_mod(double bigr, double bigd, double r, double *fc, double *dfc) {
  if (r < bigr - bigd) { *fc = 1.0; *dfc = 0.0; return; }
  const double a = 1.57079632679489662 * (r - bigr) / bigd;
  *fc = 0.5 - 0.5625 * sin(a) - 0.0625 * sin(3.0 * a);
  *dfc = -1.57079632679489662 / bigd * (0.5625 * cos(a) + 0.1875 * cos(3.0 * a));
}
TS_HD void ts_pair_fc(const TsModPairP &P, double r, double *fc, double *dfc) { ts_fc_mod(P.bigr, P.bigd, r, fc, dfc); }
TS_HD double ts_pair_cut(const TsModPairP &P) { return P.cut; }
TS_HD void ts_trip_fc(const TsModTripP &Q, double r, double *fc, double *dfc) { ts_fc_mod(Q.bigr, Q.bigd, r, fc, dfc); }

// g(cos theta) and dg/dcos of the mod form; cos == h gives c1 and 0 exactly (the reader refuses c3 = 0 where cos can reach h)
TS_HD void ts_g(const TsModTripP &Q, double c, double *g, double *dg) {
  const double x = Q.h - c, x2 = x * x, den = Q.c3 + x2;
  const double g1 = Q.c2 * x2 / den, dg1 = 2.0 * Q.c2 * Q.c3 * x / (den * den);      // d/dx
  double g2 = 1.0, dg2 = 0.0;
  if (Q.c4 != 0.0) {
    const double ex = Q.c4 * exp(-Q.c5 * x2);
    g2 = 1.0 + ex;
    dg2 = -2.0 * Q.c5 * x * ex;
  }
  *g = Q.c1 + g1 * g2;
  *dg = -(dg1 * g2 + g1 * dg2);   // (dx/dcos = -1)
}

TS_HD void ts_bond_order(const TsModPairP &P, double zeta, double *b, double *db) {
  const double t = P.beta * zeta, q = P.eta / (2.0 * P.powern);
  if (t > P.ca1) {
    const double bo = pow(t, -q);
    *b = bo;
    *db = -q * bo / zeta;
  } else if (t < P.ca4) {
    *b = 1.0;
    *db = 0.0;
  } else {
    const double te = pow(t, P.eta);
    const double bo = pow(1.0 + te, -1.0 / (2.0 * P.powern));
    *b = bo;
    *db = -q * bo * te / ((1.0 + te) * zeta);
  }
}

// the pair term of the mod form at fixed b, as ts_pair: 1/2 fC (fR + c0) is the part without b
TS_HD void ts_pair(const TsModPairP &P, double r, double fc, double dfc, double b, double *erep, double *eatt, double *fprep, double *fpatt, double *fa) {
  const double fr = P.biga * exp(-P.lam1 * r);
  const double fat = -P.bigb * exp(-P.lam2 * r);
  *erep = 0.5 * fc * (fr + P.c0);
  *eatt = 0.5 * fc * b * fat;
  *fprep = -0.5 * (dfc * (fr + P.c0) - fc * P.lam1 * fr) / r;
  *fpatt = -0.5 * b * (dfc - fc * P.lam2) * fat / r;
  *fa = fat;
}

// ---- tersoff/zbl (LAMMPS `pair_style tersoff/zbl`; Devanathan, Diaz de la Rubia, Weber, J. Nucl. Mater. 253, 47 (1998)): plain Tersoff
// whose pair term is joined to the Ziegler-Biersack-Littmark screened Coulomb repulsion by a Fermi function ----
//
//   F(r)   = 1 / (1 + exp(-A_F (r - r_C)))                 A_F = ZBLexpscale, r_C = ZBLcut of entry i j j; the exponent clamped at
//                                                          +-TS_EXPMAX: F = 0 above, 1 below
//   without b:  1/2 [ (1 - F) V_ZBL(r) + F fC fR ]         with b:  1/2 fC b (F fA); F also multiplies the fA of the zeta prefactor
//   V_ZBL  = K Z_i Z_j phi(r/a) / r,   a = 0.8854 * 0.529 / (Z_i^0.23 + Z_j^0.23) A,   K = 1/(4 pi 0.00552635) eV A
//   phi(x) = 0.1818 e^(-3.2 x) + 0.5099 e^(-0.9423 x) + 0.2802 e^(-0.4029 x) + 0.02817 e^(-0.2016 x)
//
// fC, g, zeta and b are the plain ones (TsTripP, ts_bond_order).  The (1 - F) V_ZBL part is NOT multiplied by fC, and the pair is evaluated
// for r < R + D only: the energy has a step of (1 - F) V_ZBL / 2 per ordered pair, of order e^(-A_F (R + D - r_C)), at the cutoff (1e-12 of
// V_ZBL for the silicon carbide file: A_F = 14 / A, r_C = 0.95 A, R + D = 3 A).
#define TS_ZBL_K_EV (1.0 / (4.0 * 3.14159265358979323846 * 0.00552635))   /* eV A (14.39964...) */
#define TS_ZBL_EV_REAL 0.043365121     /* energy_unit 1: K / this, kcal/mol A as `units real` has it */
typedef struct {
  TsPairP p;                 // the plain pair entry
  double kzz;                // K Z_i Z_j (kcal/mol A)
  double inva;               // 1 / a
  double zcut, zscale;       // r_C, A_F
} TsZblPairP;
typedef struct {
  int nelem, pad_;
  double cutmax;
  double cutin[TS_MAXEL * TS_MAXEL];
  TsZblPairP pair[TS_MAXEL * TS_MAXEL];
  TsTripP trip[TS_MAXEL * TS_MAXEL * TS_MAXEL];
} TsZblTable;

TS_HD void ts_pair_fc(const TsZblPairP &P, double r, double *fc, double *dfc) { ts_fc(P.p.bigr, P.p.bigd, r, fc, dfc); }
TS_HD double ts_pair_cut(const TsZblPairP &P) { return P.p.cut; }
TS_HD void ts_bond_order(const TsZblPairP &P, double zeta, double *b, double *db) { ts_bond_order(P.p, zeta, b, db); }

// the Fermi function and its derivative
TS_HD void ts_zbl_fermi(const TsZblPairP &P, double r, double *F, double *dF) {
  const double arg = -P.zscale * (r - P.zcut);
  if (arg > TS_EXPMAX) { *F = 0.0; *dF = 0.0; return; }
  if (arg < -TS_EXPMAX) { *F = 1.0; *dF = 0.0; return; }
  const double ex = exp(arg), f = 1.0 / (1.0 + ex);
  *F = f;
  *dF = P.zscale * ex * f * f;
}
// V_ZBL and its derivative
TS_HD void ts_zbl_v(const TsZblPairP &P, double r, double *v, double *dv) {
  const double x = r * P.inva;
  const double e1 = 0.1818 * exp(-3.2 * x), e2 = 0.5099 * exp(-0.9423 * x), e3 = 0.2802 * exp(-0.4029 * x), e4 = 0.02817 * exp(-0.2016 * x);
  const double phi = e1 + e2 + e3 + e4, dphi = -(3.2 * e1 + 0.9423 * e2 + 0.4029 * e3 + 0.2016 * e4) * P.inva;
  const double ir = 1.0 / r;
  *v = P.kzz * phi * ir;
  *dv = P.kzz * (dphi - phi * ir) * ir;
}
// the pair term of the ZBL form at fixed b, as ts_pair; fa = F fA for the caller's zeta prefactor
TS_HD void ts_pair(const TsZblPairP &P, double r, double fc, double dfc, double b, double *erep, double *eatt, double *fprep, double *fpatt, double *fa) {
  double F, dF, v, dv;
  ts_zbl_fermi(P, r, &F, &dF);
  ts_zbl_v(P, r, &v, &dv);
  const double fr = P.p.biga * exp(-P.p.lam1 * r);
  const double fat = -P.p.bigb * exp(-P.p.lam2 * r);
  *erep = 0.5 * ((1.0 - F) * v + F * fc * fr);
  *eatt = 0.5 * fc * b * F * fat;
  *fprep = -0.5 * ((1.0 - F) * dv - dF * v + (dF * fc + F * (dfc - fc * P.p.lam1)) * fr) / r;
  *fpatt = -0.5 * b * (F * (dfc - fc * P.p.lam2) + dF * fc) * fat / r;
  *fa = F * fat;
}
