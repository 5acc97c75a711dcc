// vs_core.h -- the Vashishta arithmetic (Vashishta, Kalia, Nakano and Rino, J. Appl. Phys. 101, 103515 (2007); `pair_style vashishta`):
// parameter tables in the layout the kernel uses, the two-body term and the three-body term with their analytic derivatives.  Compiled
// by hipcc for the kernel of md_vashishta.hip and by plain g++ for the host (host/vashishta_params.cpp fills the tables,
// tests/vashishta_host_driver.cpp pins the derivatives on the CPU), as sw/sw_core.h is.
//
//   two-body    U(r)  = H r^-eta + K Zi Zj exp(-r/lambda1)/r - D exp(-r/lambda4)/r^4 - W/r^6
//               E2(r) = U(r) - U(rc) - (r - rc) U'(rc)                                                              r < rc
//   three-body  E3    = B dc^2 / (1 + C dc^2) exp(gamma_ij/(r_ij - r0_ij) + gamma_ik/(r_ik - r0_ik)),  dc = cos th - cos th0
//                                                                                                      r_ij < r0_ij, r_ik < r0_ik
//
// with the pair quantities of (i, j) -- H eta Zi Zj lambda1 D lambda4 W rc, and gamma r0 of an arm -- taken from the file's entry `i j j`
// and B, C, cos th0 of a triplet centred on i from its entry `i j k`.  A lambda of 0 means exp(...) = 1.  The two ranges differ: rc
// reaches 7.35 A in SiC, r0 2.90 A.  A pair at or beyond rc contributes exactly zero; an arm at or beyond its r0 must never reach the
// exponential (beyond r0 the exponent is positive and large).  The callers test `r < rc` and `r < r0` first; vs_two and vs_arm assume it.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VS_HD __host__ __device__ __forceinline__
#else
#define VS_HD inline
#endif

#define VS_MAXEL 4   /* elements kept (named by pair_coeff) */

typedef struct {
  double h, eta;       // H, eta
  double kzz;          // K Zi Zj
  double il1, il4;     // 1/lambda1, 1/lambda4 (0 for a lambda of 0: the factor exp(...) is 1)
  double d, w;         // D, W
  double rc;           // the pair's cutoff
  double urc, durc;    // U(rc), U'(rc): the shift, computed once by the reader
  double r0, gamma;    // range and exponent of the pair as an arm of a triplet (r0 = 0: never an arm)
  int ieta;            // eta when it is a whole number from 1 to 32 (no pow), else 0
  int pad_;
} VsPairP;
typedef struct {
  double b, c, cos0;   // B, C, cos th0
} VsTripP;
typedef struct {
  int nelem, pad_;
  double cutmax;                                   // the largest of rc and r0 over the pairs kept
  VsPairP pair[VS_MAXEL * VS_MAXEL];               // [i][j], from entry i j j
  VsTripP trip[VS_MAXEL * VS_MAXEL * VS_MAXEL];    // [i][j][k]
} VsTable;

// r^-eta
VS_HD double vs_rpow(const VsPairP &P, double r) {
  if (P.ieta > 0) {
    double base = 1.0 / r, out = 1.0;
    for (int n = P.ieta; n; n >>= 1) {
      if (n & 1) out *= base;
      base *= base;
    }
    return out;
  }
  return pow(r, -P.eta);
}

// the unshifted pair function and its derivative
VS_HD void vs_u(const VsPairP &P, double r, double *u, double *du) {
  const double ir = 1.0 / r, ir2 = ir * ir;
  const double rep = P.h * vs_rpow(P, r);
  const double cou = P.kzz * exp(-r * P.il1) * ir;
  const double dip = P.d * exp(-r * P.il4) * ir2 * ir2;
  const double vdw = P.w * ir2 * ir2 * ir2;
  *u = rep + cou - dip - vdw;
  *du = -P.eta * rep * ir - cou * (P.il1 + ir) + dip * (P.il4 + 4.0 * ir) + 6.0 * vdw * ir;
}

// two-body term of a pair at distance r < P.rc: the whole energy of the pair (a caller that visits the pair from both ends takes half at
// each), and fp with (force on j) = fp d, (force on i) = -fp d, d = x_j - x_i
VS_HD void vs_two(const VsPairP &P, double r, double *e, double *fp) {
  double u, du;
  vs_u(P, r, &u, &du);
  *e = u - P.urc - (r - P.rc) * P.durc;
  *fp = -(du - P.durc) / r;
}

// the radial factor one arm of a triplet carries: ex = exp(gamma / (r - r0)) and da = d(exponent)/dr, r < P.r0
VS_HD void vs_arm(const VsPairP &P, double r, double *ex, double *da) {
  const double q = r - P.r0;   // < 0
  *ex = exp(P.gamma / q);
  *da = -P.gamma / (q * q);
}

// three-body term of the triplet centred on i with arms d1 = x_j - x_i (length r1) and d2 = x_k - x_i (length r2), both inside their r0,
// with the arms' radial factors from vs_arm: energy and the forces on j and k (the force on i is minus their sum).  sw_three with
// dc^2 / (1 + C dc^2) and its derivative 2 dc / (1 + C dc^2)^2 in place of dc^2 and 2 dc
VS_HD void vs_three(const VsTripP &T, const double *d1, double r1, double ex1, double da1, const double *d2, double r2, double ex2, double da2,
                    double *e, double *fj, double *fk) {
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  const double dc = c - T.cos0;
  const double den = 1.0 / (1.0 + T.c * dc * dc);
  const double pre = T.b * ex1 * ex2;
  const double erad = pre * dc * dc * den;        // the energy; its radial derivatives are erad da1, erad da2
  const double eang = 2.0 * pre * dc * den * den; // d E3 / d cos
  *e = erad;
  // d cos / d d1 = d2 / (r1 r2) - cos d1 / r1^2
  const double a12 = eang * ir1 * ir2;
  const double g1 = erad * da1 * ir1 - eang * c * ir1 * ir1;
  const double g2 = erad * da2 * ir2 - eang * c * ir2 * ir2;
  for (int k = 0; k < 3; k++) {
    fj[k] = -(g1 * d1[k] + a12 * d2[k]);
    fk[k] = -(g2 * d2[k] + a12 * d1[k]);
  }
}
