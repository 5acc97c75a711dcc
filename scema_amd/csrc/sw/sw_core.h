// sw_core.h -- the Stillinger-Weber arithmetic (Stillinger and Weber, Phys. Rev. B 31, 5262 (1985); `pair_style sw` of the reference's
// examples/streched_polyhedron/lammps_scripts_sisw): parameter tables in the layout the kernels use, the two-body term and the
// three-body term with their analytic derivatives.  Compiled by hipcc for the kernels of md_sw.hip and by plain g++ for the host
// (host/sw_params.cpp fills the tables, tests/sw_host_driver.cpp pins the derivatives on the CPU), as reax/rx_core.h is.
//
//   two-body    phi2(r)          = A eps (B (sigma/r)^p - (sigma/r)^q) exp(sigma / (r - a sigma))                      r < a sigma
//   three-body  phi3(r1, r2, th) = lambda eps (cos th - cos th0)^2 exp(g1 s1 / (r1 - a1 s1) + g2 s2 / (r2 - a2 s2))   r1 < a1 s1, r2 < a2 s2
//
// with the pair parameters of (i, j) taken from the file's entry `i j j` and lambda, eps, cos th0 of a triplet from its entry `i j k`, as
// pair_sw.cpp does.  A pair at or beyond its cutoff a sigma contributes exactly zero and must never reach the exponential: beyond the
// cutoff the exponent is positive and large.  The callers test `r < cut` first; sw_arm and sw_two assume it.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SW_HD __host__ __device__ __forceinline__
#else
#define SW_HD inline
#endif

#include "../md_row_entry.h"   /* the row entries sw_owns reads: ROW_JMASK, ROW_CODE0 */

#define SW_MAXEL 4           /* elements kept (named by pair_coeff) */
#define SW_JMASK ROW_JMASK   /* the entry's atom field under this header's own name, for code written against it (tests/sw_host_driver.cpp) */

typedef struct {
  double aeps;     // A eps
  double bigb, sigma, powp, powq;
  double cut;      // a sigma
  double gs;       // gamma sigma
  int fast;        // 1: p == 4 and q == 0 (the silicon parameters): no pow
  int pad_;
} SwPairP;
typedef struct {
  double leps;     // lambda eps
  double cos0;
} SwTripP;
typedef struct {
  int nelem, pad_;
  double cutmax;                                   // the largest a sigma of the pairs kept
  SwPairP pair[SW_MAXEL * SW_MAXEL];               // [i][j], from entry i j j
  SwTripP trip[SW_MAXEL * SW_MAXEL * SW_MAXEL];    // [i][j][k]
} SwTable;

// does row entry `ent` of atom i name a pair that i evaluates?  Every pair (i, j, image) is listed at both ends: the lower index owns it; an
// atom's pair with its own image is listed twice in its own row, under a code and under the mirrored one: the upper code owns it.
SW_HD bool sw_owns(int i, int ent) {
  const int j = ent & ROW_JMASK;
  return j > i || (j == i && ((ent >> 24) & 0x7F) > ROW_CODE0);
}

// (sigma/r)^p and (sigma/r)^q
SW_HD void sw_powers(const SwPairP &P, double r, double *srp, double *srq) {
  const double sr = P.sigma / r;
  if (P.fast) {
    const double s2 = sr * sr;
    *srp = s2 * s2;
    *srq = 1.0;
  } else {
    *srp = pow(sr, P.powp);
    *srq = pow(sr, P.powq);
  }
}

// two-body term of a pair at distance r < P.cut: energy, and fp with (force on j) = fp d, (force on i) = -fp d, d = x_j - x_i
SW_HD void sw_two(const SwPairP &P, double r, double *e, double *fp) {
  double srp, srq;
  sw_powers(P, r, &srp, &srq);
  const double rc = r - P.cut;                 // < 0
  const double ex = exp(P.sigma / rc);
  const double poly = P.bigb * srp - srq;
  *e = P.aeps * poly * ex;
  // d phi2 / dr = A eps exp(..) [ (-p B (s/r)^p + q (s/r)^q) / r - poly sigma / (r - a s)^2 ]
  const double dedr = P.aeps * ex * ((P.powq * srq - P.powp * P.bigb * srp) / r - poly * P.sigma / (rc * rc));
  *fp = -dedr / r;
}

// the radial factor one arm of a triplet carries: ex = exp(gamma sigma / (r - a sigma)) and da = d(exponent)/dr, r < P.cut
SW_HD void sw_arm(const SwPairP &P, double r, double *ex, double *da) {
  const double rc = r - P.cut;
  *ex = exp(P.gs / rc);
  *da = -P.gs / (rc * rc);
}

// three-body term of the triplet centred on i with arms d1 = x_j - x_i (length r1) and d2 = x_k - x_i (length r2), both inside their
// cutoffs, with the arms' radial factors from sw_arm: energy and the forces on j and k (the force on i is minus their sum)
SW_HD void sw_three(const SwTripP &T, const double *d1, double r1, double ex1, double da1, const double *d2, double r2, double ex2, double da2,
                    double *e, double *fj, double *fk) {
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  const double dc = c - T.cos0;
  const double pre = T.leps * ex1 * ex2;
  const double erad = pre * dc * dc;      // the energy; its radial derivatives are erad da1, erad da2
  const double eang = 2.0 * pre * dc;     // d phi3 / d cos
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
