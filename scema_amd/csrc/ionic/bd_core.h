// bd_core.h -- the arithmetic of the ionic stage (`pair_style born/coul/dsf`): a Born-Mayer-Huggins short-range term (Buckingham is
// sigma = 0, D = 0) and the damped-shifted-force Coulomb sum of Fennell and Gezelter (J. Chem. Phys. 124, 234104 (2006)).  Compiled by
// hipcc for the kernel of md_born_dsf.hip and by plain g++ for the host (host/born_dsf_params.cpp fills the table,
// tests/born_dsf_host_driver.cpp pins the derivatives on the CPU), as eam/eam_core.h and vashishta/vs_core.h are.
//
//   E_born = A exp((sigma - r)/rho) - C/r^6 + D/r^8                               r < cut_lj[ti][tj], not shifted at its cutoff
//   E_coul = K q_i q_j [ erfc(alpha r)/r - erfc(alpha rc)/rc + f_s (r - rc) ]     r < rc (cut_coul)
//   f_s    = erfc(alpha rc)/rc^2 + (2 alpha/sqrt(pi)) exp(-alpha^2 rc^2)/rc
//   E_self = - K q_i^2 [ e_s/2 + alpha/sqrt(pi) ] per atom,   e_s = erfc(alpha rc)/rc + f_s rc
//
// so that E_coul = K q_i q_j [ erfc(alpha r)/r + f_s r - e_s ].  Forces are the exact gradients: energy and force of the Coulomb term
// both reach 0 at rc.  The self term has no force and no virial.  A pair at or beyond a cutoff contributes exactly zero to that term:
// bd_pair tests both itself.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BD_HD __host__ __device__ __forceinline__
#else
#define BD_HD inline
#endif

#define BD_MAXEL 4   /* atom types (pair_coeff names types, not elements) */
#define BD_TWO_OVER_SQRTPI 1.1283791670955126
#define BD_ONE_OVER_SQRTPI 0.5641895835477563

typedef struct {
  double a, irho, sigma;   // A, 1/rho, sigma
  double c, d;             // C, D
  double cut_lj2;          // the square of the pair's Born cutoff
} BdPairP;
typedef struct {
  int ntypes, pad_;
  double alpha, cut_coul;
  double e_s, f_s;         // the shift constants of the Coulomb term (above), computed once by the reader
  double k;                // the Coulomb constant in kcal A/mol
  double cutmax;           // the largest of all cutoffs
  BdPairP pair[BD_MAXEL * BD_MAXEL];   // [ti][tj], symmetric
} BdTable;

// e_s and f_s of a damping parameter and a cutoff
BD_HD void bd_shift(double alpha, double rc, double *e_s, double *f_s) {
  const double erfcc = erfc(alpha * rc), erfcd = exp(-alpha * alpha * rc * rc);
  *f_s = erfcc / (rc * rc) + BD_TWO_OVER_SQRTPI * alpha * erfcd / rc;
  *e_s = erfcc / rc + *f_s * rc;
}

// A pair of atoms with charges qi, qj at squared distance r2 > 0: the whole energies of the pair (a caller that visits the pair from both
// ends takes half at each) and the force factors fb, fc with (force on i) = -(fb + fc) d, d = x_j - x_i.  Beyond a term's cutoff its two
// outputs are exactly 0.
BD_HD void bd_pair(const BdTable &T, const BdPairP &P, double qi, double qj, double r2, double *e_born, double *e_coul, double *fb, double *fc) {
  const double r = sqrt(r2), ir = 1.0 / r, ir2 = ir * ir;
  *e_born = *e_coul = *fb = *fc = 0.0;
  if (r2 < P.cut_lj2) {
    const double ir6 = ir2 * ir2 * ir2;
    const double rep = P.a * exp((P.sigma - r) * P.irho);
    *e_born = rep - P.c * ir6 + P.d * ir6 * ir2;
    *fb = (rep * P.irho * r - 6.0 * P.c * ir6 + 8.0 * P.d * ir6 * ir2) * ir2;
  }
  const double qq = T.k * qi * qj;
  if (r < T.cut_coul && qq != 0.0) {
    const double ar = T.alpha * r;
    const double erfcc = erfc(ar), erfcd = exp(-ar * ar);
    *e_coul = qq * (erfcc * ir + T.f_s * r - T.e_s);
    *fc = qq * (erfcc * ir2 + BD_TWO_OVER_SQRTPI * T.alpha * erfcd * ir - T.f_s) * ir;
  }
}

// the self energy of one atom
BD_HD double bd_self(const BdTable &T, double q) { return -T.k * q * q * (0.5 * T.e_s + T.alpha * BD_ONE_OVER_SQRTPI); }
