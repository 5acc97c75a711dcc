// adp_core.h -- the angular-dependent potential (Mishin, Mehl and Papaconstantopoulos, Acta Mater. 53, 4029 (2005); LAMMPS `pair_style
// adp` on the extended setfl tables): the embedded-atom method of eam_core.h plus a dipole vector and a quadrupole tensor per atom.
// Compiled by hipcc for the kernels of md_adp.hip and by plain g++ for the host (host/eam_setfl.cpp builds the tables,
// tests/adp_host_driver.cpp pins the derivatives on the CPU).  The spline build, the lookups, the embedding term and the pair term are
// those of eam_core.h, unchanged.  With d = x_j - x_i over 0 < r^2 < cutoff^2:
//
//   rho_i     = sum_j rho_{el(j)}(r)
//   mu_i[a]   = sum_j u_{el(i) el(j)}(r) d[a]
//   lam_i[ab] = sum_j w_{el(i) el(j)}(r) d[a] d[b]                  stored xx yy zz yz xz xy
//   nu_i      = lam_i[xx] + lam_i[yy] + lam_i[zz]
//   E = sum_i [ F(rho_i) + 1/2 sum_a mu_i[a]^2 + 1/2 sum_{ab, all nine} lam_i[ab]^2 - nu_i^2 / 6 ] + 1/2 sum_i sum_j phi(r)
//
// Forces are the exact gradient.  With Lambda_i = lam_i - (nu_i / 3) I (what dE / d lam_i[ab] is), the pair (i, j) adds to the force on i
//   the eam_pair term,   u (mu_i - mu_j) + u' ((mu_i - mu_j) . d) d / r,   2 w (Lambda_i + Lambda_j) d + w' (d . (Lambda_i + Lambda_j) . d) d / r
// and its exact negative to the force on j: the two angular terms are not central, a pair's virial (x_i - x_j) (x) f_i is not symmetric,
// the sum over all pairs is.
//
// Per atom the second pass needs ten doubles of the first: one record {F', mu x y z, lam xx yy zz yz xz xy} (ADP_REC).
#pragma once
#include "eam_core.h"

#define ADP_REC 10   /* doubles of an atom's record: F', mu[3], lam[6] */

// the head of a material's block: the embedded-atom head first (the EAM part of the block is laid out as read_eam_setfl lays it out), then
// the value records of u and w by pair [i][j], symmetric, derivative records at + 4 nr as for every function
typedef struct {
  EamHead eam;
  int off_u[EAM_MAXEL * EAM_MAXEL];
  int off_w[EAM_MAXEL * EAM_MAXEL];
} AdpHead;
static_assert(sizeof(AdpHead) <= EAM_HEAD_DOUBLES * sizeof(double), "the head fits the room of the embedded-atom head");

// the angular self-energy of an atom: 1/2 |mu|^2 + 1/2 sum over all nine lam[ab]^2 - nu^2 / 6
EAM_HD double adp_self(const double (&mu)[3], const double (&lam)[6]) {
  const double nu = lam[0] + lam[1] + lam[2];
  return 0.5 * (mu[0] * mu[0] + mu[1] * mu[1] + mu[2] * mu[2]) + 0.5 * (lam[0] * lam[0] + lam[1] * lam[1] + lam[2] * lam[2]) +
         (lam[3] * lam[3] + lam[4] * lam[4] + lam[5] * lam[5]) - nu * nu / 6.0;
}

// what an entry adds to the sums of its central atom: u d into mu, w d (x) d into lam
EAM_HD void adp_gather(double u, double w, const double (&d)[3], double (&mu)[3], double (&lam)[6]) {
  mu[0] += u * d[0]; mu[1] += u * d[1]; mu[2] += u * d[2];
  lam[0] += w * d[0] * d[0]; lam[1] += w * d[1] * d[1]; lam[2] += w * d[2] * d[2];
  lam[3] += w * d[1] * d[2]; lam[4] += w * d[0] * d[2]; lam[5] += w * d[0] * d[1];
}

// the angular force of the pair on atom i (d = x_j - x_i, r = |d|) from u, u', w, w' at r and mu, lam of both ends
EAM_HD void adp_pair(double r, const double (&d)[3], double u, double du, double w, double dw, const double (&mu_i)[3], const double (&lam_i)[6],
                     const double (&mu_j)[3], const double (&lam_j)[6], double (&f)[3]) {
  const double ri = 1.0 / r;
  const double m0 = mu_i[0] - mu_j[0], m1 = mu_i[1] - mu_j[1], m2 = mu_i[2] - mu_j[2];
  // Lambda_i + Lambda_j: the two tensors summed, a third of the trace off the diagonal
  double L[6];
  for (int k = 0; k < 6; k++) L[k] = lam_i[k] + lam_j[k];
  const double tr = (L[0] + L[1] + L[2]) / 3.0;
  L[0] -= tr; L[1] -= tr; L[2] -= tr;
  const double g0 = L[0] * d[0] + L[5] * d[1] + L[4] * d[2];
  const double g1 = L[5] * d[0] + L[1] * d[1] + L[3] * d[2];
  const double g2 = L[4] * d[0] + L[3] * d[1] + L[2] * d[2];
  const double radial = (du * (m0 * d[0] + m1 * d[1] + m2 * d[2]) + dw * (g0 * d[0] + g1 * d[1] + g2 * d[2])) * ri;
  f[0] = u * m0 + 2.0 * w * g0 + radial * d[0];
  f[1] = u * m1 + 2.0 * w * g1 + radial * d[1];
  f[2] = u * m2 + 2.0 * w * g2 + radial * d[2];
}

// half of the pair's virial (x_i - x_j) (x) f_i = -d (x) f into vir (xx yy zz xy xz yz): the other end adds the other half
EAM_HD void adp_virial(const double (&d)[3], const double (&f)[3], double (&vir)[6]) {
  vir[0] -= 0.5 * d[0] * f[0]; vir[1] -= 0.5 * d[1] * f[1]; vir[2] -= 0.5 * d[2] * f[2];
  vir[3] -= 0.5 * d[0] * f[1]; vir[4] -= 0.5 * d[0] * f[2]; vir[5] -= 0.5 * d[1] * f[2];
}
