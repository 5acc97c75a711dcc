// eam_core.h -- the embedded-atom arithmetic (Daw and Baskes, Phys. Rev. B 29, 6443 (1984); LAMMPS `pair_style eam/alloy` on DYNAMO setfl
// tables): the layout of a material's tables, the spline build, the two lookups with their clamps, the embedding term with its
// extrapolation and the pair term.  Compiled by hipcc for the kernels of md_eam.hip and by plain g++ for the host (host/eam_setfl.cpp
// builds the tables, tests/eam_host_driver.cpp pins the derivatives on the CPU), as tersoff/ts_core.h is.
//
//   E      = sum_i F_{el(i)}(rho_i) + 1/2 sum_i sum_{j != i} phi_{el(i) el(j)}(r_ij)       over 0 < r^2 < cutoff^2
//   rho_i  = sum_{j != i} rho_{el(j)}(r_ij)
//
// A function is tabulated as f[0..n-1] at x_k = k delta.  Knot k holds the cubic of its interval in p = x / delta - k,
//   value       ((s3 p + s4) p + s5) p + s6
//   derivative  (s0 p + s1) p + s2,      s2 = s5 / delta, s1 = 2 s4 / delta, s0 = 3 s3 / delta
// with s6 = f[k], s5 the five-point slope ((f[k-2] - f[k+2]) + 8 (f[k+1] - f[k-1])) / 12 (three-point and one-sided at the two ends),
// s4 = 3 (f[k+1] - f[k]) - 2 s5[k] - s5[k+1], s3 = s5[k] + s5[k+1] - 2 (f[k+1] - f[k]), both 0 at the last knot.  The derivative is
// exactly that of the cubic: forces are the exact gradient of the energy.  Lookup: p = x / delta, k = min(int(p), n - 2) (not below 0),
// p = min(p - k, 1).  Above rhomax = (Nrho - 1) drho the embedding energy continues with the slope of the clamped lookup.
//
// Layout.  The seven coefficients of a knot are split into two records of four doubles, value {s3, s4, s5, s6} and derivative
// {s0, s1, s2, 0}, in two arrays per function: the density pass reads value records only, the force pass reads the derivative records of
// the densities and both records of r phi; a record is 32 bytes and 32-byte aligned.  One material is one flat block: an EamHead, then
// the arrays, addressed by offsets in doubles from the start of the block.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EAM_HD __host__ __device__ __forceinline__
#else
#define EAM_HD inline
#endif

#define EAM_MAXEL 4           /* elements kept (named by pair_coeff) */
#define EAM_HEAD_DOUBLES 64   /* the head's room at the start of the block, in doubles (tables start 32-byte aligned) */

typedef struct {
  int nelem, nrho, nr, pad_;
  double drho, dr, rdrho, rdr;   // spacings and their reciprocals
  double cutoff, cut2, rhomax;
  long long ndoubles;            // the block's size in doubles, head included
  // offsets of the value records; the derivative records of the same function follow at + 4 n
  int off_f[EAM_MAXEL];                   // F of element i: [nrho][4]
  int off_rho[EAM_MAXEL * EAM_MAXEL];     // [i][j]: density at an atom of element i from a neighbour of element j.  eam/alloy: one table
                                          // per source element j, the same for every i (eam/fs would point each (i, j) to its own)
  int off_z[EAM_MAXEL * EAM_MAXEL];       // [i][j]: r phi_ij, symmetric
} EamHead;
static_assert(sizeof(EamHead) <= EAM_HEAD_DOUBLES * sizeof(double), "the head fits its room");

// the records of n knots from f[0..n-1]: val [n][4], der [n][4]
EAM_HD void eam_spline_build(const double *f, int n, double delta, double *val, double *der) {
  for (int k = 0; k < n; k++) val[4 * k + 3] = f[k];
  val[4 * 0 + 2] = f[1] - f[0];
  val[4 * 1 + 2] = 0.5 * (f[2] - f[0]);
  val[4 * (n - 2) + 2] = 0.5 * (f[n - 1] - f[n - 3]);
  val[4 * (n - 1) + 2] = f[n - 1] - f[n - 2];
  for (int k = 2; k < n - 2; k++) val[4 * k + 2] = ((f[k - 2] - f[k + 2]) + 8.0 * (f[k + 1] - f[k - 1])) / 12.0;
  for (int k = 0; k < n - 1; k++) {
    const double df = f[k + 1] - f[k];
    val[4 * k + 1] = 3.0 * df - 2.0 * val[4 * k + 2] - val[4 * (k + 1) + 2];
    val[4 * k + 0] = val[4 * k + 2] + val[4 * (k + 1) + 2] - 2.0 * df;
  }
  val[4 * (n - 1) + 1] = 0.0;
  val[4 * (n - 1) + 0] = 0.0;
  for (int k = 0; k < n; k++) {
    der[4 * k + 2] = val[4 * k + 2] / delta;
    der[4 * k + 1] = 2.0 * val[4 * k + 1] / delta;
    der[4 * k + 0] = 3.0 * val[4 * k + 0] / delta;
    der[4 * k + 3] = 0.0;
  }
}

// knot and fraction of x.  The knot stays inside [0, n - 2] whatever x is (a distance is never negative, a density may be; a NaN lands on
// the last interval): nothing but k is ever used as an index into a table.
EAM_HD void eam_locate(double x, double rdelta, int n, int *k, double *p) {
  const double q = x * rdelta;
  int kk = (q < (double)(n - 2)) ? (int)q : n - 2;
  if (kk < 0) kk = 0;
  *k = kk;
  *p = fmin(q - (double)kk, 1.0);
}
// T: pointer to the records (const double *, in device code with its address space)
template <class T>
EAM_HD double eam_value(T val, int k, double p) {
  return ((val[4 * k] * p + val[4 * k + 1]) * p + val[4 * k + 2]) * p + val[4 * k + 3];
}
template <class T>
EAM_HD double eam_deriv(T der, int k, double p) {
  return (der[4 * k] * p + der[4 * k + 1]) * p + der[4 * k + 2];
}

// embedding energy and F' of an atom with density rho: the clamped lookup, continued linearly above rhomax
template <class T>
EAM_HD void eam_embed(T val, T der, int nrho, double rdrho, double rhomax, double rho, double *e, double *fp) {
  int k;
  double p;
  eam_locate(rho, rdrho, nrho, &k, &p);
  *fp = eam_deriv(der, k, p);
  *e = eam_value(val, k, p);
  if (rho > rhomax) *e += *fp * (rho - rhomax);
}

// the pair term at distance r (0 < r < cutoff) from z = r phi, z', and the two density slopes: rho'_{el(j)} (what j adds to the density at
// i, weighted by F'_i) and rho'_{el(i)} (what i adds at j, weighted by F'_j).  phi counts once per pair; fpair_* multiply x_i - x_j to
// give the force on i.
EAM_HD void eam_pair(double r, double z, double dz, double fp_i, double drho_j, double fp_j, double drho_i, double *phi, double *fpair_phi, double *fpair_emb) {
  const double ri = 1.0 / r;
  const double ph = z * ri;
  const double dphi = dz * ri - ph * ri;
  *phi = ph;
  *fpair_phi = -dphi * ri;
  *fpair_emb = -(fp_i * drho_j + fp_j * drho_i) * ri;
}
