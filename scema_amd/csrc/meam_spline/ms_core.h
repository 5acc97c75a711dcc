// ms_core.h -- the arithmetic of the spline form of the modified embedded-atom method (Lenosky et al., Modelling Simul. Mater. Sci. Eng. 8,
// 825 (2000); Hennig et al., Phys. Rev. B 78, 054121 (2008); `pair_style meam/spline`): the table of its cubic splines in the layout the
// kernels use, the evaluation of one spline, the pair term, the record of a triplet arm and the triplet term.  Compiled by hipcc for the
// kernels of md_meam_spline.hip and by plain g++ for the host (host/meam_spline_params.cpp fills the table,
// tests/meam_spline_host_driver.cpp pins the derivatives on the CPU), as vashishta/vs_core.h is.
//
//   E     = sum_{i<j} phi_{ti tj}(r_ij) + sum_i [ U_ti(rho_i) - U_ti(0) ]
//   rho_i = sum_j rho_tj(r_ij) + sum_{j<k} f_tj(r_ij) f_tk(r_ik) g_{tj tk}(cos theta_jik)
//
// Five families of clamped cubic splines: phi and g per unordered pair of elements (upper triangle, row-major: 11, 12, .., 1n, 22, ..),
// rho, U and f per element.  phi, rho and f are zero at and beyond their last knot (the callers test `r < last knot` strictly, and the
// reader refuses a file in which one of them does not end with value 0 and slope 0); outside its knots a spline continues linearly with
// its end slope, which U uses in both directions (rho_i may be negative, because g may be) and g where cos theta rounds past +-1.
// The forces are the gradient of E: a pair (i, j) carries phi' + U'_i rho'_tj + U'_j rho'_ti along its vector, a triplet around i the
// gradient of f f g scaled by U'_i alone.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MS_HD __host__ __device__ __forceinline__
#else
#define MS_HD inline
#endif

#define MS_MAXEL 2      /* elements kept (named by pair_coeff) */
#define MS_MAXKNOT 32   /* knots of one spline */
#define MS_NPAIR (MS_MAXEL * (MS_MAXEL + 1) / 2)
#define MS_NFN (2 * MS_NPAIR + 3 * MS_MAXEL)

typedef struct {
  int n;                 // knots
  int uniform;           // 1: equidistant knots, the interval comes from ih
  double ih;             // 1 / spacing of an equidistant set, else 0
  double d0, dn;         // slopes at the first and the last knot: the clamp of the spline and its linear continuation
  double x[MS_MAXKNOT], y[MS_MAXKNOT], y2[MS_MAXKNOT];   // knots, values, second derivatives (the tridiagonal solve of the reader)
} MsFn;

// the functions of the nelem elements kept stand in the file's order: phi (np = nelem (nelem + 1) / 2), rho, U, f (nelem each), g (np)
typedef struct {
  int nelem, nfn;
  int off_phi, off_rho, off_u, off_f, off_g, pad_;   // first function of every family in fn[]
  double cutmax;                                     // the largest last knot of phi, rho and f: the range of the rows
  double cut_f[MS_MAXEL][MS_MAXEL];                  // [ti][tj] the triplet range: the last knot of f of the partner's element
  double u0[MS_MAXEL];                               // U(0) of every element
  MsFn fn[MS_NFN];
} MsTable;

// place of the unordered pair (a, b) in the upper triangle of n elements, row-major
MS_HD int ms_pair_index(int n, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * n - lo * (lo - 1) / 2 + (hi - lo);
}

// the interval k (x[k] <= x < x[k + 1], clamped to the set) of a point inside the knots: by bisection
MS_HD int ms_interval_search(const MsFn &F, double x) {
  int lo = 0, hi = F.n - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (F.x[mid] > x) hi = mid;
    else lo = mid;
  }
  return lo;
}

// the same interval of an equidistant set from the inverse spacing, moved by one where the product rounds across a knot: both ways name
// one interval, so they agree to the last bit
MS_HD int ms_interval_grid(const MsFn &F, double x) {
  int k = (int)((x - F.x[0]) * F.ih);
  k = k < 0 ? 0 : (k > F.n - 2 ? F.n - 2 : k);
  if (x < F.x[k]) { if (k > 0) k--; }
  else if (x >= F.x[k + 1]) { if (k < F.n - 2) k++; }
  return k;
}

// value and derivative of the spline on interval k
MS_HD double ms_cubic(const MsFn &F, int k, double x, double *dy) {
  const double h = F.x[k + 1] - F.x[k];
  const double a = (F.x[k + 1] - x) / h, b = (x - F.x[k]) / h;
  *dy = (F.y[k + 1] - F.y[k]) / h + ((3.0 * b * b - 1.0) * F.y2[k + 1] - (3.0 * a * a - 1.0) * F.y2[k]) * h / 6.0;
  return a * F.y[k] + b * F.y[k + 1] + ((a * a * a - a) * F.y2[k] + (b * b * b - b) * F.y2[k + 1]) * (h * h) / 6.0;
}

// value and derivative at any x: the linear continuation beyond either end, else the cubic of the interval (`search`: by bisection even
// on an equidistant set)
MS_HD double ms_eval_by(const MsFn &F, double x, double *dy, bool search) {
  const int n = F.n;
  if (!(x >= F.x[0])) { *dy = F.d0; return F.y[0] + F.d0 * (x - F.x[0]); }   // (a NaN goes here and stays one: no interval is sought for it)
  if (x > F.x[n - 1]) { *dy = F.dn; return F.y[n - 1] + F.dn * (x - F.x[n - 1]); }
  return ms_cubic(F, (F.uniform && !search) ? ms_interval_grid(F, x) : ms_interval_search(F, x), x, dy);
}
MS_HD double ms_eval(const MsFn &F, double x, double *dy) { return ms_eval_by(F, x, dy, false); }

// Pair term of the pair (i, j) at distance r inside cutmax, seen from i: phi(r) (the whole energy of the pair: a caller that visits it
// from both ends takes half at each) and the two parts of fp with (force on i) = fp d, d = x_j - x_i: fa from phi', fb from
// U'_i rho'_tj + U'_j rho'_ti.  Each function counts only inside its own last knot.
MS_HD void ms_pair(const MsFn &phi, const MsFn &rho_j, const MsFn &rho_i, double r, double upi, double upj, double *e, double *fa, double *fb) {
  double dphi = 0.0, drj = 0.0, dri = 0.0;
  *e = r < phi.x[phi.n - 1] ? ms_eval(phi, r, &dphi) : 0.0;
  if (r < rho_j.x[rho_j.n - 1]) (void)ms_eval(rho_j, r, &drj);
  if (r < rho_i.x[rho_i.n - 1]) (void)ms_eval(rho_i, r, &dri);
  *fa = dphi / r;
  *fb = (upi * drj + upj * dri) / r;
}

// the record of a triplet arm: f and f' of the partner's element at r inside its last knot
MS_HD void ms_arm(const MsFn &f, double r, double *fv, double *df) { *fv = ms_eval(f, r, df); }

// cosine of the angle between two arms
MS_HD double ms_cos(const double *d1, double r1, const double *d2, double r2) { return (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) / (r1 * r2); }

// Triplet term around i with arms d1 = x_j - x_i (length r1, record f1, df1) and d2 = x_k - x_i: its part f1 f2 g(cos) of rho_i, and the
// derivatives of that part with respect to the ends of the arms, gj = d/d x_j, gk = d/d x_k (the derivative for x_i is minus their sum).
// The forces are -U'_i gj, -U'_i gk.
MS_HD double ms_three(const MsFn &g, const double *d1, double r1, double f1, double df1, const double *d2, double r2, double f2, double df2, double *gj,
                      double *gk) {
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2;
  double dg;
  const double gv = ms_eval(g, c, &dg);
  // d cos / d d1 = d2 / (r1 r2) - cos d1 / r1^2
  const double ang = f1 * f2 * dg;
  const double a12 = ang * ir1 * ir2;
  const double g1 = df1 * f2 * gv * ir1 - ang * c * ir1 * ir1;
  const double g2 = f1 * df2 * gv * ir2 - ang * c * ir2 * ir2;
  for (int k = 0; k < 3; k++) {
    gj[k] = g1 * d1[k] + a12 * d2[k];
    gk[k] = g2 * d2[k] + a12 * d1[k];
  }
  return f1 * f2 * gv;
}
