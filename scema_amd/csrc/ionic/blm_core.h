// blm_core.h -- what the mesh reciprocal solver of the Ewald ionic stage (md_born_long_mesh.hip) has of its own.  The PPPM arithmetic
// -- order-5 assignment, ik differentiation, the optimal influence function of the step's box, the per-mode energy / virial term -- is
// pppm/pppm_core.h, shared with the molecular path and called here with the table's K and the inverse box of bl_hinv; E_self and the
// background are bl_self of bl_core.h.  This file adds the fractional coordinate of an atom on the row layout, the fixed-point charge
// grid and the limits of the set-up.  Compiled by hipcc for the kernels and by plain g++ for the host
// (tests/born_long_mesh_host_driver.cpp runs it with a plain DFT on the CPU).
//
// The charge grid is summed in 64-bit fixed point: integer addition commutes, so the grid does not depend on the order in which the
// atoms arrive.  The scale is 2^s with s = BLM_FIXED_BITS - e, 2^(e-1) <= M < 2^e, M = (sum |q_i|) NG/V: a grid point never exceeds M in
// magnitude (weights lie in [0, 1] and sum to 1 per atom), so every sum stays below 2^62, and one unit is 2^(e-62) < 2^-60 M.
#pragma once
#include "../pppm/pppm_core.h"
#include "bl_core.h"

#define BLM_MAXGRID 4194304   /* mesh points one replica may hold */
#define BLM_MAXDIM 4096       /* where the grid search of the set-up stops: a dimension that reaches it is refused */
#define BLM_FIXED_BITS 62

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
