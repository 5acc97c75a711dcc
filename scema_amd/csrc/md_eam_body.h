// md_eam_body.h -- what the embedded-atom kernels of md_eam.hip (k_eam_density, k_eam_force) and of md_eam_coul.hip (k_ec_density,
// k_ec_force) share: the density pass as one body on the gather skeleton of md_rowforce.h, and the lookups of one entry of the force
// pass.  Device code.
#pragma once
#include "eam/eam_core.h"
#include "md_kernels.h"
#include "md_rowforce.h"

typedef const double ROW_G *EamTab;

// Densities.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time; the group's
// first lane evaluates F and F' (into fp).  Value records only (eam_core.h).  blk: the material's EAM block.  The sums go to eacc: the
// embedding energy to slot EMBED, the ordered pairs inside the cutoff to slot 2 and, where ABOVE, the atoms above rhomax to slot 3.
template <int EMBED, bool ABOVE>
__device__ __forceinline__ void eam_density_body(const RowView &V, const EamTab blk, double ROW_G *fp) {
  const int n = V.n;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ EamHead s_hd;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<int>(&s_hd, blk);   // (offsets are read per lane, by the partner's element)
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int nr = s_hd.nr;
  const double rdr = s_hd.rdr, cut2 = s_hd.cut2;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // pair energy (the force pass), embedding energy, ordered pairs, atoms above rhomax
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ti = V.stype[min(i, n - 1)];
    double rho = 0.0;
    rowf_walk(V, s_sh, i, l16, [&](int j, double, double, double, double r2) __attribute__((always_inline)) {
      if (!(r2 < cut2 && r2 > 0.0)) return;
      int k;
      double p;
      eam_locate(sqrt(r2), rdr, nr, &k, &p);
      rho += eam_value(blk + s_hd.off_rho[ti * EAM_MAXEL + V.stype[j]], k, p);
      esum[2] += 1.0;
    });
    rho = row_sum(rho);
    if (i < n && l16 == 0) {
      const EamTab fv = blk + s_hd.off_f[ti];
      double e, d;
      eam_embed(fv, fv + 4 * (size_t)s_hd.nrho, s_hd.nrho, s_hd.rdrho, s_hd.rhomax, rho, &e, &d);
      fp[i] = d;
      esum[EMBED] += e;
      if (ABOVE && rho > s_hd.rhomax) esum[3] += 1.0;
    }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
}

// One entry of the force pass at distance r inside the cutoff: the derivative records of the two densities and both records of r phi,
// F' of both ends, into the pair term (eam_pair): phi, and the force factors of phi' and of the embedding terms.  hd: the head in LDS
// (its offsets are read per lane); nr, rdr: its two numbers every entry needs, read once by the kernel
__device__ __forceinline__ void eam_entry(const EamTab blk, const EamHead &hd, int nr, double rdr, int ti, int tj, double r, double fp_i, double fp_j,
                                          double *phi, double *fa, double *fb) {
  const size_t der = 4 * (size_t)nr;   // from a function's value records to its derivative records
  int k;
  double p;
  eam_locate(r, rdr, nr, &k, &p);
  const EamTab zt = blk + hd.off_z[ti * EAM_MAXEL + tj];
  const double z = eam_value(zt, k, p), dz = eam_deriv(zt + der, k, p);
  const double drho_j = eam_deriv(blk + hd.off_rho[ti * EAM_MAXEL + tj] + der, k, p);   // what j adds to the density at i
  const double drho_i = eam_deriv(blk + hd.off_rho[tj * EAM_MAXEL + ti] + der, k, p);   // what i adds at j
  eam_pair(r, z, dz, fp_i, drho_j, fp_j, drho_i, phi, fa, fb);
}
