// md_adp.hip -- gfx950 kernels of the angular-dependent potential (`pair_style adp`), on the neighbour rows of the row part
// (mdk_rows_build, md_rows.hip) in the launch shape of md_eam.hip: 256 lanes, a group of 16 lanes per central atom, four rounds per tile
// of 64 atoms, one launch for every replica of the batch (blockIdx.y).
//   k_adp_density .. rho_i, mu_i and lam_i over the entries of atom i's row inside the cutoff: ten sums per group; F(rho_i) and the angular
//                    self-energy into the step's energy, the record {F', mu, lam} of the atom into AdpView::rec
//   k_adp_force .... the same walk with the embedded-atom pair term and the two angular terms (eam/adp_core.h); a lane gathers its
//                    partner's record, 80 bytes, per entry
// With full rows every atom sums its own force, the partner's end of a pair is summed by the partner: no atomic on a force, a density, a
// dipole or a quadrupole; rows are sorted and a group's sum has a fixed order, so forces do not depend on the schedule.
// Engine parts: phi and its virial go to P_LJ; the embedding and angular energies and their virial to P_ANGLE.
#include <hip/hip_runtime.h>

#include "md_adp.h"
#include "md_kernels.h"
#include "md_rowforce.h"

typedef const double ROW_G *AdpTab;

// Densities, dipoles and quadrupoles.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them
// at a time; the group's first lane evaluates F, F' and the angular self-energy and writes the atom's record.  Value records only.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_adp_density(const SimDev *sims, const RowView *views, const AdpView *aux) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const AdpTab blk = (AdpTab)V.tab;
  double ROW_G *rec = aux[blockIdx.y].rec;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ AdpHead s_hd;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<int>(&s_hd, blk);   // (offsets are read per lane, by the partner's element)
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int nr = s_hd.eam.nr;
  const double rdr = s_hd.eam.rdr, cut2 = s_hd.eam.cut2;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // pair energy (the force pass), embedding + angular energy, ordered pairs, atoms above rhomax
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ti = V.stype[min(i, n - 1)];
    double rho = 0.0, mu[3] = {0.0, 0.0, 0.0}, lam[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      if (!(r2 < cut2 && r2 > 0.0)) return;
      const double d[3] = {d0, d1, d2};
      const int tj = V.stype[j], pr = ti * EAM_MAXEL + tj;
      int k;
      double p;
      eam_locate(sqrt(r2), rdr, nr, &k, &p);
      rho += eam_value(blk + s_hd.eam.off_rho[pr], k, p);
      adp_gather(eam_value(blk + s_hd.off_u[pr], k, p), eam_value(blk + s_hd.off_w[pr], k, p), d, mu, lam);
      esum[2] += 1.0;
    });
    rho = row_sum(rho);
#pragma unroll
    for (int a = 0; a < 3; a++) mu[a] = row_sum(mu[a]);
#pragma unroll
    for (int a = 0; a < 6; a++) lam[a] = row_sum(lam[a]);
    if (i < n && l16 == 0) {
      const AdpTab fv = blk + s_hd.eam.off_f[ti];
      double e, fp;
      eam_embed(fv, fv + 4 * (size_t)s_hd.eam.nrho, s_hd.eam.nrho, s_hd.eam.rdrho, s_hd.eam.rhomax, rho, &e, &fp);
      double ROW_G *o = rec + (size_t)ADP_REC * i;
      o[0] = fp;
#pragma unroll
      for (int a = 0; a < 3; a++) o[1 + a] = mu[a];
#pragma unroll
      for (int a = 0; a < 6; a++) o[4 + a] = lam[a];
      esum[1] += e + adp_self(mu, lam);
      if (rho > s_hd.eam.rhomax) esum[3] += 1.0;
    }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
}

// Forces: the same walk; a lane's entry takes the derivative records of the two densities and both records of r phi, u and w, and the
// records of both ends.  The group's sum is the atom's force, stored once.  Half of a pair's phi and half of its virial go to each end.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_adp_force(const SimDev *sims, const RowView *views, const AdpView *aux) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const AdpTab blk = (AdpTab)V.tab;
  const double ROW_G *rec = aux[blockIdx.y].rec;
  SimScalars &sc = *sims[blockIdx.y].sc;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ AdpHead s_hd;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<int>(&s_hd, blk);   // (offsets are read per lane, by the partner's element)
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int nr = s_hd.eam.nr;
  const size_t der = 4 * (size_t)nr;   // from a function's value records to its derivative records
  const double rdr = s_hd.eam.rdr, cut2 = s_hd.eam.cut2;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};
  double wa[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ic = min(i, n - 1);
    const int ti = V.stype[ic];
    const double ROW_G *ri = rec + (size_t)ADP_REC * ic;
    const double fpi = ri[0];
    const double mu_i[3] = {ri[1], ri[2], ri[3]}, lam_i[6] = {ri[4], ri[5], ri[6], ri[7], ri[8], ri[9]};
    double fi[3] = {0.0, 0.0, 0.0};
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      if (!(r2 < cut2 && r2 > 0.0)) return;
      const double d[3] = {d0, d1, d2};
      const int tj = V.stype[j], pr = ti * EAM_MAXEL + tj;
      const double ROW_G *rj = rec + (size_t)ADP_REC * j;
      const double mu_j[3] = {rj[1], rj[2], rj[3]}, lam_j[6] = {rj[4], rj[5], rj[6], rj[7], rj[8], rj[9]};
      const double r = sqrt(r2);
      int k;
      double p;
      eam_locate(r, rdr, nr, &k, &p);
      const AdpTab zt = blk + s_hd.eam.off_z[pr], ut = blk + s_hd.off_u[pr], wt = blk + s_hd.off_w[pr];
      const double z = eam_value(zt, k, p), dz = eam_deriv(zt + der, k, p);
      const double drho_j = eam_deriv(blk + s_hd.eam.off_rho[pr] + der, k, p);                        // what j adds to the density at i
      const double drho_i = eam_deriv(blk + s_hd.eam.off_rho[tj * EAM_MAXEL + ti] + der, k, p);     // what i adds at j
      double phi, fa, fb, g[3];
      eam_pair(r, z, dz, fpi, drho_j, rj[0], drho_i, &phi, &fa, &fb);
      adp_pair(r, d, eam_value(ut, k, p), eam_deriv(ut + der, k, p), eam_value(wt, k, p), eam_deriv(wt + der, k, p), mu_i, lam_i, mu_j, lam_j, g);
      const double fpair = fa + fb;
      fi[0] += g[0] - d[0] * fpair; fi[1] += g[1] - d[1] * fpair; fi[2] += g[2] - d[2] * fpair;   // (x_i - x_j = -d)
      esum[0] += 0.5 * phi;
      rowf_virial(wa, 0.5 * fa, d0, d1, d2);
      rowf_virial(wb, 0.5 * fb, d0, d1, d2);
      adp_virial(d, g, wb);
    });
    fi[0] = row_sum(fi[0]); fi[1] = row_sum(fi[1]); fi[2] = row_sum(fi[2]);
    if (i < n && l16 == 0) { V.f[3 * i] = fi[0]; V.f[3 * i + 1] = fi[1]; V.f[3 * i + 2] = fi[2]; }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wa, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_ANGLE * 6], s_red);
}

void mdk_adp_forces(hipStream_t st, const SimDev *d, RowView *v, const AdpView *a, int ns, int maxatoms) {
  mdk_row_stage(st, d, v, ns, maxatoms, [&](dim3 gt) {
    hipLaunchKernelGGL(k_adp_density, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
    hipLaunchKernelGGL(k_adp_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
  });
}
