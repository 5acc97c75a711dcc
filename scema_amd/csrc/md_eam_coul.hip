// md_eam_coul.hip -- gfx950 kernels of the real-space part of the EAM + long-range Coulomb stage (`pair_style hybrid/overlay coul/long
// <cut_coul> eam/alloy` with `kspace_style ewald|pppm <accuracy>`: the many-body oxide models of the Cooper-Rushton-Grimes form).  The
// first stage made of two potentials: the embedded-atom terms of md_eam.hip and the Ewald real-space term of md_born_long.hip over ONE
// walk of an atom's row; the reciprocal part, self and background terms are the Born/long stage's kernels, which read nothing of the
// table but K (eam/ec_core.h has the layout).  Launch shape of k_eam_force and k_bl_force: blockIdx.y = replica.
//   k_ec_density ... the density pass of k_eam_density (eam_density_body, md_eam_body.h) over the entries inside the setfl cutoff: F'
//                    into fp[i], the embedding energy into eacc[0], the ordered pairs into eacc[2]
//   k_ec_force ..... one rowf_walk over the entries inside cutmax = max(setfl cutoff, cut_coul); each term is tested against its own
//                    cutoff, so either may be the larger: the EAM pair term (eam_entry) where r^2 < cut2, the Ewald real-space term
//                    (bl_coul, ionic/bl_core.h) at the replica's g where r < cut_coul.  The group's sum is the atom's force, stored once
// No atomic touches a force, rows are sorted and a group's sum has a fixed order: two evaluations of one state give the same forces bit
// for bit, as in both parents.  The EAM virial is one six-vector (P_LJ: only the sum of the phi' and the F' halves enters the stress),
// which keeps the kernel at the twelve virial accumulators of k_bl_force; the Coulomb virial goes to P_COUL.
#include <hip/hip_runtime.h>

#include "md_eam_body.h"
#include "md_eam_coul.h"

__global__ __launch_bounds__(ROW_FORCE_TPB) void k_ec_density(const SimDev *sims, const RowView *views, const EamView *aux) {
  const RowView V = views[blockIdx.y];
  if ((int)(blockIdx.x * ROW_TILE) >= V.n) return;   // (the whole workgroup)
  eam_density_body<0, false>(V, (EamTab)V.tab + EC_EAM_OFF, aux[blockIdx.y].fp);
}

__global__ __launch_bounds__(ROW_FORCE_TPB) void k_ec_force(const SimDev *sims, const RowView *views, const EamView *aux, const BlView *bls) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const BlTable ROW_G *T = (const BlTable ROW_G *)V.tab;
  const EamTab blk = (EamTab)V.tab + EC_EAM_OFF;
  const double ROW_G *fp = aux[blockIdx.y].fp;
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  const double MD_G *q = S.q;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ EamHead s_hd;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<int>(&s_hd, blk);   // (offsets are read per lane, by the partner's element)
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int nr = s_hd.nr;
  const double rdr = s_hd.rdr, cut2 = s_hd.cut2;
  const double kc = T->bd.k, cut_coul = T->bd.cut_coul, cutmax2 = T->bd.cutmax * T->bd.cutmax, g = bls[blockIdx.y].g;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // half the pair energies phi, real-space Coulomb energy, (the density pass), ordered pairs inside cut_coul
  double we[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ic = min(i, n - 1);
    const int ti = V.stype[ic];
    const double fpi = fp[ic], qi = q[ic];
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      if (!(r2 < cutmax2 && r2 > 0.0)) return;
      const double r = sqrt(r2);
      double fe = 0.0, ec, fc;
      if (r2 < cut2) {
        double phi, fa, fb;
        eam_entry(blk, s_hd, nr, rdr, ti, V.stype[j], r, fpi, fp[j], &phi, &fa, &fb);
        fe = fa + fb;
        esum[0] += 0.5 * phi;
      }
      bl_coul(kc, cut_coul, g, qi, q[j], r, &ec, &fc);
      if (r < cut_coul) esum[3] += 1.0;
      const double fpair = fe + fc;
      fi0 -= d0 * fpair; fi1 -= d1 * fpair; fi2 -= d2 * fpair;   // (x_i - x_j = -d)
      esum[1] += 0.5 * ec;
      rowf_virial(we, 0.5 * fe, d0, d1, d2);
      rowf_virial(wc, 0.5 * fc, d0, d1, d2);
    });
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (i < n && l16 == 0) { V.f[3 * i] = fi0; V.f[3 * i + 1] = fi1; V.f[3 * i + 2] = fi2; }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(we, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wc, &sc.vir[P_COUL * 6], s_red);
}

void mdk_ec_real(hipStream_t st, dim3 gt, const SimDev *d, const RowView *v, const EamView *a, const BlView *b) {
  hipLaunchKernelGGL(k_ec_density, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
  hipLaunchKernelGGL(k_ec_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a, b);
}
