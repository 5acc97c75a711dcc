// md_ionic_force.h -- the real-space force kernel of the ionic stages (k_bd_force, md_born_dsf.hip; k_bl_force, md_born_long.hip): one
// body on the gather skeleton of md_rowforce.h.  Device code.
#pragma once
#include "ionic/bd_core.h"
#include "md_kernels.h"
#include "md_rowforce.h"

// A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time, a lane per entry of its
// row inside cutmax (rowf_walk).  Half of a pair's energies and half of its virial go to each end; the group's sum is the atom's force,
// stored once.  Plain FP64 erfc and exp.  Table is the stage's table (RowView::tab, copied into LDS as doubles); Terms tells the stages
// apart:
//   const BdTable &bd(const Table &)                                       where the Born table sits in it
//   void pair(const Table &, const BdPairP &, qi, qj, r2, *eb, *ec, *fb, *fc)   the pair term (bd_pair, bl_pair)
//   void self(const Table &, qi, double &ecoul)                            what the group's first lane adds for the atom itself
template <class Table, class Terms>
__device__ __forceinline__ void ionic_force(const SimDev *sims, const RowView *views, const Terms terms) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  const double MD_G *q = S.q;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ Table s_tab;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<double>(&s_tab, V.tab);
  __syncthreads();
  const BdTable &B = terms.bd(s_tab);
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const double cutmax2 = B.cutmax * B.cutmax, cut_coul = B.cut_coul;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // Born energy, Coulomb energy (real space, with the self term), ordered pairs inside cutmax, inside cut_coul
  double wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ic = min(i, n - 1);
    const int ti = min(max(V.stype[ic], 0), BD_MAXEL - 1);
    const double qi = q[ic];
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      if (!(r2 < cutmax2 && r2 > 0.0)) return;
      const int tj = min(max(V.stype[j], 0), BD_MAXEL - 1);
      double eb, ec, fb, fc;
      terms.pair(s_tab, B.pair[ti * BD_MAXEL + tj], qi, q[j], r2, &eb, &ec, &fb, &fc);
      const double fpair = fb + fc;
      fi0 -= d0 * fpair; fi1 -= d1 * fpair; fi2 -= d2 * fpair;   // (x_i - x_j = -d)
      esum[0] += 0.5 * eb; esum[1] += 0.5 * ec; esum[2] += 1.0;
      if (sqrt(r2) < cut_coul) esum[3] += 1.0;
      rowf_virial(wb, 0.5 * fb, d0, d1, d2);
      rowf_virial(wc, 0.5 * fc, d0, d1, d2);
    });
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (i < n && l16 == 0) {
      V.f[3 * i] = fi0; V.f[3 * i + 1] = fi1; V.f[3 * i + 2] = fi2;
      terms.self(s_tab, qi, esum[1]);
    }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wc, &sc.vir[P_COUL * 6], s_red);
}
