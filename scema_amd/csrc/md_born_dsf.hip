// md_born_dsf.hip -- gfx950 kernel of the ionic force stage (`pair_style born/coul/dsf`: rock-salt halides, MgO, UO2, Buckingham and
// Born-Mayer-Huggins models of oxides and glasses), the first row stage that reads a charge.  The neighbour rows are those of the row
// part (mdk_rows_build, md_rows.hip: full rows inside cutmax + skin, sorted by partner, image codes in the convention of the ReaxFF
// rows); the integrator, thermostat, fix deform, pressure sampling and the batch machinery are the ones of the OPLS path.  One launch
// covers every replica of the batch (blockIdx.y).
//   k_bd_force ..... the Born term and the damped-shifted-force Coulomb term (ionic/bd_core.h) over every entry of an atom's row inside
//                    cutmax, in the shape of k_eam_force (md_eam.hip)
// between the row part and k_row_finish.  With full rows every atom sums its own force: no atomic on a force, rows are sorted and the
// sum over a group has a fixed order, so two evaluations of one state give the same forces bit for bit.  Nothing is kept in a list of
// ROW_MAXIN: any number of neighbours is taken (rock salt has about 190 inside 10 A).
// Engine parts: the virial of the Born term goes to P_LJ, that of the Coulomb term to P_COUL; the energies reach SimScalars through
// k_row_finish, which the row stages share (eacc[0] -> eng[P_LJ], eacc[1] -> eng[P_ANGLE]).  Only the sums enter the stress and the
// total energy; the split is what scema_md_born_dsf_debug_compute reports as e_born and e_coul.
#include <hip/hip_runtime.h>

#include "md_born_dsf.h"
#include "md_kernels.h"
#include "md_rowforce.h"

// Forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time, a lane per
// entry of its row with the entry's image shift.  Index and image code are clamped to what the builder can have written.  A group past
// the replica's last atom (i >= n) walks nothing; no lane leaves, so the group sums see whole waves.  Half of a pair's energies and half
// of its virial go to each end; the group's first lane adds the atom's self energy.  Plain FP64 erfc and exp.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_bd_force(const SimDev *sims, const RowView *views) {
  const RowView V = views[blockIdx.y];
  const int n = V.n, cap = V.cap;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  const double MD_G *q = S.q;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ BdTable s_tab;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  static_assert(sizeof(BdTable) % 8 == 0, "BdTable is copied as doubles");
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(BdTable) / 8); k += ROW_FORCE_TPB) ((double *)&s_tab)[k] = ((const double ROW_G *)V.tab)[k];
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const double cutmax2 = s_tab.cutmax * s_tab.cutmax, cut_coul = s_tab.cut_coul;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // Born energy, Coulomb energy with the self term, ordered pairs inside cutmax, inside cut_coul
  double wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    const int ti = min(max(V.stype[ic], 0), BD_MAXEL - 1);
    const double qi = q[ic];
    const int cnt = valid ? min(V.cnt[ic], cap) : 0;
    const double xi0 = V.x[3 * ic], xi1 = V.x[3 * ic + 1], xi2 = V.x[3 * ic + 2];
    const size_t base = (size_t)ic * cap;
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    for (int c = l16; c < cnt; c += 16) {
      const int ent = V.rows[base + c];
      const int j = min(ent & ROW_JMASK, n - 1), code = min((ent >> 24) & 0x7F, ROW_NSHIFT - 1);
      const double *sh = s_sh + 3 * code;
      const double d0 = V.x[3 * j] - xi0 + sh[0], d1 = V.x[3 * j + 1] - xi1 + sh[1], d2 = V.x[3 * j + 2] - xi2 + sh[2];
      const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
      if (r2 < cutmax2 && r2 > 0.0) {
        const int tj = min(max(V.stype[j], 0), BD_MAXEL - 1);
        double eb, ec, fb, fc;
        bd_pair(s_tab, s_tab.pair[ti * BD_MAXEL + tj], qi, q[j], r2, &eb, &ec, &fb, &fc);
        const double fpair = fb + fc;
        fi0 -= d0 * fpair; fi1 -= d1 * fpair; fi2 -= d2 * fpair;   // (x_i - x_j = -d)
        esum[0] += 0.5 * eb; esum[1] += 0.5 * ec; esum[2] += 1.0;
        if (sqrt(r2) < cut_coul) esum[3] += 1.0;
        const double hb = 0.5 * fb, hc = 0.5 * fc;
        wb[0] += hb * d0 * d0; wb[1] += hb * d1 * d1; wb[2] += hb * d2 * d2; wb[3] += hb * d0 * d1; wb[4] += hb * d0 * d2; wb[5] += hb * d1 * d2;
        wc[0] += hc * d0 * d0; wc[1] += hc * d1 * d1; wc[2] += hc * d2 * d2; wc[3] += hc * d0 * d1; wc[4] += hc * d0 * d2; wc[5] += hc * d1 * d2;
      }
    }
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (valid && l16 == 0) {
      V.f[3 * i] = fi0; V.f[3 * i + 1] = fi1; V.f[3 * i + 2] = fi2;
      esum[1] += bd_self(s_tab, qi);
    }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wc, &sc.vir[P_COUL * 6], s_red);
}

void mdk_bd_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  if (ns <= 0 || maxatoms <= 0) return;
  const dim3 gt((unsigned)((maxatoms + ROW_TILE - 1) / ROW_TILE), (unsigned)ns, 1);
  mdk_rows_build(st, d, v, ns, maxatoms);
  hipLaunchKernelGGL(k_bd_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v);
  mdk_rows_finish(st, d, v, ns);
}
