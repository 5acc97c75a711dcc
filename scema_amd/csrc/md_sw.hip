// md_sw.hip -- gfx950 kernel of the Stillinger-Weber force stage (`pair_style sw`: the reference's examples/streched_polyhedron, 192-atom
// silicon replicas under lammps_scripts_sisw).  The neighbour rows, the launch sequence and k_row_finish (energies and fault bits into the
// engine's scalars) are those of the row part (mdk_row_forces, md_rows.hip).  One launch covers every replica of the batch (blockIdx.y).
//   k_sw_force ..... pair and triplet terms (sw/sw_core.h) around a central atom, forces summed in LDS (skeleton: md_rowforce.h)
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_rowforce.h"
#include "md_sw.h"

static_assert(ROW_TILE == 64, "tile shape of md_sw.hip");

// Forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.  The group first
// filters the atom's row to the entries INSIDE their pair cutoff -- vector, distance and the radial factor of a triplet arm, computed once
// per neighbour -- into LDS (rowf_filter, md_rowforce.h); only these reach an exponential.  Then its lanes take the pairs the atom owns
// (sw_owns: each pair once) and the triplets (a < b) of the filtered list.  Forces go into the LDS table or to global memory (LACC,
// md_rowforce.h).  Energies, virial and counts are summed per workgroup.
template <bool LACC>
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_sw_force(const SimDev *sims, const RowView *views) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const SwTable ROW_G *tab = (const SwTable ROW_G *)V.tab;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ SwPairP s_pair[SW_MAXEL * SW_MAXEL];
  __shared__ SwTripP s_trip[SW_MAXEL * SW_MAXEL * SW_MAXEL];
  __shared__ double s_nb[6][ROW_NGRP][ROW_MAXIN];   // d (3), r, arm factor, d(arm exponent)/dr
  __shared__ int s_ent[ROW_NGRP][ROW_MAXIN], s_tj[ROW_NGRP][ROW_MAXIN];
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += ROW_FORCE_TPB) ((double *)s_pair)[k] = ((const double ROW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += ROW_FORCE_TPB) ((double *)s_trip)[k] = ((const double ROW_G *)&tab->trip[0])[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // e2, e3, pairs, triplets
  double w2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) { rowf_add<LACC>(V.f, np, a, g0, g1, g2); };
  bool crowded = false;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ti = V.stype[min(i, n - 1)];
    const int nn = rowf_filter(
        V, s_sh, i, ti, l16, shift16, crowded, [&](int a, int b) __attribute__((always_inline)) { return s_pair[a * SW_MAXEL + b].cut; },
        [&](int pos, int ent, int tj, double d0, double d1, double d2, double r) __attribute__((always_inline)) {
          double ex, da;
          sw_arm(s_pair[ti * SW_MAXEL + tj], r, &ex, &da);
          s_nb[0][grp][pos] = d0; s_nb[1][grp][pos] = d1; s_nb[2][grp][pos] = d2; s_nb[3][grp][pos] = r; s_nb[4][grp][pos] = ex; s_nb[5][grp][pos] = da;
          s_ent[grp][pos] = ent; s_tj[grp][pos] = tj;
        });
    __syncthreads();   // the groups' lists are complete
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    for (int m = l16; m < nn; m += 16) {
      const int ent = s_ent[grp][m];
      if (!sw_owns(i, ent)) continue;
      const double d0 = s_nb[0][grp][m], d1 = s_nb[1][grp][m], d2 = s_nb[2][grp][m];
      double e, fp;
      sw_two(s_pair[ti * SW_MAXEL + s_tj[grp][m]], s_nb[3][grp][m], &e, &fp);
      const double g0 = fp * d0, g1 = fp * d1, g2 = fp * d2;   // force on the partner
      add_force(ent & ROW_JMASK, g0, g1, g2);
      fi0 -= g0; fi1 -= g1; fi2 -= g2;
      esum[0] += e; esum[2] += 1.0;
      w2[0] += d0 * g0; w2[1] += d1 * g1; w2[2] += d2 * g2; w2[3] += d0 * g1; w2[4] += d0 * g2; w2[5] += d1 * g2;
    }
    const int ntrip = nn * (nn - 1) / 2;
    for (int t = l16; t < ntrip; t += 16) {
      // t -> (a, b), a < b < nn: t = b (b - 1) / 2 + a
      int b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
      while (b * (b - 1) / 2 > t) b--;
      while ((b + 1) * b / 2 <= t) b++;
      const int a = t - b * (b - 1) / 2;
      const double da_[3] = {s_nb[0][grp][a], s_nb[1][grp][a], s_nb[2][grp][a]}, db_[3] = {s_nb[0][grp][b], s_nb[1][grp][b], s_nb[2][grp][b]};
      double e, fj[3], fk[3];
      sw_three(s_trip[(ti * SW_MAXEL + s_tj[grp][a]) * SW_MAXEL + s_tj[grp][b]], da_, s_nb[3][grp][a], s_nb[4][grp][a], s_nb[5][grp][a], db_, s_nb[3][grp][b],
               s_nb[4][grp][b], s_nb[5][grp][b], &e, fj, fk);
      add_force(s_ent[grp][a] & ROW_JMASK, fj[0], fj[1], fj[2]);
      add_force(s_ent[grp][b] & ROW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      esum[1] += e; esum[3] += 1.0;
      w3[0] += da_[0] * fj[0] + db_[0] * fk[0]; w3[1] += da_[1] * fj[1] + db_[1] * fk[1]; w3[2] += da_[2] * fj[2] + db_[2] * fk[2];
      w3[3] += da_[0] * fj[1] + db_[0] * fk[1]; w3[4] += da_[0] * fj[2] + db_[0] * fk[2]; w3[5] += da_[1] * fj[2] + db_[1] * fk[2];
    }
    rowf_add_own<LACC>(V, np, i, l16, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  rowf_finish<LACC>(V, sc, np, crowded, esum, w2, w3, s_red);
}

void mdk_sw_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_sw_force<true>, k_sw_force<false>);
}
