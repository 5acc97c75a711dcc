// md_edip.hip -- gfx950 kernel of the EDIP force stage (`pair_style edip`, `pair_style edip/multi`: silicon past yield, SiC).  The neighbour
// rows, the launch sequence and k_row_finish (energies and fault bits into the engine's scalars) are those of the row part
// (mdk_row_forces, md_rows.hip).  One launch covers every replica of the batch (blockIdx.y).
//   k_edip_force ... coordination, pair, triplet and coordination-force terms (edip/edip_core.h) around a central atom, forces summed
//                    in LDS (skeleton: md_rowforce.h)
// Every energy term around atom i depends on Z_i, the smooth count of i's neighbours, so the force has a part no other stage has:
// (dE_i/dZ_i) f'(r_im) on every neighbour m, which can be applied only after all pairs and triplets around i have been summed.  All of
// it stands on i's own row.
#include <hip/hip_runtime.h>

#include "md_edip.h"
#include "md_kernels.h"
#include "md_rowforce.h"

static_assert(ROW_TILE == 64, "tile shape of md_edip.hip");

// Forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.
//   1. The group filters the atom's row to the entries INSIDE a of their pair (rowf_filter) and keeps vector, distance, f', the arm g and
//      its slope with each; only these reach an exponential.  Z_i is the group's sum of f.
//   2. A lane per entry takes V2(r, Z_i) (every entry: the pair sum is over ordered pairs, so no atom "owns" a pair), a lane per pair of
//      entries (a < b) the triplet.  Forces on partners at fixed Z_i go into the LDS table or to global memory (LACC, md_rowforce.h);
//      each lane sums its share of dE_i/dZ_i.
//   3. That sum over the group, then a lane per entry once more: (dE_i/dZ_i) f'(r) along the entry's vector.  Entries inside c have
//      f' = 0 and are skipped -- in diamond silicon all of them.
// Energies, virial and counts are summed per workgroup.  More than ROW_MAXIN entries inside a set the crowded bit.
template <bool LACC>
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_edip_force(const SimDev *sims, const RowView *views) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const EdipTable ROW_G *tab = (const EdipTable ROW_G *)V.tab;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ EdipPairP s_pair[EDIP_MAXEL * EDIP_MAXEL];
  __shared__ EdipTripP s_trip[EDIP_MAXEL * EDIP_MAXEL * EDIP_MAXEL];
  __shared__ double s_nb[7][ROW_NGRP][ROW_MAXIN];   // d (3), r, f', arm g, g'/g
  __shared__ int s_jt[ROW_NGRP][ROW_MAXIN];         // partner (ROW_JMASK) and its element (from bit 24)
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  static_assert(sizeof(s_sh) + sizeof(s_pair) + sizeof(s_trip) + sizeof(s_nb) + sizeof(s_jt) + sizeof(s_red) + 3 * ROW_LDS_MAXPAD * 8 < 65536,
                "LDS of k_edip_force with the force table of ROW_LDS_MAXPAD atoms");
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += ROW_FORCE_TPB) ((double *)s_pair)[k] = ((const double ROW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += ROW_FORCE_TPB) ((double *)s_trip)[k] = ((const double ROW_G *)&tab->trip[0])[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // e2, e3, ordered pairs inside a, triplets
  double w2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) { rowf_add<LACC>(V.f, np, a, g0, g1, g2); };
  bool crowded = false;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ti = V.stype[min(i, n - 1)];
    double z = 0.0;
    const int nn = rowf_filter(
        V, s_sh, i, ti, l16, shift16, crowded, [&](int a, int b) __attribute__((always_inline)) { return s_pair[a * EDIP_MAXEL + b].a; },
        [&](int pos, int ent, int tj, double d0, double d1, double d2, double r) __attribute__((always_inline)) {
          const EdipPairP &P = s_pair[ti * EDIP_MAXEL + tj];
          double f, df, g, da;
          edip_f(P, r, &f, &df);
          edip_arm(P, r, &g, &da);
          z += f;
          s_nb[0][grp][pos] = d0; s_nb[1][grp][pos] = d1; s_nb[2][grp][pos] = d2; s_nb[3][grp][pos] = r;
          s_nb[4][grp][pos] = df; s_nb[5][grp][pos] = g; s_nb[6][grp][pos] = da;
          s_jt[grp][pos] = (ent & ROW_JMASK) | (tj << 24);
        });
    z = row_sum(z);   // Z_i
    __syncthreads();   // the groups' lists are complete
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0, dz = 0.0;
    for (int m = l16; m < nn; m += 16) {
      const int jt = s_jt[grp][m];
      const double d0 = s_nb[0][grp][m], d1 = s_nb[1][grp][m], d2 = s_nb[2][grp][m], r = s_nb[3][grp][m];
      double e, de_dr, de_dz;
      edip_v2(s_pair[ti * EDIP_MAXEL + (jt >> 24)], r, z, &e, &de_dr, &de_dz);
      const double fp = -de_dr / r;
      const double g0 = fp * d0, g1 = fp * d1, g2 = fp * d2;   // force on the partner at fixed Z_i
      add_force(jt & ROW_JMASK, g0, g1, g2);
      fi0 -= g0; fi1 -= g1; fi2 -= g2;
      dz += de_dz;
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
      const int ja = s_jt[grp][a], jb = s_jt[grp][b];
      const double da_[3] = {s_nb[0][grp][a], s_nb[1][grp][a], s_nb[2][grp][a]}, db_[3] = {s_nb[0][grp][b], s_nb[1][grp][b], s_nb[2][grp][b]};
      double e, fj[3], fk[3], de_dz;
      edip_three(s_trip[(ti * EDIP_MAXEL + (ja >> 24)) * EDIP_MAXEL + (jb >> 24)], z, da_, s_nb[3][grp][a], s_nb[5][grp][a], s_nb[6][grp][a], db_,
                 s_nb[3][grp][b], s_nb[5][grp][b], s_nb[6][grp][b], &e, fj, fk, &de_dz);
      add_force(ja & ROW_JMASK, fj[0], fj[1], fj[2]);
      add_force(jb & ROW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      dz += de_dz;
      esum[1] += e; esum[3] += 1.0;
      w3[0] += da_[0] * fj[0] + db_[0] * fk[0]; w3[1] += da_[1] * fj[1] + db_[1] * fk[1]; w3[2] += da_[2] * fj[2] + db_[2] * fk[2];
      w3[3] += da_[0] * fj[1] + db_[0] * fk[1]; w3[4] += da_[0] * fj[2] + db_[0] * fk[2]; w3[5] += da_[1] * fj[2] + db_[1] * fk[2];
    }
    dz = row_sum(dz);   // dE_i/dZ_i
    for (int m = l16; m < nn; m += 16) {
      const double df = s_nb[4][grp][m];
      if (df == 0.0) continue;   // (inside c, or next to a where f' underflows)
      const double d0 = s_nb[0][grp][m], d1 = s_nb[1][grp][m], d2 = s_nb[2][grp][m];
      const double fp = -dz * df / s_nb[3][grp][m];
      const double g0 = fp * d0, g1 = fp * d1, g2 = fp * d2;   // force on the neighbour through Z_i
      add_force(s_jt[grp][m] & ROW_JMASK, g0, g1, g2);
      fi0 -= g0; fi1 -= g1; fi2 -= g2;
      w3[0] += d0 * g0; w3[1] += d1 * g1; w3[2] += d2 * g2; w3[3] += d0 * g1; w3[4] += d0 * g2; w3[5] += d1 * g2;
    }
    rowf_add_own<LACC>(V, np, i, l16, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  rowf_finish<LACC>(V, sc, np, crowded, esum, w2, w3, s_red);
}

void mdk_edip_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_edip_force<true>, k_edip_force<false>);
}
