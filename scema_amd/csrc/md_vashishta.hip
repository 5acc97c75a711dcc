// md_vashishta.hip -- gfx950 kernel of the Vashishta force stage (`pair_style vashishta`: SiC, SiO2, Al2O3, InP).  The neighbour rows, the
// launch sequence and k_row_finish (energies and fault bits into the engine's scalars) are those of the row part (mdk_row_forces,
// md_rows.hip).  One launch covers every replica of the batch (blockIdx.y).
//   k_vs_force ..... pair terms over every entry inside rc and triplet terms over the few inside r0 (vashishta/vs_core.h) around a
//                    central atom, in one walk of its row (skeleton: md_rowforce.h)
// The potential has two ranges: the screened-Coulomb pair term reaches rc (7.35 A in SiC: 158 neighbours), the three-body term r0 (2.90 A:
// 4 neighbours).  The list of ROW_MAXIN entries in LDS therefore holds the entries inside r0 alone; the pair term is evaluated in place,
// at any count.
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_rowforce.h"
#include "md_vashishta.h"

static_assert(ROW_TILE == 64, "tile shape of md_vashishta.hip");

// Forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.  The group walks
// the atom's row once, a lane per entry.  An entry inside rc of its pair takes the pair term where it stands, as k_eam_force does: rows
// are full, so each end of a pair sums its own force, with half of the pair's energy and half of its virial -- no atomic for the 158
// pairs of an atom.  In the same trip an entry inside r0 of its pair goes to the group's list in LDS, in the row's order (ballot order),
// with vector, distance and the radial factor of a triplet arm; only these reach the arm's exponential.  Then the lanes take the triplets
// (a < b) of the list as k_sw_force does: forces on the two partners go into the LDS table or to global memory (LACC, md_rowforce.h), the
// central atom's share joins its pair forces in the group's sum.  Energies, virial and counts are summed per workgroup.  More than
// ROW_MAXIN entries inside r0 set the crowded bit; the number inside rc is not limited.
template <bool LACC>
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_vs_force(const SimDev *sims, const RowView *views) {
  const RowView V = views[blockIdx.y];
  const int n = V.n, cap = V.cap;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const VsTable ROW_G *tab = (const VsTable ROW_G *)V.tab;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ VsPairP s_pair[VS_MAXEL * VS_MAXEL];
  __shared__ VsTripP s_trip[VS_MAXEL * VS_MAXEL * VS_MAXEL];
  __shared__ double s_nb[6][ROW_NGRP][ROW_MAXIN];   // d (3), r, arm factor, d(arm exponent)/dr
  __shared__ int s_ent[ROW_NGRP][ROW_MAXIN], s_tj[ROW_NGRP][ROW_MAXIN];
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  static_assert(sizeof(s_sh) + sizeof(s_pair) + sizeof(s_trip) + sizeof(s_nb) + sizeof(s_ent) + sizeof(s_tj) + sizeof(s_red) + 3 * ROW_LDS_MAXPAD * 8 < 65536,
                "LDS of k_vs_force with the force table of ROW_LDS_MAXPAD atoms");
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += ROW_FORCE_TPB) ((double *)s_pair)[k] = ((const double ROW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += ROW_FORCE_TPB) ((double *)s_trip)[k] = ((const double ROW_G *)&tab->trip[0])[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // e2, e3, ordered pairs inside rc, pairs (a, b) of the lists inside r0
  double w2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) { rowf_add<LACC>(V.f, np, a, g0, g1, g2); };
  bool crowded = false;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    const int ti = V.stype[ic];
    const int cnt = valid ? min(V.cnt[ic], cap) : 0;   // (a group past the replica's last atom walks nothing)
    const double xi0 = V.x[3 * ic], xi1 = V.x[3 * ic + 1], xi2 = V.x[3 * ic + 2];
    const size_t base = (size_t)ic * cap;
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    int nn = 0;
    // the walk: a lane per entry, 16 entries a trip
    for (int c0 = 0; c0 < cnt; c0 += 16) {
      const int c = c0 + l16;
      int ent = (c < cnt) ? V.rows[base + c] : -1;
      bool arm = false;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, r = 1.0;
      int tj = 0;
      if (ent >= 0) {
        const int j = min(ent & ROW_JMASK, n - 1), code = min((ent >> 24) & 0x7F, ROW_NSHIFT - 1);
        ent = j | (code << 24);   // (what the builder wrote; nothing else is ever used as an index)
        const double *sh = s_sh + 3 * code;
        d0 = V.x[3 * j] - xi0 + sh[0]; d1 = V.x[3 * j + 1] - xi1 + sh[1]; d2 = V.x[3 * j + 2] - xi2 + sh[2];
        tj = V.stype[j];
        const VsPairP &P = s_pair[ti * VS_MAXEL + tj];
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2;
        r = sqrt(r2);
        if (r2 > 0.0 && r < P.rc) {   // the pair term, this end's half
          double e, fp;
          vs_two(P, r, &e, &fp);
          fi0 -= fp * d0; fi1 -= fp * d1; fi2 -= fp * d2;   // (x_i - x_j = -d)
          esum[0] += 0.5 * e; esum[2] += 1.0;
          const double hf = 0.5 * fp;
          w2[0] += hf * d0 * d0; w2[1] += hf * d1 * d1; w2[2] += hf * d2 * d2; w2[3] += hf * d0 * d1; w2[4] += hf * d0 * d2; w2[5] += hf * d1 * d2;
        }
        arm = r2 > 0.0 && r < P.r0;   // (the strict test: an arm at or beyond its r0 never reaches the exponential; r0 = 0: never an arm)
      }
      const unsigned m16 = (unsigned)(__ballot(arm) >> shift16) & 0xFFFFu;
      const int pos = nn + __popc(m16 & ((1u << l16) - 1u));
      if (arm && pos < ROW_MAXIN) {
        double ex, da;
        vs_arm(s_pair[ti * VS_MAXEL + tj], r, &ex, &da);
        s_nb[0][grp][pos] = d0; s_nb[1][grp][pos] = d1; s_nb[2][grp][pos] = d2; s_nb[3][grp][pos] = r; s_nb[4][grp][pos] = ex; s_nb[5][grp][pos] = da;
        s_ent[grp][pos] = ent; s_tj[grp][pos] = tj;
      }
      nn += __popc(m16);
    }
    if (nn > ROW_MAXIN) { crowded = true; nn = ROW_MAXIN; }
    __syncthreads();   // the groups' lists are complete
    const int ntrip = nn * (nn - 1) / 2;
    for (int t = l16; t < ntrip; t += 16) {
      // t -> (a, b), a < b < nn: t = b (b - 1) / 2 + a
      int b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
      while (b * (b - 1) / 2 > t) b--;
      while ((b + 1) * b / 2 <= t) b++;
      const int a = t - b * (b - 1) / 2;
      esum[3] += 1.0;
      const VsTripP &Q = s_trip[(ti * VS_MAXEL + s_tj[grp][a]) * VS_MAXEL + s_tj[grp][b]];
      if (Q.b == 0.0) continue;   // (SiC: the triplets around a like pair of arms only)
      const double da_[3] = {s_nb[0][grp][a], s_nb[1][grp][a], s_nb[2][grp][a]}, db_[3] = {s_nb[0][grp][b], s_nb[1][grp][b], s_nb[2][grp][b]};
      double e, fj[3], fk[3];
      vs_three(Q, da_, s_nb[3][grp][a], s_nb[4][grp][a], s_nb[5][grp][a], db_, s_nb[3][grp][b], s_nb[4][grp][b], s_nb[5][grp][b], &e, fj, fk);
      add_force(s_ent[grp][a] & ROW_JMASK, fj[0], fj[1], fj[2]);
      add_force(s_ent[grp][b] & ROW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      esum[1] += e;
      w3[0] += da_[0] * fj[0] + db_[0] * fk[0]; w3[1] += da_[1] * fj[1] + db_[1] * fk[1]; w3[2] += da_[2] * fj[2] + db_[2] * fk[2];
      w3[3] += da_[0] * fj[1] + db_[0] * fk[1]; w3[4] += da_[0] * fj[2] + db_[0] * fk[2]; w3[5] += da_[1] * fj[2] + db_[1] * fk[2];
    }
    rowf_add_own<LACC>(V, np, i, l16, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  rowf_finish<LACC>(V, sc, np, crowded, esum, w2, w3, s_red);
}

void mdk_vs_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_vs_force<true>, k_vs_force<false>);
}
