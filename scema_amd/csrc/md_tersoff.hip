// md_tersoff.hip -- gfx950 kernels of the Tersoff force stage (`pair_style tersoff`, and its forms `tersoff/mod`, `tersoff/mod/c`,
// `tersoff/zbl` as further instances of the same kernel).  The neighbour rows are those of the row part
// (mdk_rows_build, md_rows.hip: full rows inside the largest R + D + skin, image codes in the convention of the ReaxFF rows); the
// integrator, thermostat, fix deform, pressure sampling and the batch machinery are the ones of the OPLS path.  One launch covers every
// replica of the batch (blockIdx.y).
//   k_ts_force ..... pair terms, bond orders and their gradients (tersoff/ts_core.h) around a central atom, forces summed in LDS
// on the skeleton of md_rowforce.h; the row part, the launch shape and k_row_finish (energies and fault bits into the engine's scalars) come
// with mdk_row_forces (md_rows.hip).
// Engine parts: the repulsive term 1/2 fC fR and its virial go to P_LJ, everything that carries b_ij (1/2 fC b fA and the gradient of zeta)
// to P_ANGLE; of the forms, the c0 term of mod/c and the ZBL repulsion carry no b and go to P_LJ.  Only their sum enters the stress; the
// split is what scema_md_tersoff_debug_compute reports as e_rep and e_att.
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_rowforce.h"
#include "md_tersoff.h"

#include <type_traits>

// Forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.  The group first
// filters the atom's row to the entries INSIDE the cutoff under which the pair (i, k) is used -- vector, distance, fC and fC' of the pair,
// computed once per neighbour -- into LDS (rowf_filter, md_rowforce.h).  Pass 1, a lane per neighbour j: zeta_ij over the other
// entries, b and b', the pair term at fixed b and its force, and pref_j = 1/2 fC fA b' left in LDS (in the slot of fC', which nothing reads
// any more).  The pair term is not owned by one end: V_ij != V_ji, every atom does all of its own ordered pairs.  Pass 2, the lanes over
// the nn (nn - 1) ordered (j, k): pref_j d zeta_ij / d(x_j, x_k) onto j and k.  Forces go into the LDS table or to global memory (LACC,
// md_rowforce.h).  Energies, virial and counts are summed per workgroup.
// The form is the kernel's table type (TsTable: plain; TsModTable: tersoff/mod and mod/c; TsZblTable: tersoff/zbl): the pair and triplet
// records in LDS are the table's, and ts_pair_fc, ts_pair_cut, ts_bond_order, ts_pair, ts_zeta_term and ts_zeta_force are chosen by their
// types (tersoff/ts_core.h).  Nothing else differs, so the plain instances compile to the code they had before the forms came.
template <class Table, bool LACC>
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_ts_force(const SimDev *sims, const RowView *views) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  typedef typename std::remove_extent<decltype(Table::pair)>::type PairP;   // (the form's records: TsPairP / TsModPairP / TsZblPairP,
  typedef typename std::remove_extent<decltype(Table::trip)>::type TripP;   //  TsTripP / TsModTripP)
  // (a load of its own, which the compiler may not merge: read as V.tab the pointer joins stype, x, f, cnt, rows, eacc and stat in one
  // 16-dword scalar load, a tuple this kernel's SGPR spilling then reloads whole around every use -- 312 v_readlane for 200, 1 % of an update)
  const Table ROW_G *tab = (const Table ROW_G *)__atomic_load_n(&views[blockIdx.y].tab, __ATOMIC_RELAXED);
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ PairP s_pair[TS_MAXEL * TS_MAXEL];
  __shared__ TripP s_trip[TS_MAXEL * TS_MAXEL * TS_MAXEL];
  __shared__ double s_cutin[TS_MAXEL * TS_MAXEL];
  __shared__ double s_nb[6][ROW_NGRP][ROW_MAXIN];   // d (3), r, fC of the pair, fC' of the pair -> pref after pass 1
  __shared__ int s_ent[ROW_NGRP][ROW_MAXIN], s_tj[ROW_NGRP][ROW_MAXIN];
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += ROW_FORCE_TPB) ((double *)s_pair)[k] = ((const double ROW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += ROW_FORCE_TPB) ((double *)s_trip)[k] = ((const double ROW_G *)&tab->trip[0])[k];
  for (int k = threadIdx.x; k < TS_MAXEL * TS_MAXEL; k += ROW_FORCE_TPB) s_cutin[k] = tab->cutin[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // repulsive, bond-order energy, ordered pairs, ordered (j, k)
  double wr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) { rowf_add<LACC>(V.f, np, a, g0, g1, g2); };
  bool crowded = false;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ti = V.stype[min(i, n - 1)];
    const int nn = rowf_filter(
        V, s_sh, i, ti, l16, shift16, crowded, [&](int a, int b) __attribute__((always_inline)) { return s_cutin[a * TS_MAXEL + b]; },
        [&](int pos, int ent, int tj, double d0, double d1, double d2, double r) __attribute__((always_inline)) {
          const PairP &P = s_pair[ti * TS_MAXEL + tj];
          double fc = 0.0, dfc = 0.0;
          if (r < ts_pair_cut(P)) ts_pair_fc(P, r, &fc, &dfc);   // (a pair at or beyond its R + D: a third atom only)
          s_nb[0][grp][pos] = d0; s_nb[1][grp][pos] = d1; s_nb[2][grp][pos] = d2; s_nb[3][grp][pos] = r; s_nb[4][grp][pos] = fc; s_nb[5][grp][pos] = dfc;
          s_ent[grp][pos] = ent; s_tj[grp][pos] = tj;
        });
    __syncthreads();   // the groups' lists are complete
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    // pass 1: a lane per neighbour j
    for (int m = l16; m < nn; m += 16) {
      const int tj = s_tj[grp][m];
      const PairP &P = s_pair[ti * TS_MAXEL + tj];
      const double r1 = s_nb[3][grp][m];
      double pref = 0.0;
      if (r1 < ts_pair_cut(P)) {
        const double dj[3] = {s_nb[0][grp][m], s_nb[1][grp][m], s_nb[2][grp][m]};
        double zeta = 0.0;
        for (int k = 0; k < nn; k++) {
          if (k == m) continue;
          const TripP &Q = s_trip[(ti * TS_MAXEL + tj) * TS_MAXEL + s_tj[grp][k]];
          const double r2 = s_nb[3][grp][k];
          if (!(r2 < Q.cut)) continue;
          const double dk[3] = {s_nb[0][grp][k], s_nb[1][grp][k], s_nb[2][grp][k]};
          zeta += ts_zeta_term(Q, dj, r1, dk, r2);
        }
        double b, db, erep, eatt, fprep, fpatt, fa;
        ts_bond_order(P, zeta, &b, &db);
        const double fc = s_nb[4][grp][m];
        ts_pair(P, r1, fc, s_nb[5][grp][m], b, &erep, &eatt, &fprep, &fpatt, &fa);
        pref = 0.5 * fc * fa * db;
        const double fp = fprep + fpatt;
        const double g0 = fp * dj[0], g1 = fp * dj[1], g2 = fp * dj[2];   // force on the partner
        add_force(s_ent[grp][m] & ROW_JMASK, g0, g1, g2);
        fi0 -= g0; fi1 -= g1; fi2 -= g2;
        esum[0] += erep; esum[1] += eatt; esum[2] += 1.0;
        const double q0 = fprep * dj[0], q1 = fprep * dj[1], q2 = fprep * dj[2];
        wr[0] += dj[0] * q0; wr[1] += dj[1] * q1; wr[2] += dj[2] * q2; wr[3] += dj[0] * q1; wr[4] += dj[0] * q2; wr[5] += dj[1] * q2;
        const double p0 = fpatt * dj[0], p1 = fpatt * dj[1], p2 = fpatt * dj[2];
        wb[0] += dj[0] * p0; wb[1] += dj[1] * p1; wb[2] += dj[2] * p2; wb[3] += dj[0] * p1; wb[4] += dj[0] * p2; wb[5] += dj[1] * p2;
      }
      s_nb[5][grp][m] = pref;   // (only this lane read the slot's fC')
    }
    __syncthreads();   // every pref is in place
    // pass 2: the lanes over the ordered (j, k), k != j
    const int nk = nn - 1, nord = nn * nk;
    for (int t = l16; t < nord; t += 16) {
      const int j = t / nk, kk = t - j * nk;
      const int k = kk + (kk >= j ? 1 : 0);
      const int tj = s_tj[grp][j];
      const double r1 = s_nb[3][grp][j], r2 = s_nb[3][grp][k];
      const TripP &Q = s_trip[(ti * TS_MAXEL + tj) * TS_MAXEL + s_tj[grp][k]];
      if (!(r1 < ts_pair_cut(s_pair[ti * TS_MAXEL + tj])) || !(r2 < Q.cut)) continue;
      esum[3] += 1.0;
      const double pref = s_nb[5][grp][j];
      if (pref == 0.0) continue;   // (b' = 0: the small-zeta end of b, or beta = 0)
      const double dj[3] = {s_nb[0][grp][j], s_nb[1][grp][j], s_nb[2][grp][j]}, dk[3] = {s_nb[0][grp][k], s_nb[1][grp][k], s_nb[2][grp][k]};
      double fj[3], fk[3];
      ts_zeta_force(Q, pref, dj, r1, dk, r2, fj, fk);
      add_force(s_ent[grp][j] & ROW_JMASK, fj[0], fj[1], fj[2]);
      add_force(s_ent[grp][k] & ROW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      wb[0] += dj[0] * fj[0] + dk[0] * fk[0]; wb[1] += dj[1] * fj[1] + dk[1] * fk[1]; wb[2] += dj[2] * fj[2] + dk[2] * fk[2];
      wb[3] += dj[0] * fj[1] + dk[0] * fk[1]; wb[4] += dj[0] * fj[2] + dk[0] * fk[2]; wb[5] += dj[1] * fj[2] + dk[1] * fk[2];
    }
    rowf_add_own<LACC>(V, np, i, l16, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  rowf_finish<LACC>(V, sc, np, crowded, esum, wr, wb, s_red);
}

void mdk_ts_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_ts_force<TsTable, true>, k_ts_force<TsTable, false>);
}

// Static LDS of the forms' instances: the mod form's triplet record is 88 B against 72 B (+1 024 B), the ZBL pair record 136 B against
// 104 B (+512 B).  With the force table of ROW_LDS_MAXPAD atoms (24 576 B) that is 63 936 B and 63 424 B: both forms keep the limit of
// the plain one.
static_assert(sizeof(TsModPairP) * TS_MAXEL * TS_MAXEL + sizeof(TsModTripP) * TS_MAXEL * TS_MAXEL * TS_MAXEL + 32064 + 3 * ROW_LDS_MAXPAD * 8 < 65536 &&
                  sizeof(TsZblPairP) * TS_MAXEL * TS_MAXEL + sizeof(TsTripP) * TS_MAXEL * TS_MAXEL * TS_MAXEL + 32064 + 3 * ROW_LDS_MAXPAD * 8 < 65536,
              "LDS of k_ts_force with the force table of ROW_LDS_MAXPAD atoms");

void mdk_ts_mod_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_ts_force<TsModTable, true>, k_ts_force<TsModTable, false>);
}

void mdk_ts_zbl_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_ts_force<TsZblTable, true>, k_ts_force<TsZblTable, false>);
}
