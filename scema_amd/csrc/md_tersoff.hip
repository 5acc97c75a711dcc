// md_tersoff.hip -- gfx950 kernels of the Tersoff force stage (`pair_style tersoff`).  The neighbour rows are those of the Stillinger-Weber
// stage (mdk_sw_rows, md_sw.hip: full rows inside the largest R + D + skin, image codes in the convention of the ReaxFF rows); the
// integrator, thermostat, fix deform, pressure sampling and the batch machinery are the ones of the OPLS path.  One launch covers every
// replica of the batch (blockIdx.y).
//   k_ts_force ..... pair terms, bond orders and their gradients (tersoff/ts_core.h) around a central atom, forces summed in LDS
//   k_ts_finish .... energies and fault bits into the engine's scalars
// Engine parts: the repulsive term 1/2 fC fR and its virial go to P_LJ, everything that carries b_ij (1/2 fC b fA and the gradient of zeta)
// to P_ANGLE.  Only their sum enters the stress; the split is what scema_md_tersoff_debug_compute reports as e_rep and e_att.
#include <hip/hip_runtime.h>

#include "md_device.h"
#include "md_kernels.h"
#include "md_tersoff.h"
#include "md_types.h"

#define TS_NSHIFT 125
#define TS_FORCE_TPB 256     /* 16 groups of 16 lanes, a group per central atom */
#define TS_NGRP (TS_FORCE_TPB / 16)
static_assert(SW_TILE % TS_NGRP == 0 && TS_MAXIN <= 32, "tile shapes of md_tersoff.hip");

// LDS FP64 atomic add without return value (ds_add_f64)
__device__ __forceinline__ void ts_lds_add(double *p, double v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Forces.  A workgroup owns SW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.  The group first
// filters the atom's row to the entries INSIDE the cutoff under which the pair (i, k) is used -- vector, distance, fC and fC' of the pair,
// computed once per neighbour -- into LDS (ballot order: the row's order).  Pass 1, a lane per neighbour j: zeta_ij over the other
// entries, b and b', the pair term at fixed b and its force, and pref_j = 1/2 fC fA b' left in LDS (in the slot of fC', which nothing reads
// any more).  The pair term is not owned by one end: V_ij != V_ji, every atom does all of its own ordered pairs.  Pass 2, the lanes over
// the nn (nn - 1) ordered (j, k): pref_j d zeta_ij / d(x_j, x_k) onto j and k.  Forces on the partners go into a table of the replica's
// forces in LDS (LACC; ds_add_f64), flushed with one global FP64 atomic per touched atom and component; replicas beyond SW_LDS_MAXPAD atoms
// add to global memory directly.  Energies, virial and counts are summed per workgroup.
extern __shared__ double s_tsf[];   // LACC: [3][npad]
template <bool LACC>
__global__ __launch_bounds__(TS_FORCE_TPB) void k_ts_force(const SimDev *sims, const SwView *views, const TsView *tviews) {
  const SwView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * SW_TILE) >= n) return;   // (the whole workgroup)
  const TsTable SW_G *tab = tviews[blockIdx.y].tab;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * TS_NSHIFT];
  __shared__ TsPairP s_pair[TS_MAXEL * TS_MAXEL];
  __shared__ TsTripP s_trip[TS_MAXEL * TS_MAXEL * TS_MAXEL];
  __shared__ double s_cutin[TS_MAXEL * TS_MAXEL];
  __shared__ double s_nb[6][TS_NGRP][TS_MAXIN];   // d (3), r, fC of the pair, fC' of the pair -> pref after pass 1
  __shared__ int s_ent[TS_NGRP][TS_MAXIN], s_tj[TS_NGRP][TS_MAXIN];
  __shared__ double s_red[8 * (TS_FORCE_TPB / 64)];
  for (int code = threadIdx.x; code < TS_NSHIFT; code += TS_FORCE_TPB) {
    const int sx = code % 5 - 2, sy = (code / 5) % 5 - 2, sz = code / 25 - 2;
    s_sh[3 * code] = sx * V.h[0] + sy * V.h[5] + sz * V.h[4];
    s_sh[3 * code + 1] = sy * V.h[1] + sz * V.h[3];
    s_sh[3 * code + 2] = sz * V.h[2];
  }
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += TS_FORCE_TPB) ((double *)s_pair)[k] = ((const double SW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += TS_FORCE_TPB) ((double *)s_trip)[k] = ((const double SW_G *)&tab->trip[0])[k];
  for (int k = threadIdx.x; k < TS_MAXEL * TS_MAXEL; k += TS_FORCE_TPB) s_cutin[k] = tab->cutin[k];
  if (LACC)
    for (int k = threadIdx.x; k < 3 * (int)np; k += TS_FORCE_TPB) s_tsf[k] = 0.0;
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  const int cap = V.cap;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // repulsive, bond-order energy, ordered pairs, ordered (j, k)
  double wr[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) {
    if (LACC) { ts_lds_add(&s_tsf[a], g0); ts_lds_add(&s_tsf[np + a], g1); ts_lds_add(&s_tsf[2 * np + a], g2); }
    else { atomicAdd((double *)&V.f[3 * a], g0); atomicAdd((double *)&V.f[3 * a + 1], g1); atomicAdd((double *)&V.f[3 * a + 2], g2); }
  };
  bool crowded = false;
  for (int it = 0; it < SW_TILE / TS_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * SW_TILE + it * TS_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    const int cnt = valid ? min(V.cnt[ic], cap) : 0;
    const int ti = V.stype[ic];
    const double xi0 = V.x[3 * ic], xi1 = V.x[3 * ic + 1], xi2 = V.x[3 * ic + 2];
    const size_t base = (size_t)ic * cap;
    int nn = 0;
    for (int c0 = 0; c0 < cnt; c0 += 16) {
      const int c = c0 + l16;
      int ent = (c < cnt) ? V.rows[base + c] : -1;
      bool in = false;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, r = 1.0;
      int tj = 0;
      if (ent >= 0) {
        const int j = min(ent & SW_JMASK, n - 1), code = min((ent >> 24) & 0x7F, TS_NSHIFT - 1);
        ent = j | (code << 24);   // (what the builder wrote; nothing else is ever used as an index)
        const double *sh = s_sh + 3 * code;
        d0 = V.x[3 * j] - xi0 + sh[0]; d1 = V.x[3 * j + 1] - xi1 + sh[1]; d2 = V.x[3 * j + 2] - xi2 + sh[2];
        tj = V.stype[j];
        const double r2 = d0 * d0 + d1 * d1 + d2 * d2, rc = s_cutin[ti * TS_MAXEL + tj];
        in = r2 < rc * rc && r2 > 0.0;
        r = sqrt(r2);
        in = in && r < rc;
      }
      const unsigned m16 = (unsigned)(__ballot(in) >> shift16) & 0xFFFFu;
      const int pos = nn + __popc(m16 & ((1u << l16) - 1u));
      if (in && pos < TS_MAXIN) {
        const TsPairP &P = s_pair[ti * TS_MAXEL + tj];
        double fc = 0.0, dfc = 0.0;
        if (r < P.cut) ts_fc(P.bigr, P.bigd, r, &fc, &dfc);   // (a pair at or beyond its R + D: a third atom only)
        s_nb[0][grp][pos] = d0; s_nb[1][grp][pos] = d1; s_nb[2][grp][pos] = d2; s_nb[3][grp][pos] = r; s_nb[4][grp][pos] = fc; s_nb[5][grp][pos] = dfc;
        s_ent[grp][pos] = ent; s_tj[grp][pos] = tj;
      }
      nn += __popc(m16);
    }
    if (nn > TS_MAXIN) { crowded = true; nn = TS_MAXIN; }
    __syncthreads();   // the groups' lists are complete
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    // pass 1: a lane per neighbour j
    for (int m = l16; m < nn; m += 16) {
      const int tj = s_tj[grp][m];
      const TsPairP &P = s_pair[ti * TS_MAXEL + tj];
      const double r1 = s_nb[3][grp][m];
      double pref = 0.0;
      if (r1 < P.cut) {
        const double dj[3] = {s_nb[0][grp][m], s_nb[1][grp][m], s_nb[2][grp][m]};
        double zeta = 0.0;
        for (int k = 0; k < nn; k++) {
          if (k == m) continue;
          const TsTripP &Q = s_trip[(ti * TS_MAXEL + tj) * TS_MAXEL + s_tj[grp][k]];
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
        add_force(s_ent[grp][m] & SW_JMASK, g0, g1, g2);
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
      const TsTripP &Q = s_trip[(ti * TS_MAXEL + tj) * TS_MAXEL + s_tj[grp][k]];
      if (!(r1 < s_pair[ti * TS_MAXEL + tj].cut) || !(r2 < Q.cut)) continue;
      esum[3] += 1.0;
      const double pref = s_nb[5][grp][j];
      if (pref == 0.0) continue;   // (b' = 0: the small-zeta end of b, or beta = 0)
      const double dj[3] = {s_nb[0][grp][j], s_nb[1][grp][j], s_nb[2][grp][j]}, dk[3] = {s_nb[0][grp][k], s_nb[1][grp][k], s_nb[2][grp][k]};
      double fj[3], fk[3];
      ts_zeta_force(Q, pref, dj, r1, dk, r2, fj, fk);
      add_force(s_ent[grp][j] & SW_JMASK, fj[0], fj[1], fj[2]);
      add_force(s_ent[grp][k] & SW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      wb[0] += dj[0] * fj[0] + dk[0] * fk[0]; wb[1] += dj[1] * fj[1] + dk[1] * fk[1]; wb[2] += dj[2] * fj[2] + dk[2] * fk[2];
      wb[3] += dj[0] * fj[1] + dk[0] * fk[1]; wb[4] += dj[0] * fj[2] + dk[0] * fk[2]; wb[5] += dj[1] * fj[2] + dk[1] * fk[2];
    }
    // the central atom's own force: the sum over its group (a row of 16 lanes)
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (valid && l16 == 0 && (fi0 != 0.0 || fi1 != 0.0 || fi2 != 0.0)) add_force(i, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  if (LACC) {
    for (int k = threadIdx.x; k < 3 * n; k += TS_FORCE_TPB) {
      const int a = k / 3, c = k - 3 * a;
      const double v = s_tsf[(size_t)c * np + a];
      if (v != 0.0) atomicAdd((double *)&V.f[k], v);
    }
  }
  if (crowded) atomicOr(&V.stat[0], 2);
  block_atomic_add_n<4, TS_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, TS_FORCE_TPB / 64>(wr, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, TS_FORCE_TPB / 64>(wb, &sc.vir[P_ANGLE * 6], s_red);
}

// energies and fault bits of the step into the engine's scalars: row full -> bit 1 (the host regrows and retries), crowded -> bit 128
__global__ void k_ts_finish(const SimDev *sims, const SwView *views) {
  const SwView &V = views[blockIdx.x];
  SimScalars &sc = *sims[blockIdx.x].sc;
  if (threadIdx.x != 0) return;
  sc.eng[P_LJ] = V.eacc[0];
  sc.eng[P_ANGLE] = V.eacc[1];
  const int st = V.stat[0];
  if (st) atomicOr(&sc.overflow, ((st & 1) ? 1 : 0) | ((st & 2) ? 128 : 0));
}

void mdk_ts_forces(hipStream_t st, const SimDev *d, SwView *v, const TsView *t, int ns, int maxatoms) {
  if (ns <= 0 || maxatoms <= 0) return;
  mdk_sw_rows(st, d, v, ns, maxatoms);
  const dim3 gt((unsigned)((maxatoms + SW_TILE - 1) / SW_TILE), (unsigned)ns, 1);
  const int maxpad = (maxatoms + 63) / 64 * 64;
  if (maxpad <= SW_LDS_MAXPAD) hipLaunchKernelGGL(k_ts_force<true>, gt, dim3(TS_FORCE_TPB), 3 * (size_t)maxpad * sizeof(double), st, d, v, t);
  else hipLaunchKernelGGL(k_ts_force<false>, gt, dim3(TS_FORCE_TPB), 0, st, d, v, t);
  hipLaunchKernelGGL(k_ts_finish, dim3(ns), dim3(64), 0, st, d, v);
}
