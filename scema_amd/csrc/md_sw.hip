// md_sw.hip -- gfx950 kernels of the Stillinger-Weber force stage (`pair_style sw`: the reference's examples/streched_polyhedron, 192-atom
// silicon replicas under lammps_scripts_sisw).  The integrator, thermostat, fix deform, pressure sampling and the batch machinery are the
// ones of the OPLS path (md_kernels.hip); only the force stage differs, as for ReaxFF (md_reax.hip).  One launch covers every replica of
// the batch (blockIdx.y).
//   k_sw_prepare ... box -> view, rebuild bookkeeping, zero the step's sums
//   k_sw_wrap ...... zero the forces; at a rebuild wrap the atoms into the box (image counts keep the unwrapped information)
//   k_sw_rows ...... full neighbour rows inside cutoff + skin, rebuilt when the engine's displacement test says so (`neighbor 1.0 nsq`,
//                    `neigh_modify every 1 delay 0 check yes`): an N^2 search, the replica's positions streamed through LDS
//   k_sw_force ..... pair and triplet terms (sw/sw_core.h) around a central atom, forces summed in LDS (skeleton: md_rowforce.h)
//   k_sw_finish .... energies and fault bits into the engine's scalars (the Tersoff and the embedded-atom stage's too)
// Row entries carry an image code in the convention of the ReaxFF rows: the shift of an entry is code . h with the box of the STEP, so
// the rows hold while fix deform remaps the atoms with the box; a box flip forces a rebuild.
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_rowforce.h"

#define SW_ROWS_TPB 512      /* row build: 8 waves of 8 rows */
#define SW_NBR 8
#define SW_JT 512            /* partners staged in LDS per pass of the row build */
static_assert(SW_TILE == 64 && SW_ROWS_TPB / 64 * SW_NBR == SW_TILE, "tile shapes of md_sw.hip");

__global__ void k_sw_prepare(const SimDev *sims, SwView *views) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  SwView &V = views[blockIdx.x];
  if (threadIdx.x == 0) {
    V.h[0] = sc.box[3] - sc.box[0]; V.h[1] = sc.box[4] - sc.box[1]; V.h[2] = sc.box[5] - sc.box[2];
    V.h[3] = sc.box[8]; V.h[4] = sc.box[7]; V.h[5] = sc.box[6];
    V.lo[0] = sc.box[0]; V.lo[1] = sc.box[1]; V.lo[2] = sc.box[2];
    V.stat[0] = 0;
    if (sc.rebuild) {
      sc.ago = 0;
      sc.nbuilds += 1;
      V.stat[1] = 0;
      box_corners(sc.box, sc.corners_hold);   // (the neighbour trigger of k_pre takes the corners' motion off the skin)
    }
  }
  if (threadIdx.x < 4) V.eacc[threadIdx.x] = 0.0;
}

__global__ __launch_bounds__(TPB) void k_sw_wrap(const SimDev *sims, const SwView *views) {
  const SimDev &S = sims[blockIdx.y];
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  S.f[3 * i] = 0.0; S.f[3 * i + 1] = 0.0; S.f[3 * i + 2] = 0.0;
  if (!S.sc->rebuild) return;
  const SwView &V = views[blockIdx.y];
  double x0 = S.x[3 * i], x1 = S.x[3 * i + 1], x2 = S.x[3 * i + 2];
  const double l2 = (x2 - V.lo[2]) / V.h[2];
  const double l1 = ((x1 - V.lo[1]) - V.h[3] * l2) / V.h[1];
  const double l0 = ((x0 - V.lo[0]) - V.h[5] * l1 - V.h[4] * l2) / V.h[0];
  const double w0 = floor(l0), w1 = floor(l1), w2 = floor(l2);
  x0 -= w0 * V.h[0] + w1 * V.h[5] + w2 * V.h[4];
  x1 -= w1 * V.h[1] + w2 * V.h[3];
  x2 -= w2 * V.h[2];
  S.x[3 * i] = x0; S.x[3 * i + 1] = x1; S.x[3 * i + 2] = x2;
  S.xhold[3 * i] = x0; S.xhold[3 * i + 1] = x1; S.xhold[3 * i + 2] = x2;
  S.wrapn[3 * i] += (int)w0; S.wrapn[3 * i + 1] += (int)w1; S.wrapn[3 * i + 2] += (int)w2;
}

// Neighbour rows: a workgroup owns SW_TILE consecutive atoms, wave w their rows 8 w .. 8 w + 7; the replica's positions pass through LDS
// SW_JT at a time, the wave's lanes over the staged partners 64 at a time.  A chunk's accepted partners leave as one contiguous store into
// the row (ballot + lane rank): rows come out sorted by partner (with several images per partner, image-major inside a chunk) whatever
// the schedule.  An entry is written only below the row's capacity; the count is clamped; a row that asked for more raises fault bit 1 and
// reports what it asked for, so the regrow-and-retry of the host finds the capacity in one step.
__global__ __launch_bounds__(SW_ROWS_TPB) void k_sw_rows(const SimDev *sims, const SwView *views) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  const SwView &V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * SW_TILE) >= n) return;   // (the whole workgroup: no barrier is left waiting)
  __shared__ double s_x[3][SW_JT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cap = V.cap;
  const int r0 = blockIdx.x * SW_TILE + wave * SW_NBR;
  const int nr = max(0, min(SW_NBR, n - r0));      // (a wave without rows still stages and waits at the barriers)
  const double rl2 = V.rlist * V.rlist;
  const double h0 = wave_uniform(V.h[0]), h1 = wave_uniform(V.h[1]), h2 = wave_uniform(V.h[2]), h3 = wave_uniform(V.h[3]), h4 = wave_uniform(V.h[4]),
               h5 = wave_uniform(V.h[5]);
  const double ih0 = 1.0 / h0, ih1 = 1.0 / h1, ih2 = 1.0 / h2;
  const int m0 = V.mimg[0], m1 = V.mimg[1], m2 = V.mimg[2];
  const bool minimage = (m0 | m1 | m2) == 0;
  double xr[SW_NBR], yr[SW_NBR], zr[SW_NBR];
  int len[SW_NBR];
#pragma unroll
  for (int g = 0; g < SW_NBR; g++) {
    const int row = min(r0 + g, n - 1);
    xr[g] = wave_uniform(S.x[3 * row]); yr[g] = wave_uniform(S.x[3 * row + 1]); zr[g] = wave_uniform(S.x[3 * row + 2]);
    len[g] = 0;
  }
  auto append = [&](int g, bool ok, int ent) __attribute__((always_inline)) {
    const unsigned long long m = __ballot(ok);
    if (m == 0) return;
    const int pos = len[g] + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
    if (ok && pos < cap) V.rows[(size_t)(r0 + g) * cap + pos] = ent;
    len[g] += __popcll(m);
  };
  for (int t0 = 0; t0 < n; t0 += SW_JT) {
    __syncthreads();   // (the pass before has been read)
    for (int k = threadIdx.x; k < SW_JT; k += SW_ROWS_TPB) {
      const int j = min(t0 + k, n - 1);
      s_x[0][k] = S.x[3 * j]; s_x[1][k] = S.x[3 * j + 1]; s_x[2][k] = S.x[3 * j + 2];
    }
    __syncthreads();
    const int tn = min(SW_JT, n - t0);
    for (int c0 = 0; c0 < tn; c0 += 64) {
      const int k = c0 + lane;                 // < SW_JT: c0 < tn <= SW_JT, both multiples of 64 or the last chunk
      const bool jl = k < tn;
      const int j = t0 + k;
      const double xj = s_x[0][k], yj = s_x[1][k], zj = s_x[2][k];
#pragma unroll
      for (int g = 0; g < SW_NBR; g++) {
        if (g >= nr) break;   // (wave-uniform)
        double dx = xj - xr[g], dy = yj - yr[g], dz = zj - zr[g];
        if (minimage) {
          const double n2 = rint(dz * ih2);
          dz -= n2 * h2; dy -= n2 * h3; dx -= n2 * h4;
          const double n1 = rint(dy * ih1);
          dy -= n1 * h1; dx -= n1 * h5;
          const double n0 = rint(dx * ih0);
          dx -= n0 * h0;
          const double r2 = dx * dx + dy * dy + dz * dz;
          const int c0i = 2 - (int)n0, c1i = 2 - (int)n1, c2i = 2 - (int)n2;
          const bool coded = (unsigned)c0i < 5u && (unsigned)c1i < 5u && (unsigned)c2i < 5u;   // (atoms are wrapped at a build: |n| <= 1)
          append(g, jl && coded && j != r0 + g && !(r2 > rl2), j | ((c0i + 5 * c1i + 25 * c2i) << 24));
        } else {
          for (int sz = -m2; sz <= m2; sz++)
            for (int sy = -m1; sy <= m1; sy++)
              for (int sx = -m0; sx <= m0; sx++) {
                const double ex = dx + sx * h0 + sy * h5 + sz * h4, ey = dy + sy * h1 + sz * h3, ez = dz + sz * h2;
                const double r2 = ex * ex + ey * ey + ez * ez;
                const bool self = j == r0 + g && sx == 0 && sy == 0 && sz == 0;
                append(g, jl && !self && !(r2 > rl2), j | (((sx + 2) + 5 * (sy + 2) + 25 * (sz + 2)) << 24));
              }
        }
      }
    }
  }
  bool full = false;
  int most = 0;
#pragma unroll
  for (int g = 0; g < SW_NBR; g++) {
    if (g >= nr) break;
    full |= len[g] > cap;
    most = max(most, len[g]);
    if (lane == 0) V.cnt[r0 + g] = min(len[g], cap);
  }
  if (lane == 0 && nr > 0) {
    if (full) atomicOr(&V.stat[0], 1);
    atomicMax(&V.stat[1], most);
    atomicMax(&S.sc->maxneigh_seen, most);
  }
}

// Forces.  A workgroup owns SW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them at a time.  The group first
// filters the atom's row to the entries INSIDE their pair cutoff -- vector, distance and the radial factor of a triplet arm, computed once
// per neighbour -- into LDS (rowf_filter, md_rowforce.h); only these reach an exponential.  Then its lanes take the pairs the atom owns
// (sw_owns: each pair once) and the triplets (a < b) of the filtered list.  Forces go into the LDS table or to global memory (LACC,
// md_rowforce.h).  Energies, virial and counts are summed per workgroup.
template <bool LACC>
__global__ __launch_bounds__(SW_FORCE_TPB) void k_sw_force(const SimDev *sims, const SwView *views) {
  const SwView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * SW_TILE) >= n) return;   // (the whole workgroup)
  const SwTable SW_G *tab = (const SwTable SW_G *)V.tab;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * SW_NSHIFT];
  __shared__ SwPairP s_pair[SW_MAXEL * SW_MAXEL];
  __shared__ SwTripP s_trip[SW_MAXEL * SW_MAXEL * SW_MAXEL];
  __shared__ double s_nb[6][SW_NGRP][SW_MAXIN];   // d (3), r, arm factor, d(arm exponent)/dr
  __shared__ int s_ent[SW_NGRP][SW_MAXIN], s_tj[SW_NGRP][SW_MAXIN];
  __shared__ double s_red[8 * (SW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < (int)(sizeof(s_pair) / 8); k += SW_FORCE_TPB) ((double *)s_pair)[k] = ((const double SW_G *)&tab->pair[0])[k];
  for (int k = threadIdx.x; k < (int)(sizeof(s_trip) / 8); k += SW_FORCE_TPB) ((double *)s_trip)[k] = ((const double SW_G *)&tab->trip[0])[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // e2, e3, pairs, triplets
  double w2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  auto add_force = [&](int a, double g0, double g1, double g2) __attribute__((always_inline)) { rowf_add<LACC>(V.f, np, a, g0, g1, g2); };
  bool crowded = false;
  for (int it = 0; it < SW_TILE / SW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * SW_TILE + it * SW_NGRP + grp;
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
      add_force(ent & SW_JMASK, g0, g1, g2);
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
      add_force(s_ent[grp][a] & SW_JMASK, fj[0], fj[1], fj[2]);
      add_force(s_ent[grp][b] & SW_JMASK, fk[0], fk[1], fk[2]);
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

// energies and fault bits of the step into the engine's scalars: row full -> bit 1 (the host regrows and retries), crowded -> bit 128
__global__ void k_sw_finish(const SimDev *sims, const SwView *views) {
  const SwView &V = views[blockIdx.x];
  SimScalars &sc = *sims[blockIdx.x].sc;
  if (threadIdx.x != 0) return;
  sc.eng[P_LJ] = V.eacc[0];
  sc.eng[P_ANGLE] = V.eacc[1];
  const int st = V.stat[0];
  if (st) atomicOr(&sc.overflow, ((st & 1) ? 1 : 0) | ((st & 2) ? 128 : 0));
}

static inline int sw_cdv(int a, int b) { return (a + b - 1) / b; }

void mdk_sw_rows(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms) {
  if (ns <= 0 || maxatoms <= 0) return;
  const dim3 gt((unsigned)sw_cdv(maxatoms, SW_TILE), (unsigned)ns, 1);
  hipLaunchKernelGGL(k_sw_prepare, dim3(ns), dim3(64), 0, st, d, v);
  hipLaunchKernelGGL(k_sw_wrap, dim3((unsigned)sw_cdv(maxatoms, TPB), (unsigned)ns, 1), dim3(TPB), 0, st, d, v);
  hipLaunchKernelGGL(k_sw_rows, gt, dim3(SW_ROWS_TPB), 0, st, d, v);
}

void mdk_sw_finish(hipStream_t st, const SimDev *d, SwView *v, int ns) {
  if (ns > 0) hipLaunchKernelGGL(k_sw_finish, dim3(ns), dim3(64), 0, st, d, v);
}

void mdk_row_forces(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms, SwForceKernel lacc, SwForceKernel direct) {
  if (ns <= 0 || maxatoms <= 0) return;
  const dim3 gt((unsigned)sw_cdv(maxatoms, SW_TILE), (unsigned)ns, 1);
  mdk_sw_rows(st, d, v, ns, maxatoms);
  const int maxpad = (maxatoms + 63) / 64 * 64;
  if (maxpad <= SW_LDS_MAXPAD) hipLaunchKernelGGL(lacc, gt, dim3(SW_FORCE_TPB), 3 * (size_t)maxpad * sizeof(double), st, d, v);
  else hipLaunchKernelGGL(direct, gt, dim3(SW_FORCE_TPB), 0, st, d, v);
  mdk_sw_finish(st, d, v, ns);
}

void mdk_sw_forces(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms) {
  mdk_row_forces(st, d, v, ns, maxatoms, k_sw_force<true>, k_sw_force<false>);
}
