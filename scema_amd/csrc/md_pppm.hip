// md_pppm.hip -- PPPM reciprocal part: what `kspace_style pppm 0.0001` (in.set.lammps:36,
// ELASTIC/potential.mod.lammps:11) asks LAMMPS for, as an alternative to the Ewald sum of md_kernels.hip (scema_md_params::kspace_style).
// Published algorithm (Hockney & Eastwood; LAMMPS pppm.cpp 17Nov16 as remembered [LAMMPS-ext], restated first in
// oracle/md_oracle.c pppm_*): order-5 charge assignment on a grid in lamda coordinates (triclinic boxes need nothing special),
// optimal influence function for ik differentiation with direct alias sums, energy and virial in reciprocal space, three
// inverse transforms for the field, forces by the same weights.  Transforms: hipFFT, one batched plan for all replicas of a
// launch group (they share the grid).  One launch per stage for the whole batch:
//   k_pppm_spread   a few workgroups per replica, each with a private copy of the real grid in LDS while its atoms are spread
//                   (ds_add_f64), added to the complex input of the transform at the end (grids beyond the LDS: global atomics)
//   k_pppm_bins, k_pppm_spread_binned   large launches of meshes whose padded copy fits: the atoms grouped by nearest grid point first, a
//                   lane adds the sum of a few atoms with one set of 125 atomics
//   k_pppm_gf       influence function of the current box, 125 alias terms per mode; only when the box has changed
//   k_pppm_poisson  energy, virial, field spectra -i k G rho(k)
//   k_pppm_force    per atom: the 125 grid points of three field grids (staged in LDS when they fit), added to the forces the
//                   other kernels assembled
//   k_pppm_keys, k_pppm_spread_tiled, k_pppm_force_tiled   meshes beyond the LDS: the two atom kernels over bricks of the mesh (md_pppm_tile.h)
#include <hip/hip_runtime.h>

#include "md_device.h"
#include "md_env.h"
#include "md_pppm.h"
#include "md_pppm_fstride.h"
#include "md_pppm_tile.h"
#include "md_types.h"
#include "pppm/pppm_core.h"

#include <algorithm>
#include <cstdlib>

static inline dim3 grid2(int nx, int ns) { return dim3((unsigned)nx, (unsigned)ns, 1); }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

#define PP_TPB 1024
#define PP_SOLVE_MAX 2900   // grid points up to which k_pppm_solve keeps three complex grids and the twiddles in 144 KB of LDS

__device__ __forceinline__ void pos_lamda(const BoxD &b, double x0, double x1, double x2, double &t0, double &t1, double &t2) {
  const double d0 = x0 - b.lo[0], d1 = x1 - b.lo[1], d2 = x2 - b.lo[2];
  const double l0 = b.hinv[0] * d0 + b.hinv[5] * d1 + b.hinv[4] * d2, l1 = b.hinv[1] * d1 + b.hinv[3] * d2, l2 = b.hinv[2] * d2;
  t0 = l0 - floor(l0); t1 = l1 - floor(l1); t2 = l2 - floor(l2);
}
__device__ __forceinline__ void atom_lamda(const SimDev &S, const BoxD &b, int a, double &t0, double &t1, double &t2) {
  pos_lamda(b, S.x[3 * a], S.x[3 * a + 1], S.x[3 * a + 2], t0, t1, t2);
}

// grid 0 <- 0 for the spreading kernels that add to it from several workgroups
__global__ __launch_bounds__(256) void k_pppm_zero(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int NG = S.pg[0] * S.pg[1] * S.pg[2], idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < NG) ((double2 *)S.pgrid)[idx] = make_double2(0.0, 0.0);
}

extern __shared__ double s_grid[];
// The workgroup's LDS copy of the charge grid leaves: added to grid 0 (a direct store when the replica has one workgroup).  PADX: after the
// five pad columns of every row are folded back onto the points they alias.
template <bool PADX>
__device__ __forceinline__ void pppm_grid_out(const SimDev &S, int nx, int ny, int nz, int split) {
  const int NG = nx * ny * nz, T = (int)blockDim.x, nxp = PADX ? nx + 5 : nx;
  double2 *rho = (double2 *)S.pgrid;
  __syncthreads();
  if (PADX) {
    // column c of a padded row holds grid point c - 2: columns 0, 1 belong to nx - 2, nx - 1 and columns nx + 2 .. nx + 4 to 0, 1, 2
    // (five distinct targets per row as nx >= 5: plain additions, one thread each)
    const int nrow = ny * nz;
    for (int k = threadIdx.x; k < 5 * nrow; k += T) {
      const int row = k / 5, pc = k - 5 * row;
      const int src = pc < 2 ? pc : nx + pc, dst = (pc < 2 ? nx - 2 + pc : pc - 2) + 2;
      s_grid[row * nxp + dst] += s_grid[row * nxp + src];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NG; k += T) {
      const int row = k / nx, x = k - row * nx;
      const double v = s_grid[row * nxp + x + 2];
      if (split == 1) rho[k] = make_double2(v, 0.0);
      else if (v != 0.0) atomicAdd(&rho[k].x, v);
    }
  } else if (split == 1) {
    for (int k = threadIdx.x; k < NG; k += T) rho[k] = make_double2(s_grid[k], 0.0);
  } else {
    for (int k = threadIdx.x; k < NG; k += T) {
      const double v = s_grid[k];
      if (v != 0.0) atomicAdd(&rho[k].x, v);
    }
  }
}

// Charge assignment.  Workgroup (s, r) takes the s-th of `split` contiguous atom ranges of replica r.  Within a wave the lanes
// take atoms that are far apart in the file (lane l: atoms l*rows .. (l+1)*rows - 1 of the range, one per iteration): bonded
// neighbours share their 125 grid points, and 64 lanes adding to the same addresses would be serialised by the LDS.  LDS = true:
// a private copy of the real grid in LDS (ds_add_f64), added to grid 0 at the end (the only global atomics: one per grid point
// and workgroup; a direct store when the replica has one workgroup).  LDS = false (grid beyond the LDS): global atomics throughout.
// PADX (LDS only, nx >= 5): the LDS copy has nx + 5 points per x row -- an atom's five x points are columns i .. i + 4 of the padded row, never
// wrapped, so the address of a point is the row's plus a CONSTANT (the offset field of ds_add_f64) instead of an addition per point; the five
// pad columns are folded back onto the points they alias before the copy leaves.
template <bool LDS, int TPB_, bool PADX = false>
__global__ __launch_bounds__(TPB_) void k_pppm_spread(const SimDev *sims, int split) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  const int NG = nx * ny * nz, T = (int)blockDim.x;
  const int nxp = PADX ? nx + 5 : nx, NGP = nxp * ny * nz;
  const int chunk = (S.natoms + split - 1) / split, a0 = (int)blockIdx.x * chunk, a1 = min(S.natoms, a0 + chunk);
  if (a0 >= a1) return;
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  double2 *rho = (double2 *)S.pgrid;
  if (LDS) {
    for (int k = threadIdx.x; k < NGP; k += T) s_grid[k] = 0.0;
    __syncthreads();
  }
  const double delvolinv = (double)NG / b.vol;
  const int rows = (a1 - a0 + 63) >> 6, lane = threadIdx.x & 63;
  // Two consecutive atoms per lane and turn.  Neighbours in the file are bonded neighbours: about half of such pairs have the same
  // nearest grid point, hence the same 125 grid points, and then ONE atomic per point carries both contributions (the LDS
  // atomics, at ~26 cycles per wave instruction, are what this kernel waits for).
  for (int r = 2 * ((int)threadIdx.x >> 6); r < rows; r += 2 * (T >> 6)) {
    const int aA = a0 + lane * rows + r, aB = aA + 1;
    const bool vA = aA < a1, vB = r + 1 < rows && aB < a1;
    if (!vA) continue;
    double wxA[PPPM_ORDER], wyA[PPPM_ORDER], wzA[PPPM_ORDER], wxB[PPPM_ORDER] = {0, 0, 0, 0, 0}, wyB[PPPM_ORDER] = {0, 0, 0, 0, 0}, wzB[PPPM_ORDER] = {0, 0, 0, 0, 0};
    int gxA[PPPM_ORDER], gyA[PPPM_ORDER], gzA[PPPM_ORDER], gxB[PPPM_ORDER] = {0, 0, 0, 0, 0}, gyB[PPPM_ORDER] = {0, 0, 0, 0, 0}, gzB[PPPM_ORDER] = {0, 0, 0, 0, 0};
    double l0, l1, l2;
    atom_lamda(S, b, aA, l0, l1, l2);
    const int ixA = pppm_weights(l0 * nx, wxA), iyA = pppm_weights(l1 * ny, wyA), izA = pppm_weights(l2 * nz, wzA);
    pppm_wrap(ixA, nx, gxA); pppm_wrap(iyA, ny, gyA); pppm_wrap(izA, nz, gzA);
    const double zA = delvolinv * S.q[aA];
    double zB = 0.0;
    int ixB = -1000, iyB = 0, izB = 0;
    if (vB) {
      atom_lamda(S, b, aB, l0, l1, l2);
      ixB = pppm_weights(l0 * nx, wxB); iyB = pppm_weights(l1 * ny, wyB); izB = pppm_weights(l2 * nz, wzB);
      pppm_wrap(ixB, nx, gxB); pppm_wrap(iyB, ny, gyB); pppm_wrap(izB, nz, gzB);
      zB = delvolinv * S.q[aB];
    }
    const bool merged = vB && ixA == ixB && iyA == iyB && izA == izB;
#pragma unroll
    for (int k = 0; k < PPPM_ORDER; k++) { wxA[k] *= zA; if (vB) wxB[k] *= zB; }
    if (zA != 0.0 || (merged && zB != 0.0)) {
#pragma unroll
      for (int c = 0; c < PPPM_ORDER; c++) {
#pragma unroll
        for (int bb = 0; bb < PPPM_ORDER; bb++) {
          const double zyA = wzA[c] * wyA[bb], zyB = merged ? wzB[c] * wyB[bb] : 0.0;   // (B's weights are zeros where there is no B)
          const int row = (gzA[c] * ny + gyA[bb]) * nxp;
          double *prow = s_grid + row + ixA;   // PADX
#pragma unroll
          for (int k = 0; k < PPPM_ORDER; k++) {
            const double val = fma(zyB, wxB[k], zyA * wxA[k]);
            if (LDS && PADX) (void)__hip_atomic_fetch_add(prow + k, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (LDS) (void)__hip_atomic_fetch_add(&s_grid[row + gxA[k]], val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else atomicAdd(&rho[row + gxA[k]].x, val);
          }
        }
      }
    }
    if (vB && !merged && zB != 0.0) {
#pragma unroll
      for (int c = 0; c < PPPM_ORDER; c++) {
#pragma unroll
        for (int bb = 0; bb < PPPM_ORDER; bb++) {
          const double zyB = wzB[c] * wyB[bb];
          const int row = (gzB[c] * ny + gyB[bb]) * nxp;
          double *prow = s_grid + row + ixB;   // PADX
#pragma unroll
          for (int k = 0; k < PPPM_ORDER; k++) {
            if (LDS && PADX) (void)__hip_atomic_fetch_add(prow + k, zyB * wxB[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else if (LDS) (void)__hip_atomic_fetch_add(&s_grid[row + gxB[k]], zyB * wxB[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            else atomicAdd(&rho[row + gxB[k]].x, zyB * wxB[k]);
          }
        }
      }
    }
  }
  if (LDS) pppm_grid_out<PADX>(S, nx, ny, nz, split);
}

// (the home-tile keys of a simulation (k_pppm_keys below), or its binned lists, lie behind its influence function, pgstride doubles into the block the engine lays out: engine_run.cpp lay_out_kspace)
__device__ __forceinline__ int MD_G *pppm_keys_of(const SimDev &S) { return (int MD_G *)(S.pgf + S.pgstride); }

// ---- binned charge assignment (whole padded mesh in LDS): the atoms of a replica grouped by nearest grid point, so that one set of 125 LDS
// atomics carries up to PP_BIN_M atoms ----
// k_pppm_spread waits for its ds_add_f64 at the rate the LDS executes them, and all atoms with the same nearest grid point add to the same 125
// addresses (PE-10k on 12 x 12 x 12: six atoms per point).  k_pppm_bins, one workgroup per replica and step, sorts the charged atoms by
// the BIN of their nearest point -- x as the unwrapped index 0 .. nx (in the padded rows the points nx and 0 are different columns), y and z
// mod n -- and cuts every bin into ITEMS of up to M atoms; a lane of k_pppm_spread_binned takes one item, sums its atoms' products in
// registers and issues the 125 atomics once.  The lists lie where the home-tile keys of the tiled kernels lie (pppm_keys_of; a launch
// takes either), as ints: [0] the number of items, [1] unused, then natoms items (bin | count << 24, first index into perm), then perm,
// the charged atoms by bin.  Order of the items: round r holds part r of every bin that has one, in bin order (consecutive bins along x are
// consecutive LDS words), so that the lanes of a wave address distinct points; the parts from PP_BIN_ROUNDS - 1 on of a bin share the last round.
#ifndef PP_BIN_M
#define PP_BIN_M 4
#endif
#define PP_BIN_TPB 1024
#define PP_BIN_ROUNDS 4
#define PP_BIN_BATCH 4
extern __shared__ int s_bins[];
// exclusive prefix sums of NV values per thread over the PP_BIN_TPB threads; tot: the sums over the workgroup
template <int NV>
__device__ __forceinline__ void pppm_block_scan(int (&v)[NV], int (&tot)[NV], int *lds /* NV * waves */) {
  constexpr int NW = PP_BIN_TPB / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc[NV];
#pragma unroll
  for (int i = 0; i < NV; i++) {
    int x = v[i];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    inc[i] = x;
    if (lane == 63) lds[i * NW + wave] = x;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; i++) {
    int before = 0, all = 0;
    for (int w = 0; w < NW; w++) { const int t = lds[i * NW + w]; all += t; if (w < wave) before += t; }
    v[i] = before + inc[i] - v[i];
    tot[i] = all;
  }
  __syncthreads();
}
__global__ __launch_bounds__(PP_BIN_TPB) void k_pppm_bins(const SimDev *sims, int M) {
  const SimDev &S = sims[blockIdx.x];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  const int nbx = nx + 1, nbins = nbx * ny * nz, natoms = S.natoms;
  int *s_cnt = s_bins, *s_start = s_bins + nbins;
  __shared__ int s_scan[(PP_BIN_ROUNDS + 1) * (PP_BIN_TPB / 64)];
  int MD_G *head = pppm_keys_of(S);
  int2 MD_G *items = (int2 MD_G *)(head + 2);
  int MD_G *perm = head + 2 + 2 * (size_t)natoms;
  for (int k = threadIdx.x; k < nbins; k += PP_BIN_TPB) s_cnt[k] = 0;
  __syncthreads();
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  // bin and rank within the bin of every atom (kept in the room of the items until the bins have their places).  Four atoms per thread and
  // turn, their charges and positions requested together: the kernel waits for memory, not for arithmetic.
  for (int a0 = threadIdx.x; a0 < natoms; a0 += PP_BIN_BATCH * PP_BIN_TPB) {
    double q[PP_BIN_BATCH], x0[PP_BIN_BATCH], x1[PP_BIN_BATCH], x2[PP_BIN_BATCH];
#pragma unroll
    for (int j = 0; j < PP_BIN_BATCH; j++) {
      const int a = min(a0 + j * PP_BIN_TPB, natoms - 1);
      q[j] = S.q[a]; x0[j] = S.x[3 * a]; x1[j] = S.x[3 * a + 1]; x2[j] = S.x[3 * a + 2];
    }
#pragma unroll
    for (int j = 0; j < PP_BIN_BATCH; j++) {
      const int a = a0 + j * PP_BIN_TPB;
      if (a >= natoms) break;
      int bin = -1, rank = 0;
      if (q[j] != 0.0) {
        double l0, l1, l2;
        pos_lamda(b, x0[j], x1[j], x2[j], l0, l1, l2);
        const int ix = min(max(pppm_nearest(l0 * nx), 0), nx), iy = pppm_mod(pppm_nearest(l1 * ny), ny), iz = pppm_mod(pppm_nearest(l2 * nz), nz);
        bin = (iz * ny + iy) * nbx + ix;
        rank = atomicAdd(&s_cnt[bin], 1);
      }
      items[a] = make_int2(bin, rank);
    }
  }
  __syncthreads();
  // thread t owns the bins t per .. (t + 1) per - 1: atoms before them, and items before them in every round
  const int per = (nbins + PP_BIN_TPB - 1) / PP_BIN_TPB, b0 = min(nbins, (int)threadIdx.x * per), b1 = min(nbins, b0 + per);
  int v[PP_BIN_ROUNDS + 1], tot[PP_BIN_ROUNDS + 1];
#pragma unroll
  for (int r = 0; r <= PP_BIN_ROUNDS; r++) v[r] = 0;
  for (int k = b0; k < b1; k++) {
    const int n = s_cnt[k], parts = (n + M - 1) / M;
    v[PP_BIN_ROUNDS] += n;
#pragma unroll
    for (int r = 0; r < PP_BIN_ROUNDS - 1; r++) v[r] += parts > r ? 1 : 0;
    v[PP_BIN_ROUNDS - 1] += max(parts - (PP_BIN_ROUNDS - 1), 0);
  }
  pppm_block_scan<PP_BIN_ROUNDS + 1>(v, tot, s_scan);
  {
    int at = v[PP_BIN_ROUNDS];
    for (int k = b0; k < b1; k++) { s_start[k] = at; at += s_cnt[k]; }
  }
  __syncthreads();
  for (int a0 = threadIdx.x; a0 < natoms; a0 += PP_BIN_BATCH * PP_BIN_TPB) {
    int2 br[PP_BIN_BATCH];
#pragma unroll
    for (int j = 0; j < PP_BIN_BATCH; j++) br[j] = items[min(a0 + j * PP_BIN_TPB, natoms - 1)];   // (this thread's own stores above)
#pragma unroll
    for (int j = 0; j < PP_BIN_BATCH; j++) {
      const int a = a0 + j * PP_BIN_TPB;
      if (a < natoms && br[j].x >= 0) perm[s_start[br[j].x] + br[j].y] = a;
    }
  }
  __syncthreads();   // every (bin, rank) has been read: the items take their room
  {
    int at[PP_BIN_ROUNDS], base = 0;
#pragma unroll
    for (int r = 0; r < PP_BIN_ROUNDS; r++) { at[r] = base + v[r]; base += tot[r]; }
    if (threadIdx.x == 0) head[0] = base;
    for (int k = b0; k < b1; k++) {
      const int n = s_cnt[k], first = s_start[k];
      for (int p = 0, left = n; left > 0; p++, left -= M) {
        int idx = 0;
#pragma unroll
        for (int r = 0; r < PP_BIN_ROUNDS; r++)
          if (min(p, PP_BIN_ROUNDS - 1) == r) idx = at[r]++;
        items[idx] = make_int2(k | (min(left, M) << 24), first + p * M);
      }
    }
  }
}

// Workgroup (s, r) takes the s-th of `split` ranges of replica r's items, a lane one item at a time.  The positions and charges of the
// item's atoms are requested up front; every atom's weights are taken around the BIN's point (as the tiled kernels take theirs around the key:
// an atom has one home, whatever its coordinate rounds to here), kept in registers, and the 25 rows of five points are summed over the atoms and
// added one after the other.  The private padded LDS grid and its way out are those of k_pppm_spread<true, 256, true>.
template <int M>
__global__ __launch_bounds__(256) void k_pppm_spread_binned(const SimDev *sims, int split) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  const int NG = nx * ny * nz, nxp = nx + 5, NGP = nxp * ny * nz, nbx = nx + 1;
  const int MD_G *head = pppm_keys_of(S);
  const int2 MD_G *items = (const int2 MD_G *)(head + 2);
  const int MD_G *perm = head + 2 + 2 * (size_t)S.natoms;
  const int nitems = head[0];
  const int chunk = (nitems + split - 1) / split, i0 = (int)blockIdx.x * chunk, i1 = min(nitems, i0 + chunk);
  if (i0 >= i1 && split > 1) return;   // (a lone workgroup stores the grid, zeros included)
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  for (int k = threadIdx.x; k < NGP; k += 256) s_grid[k] = 0.0;
  __syncthreads();
  const double delvolinv = (double)NG / b.vol;
  for (int it = i0 + (int)threadIdx.x; it < i1; it += 256) {
    const int2 item = items[it];
    const int bin = item.x & 0xffffff, n = item.x >> 24, first = item.y;
    const int rowb = bin / nbx, ix = bin - rowb * nbx, iz = rowb / ny, iy = rowb - iz * ny;
    int at[M];
    double px[M], py[M], pz[M], zq[M];
#pragma unroll
    for (int j = 0; j < M; j++) at[j] = perm[first + min(j, n - 1)];   // (a short item repeats its last atom with charge 0)
#pragma unroll
    for (int j = 0; j < M; j++) {
      px[j] = S.x[3 * at[j]]; py[j] = S.x[3 * at[j] + 1]; pz[j] = S.x[3 * at[j] + 2];
      zq[j] = j < n ? delvolinv * S.q[at[j]] : 0.0;
    }
    double wx[M][PPPM_ORDER], wy[M][PPPM_ORDER], wz[M][PPPM_ORDER];
#pragma unroll
    for (int j = 0; j < M; j++) {
      double l0, l1, l2;
      pos_lamda(b, px[j], py[j], pz[j], l0, l1, l2);
      pppm_blend(0.5 - ((double)ix - l0 * nx), wx[j]);
      pppm_weights_at(l1 * ny, ny, iy, wy[j]); pppm_weights_at(l2 * nz, nz, iz, wz[j]);
#pragma unroll
      for (int k = 0; k < PPPM_ORDER; k++) wx[j][k] *= zq[j];
    }
    int gy[PPPM_ORDER], gz[PPPM_ORDER];
    pppm_wrap(iy, ny, gy); pppm_wrap(iz, nz, gz);
#pragma unroll
    for (int c = 0; c < PPPM_ORDER; c++) {
#pragma unroll
      for (int bb = 0; bb < PPPM_ORDER; bb++) {
        double acc[PPPM_ORDER] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < M; j++) {
          const double zy = wz[j][c] * wy[j][bb];
#pragma unroll
          for (int k = 0; k < PPPM_ORDER; k++) acc[k] = fma(zy, wx[j][k], acc[k]);
        }
        double *prow = s_grid + (gz[c] * ny + gy[bb]) * nxp + ix;
#pragma unroll
        for (int k = 0; k < PPPM_ORDER; k++) (void)__hip_atomic_fetch_add(prow + k, acc[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  pppm_grid_out<true>(S, nx, ny, nz, split);
}

// optimal influence function of the current box (ik differentiation), alias sums |m| <= 2 per dimension
__global__ __launch_bounds__(256) void k_pppm_gf(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  const int NG = nx * ny * nz, idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= NG) return;
  BoxD b;
  box_derive(S.sc->box, b);
  S.pgf[idx] = pppm_gf(b.hinv, S.g_ewald, nx, ny, nz, idx % nx, (idx / nx) % ny, idx / (nx * ny));
}

// one reciprocal mode: wave vector of grid index idx, and -- with the (unnormalised) transform r of the charge grid -- its share of
// energy and virial; returns the potential G rho(k) / NG whose products with -i k are the field spectra
__device__ __forceinline__ double2 pppm_mode(const SimDev &S, const BoxD &b, int idx, int nx, int ny, int nz, double2 r, double (&kv)[3], double (&v)[6], double &e) {
  const int NG = nx * ny * nz;
  const int m1 = idx % nx, m2 = (idx / nx) % ny, m3 = idx / (nx * ny);
  double kx, ky, kz;
  pppm_kvec(b.hinv, pppm_signed(m1, nx), pppm_signed(m2, ny), pppm_signed(m3, nz), kx, ky, kz);
  kv[0] = kx; kv[1] = ky; kv[2] = kz;
  const double gf = S.pgf[idx], scaleinv = 1.0 / (double)NG;
  const double ar = r.x * scaleinv, ai = r.y * scaleinv;
  double pr, pi;
  pppm_mode_term(b.vol, MD_QQRD2E, S.g_ewald, kx, ky, kz, ar, ai, gf, v, e, pr, pi);
  if (idx == 0)   // self energy and neutralising background
    e -= MD_QQRD2E * (S.g_ewald * S.qsqsum / sqrt(MD_PI) + 0.5 * MD_PI * S.qsum * S.qsum / (S.g_ewald * S.g_ewald * b.vol));
  return make_double2(pr, pi);
}

// energy, virial and the three field spectra; the charge grid holds rho(k) (unnormalised), the field grids receive E_x, E_y, E_z (k)
__global__ __launch_bounds__(256) void k_pppm_poisson(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  __shared__ double s_red[8 * 4];
  const int NG = nx * ny * nz, idx = blockIdx.x * 256 + threadIdx.x;
  if ((int)(blockIdx.x * 256) >= NG) return;
  double v[6] = {0, 0, 0, 0, 0, 0}, e[1] = {0};
  BoxD b;
  box_derive(S.sc->box, b);
  if (idx < NG) {
    double kv[3];
    const double2 p = pppm_mode(S, b, idx, nx, ny, nz, ((const double2 *)S.pgrid)[idx], kv, v, e[0]);
    const size_t gs = (size_t)S.pgstride;
    double2 *field = (double2 *)S.pfield;
    field[idx] = make_double2(kv[0] * p.y, -kv[0] * p.x);       // (a + i b)(-i k) = b k - i a k
    field[gs + idx] = make_double2(kv[1] * p.y, -kv[1] * p.x);
    field[2 * gs + idx] = make_double2(kv[2] * p.y, -kv[2] * p.x);
  }
  block_atomic_add_n<6, 4>(v, S.sc->vir + P_KSPACE * 6, s_red);
  block_atomic_add_n<1, 4>(e, S.sc->eng + P_KSPACE, s_red);
}

// Small grids (3 NG complex numbers + the twiddles fit the LDS: NG <= PP_SOLVE_MAX): the whole solve of a replica -- forward
// transform, energy / virial / field spectra, the inverse transforms (two: x and y ride together) -- in ONE launch, one workgroup per replica, the grid never
// leaving the LDS.  The transforms are plain DFTs along one dimension at a time (a 10 x 10 x 9 grid is 29 multiply-adds per
// point and pass; the twiddles exp(-2 pi i j / n) come from sincospi once per launch), ping-ponging between two LDS buffers;
// a third keeps rho(k) while the three field components are transformed back.  Replaces eight to ten library launches of a few
// microseconds each per step (what a single replica or a 72-replica share waits for) and leaves the charge grid zeroed for the
// next spreading pass.  Replicas of one launch may have different grids.
// Two shapes (round 5).  <1 024, false>: sixteen waves and rho(k) in a third LDS buffer -- one grid point per thread and pass for grids of up
// to 1 024 points: what a single replica or a handful waits for.  <512, true>: eight waves, two LDS buffers, rho(k) in the replica's charge
// grid in memory (written once, read three times: cache traffic) -- 56 KB and 512 threads for a 12 x 12 x 12 grid, which is what ONE retiring
// k_pair workgroup leaves free on a CU.  The first shape (83 KB, 1 024 threads) needs both of a CU's k_pair workgroups gone, so beside a pair
// launch it only ever started in that launch's tail: 899 instead of 90 us per step at 72 replicas, the k-space chain behind it stalled.
extern __shared__ double2 s_fft[];
template <int PP_SOLVE_TPB, bool BGLOBAL>
__global__ __launch_bounds__(PP_SOLVE_TPB) void k_pppm_solve(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.x];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  __shared__ double s_red[8 * (PP_SOLVE_TPB / 64)];
  const int NG = nx * ny * nz;
  double2 *A = s_fft, *C = A + NG, *B = BGLOBAL ? (double2 *)S.pgrid : C + NG, *tw = (BGLOBAL ? C : B) + NG;   // twiddles: x at 0, y at nx, z at nx + ny
#ifdef PAIR_TIMING
  unsigned long long tq[8]; int ntq = 0;
#define PP_CLK() tq[ntq++] = __builtin_readcyclecounter()
#else
#define PP_CLK()
#endif
  PP_CLK();
  for (int k = threadIdx.x; k < nx + ny + nz; k += PP_SOLVE_TPB) {
    const int n = k < nx ? nx : (k < nx + ny ? ny : nz), j = k < nx ? k : (k < nx + ny ? k - nx : k - nx - ny);
    double sn, cs;
    sincospi(2.0 * (double)j / (double)n, &sn, &cs);
    tw[k] = make_double2(cs, -sn);
  }
  // Two workgroups per replica (gridDim.y == 2; the shape with rho(k) in LDS only): each makes the forward transform and ONE of the two
  // transforms back -- six one-dimensional passes instead of nine on the critical path of a batch of a few replicas, which waits for
  // this kernel.  Energy and virial are taken by the first.  The charge grid must leave zeroed but not before both
  // have read it: each takes a ticket once its copy is in LDS, the last one zeroes.
  const bool two = !BGLOBAL && gridDim.y == 2;
  const int c_lo = two ? (int)blockIdx.y : 0, c_hi = two ? (int)blockIdx.y + 1 : 2;
  double2 *rho = (double2 *)S.pgrid;
  for (int k = threadIdx.x; k < NG; k += PP_SOLVE_TPB) { A[k] = make_double2(rho[k].x, 0.0); if (!BGLOBAL && !two) rho[k] = make_double2(0.0, 0.0); }
  __syncthreads();
  if (two) {
    __shared__ int s_last;
    if (threadIdx.x == 0) {
      // (relaxed: this workgroup's reads of the grid are complete -- their values are in LDS, behind the barrier above --, and nothing it wrote is
      // read by the other; a release / acquire at device scope would write back and invalidate this XCD's L2)
      const int t = __hip_atomic_fetch_add(&S.sc->pppm_ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      s_last = (t == 1);
      if (t == 1) __hip_atomic_store(&S.sc->pppm_ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_last)
      for (int k = threadIdx.x; k < NG; k += PP_SOLVE_TPB) rho[k] = make_double2(0.0, 0.0);
  }
  PP_CLK();   // 1: twiddles + charge grid in
  // out[.., m, ..] = sum_k in[.., k, ..] w^(m k) along dimension dim (w = exp(-+2 pi i / n)); ends with a barrier.  A work item is one
  // line of the grid and one m in 0 .. n/2: it also produces the output n - m, whose twiddles are the complex conjugates (8 multiply-adds
  // and two LDS reads per k for two outputs; one output per item took 4 and two: 7 / 12 of the items, and a 12 x 12 x 12 grid is one
  // round of the 1 024 threads instead of two).  The items of a thread are the same in the three passes of a dimension: their line
  // offsets and m come from integer divisions done once.
  int it_m[3][2], it_base[3][2];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const int n = d == 0 ? nx : (d == 1 ? ny : nz), stride = d == 0 ? 1 : (d == 1 ? nx : nx * ny), nh = n / 2 + 1;
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const int it = (int)threadIdx.x + r * PP_SOLVE_TPB, L = it / nh;
      it_m[d][r] = it - L * nh;
      it_base[d][r] = (L / stride) * stride * n + (L % stride);
    }
  }
  auto pass = [&](const double2 *in, double2 *out, int dim, bool inverse) {
    const int n = dim == 0 ? nx : (dim == 1 ? ny : nz), stride = dim == 0 ? 1 : (dim == 1 ? nx : nx * ny), nh = n / 2 + 1;
    const int nitems = (NG / n) * nh;
    const double2 *t = tw + (dim == 0 ? 0 : (dim == 1 ? nx : nx + ny));
    for (int it = threadIdx.x, r = 0; it < nitems; it += PP_SOLVE_TPB, r++) {
      int m, base;
      if (r < 2) { m = r == 0 ? it_m[dim][0] : it_m[dim][1]; base = r == 0 ? it_base[dim][0] : it_base[dim][1]; }
      else { const int L = it / nh; m = it - L * nh; base = (L / stride) * stride * n + (L % stride); }
      double ar = 0.0, ai = 0.0, br = 0.0, bi = 0.0;
      int j = 0;   // (m k) mod n
#pragma unroll 4
      for (int k = 0; k < n; k++) {
        const double2 vv = in[base + k * stride], w = t[j];
        const double wi = inverse ? -w.y : w.y;
        ar = fma(vv.x, w.x, fma(-vv.y, wi, ar));
        ai = fma(vv.x, wi, fma(vv.y, w.x, ai));
        br = fma(vv.x, w.x, fma(vv.y, wi, br));      // conj(w): output n - m
        bi = fma(-vv.x, wi, fma(vv.y, w.x, bi));
        j += m;
        if (j >= n) j -= n;
      }
      out[base + m * stride] = make_double2(ar, ai);
      if (m != 0 && 2 * m != n) out[base + (n - m) * stride] = make_double2(br, bi);
    }
    __syncthreads();
  };
  pass(A, C, 0, false); pass(C, A, 1, false); pass(A, B, 2, false);   // B = rho(k) (BGLOBAL: in the charge grid's memory; the barrier that ends a pass orders it for the workgroup)
  PP_CLK();   // 2: forward passes
  BoxD b;
  box_derive(S.sc->box, b);
  double v[6] = {0, 0, 0, 0, 0, 0}, e[1] = {0};
  const size_t gs = (size_t)S.pgstride;
  double2 *field = (double2 *)S.pfield;
  // Two transforms back instead of three: the fields are real, so E_x(k) + i E_y(k) comes back as e_x(r) + i e_y(r) -- if both
  // spectra are Hermitian.  Modes with a Nyquist component are not (the grid index n/2 stands for -n/2 only), and taking the real
  // part of each field, as the three-transform form does, is the same as transforming the Hermitian part (X(k) + conj X(-k)) / 2:
  // that is what is packed here (for every other mode it equals X(k) to the last bit).
  for (int c = c_lo; c < c_hi; c++) {
    for (int idx = threadIdx.x; idx < NG; idx += PP_SOLVE_TPB) {
      double kv[3], vd[6] = {0, 0, 0, 0, 0, 0}, ed = 0.0;
      const double2 p = (c == 0) ? pppm_mode(S, b, idx, nx, ny, nz, B[idx], kv, v, e[0]) : pppm_mode(S, b, idx, nx, ny, nz, B[idx], kv, vd, ed);
      // spectrum of one component: (a + i b)(-i k) = b k - i a k
      if (c == 0) {
        const int m1 = idx % nx, m2 = (idx / nx) % ny, m3 = idx / (nx * ny);
        const int mid = (((nz - m3) % nz) * ny + (ny - m2) % ny) * nx + (nx - m1) % nx;
        double kw[3];
        const double2 q = pppm_mode(S, b, mid, nx, ny, nz, B[mid], kw, vd, ed);
        // Hermitian parts of X = (kx p.y, -kx p.x) and Y = (ky p.y, -ky p.x), with conj of the mirror mode's (kw q.y, -kw q.x)
        const double xr = 0.5 * (kv[0] * p.y + kw[0] * q.y), xi = 0.5 * (-kv[0] * p.x + kw[0] * q.x);
        const double yr = 0.5 * (kv[1] * p.y + kw[1] * q.y), yi = 0.5 * (-kv[1] * p.x + kw[1] * q.x);
        A[idx] = make_double2(xr - yi, xi + yr);   // X_H + i Y_H
      } else A[idx] = make_double2(kv[2] * p.y, -kv[2] * p.x);
    }
    __syncthreads();
    PP_CLK();   // 3, 5: spectra
    pass(A, C, 0, true); pass(C, A, 1, true); pass(A, C, 2, true);
    PP_CLK();   // 4, 6: inverse passes
    // (the fields leave as three REAL arrays at a spacing of gs doubles inside the buffer of the three complex grids: k_pppm_force
    // then stages 8 instead of 16 bytes per point)
    for (int idx = threadIdx.x; idx < NG; idx += PP_SOLVE_TPB) {
      const double2 r = C[idx];
      double *fr = (double *)field;
      if (c == 0) { fr[idx] = r.x; fr[gs + idx] = r.y; }
      else fr[2 * gs + idx] = r.x;
    }
    __syncthreads();
  }
  if (BGLOBAL)   // the charge grid leaves zeroed for the next spreading pass, as in the other shape
    for (int k = threadIdx.x; k < NG; k += PP_SOLVE_TPB) rho[k] = make_double2(0.0, 0.0);
  if (c_lo == 0) {   // (uniform over the workgroup)
    block_atomic_add_n<6, PP_SOLVE_TPB / 64>(v, S.sc->vir + P_KSPACE * 6, s_red);
    block_atomic_add_n<1, PP_SOLVE_TPB / 64>(e, S.sc->eng + P_KSPACE, s_red);
  }
#ifdef PAIR_TIMING
  PP_CLK();   // 7: field stores of the second round + sums
  if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && ntq == 8) {
    for (int k = 1; k < 8; k++) atomicAdd(&S.sc->dbg2[k - 1], tq[k] - tq[k - 1]);
    atomicAdd(&S.sc->dbg2[7], 1ull);
  }
#endif
#undef PP_CLK
}

// forces: the field (real parts of grids 1..3 after the inverse transforms) at the atom, by the assignment weights.  LDS = true:
// workgroup (s, r) stages the three real field grids of replica r in LDS once and serves the s-th of `split` atom ranges
// (consecutive atoms in consecutive lanes: neighbours read the same grid points, which the LDS broadcasts); LDS = false reads
// the grids through the caches.
// REALF: the fields are three real arrays at a spacing of gs doubles (written by k_pppm_solve) instead of the real parts of three complex grids
// LDS layout (md_pppm_fstride.h): point (gx, gy, gz) of field f at f * ps * nz + gz * ps + gy * rs + gx; fs_budget > 0: the strides of
// pppm_fstride for the mesh of the replica where they fit the fs_lds bytes of the launch, else (and with fs_budget == 0) the dense ones
template <bool LDS, bool REALF = false, int TPB_ = 256>
__global__ __launch_bounds__(TPB_) void k_pppm_force(const SimDev *sims, int split, int add, int fs_budget, int fs_lds) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  const int NG = nx * ny * nz;
  int chunk = (S.natoms + split - 1) / split;
  chunk = (chunk + 255) & ~255;
  const int a0 = (int)blockIdx.x * chunk, a1 = min(S.natoms, a0 + chunk);
  if (a0 >= a1) return;
  const size_t gs = (size_t)S.pgstride;
  const double2 *ex = (const double2 *)S.pfield, *ey = ex + gs, *ez = ey + gs;
  int rs = nx, ps = nx * ny;
  if (LDS && fs_budget > 0) {
    const PppmFStride fs = pppm_fstride(nx, ny, nz, fs_budget);
    if (fs.bytes <= (long long)fs_lds) { rs = fs.rs; ps = fs.ps; }
  }
  const int FS = ps * nz;   // doubles of one staged field
  if (LDS) {
    // point k of the mesh goes to k + (its plane) * (pad of a plane): the plane is followed from turn to turn instead of divided out
    // (rows stay dense in every layout of the rule; a padded row takes the general form)
    const int plane = nx * ny, padz = ps - plane;
    if (rs == nx) {
      const int qz = TPB_ / plane, rz = TPB_ - qz * plane;
      int z = (int)threadIdx.x / plane, r = (int)threadIdx.x - z * plane;
      for (int k = threadIdx.x; k < NG; k += TPB_) {
        const int g = k + z * padz;
        if (REALF) { const double *fr = (const double *)S.pfield; s_grid[g] = fr[k]; s_grid[FS + g] = fr[gs + k]; s_grid[2 * FS + g] = fr[2 * gs + k]; }
        else { s_grid[g] = ex[k].x; s_grid[FS + g] = ey[k].x; s_grid[2 * FS + g] = ez[k].x; }
        z += qz; r += rz;
        if (r >= plane) { r -= plane; z += 1; }
      }
    } else {
      for (int k = threadIdx.x; k < NG; k += TPB_) {
        const int z = k / plane, yx = k - z * plane, y = yx / nx;
        const int g = z * ps + y * rs + (yx - y * nx);
        if (REALF) { const double *fr = (const double *)S.pfield; s_grid[g] = fr[k]; s_grid[FS + g] = fr[gs + k]; s_grid[2 * FS + g] = fr[2 * gs + k]; }
        else { s_grid[g] = ex[k].x; s_grid[FS + g] = ey[k].x; s_grid[2 * FS + g] = ez[k].x; }
      }
    }
    __syncthreads();
  }
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  for (int a = a0 + (int)threadIdx.x; a < a1; a += TPB_) {
    const double qa = S.q[a];
    if (qa == 0.0) {
      if (!add) { S.f[3 * a] = 0.0; S.f[3 * a + 1] = 0.0; S.f[3 * a + 2] = 0.0; }
      continue;
    }
    double l0, l1, l2;
    atom_lamda(S, b, a, l0, l1, l2);
    double wx[PPPM_ORDER], wy[PPPM_ORDER], wz[PPPM_ORDER];
    int gx[PPPM_ORDER], gy[PPPM_ORDER], gz[PPPM_ORDER];
    pppm_wrap(pppm_weights(l0 * nx, wx), nx, gx);
    pppm_wrap(pppm_weights(l1 * ny, wy), ny, gy);
    pppm_wrap(pppm_weights(l2 * nz, wz), nz, gz);
    double fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
    for (int c = 0; c < PPPM_ORDER; c++) {
#pragma unroll
      for (int bb = 0; bb < PPPM_ORDER; bb++) {
        const double zy = wz[c] * wy[bb];
        const int row = LDS ? gz[c] * ps + gy[bb] * rs : (gz[c] * ny + gy[bb]) * nx;
        double rx = 0.0, ry = 0.0, rz = 0.0;
#pragma unroll
        for (int k = 0; k < PPPM_ORDER; k++) {
          const int g = row + gx[k];
          if (LDS) { rx = fma(wx[k], s_grid[g], rx); ry = fma(wx[k], s_grid[FS + g], ry); rz = fma(wx[k], s_grid[2 * FS + g], rz); }
          else if (REALF) { const double *fr = (const double *)S.pfield; rx = fma(wx[k], fr[g], rx); ry = fma(wx[k], fr[gs + g], ry); rz = fma(wx[k], fr[2 * gs + g], rz); }
          else { rx = fma(wx[k], ex[g].x, rx); ry = fma(wx[k], ey[g].x, ry); rz = fma(wx[k], ez[g].x, rz); }
        }
        fx = fma(zy, rx, fx); fy = fma(zy, ry, fy); fz = fma(zy, rz, fz);
      }
    }
    const double qf = MD_QQRD2E * qa;
    if (add) { S.f[3 * a] += qf * fx; S.f[3 * a + 1] += qf * fy; S.f[3 * a + 2] += qf * fz; }
    else { S.f[3 * a] = qf * fx; S.f[3 * a + 1] = qf * fy; S.f[3 * a + 2] = qf * fz; }
  }
}


// ---- tiled charge assignment and interpolation: the LDS formulation of the two kernels above for meshes beyond the LDS ----
// The mesh is cut into bricks in (y, z) that span whole x rows (md_pppm_tile.h); workgroup (tile, replica).  An atom's HOME tile is the one
// that owns the (y, z) of its nearest grid point.  It is decided once per step from the current positions by k_pppm_keys (the cell order is
// stale by up to the list skin between rebuilds) and read from there by both kernels, which also centre their y and z stencils on the key
// instead of deciding the nearest point again: every atom has exactly one home, and the stencil of an atom lies within two rows of it.
// key = iy | iz << 16, bit 31: the atom is uncharged.
#define PP_KEY_Y(key) ((key) & 0xffff)
#define PP_KEY_Z(key) (((key) >> 16) & 0x7fff)
__global__ __launch_bounds__(256) void k_pppm_keys(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  if (S.pg[0] == 0) return;
  const int ny = S.pg[1], nz = S.pg[2], a = blockIdx.x * 256 + threadIdx.x;
  if (a >= S.natoms) return;
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  double l0, l1, l2;
  atom_lamda(S, b, a, l0, l1, l2);
  const int iy = pppm_mod(pppm_nearest(l1 * ny), ny), iz = pppm_mod(pppm_nearest(l2 * nz), nz);
  pppm_keys_of(S)[a] = iy | (iz << 16) | (S.q[a] == 0.0 ? (int)0x80000000 : 0);
}
// the tile of this workgroup: origin and extent of its brick (false: the replica has fewer tiles, or no mesh)
struct PppmBrick { int y0, z0, byc, bzc, hy, hz; };
__device__ __forceinline__ bool pppm_brick(int nx, int ny, int nz, int budget, int which, PppmBrick &B) {
  const PppmTile t = pppm_tile_shape(nx, ny, nz, budget, which);
  const int tile = (int)blockIdx.x;
  if (tile >= t.ty * t.tz) return false;
  const int tzi = tile / t.ty, tyi = tile - tzi * t.ty;
  B.y0 = tyi * t.by; B.z0 = tzi * t.bz;
  B.byc = min(t.by, ny - B.y0); B.bzc = min(t.bz, nz - B.z0);
  B.hy = t.by < ny ? 4 : 0; B.hz = t.bz < nz ? 4 : 0;
  return true;
}
// a - b for mesh indices 0 <= a, b < n, shifted by d (|d| <= 2), taken mod n
__device__ __forceinline__ int pppm_rel(int a, int b, int d, int n) {
  const int v = a - b + d;
  return v < 0 ? v + n : (v >= n ? v - n : v);
}

// Charge assignment, owner computes: the workgroup keeps its brick in LDS (nx byc bzc doubles), takes every charged atom whose 5 x 5 stencil in
// (y, z) touches the brick -- home within two rows of it --, adds the stencil points that fall on OWNED rows (ownership is tested per stencil
// offset: with fewer than five rows in a dimension two offsets of one atom may hit the same row, and an atom near a border is served by up to
// four tiles, in part by each), and stores the brick with plain stores, zeros included: no global atomics, no k_pppm_zero, and nothing
// depends on what the charge grid held.  Lanes and waves split the file as in k_pppm_spread (lane l: atoms l rows .. (l + 1) rows - 1, two
// consecutive ones per turn, merged into one atomic per point where they share their nearest point), but every lane walks to ITS next pair
// with a candidate on its own: the lanes of a wave stay far apart in the file, and a turn costs 125 atomics only for lanes that have work.
template <int TPB_>
__global__ __launch_bounds__(TPB_) void k_pppm_spread_tiled(const SimDev *sims, int budget) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  PppmBrick B;
  if (!pppm_brick(nx, ny, nz, budget, 0, B)) return;
  const int y0 = B.y0, z0 = B.z0, byc = B.byc, bzc = B.bzc;
  const int NG = nx * ny * nz, NB = nx * byc * bzc, T = TPB_;
  for (int k = threadIdx.x; k < NB; k += T) s_grid[k] = 0.0;
  __syncthreads();
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  const double delvolinv = (double)NG / b.vol;
  const int MD_G *pkey = pppm_keys_of(S);
  const int natoms = S.natoms, rows = (natoms + 63) >> 6, lane = threadIdx.x & 63, step = 2 * (T >> 6);
  const int cy = byc + 4, cz = bzc + 4;
  auto touches = [&](int key) { return key >= 0 && pppm_rel(PP_KEY_Y(key), y0, 2, ny) < cy && pppm_rel(PP_KEY_Z(key), z0, 2, nz) < cz; };
  int r = 2 * ((int)threadIdx.x >> 6);
  for (;;) {
    int aA = 0, kA = 0, kB = 0;
    bool vB = false, found = false;
    for (; r < rows; r += step) {
      const int a = lane * rows + r;
      if (a >= natoms) { r = rows; break; }
      const bool hasB = r + 1 < rows && a + 1 < natoms;
      const int k0 = pkey[a], k1 = hasB ? pkey[a + 1] : -1;
      const bool c0 = touches(k0), c1 = touches(k1);
      if (!c0 && !c1) continue;
      aA = c0 ? a : a + 1; kA = c0 ? k0 : k1;
      vB = c0 && c1; kB = k1;
      found = true;
      r += step;
      break;
    }
    if (!found) break;
    const int aB = aA + 1;
    double wxA[PPPM_ORDER], wyA[PPPM_ORDER], wzA[PPPM_ORDER], wxB[PPPM_ORDER] = {0, 0, 0, 0, 0}, wyB[PPPM_ORDER] = {0, 0, 0, 0, 0}, wzB[PPPM_ORDER] = {0, 0, 0, 0, 0};
    int gxA[PPPM_ORDER], gyA[PPPM_ORDER], gzA[PPPM_ORDER], gxB[PPPM_ORDER] = {0, 0, 0, 0, 0}, gyB[PPPM_ORDER] = {0, 0, 0, 0, 0}, gzB[PPPM_ORDER] = {0, 0, 0, 0, 0};
    double l0, l1, l2;
    atom_lamda(S, b, aA, l0, l1, l2);
    const int ixA = pppm_weights(l0 * nx, wxA);
    pppm_weights_at(l1 * ny, ny, PP_KEY_Y(kA), wyA); pppm_weights_at(l2 * nz, nz, PP_KEY_Z(kA), wzA);
    pppm_wrap(ixA, nx, gxA); pppm_wrap(PP_KEY_Y(kA), ny, gyA); pppm_wrap(PP_KEY_Z(kA), nz, gzA);
    const double zA = delvolinv * S.q[aA];
    double zB = 0.0;
    int ixB = -1000;
    if (vB) {
      atom_lamda(S, b, aB, l0, l1, l2);
      ixB = pppm_weights(l0 * nx, wxB);
      pppm_weights_at(l1 * ny, ny, PP_KEY_Y(kB), wyB); pppm_weights_at(l2 * nz, nz, PP_KEY_Z(kB), wzB);
      pppm_wrap(ixB, nx, gxB); pppm_wrap(PP_KEY_Y(kB), ny, gyB); pppm_wrap(PP_KEY_Z(kB), nz, gzB);
      zB = delvolinv * S.q[aB];
    }
    const bool merged = vB && ixA == ixB && kA == kB;
#pragma unroll
    for (int k = 0; k < PPPM_ORDER; k++) { wxA[k] *= zA; wxB[k] *= zB; }
#pragma unroll
    for (int c = 0; c < PPPM_ORDER; c++) {
      const int lz = gzA[c] - z0;
      if ((unsigned)lz >= (unsigned)bzc) continue;
#pragma unroll
      for (int bb = 0; bb < PPPM_ORDER; bb++) {
        const int ly = gyA[bb] - y0;
        if ((unsigned)ly >= (unsigned)byc) continue;
        const double zyA = wzA[c] * wyA[bb], zyB = merged ? wzB[c] * wyB[bb] : 0.0;
        double *prow = s_grid + (lz * byc + ly) * nx;
#pragma unroll
        for (int k = 0; k < PPPM_ORDER; k++)
          (void)__hip_atomic_fetch_add(prow + gxA[k], fma(zyB, wxB[k], zyA * wxA[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    if (vB && !merged) {
#pragma unroll
      for (int c = 0; c < PPPM_ORDER; c++) {
        const int lz = gzB[c] - z0;
        if ((unsigned)lz >= (unsigned)bzc) continue;
#pragma unroll
        for (int bb = 0; bb < PPPM_ORDER; bb++) {
          const int ly = gyB[bb] - y0;
          if ((unsigned)ly >= (unsigned)byc) continue;
          const double zyB = wzB[c] * wyB[bb];
          double *prow = s_grid + (lz * byc + ly) * nx;
#pragma unroll
          for (int k = 0; k < PPPM_ORDER; k++) (void)__hip_atomic_fetch_add(prow + gxB[k], zyB * wxB[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    }
  }
  __syncthreads();
  double2 *rho = (double2 *)S.pgrid;
  for (int k = threadIdx.x; k < NB; k += T) {
    const int row = k / nx, x = k - row * nx, lz = row / byc, ly = row - lz * byc;
    rho[((z0 + lz) * ny + y0 + ly) * nx + x] = make_double2(s_grid[k], 0.0);
  }
}

// Interpolation, gather: the workgroup stages the three field grids over its brick and a halo of two rows on each tiled side (staged row
// i of plane j holds mesh row y0 - 2 + i of plane z0 - 2 + j, wrapped; an axis that is not tiled is staged as it lies) and serves exactly the
// atoms whose home it is: their stencils need no wrap in a tiled dimension, and each atom is written by one workgroup.  Every thread walks
// the key list to ITS next home atom on its own (thread t: atoms t, t + T, ...).  add and uncharged atoms as in k_pppm_force.
template <int TPB_, bool REALF>
__global__ __launch_bounds__(TPB_) void k_pppm_force_tiled(const SimDev *sims, int budget, int add) {
  const SimDev &S = sims[blockIdx.y];
  const int nx = S.pg[0], ny = S.pg[1], nz = S.pg[2];
  if (nx == 0) return;
  PppmBrick B;
  if (!pppm_brick(nx, ny, nz, budget, 1, B)) return;
  const int y0 = B.y0, z0 = B.z0, byc = B.byc, bzc = B.bzc, hy = B.hy, hz = B.hz;
  const int sy = byc + hy, sz = bzc + hz, SN = nx * sy * sz, T = TPB_;
  const size_t gs = (size_t)S.pgstride;
  const double2 *ex = (const double2 *)S.pfield, *ey = ex + gs, *ez = ey + gs;
  const double *fr = (const double *)S.pfield;
  for (int k = threadIdx.x; k < SN; k += T) {
    const int row = k / nx, x = k - row * nx, j = row / sy, i = row - j * sy;
    const int g = ((hz ? pppm_mod(z0 - 2 + j, nz) : j) * ny + (hy ? pppm_mod(y0 - 2 + i, ny) : i)) * nx + x;
    if (REALF) { s_grid[k] = fr[g]; s_grid[SN + k] = fr[gs + g]; s_grid[2 * SN + k] = fr[2 * gs + g]; }
    else { s_grid[k] = ex[g].x; s_grid[SN + k] = ey[g].x; s_grid[2 * SN + k] = ez[g].x; }
  }
  __syncthreads();
  BoxD b;
  box_derive(S.sc->box, b);
  box_uniform(b);
  const int MD_G *pkey = pppm_keys_of(S);
  const int natoms = S.natoms;
  int a = threadIdx.x;
  for (;;) {
    int key = 0;
    for (; a < natoms; a += T) {
      key = pkey[a];
      if ((unsigned)(PP_KEY_Y(key) - y0) < (unsigned)byc && (unsigned)(PP_KEY_Z(key) - z0) < (unsigned)bzc) break;
    }
    if (a >= natoms) break;
    const int at = a;
    a += T;
    if (key < 0) {
      if (!add) { S.f[3 * at] = 0.0; S.f[3 * at + 1] = 0.0; S.f[3 * at + 2] = 0.0; }
      continue;
    }
    double l0, l1, l2;
    atom_lamda(S, b, at, l0, l1, l2);
    double wx[PPPM_ORDER], wy[PPPM_ORDER], wz[PPPM_ORDER];
    int gx[PPPM_ORDER], jy[PPPM_ORDER], jz[PPPM_ORDER];
    const int iy = PP_KEY_Y(key), iz = PP_KEY_Z(key);
    pppm_wrap(pppm_weights(l0 * nx, wx), nx, gx);
    pppm_weights_at(l1 * ny, ny, iy, wy); pppm_weights_at(l2 * nz, nz, iz, wz);
    pppm_wrap(iy, ny, jy); pppm_wrap(iz, nz, jz);
#pragma unroll
    for (int k = 0; k < PPPM_ORDER; k++) { if (hy) jy[k] = iy - y0 + k; if (hz) jz[k] = iz - z0 + k; }
    double fx = 0.0, fy = 0.0, fz = 0.0;
#pragma unroll
    for (int c = 0; c < PPPM_ORDER; c++) {
#pragma unroll
      for (int bb = 0; bb < PPPM_ORDER; bb++) {
        const double zy = wz[c] * wy[bb];
        const int row = (jz[c] * sy + jy[bb]) * nx;
        double rx = 0.0, ry = 0.0, rz = 0.0;
#pragma unroll
        for (int k = 0; k < PPPM_ORDER; k++) {
          const int g = row + gx[k];
          rx = fma(wx[k], s_grid[g], rx); ry = fma(wx[k], s_grid[SN + g], ry); rz = fma(wx[k], s_grid[2 * SN + g], rz);
        }
        fx = fma(zy, rx, fx); fy = fma(zy, ry, fy); fz = fma(zy, rz, fz);
      }
    }
    const double qf = MD_QQRD2E * S.q[at];
    if (add) { S.f[3 * at] += qf * fx; S.f[3 * at + 1] += qf * fy; S.f[3 * at + 2] += qf * fz; }
    else { S.f[3 * at] = qf * fx; S.f[3 * at + 1] = qf * fy; S.f[3 * at + 2] = qf * fz; }
  }
}


size_t mdk_pppm_lds_limit() { return 144 * 1024; }
// atom ranges per replica: enough workgroups to fill the 256 CUs several times over, none with fewer than 256 atoms
static inline int pppm_split(int ns, int maxatoms) {
  // small batches: down to one atom per thread (a single replica: spreading 27 -> 15 us, interpolation 27 -> 20 us)
  return std::max(1, std::min(std::min(ns < 32 ? 64 : 16, cdiv(2048, ns)), maxatoms / 256));
}
// which kernel shape a launch takes (md_pppm.h): the budget of the launch stands for mdk_pppm_lds_limit() in the whole-mesh tests
static inline size_t pppm_budget(const PppmLaunch *tl) { return tl && tl->budget > 0 ? (size_t)tl->budget : mdk_pppm_lds_limit(); }
static inline bool pppm_padx(int maxgridp, const PppmLaunch *tl) {
  static const bool padx_off = scema_env("SCEMA_MD_PPPM_PADX") && atoi(scema_env("SCEMA_MD_PPPM_PADX")) == 0;
  return maxgridp > 0 && !padx_off && (size_t)maxgridp * sizeof(double) <= std::min((size_t)36 * 1024, pppm_budget(tl));   // (7 / 19 kB of LDS for 12 x 12 x 12 points: no workgroup fewer)
}
int mdk_pppm_spread_path(int maxgrid, int maxgridp, const PppmLaunch *tl) {
  const size_t lds = (size_t)(pppm_padx(maxgridp, tl) ? maxgridp : maxgrid) * sizeof(double);
  if (lds <= pppm_budget(tl)) return 0;
  return tl && tl->mode != 0 && tl->sp_tiles > 0 ? 1 : 2;
}
int mdk_pppm_force_path(int maxgrid, const PppmLaunch *tl) {
  if (3 * (size_t)maxgrid * sizeof(double) <= pppm_budget(tl)) return 0;
  return tl && tl->mode != 0 && tl->fo_tiles > 0 ? 1 : 2;
}
int mdk_pppm_binned_ok(int maxgrid, int maxgridp, const PppmLaunch *tl) {
  // (the lists lie where the keys of the tiled kernels lie: not beside a tiled interpolation, which reads its keys after the spreading)
  return mdk_pppm_spread_path(maxgrid, maxgridp, tl) == 0 && pppm_padx(maxgridp, tl) && mdk_pppm_force_path(maxgrid, tl) != 1;
}
void mdk_pppm_keys(hipStream_t st, const SimDev *d, int ns, int maxatoms) { hipLaunchKernelGGL(k_pppm_keys, grid2(cdiv(maxatoms, 256), ns), dim3(256), 0, st, d); }
int mdk_pppm_spread(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxatoms, int zeroed, int maxgridp, const PppmLaunch *tl) {
  // maxgridp: the largest grid with five more points per x row (0: a grid of the batch has fewer than five points in x): the padded LDS copy
  const bool padx = pppm_padx(maxgridp, tl);
  const size_t lds = (size_t)(padx ? maxgridp : maxgrid) * sizeof(double);
  const int path = mdk_pppm_spread_path(maxgrid, maxgridp, tl);
  if (path == 1) {   // bricks of the mesh in LDS, owner computes (the keys of this step are in place: mdk_pppm_keys)
    const size_t tlds = tl->sp_lds;
    static size_t optin_tab[16] = {0};
    size_t &optin = lds_optin_slot(optin_tab);
    if (tlds > 64 * 1024 && tlds > optin) { (void)hipFuncSetAttribute((const void *)k_pppm_spread_tiled<PP_TPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tlds); optin = tlds; }
    if (tlds <= 36 * 1024) hipLaunchKernelGGL((k_pppm_spread_tiled<256>), grid2(tl->sp_tiles, ns), dim3(256), tlds, st, d, tl->budget);
    else hipLaunchKernelGGL((k_pppm_spread_tiled<PP_TPB>), grid2(tl->sp_tiles, ns), dim3(PP_TPB), tlds, st, d, tl->budget);
    return path;
  }
  const bool use_lds = path == 0;
  const int split = pppm_split(ns, maxatoms);
  if ((!use_lds || split > 1) && !zeroed) hipLaunchKernelGGL(k_pppm_zero, grid2(cdiv(maxgrid, 256), ns), dim3(256), 0, st, d);
  if (tl && tl->binned && mdk_pppm_binned_ok(maxgrid, maxgridp, tl)) {   // the atoms by nearest grid point first, then an item of them per lane
    hipLaunchKernelGGL(k_pppm_bins, dim3(ns), dim3(PP_BIN_TPB), 2 * (size_t)maxgridp * sizeof(int), st, d, PP_BIN_M);
    hipLaunchKernelGGL((k_pppm_spread_binned<PP_BIN_M>), grid2(split, ns), dim3(256), lds, st, d, split);
    return path;
  }
  if (!use_lds) {
    hipLaunchKernelGGL((k_pppm_spread<false, 256>), grid2(split, ns), dim3(256), 0, st, d, split);
    return path;
  }
  static size_t optin_tab[16] = {0};
  size_t &optin = lds_optin_slot(optin_tab);
  if (lds > 64 * 1024 && lds > optin) { (void)hipFuncSetAttribute((const void *)k_pppm_spread<true, PP_TPB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); optin = lds; }
  // a small grid leaves room for several workgroups per CU; a large one gets the CU to itself and brings its own sixteen waves
  if (padx) hipLaunchKernelGGL((k_pppm_spread<true, 256, true>), grid2(split, ns), dim3(256), lds, st, d, split);
  else if (lds <= 36 * 1024) hipLaunchKernelGGL((k_pppm_spread<true, 256>), grid2(split, ns), dim3(256), lds, st, d, split);
  else hipLaunchKernelGGL((k_pppm_spread<true, PP_TPB>), grid2(split, ns), dim3(PP_TPB), lds, st, d, split);
  return path;
}
int mdk_pppm_solve_max() { return PP_SOLVE_MAX; }
void mdk_pppm_solve(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxdims) {
  // batches: the shape that fits beside a pair workgroup; a few replicas: the one with the most threads per replica
  static const int shape_env = scema_env("SCEMA_MD_PPPM_SOLVE_WIDE") ? atoi(scema_env("SCEMA_MD_PPPM_SOLVE_WIDE")) : -1;
  const bool wide = shape_env < 0 ? ns < 8 : shape_env != 0;
  static const int two_env = scema_env("SCEMA_MD_PPPM_SOLVE_TWO") ? atoi(scema_env("SCEMA_MD_PPPM_SOLVE_TWO")) : -1;
  const bool two = wide && (two_env < 0 ? ns < 8 : two_env != 0);   // two workgroups per replica, one per transform back (the shape with rho(k) in LDS)
  const size_t lds = ((wide ? 3 : 2) * (size_t)maxgrid + (size_t)maxdims) * sizeof(double2);
  static size_t optin_tab[2][16] = {{0}, {0}};
  size_t &optin = lds_optin_slot(optin_tab[wide ? 1 : 0]);
  if (wide) {
    if (lds > 64 * 1024 && lds > optin) { (void)hipFuncSetAttribute((const void *)k_pppm_solve<1024, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); optin = lds; }
    hipLaunchKernelGGL((k_pppm_solve<1024, false>), dim3(ns, two ? 2 : 1), dim3(1024), lds, st, d);
  } else {
    if (lds > 64 * 1024 && lds > optin) { (void)hipFuncSetAttribute((const void *)k_pppm_solve<512, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); optin = lds; }
    hipLaunchKernelGGL((k_pppm_solve<512, true>), dim3(ns), dim3(512), lds, st, d);
  }
}
void mdk_pppm_gf(hipStream_t st, const SimDev *d, int ns, int maxgrid) { hipLaunchKernelGGL(k_pppm_gf, grid2(cdiv(maxgrid, 256), ns), dim3(256), 0, st, d); }
void mdk_pppm_poisson(hipStream_t st, const SimDev *d, int ns, int maxgrid) { hipLaunchKernelGGL(k_pppm_poisson, grid2(cdiv(maxgrid, 256), ns), dim3(256), 0, st, d); }
int mdk_pppm_force(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxatoms, int add, int real_fields, const PppmLaunch *tl) {
  size_t lds = 3 * (size_t)maxgrid * sizeof(double);
  const int path = mdk_pppm_force_path(maxgrid, tl);
  if (path == 1) {   // the field grids over a brick and its halo in LDS, every atom served by its home tile (keys: mdk_pppm_keys)
    const size_t tlds = tl->fo_lds;
    static size_t optin_tab[16] = {0};
    size_t &optin = lds_optin_slot(optin_tab);
    if (tlds > 64 * 1024 && tlds > optin) {
      (void)hipFuncSetAttribute((const void *)k_pppm_force_tiled<PP_TPB, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tlds);
      (void)hipFuncSetAttribute((const void *)k_pppm_force_tiled<PP_TPB, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tlds);
      optin = tlds;
    }
    const dim3 g = grid2(tl->fo_tiles, ns);
    // (a large copy gets the CU to itself and brings its own sixteen waves, as in the spreading kernels)
    if (tlds <= 36 * 1024) {
      if (real_fields) hipLaunchKernelGGL((k_pppm_force_tiled<256, true>), g, dim3(256), tlds, st, d, tl->budget, add);
      else hipLaunchKernelGGL((k_pppm_force_tiled<256, false>), g, dim3(256), tlds, st, d, tl->budget, add);
    } else {
      if (real_fields) hipLaunchKernelGGL((k_pppm_force_tiled<PP_TPB, true>), g, dim3(PP_TPB), tlds, st, d, tl->budget, add);
      else hipLaunchKernelGGL((k_pppm_force_tiled<PP_TPB, false>), g, dim3(PP_TPB), tlds, st, d, tl->budget, add);
    }
    return path;
  }
  if (path == 2) {
    // (real field arrays without LDS: only under a forced budget -- a mesh of the in-LDS solve always fits the device's)
    if (real_fields) hipLaunchKernelGGL((k_pppm_force<false, true>), grid2(cdiv(maxatoms, 256), ns), dim3(256), 0, st, d, cdiv(maxatoms, 256), add, 0, 0);
    else hipLaunchKernelGGL((k_pppm_force<false, false>), grid2(cdiv(maxatoms, 256), ns), dim3(256), 0, st, d, cdiv(maxatoms, 256), add, 0, 0);
    return path;
  }
  // the staged copy in the layout of md_pppm_fstride.h: the launch takes the largest padded size of its meshes (PppmLaunch::fs_lds, by
  // the same rule and budget the kernel evaluates per replica); without it every replica keeps the dense layout
  const int fs_budget = tl && tl->fs_lds >= lds && tl->fs_lds <= pppm_budget(tl) ? (int)pppm_budget(tl) : 0;
  if (fs_budget > 0) lds = tl->fs_lds;
  static size_t optin_tab[16] = {0};
  size_t &optin = lds_optin_slot(optin_tab);
  if (lds > 64 * 1024 && lds > optin) {
    (void)hipFuncSetAttribute((const void *)k_pppm_force<true, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void *)k_pppm_force<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void *)k_pppm_force<true, false, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void *)k_pppm_force<true, true, 512>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    optin = lds;
  }
  const int split = pppm_split(ns, maxatoms);
  // Block size: 512 threads with the strided layout, the parent's 256 with the dense one (SCEMA_MD_PPPM_FTPB forces either).  At 95
  // registers 256 threads are 3 x 4 waves per CU beside three 41 KB copies, 512 threads 2 x 8; the kernel gains from the fourth wave per
  // SIMD only once its reads no longer queue on the banks (576 x PE-10k: dense 432 / 426 us per step at 256 / 512 threads, strided 352 / 325)
  static const int ftpb_env = scema_env("SCEMA_MD_PPPM_FTPB") ? atoi(scema_env("SCEMA_MD_PPPM_FTPB")) : 0;
  const int tpb = ftpb_env == 256 || ftpb_env == 512 ? ftpb_env : (fs_budget > 0 ? 512 : 256);
  const dim3 g = grid2(split, ns);
#define PP_FORCE_LAUNCH(R, T) hipLaunchKernelGGL((k_pppm_force<true, R, T>), g, dim3(T), lds, st, d, split, add, fs_budget, (int)lds)
  if (tpb == 512) { if (real_fields) PP_FORCE_LAUNCH(true, 512); else PP_FORCE_LAUNCH(false, 512); }
  else { if (real_fields) PP_FORCE_LAUNCH(true, 256); else PP_FORCE_LAUNCH(false, 256); }
#undef PP_FORCE_LAUNCH
  return path;
}
