// md_born_long_mesh.hip -- gfx950 kernels of the mesh reciprocal solver of the Ewald ionic force stage: PPPM (order 5, ik
// differentiation, the optimal influence function of the step's box) on the row layout, for the replicas beyond the k list of
// md_born_long.hip.  The arithmetic is pppm/pppm_core.h and ionic/blm_core.h; the transforms between the kernels are the engine's batched hipFFT plans.  One
// launch covers every replica of the group (blockIdx.y); a replica on the Ewald sum (BlmView::n = 0) is left alone by every kernel.
//   k_blm_assign ... every atom adds its 125 weighted charges q w_x w_y w_z NG/V to the replica's 64-bit FIXED-POINT grid with integer
//                    atomics: integer addition commutes, so the grid does not depend on arrival order, launch shape or batch composition.
//                    A wave takes one atom at a time, a lane one of its 125 points (two passes), x fastest: a wave instruction adds to 13
//                    runs of five consecutive points in 13 rows
//   k_blm_convert .. fixed point -> the complex grid (re = v 2^-s, im = 0); zeroes the fixed-point grid for the next step
//   k_blm_gf ....... the influence function of the step's box, launched on the steps whose box changed
//   k_blm_poisson .. after the forward transform: per mode the energy and virial share and the three field spectra -i k G rho~(k); one
//                    thread adds the self and background terms; one atomic per workgroup and value (eacc[1], P_COUL)
//   k_blm_interp ... after the backward transforms: adds K q_i sum w E(grid) to f, in the launch shape of k_bl_recip: 16 lanes per atom, lane
//                    l the points l, l + 16, ... of the 125 in ascending order, row_sum, one writer per atom, no atomic on a force
// Every sum that reaches a force has a fixed order or is an integer sum: two evaluations of one state give the same forces bit for bit.
// Every index, mesh dimension and count is clamped to what the buffers hold (blm_shape).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "md_born_long_mesh.h"
#include "md_kernels.h"
#include "md_rowforce.h"

#define BLM_TPB 256
#define BLM_NPT (PPPM_ORDER * PPPM_ORDER * PPPM_ORDER)
static_assert(PPPM_ORDER == 5 && BLM_NPT <= 128, "two passes of a wave cover an atom's stencil");

// what the kernels take from a BlmView: a mesh whose dimensions or product the buffers do not hold counts as none
struct BlmShape { int n[3], ng; };
__device__ __forceinline__ BlmShape blm_shape(const BlmView &M) {
  BlmShape s;
  const long long ng = (long long)M.n[0] * (long long)M.n[1] * (long long)M.n[2];
  bool ok = ng > 0 && ng <= (long long)min(max(M.gcap, 0), BLM_MAXGRID);
  for (int d = 0; d < 3; d++) ok = ok && M.n[d] >= 2 && M.n[d] <= BLM_MAXDIM;
  for (int d = 0; d < 3; d++) s.n[d] = ok ? M.n[d] : 0;
  s.ng = ok ? (int)ng : 0;
  return s;
}
__device__ __forceinline__ void blm_box(const RowView &V, double *h, double *lo) {
  for (int k = 0; k < 6; k++) h[k] = V.h[k];
  for (int k = 0; k < 3; k++) lo[k] = V.lo[k];
}
// w[k] of a runtime k in 0 .. 4 without an indexed register array
__device__ __forceinline__ double blm_pick(const double (&w)[PPPM_ORDER], int k) {
  return k == 0 ? w[0] : (k == 1 ? w[1] : (k == 2 ? w[2] : (k == 3 ? w[3] : w[4])));
}
// the stencil of atom i: weights per dimension and the nearest grid point per dimension
__device__ __forceinline__ void blm_stencil(const RowView &V, const BlmShape &sh, const double *h, const double *lo, int i, double (&wx)[PPPM_ORDER],
                                            double (&wy)[PPPM_ORDER], double (&wz)[PPPM_ORDER], int &ix, int &iy, int &iz) {
  const double x[3] = {V.x[3 * i], V.x[3 * i + 1], V.x[3 * i + 2]};
  double t[3];
  blm_frac(h, lo, x, t);
  ix = min(max(pppm_weights(t[0] * sh.n[0], wx), 0), sh.n[0]);
  iy = min(max(pppm_weights(t[1] * sh.n[1], wy), 0), sh.n[1]);
  iz = min(max(pppm_weights(t[2] * sh.n[2], wz), 0), sh.n[2]);
}
// point p of 125 (x fastest) of that stencil: its grid index and the product of its weights
__device__ __forceinline__ int blm_point(const BlmShape &sh, int p, const double (&wx)[PPPM_ORDER], const double (&wy)[PPPM_ORDER], const double (&wz)[PPPM_ORDER],
                                         int ix, int iy, int iz, double &w) {
  const int c = p / 25, r = p - 25 * c, b = r / 5, k = r - 5 * b;
  w = blm_pick(wz, c) * blm_pick(wy, b) * blm_pick(wx, k);
  const int gx = pppm_wrap1(ix + k - 2, sh.n[0]), gy = pppm_wrap1(iy + b - 2, sh.n[1]), gz = pppm_wrap1(iz + c - 2, sh.n[2]);
  return min((gz * sh.n[1] + gy) * sh.n[0] + gx, sh.ng - 1);
}

__global__ __launch_bounds__(BLM_TPB) void k_blm_assign(const SimDev *sims, const RowView *views, const BlmView *mesh) {
  const BlmView M = mesh[blockIdx.y];
  const BlmShape sh = blm_shape(M);
  if (sh.ng == 0) return;
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;
  const double MD_G *q = sims[blockIdx.y].q;
  double h[6], lo[3];
  blm_box(V, h, lo);
  const double vol = h[0] * h[1] * h[2], delvolinv = (double)sh.ng / vol;
  const int shift = blm_fixed_shift(M.qabs, sh.ng, vol);
  unsigned long long *grid = (unsigned long long *)M.igrid;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int per_wave = ROW_TILE / (BLM_TPB / 64);
  for (int it = 0; it < per_wave; it++) {
    const int i = blockIdx.x * ROW_TILE + wave * per_wave + it;
    if (i >= n) break;   // (uniform over the wave)
    const double z = q[i] * delvolinv;
    if (z == 0.0) continue;
    double wx[PPPM_ORDER], wy[PPPM_ORDER], wz[PPPM_ORDER];
    int ix, iy, iz;
    blm_stencil(V, sh, h, lo, i, wx, wy, wz, ix, iy, iz);
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
      const int p = lane + 64 * pass;
      if (p < BLM_NPT) {
        double w;
        const int g = blm_point(sh, p, wx, wy, wz, ix, iy, iz, w);
        atomicAdd(&grid[g], (unsigned long long)blm_to_fixed(z * w, shift));   // (two's complement: the wrapped sum is the signed sum)
      }
    }
  }
}

__global__ __launch_bounds__(BLM_TPB) void k_blm_convert(const RowView *views, const BlmView *mesh) {
  const BlmView M = mesh[blockIdx.y];
  const BlmShape sh = blm_shape(M);
  const int idx = blockIdx.x * BLM_TPB + threadIdx.x;
  if (idx >= sh.ng) return;
  const RowView &V = views[blockIdx.y];
  const double vol = V.h[0] * V.h[1] * V.h[2];
  const int shift = blm_fixed_shift(M.qabs, sh.ng, vol);
  const long long v = M.igrid[idx];
  M.igrid[idx] = 0;
  M.cgrid[2 * (size_t)idx] = blm_from_fixed(v, shift);
  M.cgrid[2 * (size_t)idx + 1] = 0.0;
}

__global__ __launch_bounds__(BLM_TPB) void k_blm_gf(const RowView *views, const BlmView *mesh) {
  const BlmView M = mesh[blockIdx.y];
  const BlmShape sh = blm_shape(M);
  const int idx = blockIdx.x * BLM_TPB + threadIdx.x;
  if (idx >= sh.ng) return;
  double hinv[6];
  bl_hinv(views[blockIdx.y].h, hinv);
  const int m1 = idx % sh.n[0], m2 = (idx / sh.n[0]) % sh.n[1], m3 = idx / (sh.n[0] * sh.n[1]);
  M.gf[idx] = M.g > 0.0 ? pppm_gf(hinv, M.g, sh.n[0], sh.n[1], sh.n[2], m1, m2, m3) : 0.0;
}

// (no thread leaves before the sums: a thread past the mesh adds zeros)
__global__ __launch_bounds__(BLM_TPB) void k_blm_poisson(const SimDev *sims, const RowView *views, const BlmView *mesh) {
  const BlmView M = mesh[blockIdx.y];
  const BlmShape sh = blm_shape(M);
  if ((int)(blockIdx.x * BLM_TPB) >= sh.ng || !(M.g > 0.0)) return;   // (the whole workgroup)
  const RowView V = views[blockIdx.y];
  SimScalars &sc = *sims[blockIdx.y].sc;
  __shared__ double s_red[8 * (BLM_TPB / 64)];
  double h[6], lo[3];
  blm_box(V, h, lo);
  const double kc = ((const BlTable ROW_G *)V.tab)->bd.k;
  const int idx = blockIdx.x * BLM_TPB + threadIdx.x;
  double esum[1] = {0.0}, w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (idx < sh.ng) {
    const int m1 = idx % sh.n[0], m2 = (idx / sh.n[0]) % sh.n[1], m3 = idx / (sh.n[0] * sh.n[1]);
    double hinv[6], kv[3], pr, pi;
    bl_hinv(h, hinv);
    pppm_kvec(hinv, pppm_signed(m1, sh.n[0]), pppm_signed(m2, sh.n[1]), pppm_signed(m3, sh.n[2]), kv[0], kv[1], kv[2]);
    const double scaleinv = 1.0 / (double)sh.ng;
    pppm_mode_term(h[0] * h[1] * h[2], kc, M.g, kv[0], kv[1], kv[2], M.cgrid[2 * (size_t)idx] * scaleinv, M.cgrid[2 * (size_t)idx + 1] * scaleinv, M.gf[idx], w,
                   esum[0], pr, pi);
    const size_t gs = (size_t)M.gcap;
#pragma unroll
    for (int c = 0; c < 3; c++) {   // (a + i b)(-i k) = b k - i a k
      M.field[2 * (c * gs + idx)] = kv[c] * pi;
      M.field[2 * (c * gs + idx) + 1] = -kv[c] * pr;
    }
    if (idx == 0) {
      double ebg;
      esum[0] += bl_self(kc, M.g, h[0] * h[1] * h[2], M.qsqsum, M.qsum, &ebg);
      w[0] += ebg; w[1] += ebg; w[2] += ebg;
    }
  }
  block_atomic_add_n<1, BLM_TPB / 64>(esum, (double *)V.eacc + 1, s_red);
  block_atomic_add_n<6, BLM_TPB / 64>(w, &sc.vir[P_COUL * 6], s_red);
}

__global__ __launch_bounds__(ROW_FORCE_TPB) void k_blm_interp(const SimDev *sims, const RowView *views, const BlmView *mesh) {
  const BlmView M = mesh[blockIdx.y];
  const BlmShape sh = blm_shape(M);
  if (sh.ng == 0 || !(M.g > 0.0)) return;
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const double MD_G *q = sims[blockIdx.y].q;
  double h[6], lo[3];
  blm_box(V, h, lo);
  const double kc = ((const BlTable ROW_G *)V.tab)->bd.k;
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const size_t gs = (size_t)M.gcap;
  const double ROW_G *ex = M.field, *ey = M.field + 2 * gs, *ez = M.field + 4 * gs;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    double wx[PPPM_ORDER], wy[PPPM_ORDER], wz[PPPM_ORDER];
    int ix, iy, iz;
    blm_stencil(V, sh, h, lo, ic, wx, wy, wz, ix, iy, iz);
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
#pragma unroll
    for (int p = l16; p < BLM_NPT; p += 16) {
      double w;
      const size_t g = (size_t)blm_point(sh, p, wx, wy, wz, ix, iy, iz, w);
      f0 = fma(w, ex[2 * g], f0); f1 = fma(w, ey[2 * g], f1); f2 = fma(w, ez[2 * g], f2);
    }
    f0 = row_sum(f0); f1 = row_sum(f1); f2 = row_sum(f2);
    if (valid && l16 == 0) {
      const double kq = kc * q[i];
      V.f[3 * i] += kq * f0; V.f[3 * i + 1] += kq * f1; V.f[3 * i + 2] += kq * f2;
    }
  }
}

int mdk_bl_mesh_forces(hipStream_t st, const SimDev *d, RowView *v, const BlView *b, const BlmView *m, int ns, int maxatoms, int maxnk, bool ewald,
                       int maxgrid, bool new_box, BlmTransform transform, void *ctx, const std::function<void(dim3)> *real) {
  int rc = 0;
  const std::function<void(dim3)> chain = [&](dim3 gt) {
    if (maxgrid <= 0) return;
    const dim3 gg((unsigned)((maxgrid + BLM_TPB - 1) / BLM_TPB), (unsigned)ns, 1);
    hipLaunchKernelGGL(k_blm_assign, gt, dim3(BLM_TPB), 0, st, d, v, m);
    hipLaunchKernelGGL(k_blm_convert, gg, dim3(BLM_TPB), 0, st, v, m);
    if ((rc = transform(ctx, 0))) return;
    if (new_box) hipLaunchKernelGGL(k_blm_gf, gg, dim3(BLM_TPB), 0, st, v, m);
    hipLaunchKernelGGL(k_blm_poisson, gg, dim3(BLM_TPB), 0, st, d, v, m);
    if ((rc = transform(ctx, 1))) return;
    hipLaunchKernelGGL(k_blm_interp, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, m);
  };
  mdk_bl_forces(st, d, v, b, ns, maxatoms, maxnk, ewald, &chain, real);
  return rc;
}
