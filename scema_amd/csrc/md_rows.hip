// md_rows.hip -- gfx950 kernels of the row part every force stage on full neighbour rows shares (the Stillinger-Weber, the Tersoff and the
// embedded-atom stage: md_sw.hip, md_tersoff.hip, md_eam.hip).  The integrator, thermostat, fix deform, pressure sampling and the batch
// machinery are the ones of the OPLS path (md_kernels.hip); only the force stage differs, as for ReaxFF (md_reax.hip).  One launch covers
// every replica of the batch (blockIdx.y).
//   k_row_prepare .. box -> view, rebuild bookkeeping, zero the step's sums
//   k_row_wrap ..... zero the forces; at a rebuild wrap the atoms into the box (image counts keep the unwrapped information)
//   k_row_build .... full neighbour rows inside cutoff + skin, rebuilt when the engine's displacement test says so (`neighbor 1.0 nsq`,
//                    `neigh_modify every 1 delay 0 check yes`): an N^2 search, the replica's positions streamed through LDS.  Replicas
//                    marked RowView::cells get the same rows from the cell kernels instead (md_rowcells.hip, launched from mdk_rows_build)
//   k_row_finish ... energies and fault bits into the engine's scalars
// and the launch sequence of a stage around its force kernels (mdk_row_forces).
// Row entries carry an image code in the convention of the ReaxFF rows (md_row_entry.h): the shift of an entry is code . h with the box of
// the STEP, so the rows hold while fix deform remaps the atoms with the box; a box flip forces a rebuild.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "md_kernels.h"
#include "md_rowforce.h"

#define ROW_BUILD_TPB 512    /* row build: 8 waves of 8 rows */
#define ROW_NBR 8
#define ROW_JT 512           /* partners staged in LDS per pass of the row build */
static_assert(ROW_TILE == 64 && ROW_BUILD_TPB / 64 * ROW_NBR == ROW_TILE, "tile shapes of md_rows.hip");

__global__ void k_row_prepare(const SimDev *sims, RowView *views) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  RowView &V = views[blockIdx.x];
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

__global__ __launch_bounds__(TPB) void k_row_wrap(const SimDev *sims, const RowView *views) {
  const SimDev &S = sims[blockIdx.y];
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  S.f[3 * i] = 0.0; S.f[3 * i + 1] = 0.0; S.f[3 * i + 2] = 0.0;
  if (!S.sc->rebuild) return;
  const RowView &V = views[blockIdx.y];
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

// Neighbour rows: a workgroup owns ROW_TILE consecutive atoms, wave w their rows 8 w .. 8 w + 7; the replica's positions pass through LDS
// ROW_JT at a time, the wave's lanes over the staged partners 64 at a time.  A chunk's accepted partners leave as one contiguous store into
// the row (ballot + lane rank): rows come out sorted by partner (with several images per partner, image-major inside a chunk) whatever
// the schedule.  An entry is written only below the row's capacity; the count is clamped; a row that asked for more raises fault bit 1 and
// reports what it asked for, so the regrow-and-retry of the host finds the capacity in one step.
__global__ __launch_bounds__(ROW_BUILD_TPB) void k_row_build(const SimDev *sims, const RowView *views) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  const RowView &V = views[blockIdx.y];
  if (V.cells) return;   // (its rows come from k_cell_rows, md_rowcells.hip)
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup: no barrier is left waiting)
  __shared__ double s_x[3][ROW_JT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cap = V.cap;
  const int r0 = blockIdx.x * ROW_TILE + wave * ROW_NBR;
  const int nr = max(0, min(ROW_NBR, n - r0));      // (a wave without rows still stages and waits at the barriers)
  const double rl2 = V.rlist * V.rlist;
  const double h0 = wave_uniform(V.h[0]), h1 = wave_uniform(V.h[1]), h2 = wave_uniform(V.h[2]), h3 = wave_uniform(V.h[3]), h4 = wave_uniform(V.h[4]),
               h5 = wave_uniform(V.h[5]);
  const double ih0 = 1.0 / h0, ih1 = 1.0 / h1, ih2 = 1.0 / h2;
  const int m0 = V.mimg[0], m1 = V.mimg[1], m2 = V.mimg[2];
  const bool minimage = (m0 | m1 | m2) == 0;
  double xr[ROW_NBR], yr[ROW_NBR], zr[ROW_NBR];
  int len[ROW_NBR];
#pragma unroll
  for (int g = 0; g < ROW_NBR; g++) {
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
  for (int t0 = 0; t0 < n; t0 += ROW_JT) {
    __syncthreads();   // (the pass before has been read)
    for (int k = threadIdx.x; k < ROW_JT; k += ROW_BUILD_TPB) {
      const int j = min(t0 + k, n - 1);
      s_x[0][k] = S.x[3 * j]; s_x[1][k] = S.x[3 * j + 1]; s_x[2][k] = S.x[3 * j + 2];
    }
    __syncthreads();
    const int tn = min(ROW_JT, n - t0);
    for (int c0 = 0; c0 < tn; c0 += 64) {
      const int k = c0 + lane;                 // < ROW_JT: c0 < tn <= ROW_JT, both multiples of 64 or the last chunk
      const bool jl = k < tn;
      const int j = t0 + k;
      const double xj = s_x[0][k], yj = s_x[1][k], zj = s_x[2][k];
#pragma unroll
      for (int g = 0; g < ROW_NBR; g++) {
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
  for (int g = 0; g < ROW_NBR; g++) {
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

// energies and fault bits of the step into the engine's scalars: row full -> bit 1 (the host regrows and retries), crowded -> bit 128
__global__ void k_row_finish(const SimDev *sims, const RowView *views) {
  const RowView &V = views[blockIdx.x];
  SimScalars &sc = *sims[blockIdx.x].sc;
  if (threadIdx.x != 0) return;
  sc.eng[P_LJ] = V.eacc[0];
  sc.eng[P_ANGLE] = V.eacc[1];
  const int st = V.stat[0];
  if (st) atomicOr(&sc.overflow, ((st & 1) ? 1 : 0) | ((st & 2) ? 128 : 0));
}

static inline int cdv(int a, int b) { return (a + b - 1) / b; }

// the view array the calling thread's stage has bound last (mdk_rows_cells): its replicas on the cell path as a running count by position
namespace {
struct RowCellsBound {
  const RowView *views = nullptr;
  const RowCells *cells = nullptr;
  std::vector<int> upto;   // [ns + 1]
};
thread_local RowCellsBound t_bound;
thread_local long t_cell_groups = 0;
}  // namespace

void mdk_rows_cells(const RowView *views, const RowCells *cells, const unsigned char *on, int ns) {
  t_bound.views = views;
  t_bound.cells = cells;
  t_bound.upto.assign((size_t)std::max(ns, 0) + 1, 0);
  for (int k = 0; k < ns; k++) t_bound.upto[k + 1] = t_bound.upto[k] + (on[k] ? 1 : 0);
}

long mdk_rows_cell_groups() { return t_cell_groups; }

void mdk_rows_build(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  if (ns <= 0 || maxatoms <= 0) return;
  const dim3 gt((unsigned)cdv(maxatoms, ROW_TILE), (unsigned)ns, 1);
  hipLaunchKernelGGL(k_row_prepare, dim3(ns), dim3(64), 0, st, d, v);
  hipLaunchKernelGGL(k_row_wrap, dim3((unsigned)cdv(maxatoms, TPB), (unsigned)ns, 1), dim3(TPB), 0, st, d, v);
  // replicas of this group whose rows are built through cells: none unless the group lies inside the array the stage has bound
  int oncells = 0;
  const RowCellsBound &B = t_bound;
  const long nb = (long)B.upto.size() - 1;
  if (B.views && nb > 0 && v >= B.views && v - B.views + ns <= nb) {
    const long p0 = v - B.views;
    oncells = B.upto[p0 + ns] - B.upto[p0];
    if (oncells > 0) {
      mdk_rowcells_build(st, d, v, B.cells + p0, ns, maxatoms);
      t_cell_groups += 1;
    }
  }
  if (oncells < ns) hipLaunchKernelGGL(k_row_build, gt, dim3(ROW_BUILD_TPB), 0, st, d, v);
}

void mdk_rows_finish(hipStream_t st, const SimDev *d, RowView *v, int ns) {
  if (ns > 0) hipLaunchKernelGGL(k_row_finish, dim3(ns), dim3(64), 0, st, d, v);
}

void mdk_row_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms, RowForceKernel lacc, RowForceKernel direct) {
  if (ns <= 0 || maxatoms <= 0) return;
  const dim3 gt((unsigned)cdv(maxatoms, ROW_TILE), (unsigned)ns, 1);
  mdk_rows_build(st, d, v, ns, maxatoms);
  const int maxpad = (maxatoms + 63) / 64 * 64;
  if (maxpad <= ROW_LDS_MAXPAD) hipLaunchKernelGGL(lacc, gt, dim3(ROW_FORCE_TPB), 3 * (size_t)maxpad * sizeof(double), st, d, v);
  else hipLaunchKernelGGL(direct, gt, dim3(ROW_FORCE_TPB), 0, st, d, v);
  mdk_rows_finish(st, d, v, ns);
}
