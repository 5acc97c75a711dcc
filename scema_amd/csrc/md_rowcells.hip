// md_rowcells.hip -- gfx950 kernels of the cell-binned row build: the neighbour rows of k_row_build (md_rows.hip), entry for
// entry, for replicas whose geometry allows a cell grid (md_rowcells.h has the rule; RowView::cells marks them, RowCells holds their
// arrays).  Both kernels run behind the rebuild flag of the step and behind k_row_prepare and k_row_wrap, blockIdx.y is the replica, and a
// replica on the N^2 build leaves them at their top.
//   k_cell_bin ..... the wrapped atoms of a replica into cells: counts, exclusive scan, fill.  One workgroup per replica, so the three
//                    phases are ordered by its barriers and need neither launches of their own nor a zeroing launch; at the sizes this
//                    path is for (thousands to tens of thousands of atoms) a workgroup of 1 024 passes over the atoms a few dozen times
//   k_cell_rows .... a wave per row: the atoms of the 27 stencil cells as one flat candidate list, 64 at a time, tested with the
//                    arithmetic of the minimum-image branch of k_row_build; accepted entries staged in LDS, ranked by counting into
//                    ascending atom index and stored into the row
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_types.h"
#include "md_device.h"
#include "md_rowcells.h"
#include "md_rows.h"

#define CELL_BIN_TPB 1024
#define CELL_ROWS_TPB 256    /* 4 waves */
#define CELL_RPW 4           /* rows a wave builds one after the other: one set of closing atomics per 4 rows */
#define CELL_WG_ROWS (CELL_ROWS_TPB / 64 * CELL_RPW)

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(CELL_BIN_TPB) void k_cell_bin(const SimDev *sims, const RowView *views, const RowCells *cells) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  const RowView &V = views[blockIdx.y];
  if (!V.cells) return;
  const RowCells &C = cells[blockIdx.y];
  __shared__ int s_scan[2][CELL_BIN_TPB];
  const int t = threadIdx.x, n = V.n, ncells = C.ncells;
  const int nc[3] = {C.nc[0], C.nc[1], C.nc[2]};
  for (int c = t; c < ncells; c += CELL_BIN_TPB) C.ccur[c] = 0;
  __threadfence();
  __syncthreads();
  // counts (the atoms are wrapped: k_row_wrap)
  const double h[6] = {V.h[0], V.h[1], V.h[2], V.h[3], V.h[4], V.h[5]}, lo[3] = {V.lo[0], V.lo[1], V.lo[2]};
  for (int i = t; i < n; i += CELL_BIN_TPB) {
    const double x[3] = {S.x[3 * i], S.x[3 * i + 1], S.x[3 * i + 2]};
    double l[3];
    rowcell_frac(x, h, lo, l);
    const int c = rowcell_index(rowcell_of(l[0], nc[0]), rowcell_of(l[1], nc[1]), rowcell_of(l[2], nc[2]), nc);
    C.cellof[i] = c;
    atomicAdd(&C.ccur[c], 1);
  }
  __threadfence();
  __syncthreads();
  // exclusive scan: a thread sums `per` consecutive cells, the workgroup scans the 1 024 sums
  const int per = (ncells + CELL_BIN_TPB - 1) / CELL_BIN_TPB;
  const int c0 = min(t * per, ncells), c1 = min(c0 + per, ncells);
  int mine = 0;
  for (int c = c0; c < c1; c++) mine += __hip_atomic_load(&C.ccur[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (the counts were added beyond this CU's cache)
  s_scan[0][t] = mine;
  __syncthreads();
  int src = 0;
  for (int off = 1; off < CELL_BIN_TPB; off <<= 1) {
    const int v = s_scan[src][t] + (t >= off ? s_scan[src][t - off] : 0);
    s_scan[1 - src][t] = v;
    __syncthreads();
    src = 1 - src;
  }
  int run = s_scan[src][t] - mine;
  for (int c = c0; c < c1; c++) {
    const int k = __hip_atomic_load(&C.ccur[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    C.cstart[c] = run;
    run += k;
  }
  if (t == 0) C.cstart[ncells] = n;
  __threadfence();
  __syncthreads();   // (every count has been read)
  for (int c = c0; c < c1; c++) C.ccur[c] = C.cstart[c];
  __threadfence();
  __syncthreads();
  // fill: the order inside a cell is the order of arrival
  for (int i = t; i < n; i += CELL_BIN_TPB) {
    const int p = atomicAdd(&C.ccur[C.cellof[i]], 1);
    if ((unsigned)p < (unsigned)n) C.clist[p] = i;
  }
}

// Rows through cells.  A workgroup takes CELL_WG_ROWS consecutive places of the cell list, so its rows share their stencil in the caches;
// a wave builds its rows one after the other.  Lanes 0 .. 26 hold the stencil's cells as ranges of the cell list, a scan over them makes
// the candidates one flat list, and a lane finds its candidate's range by bisection of the 32 offsets in LDS.  Acceptance and entry word
// are those of k_row_build to the bit: d = x_j - x_i, rint reductions in z, y, x order, !(r2 > rl2), code 2 - n, the `coded` test, j != i.
// An atom lies in one cell and the 27 cells are distinct (3 and more per dimension), so a row holds a partner once and ranking by atom
// index is a permutation.  A row that asks for more than its capacity keeps `cap` of its entries (not the first in atom order, as
// k_row_build would: the host regrows and retries either way), its count is clamped, fault bit 1 and the unclamped length are reported
// as there.  The barriers order a wave's own LDS traffic; no wave reads another's.
__global__ __launch_bounds__(CELL_ROWS_TPB) void k_cell_rows(const SimDev *sims, const RowView *views, const RowCells *cells) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  const RowView &V = views[blockIdx.y];
  if (!V.cells) return;
  const int n = V.n;
  if ((int)(blockIdx.x * CELL_WG_ROWS) >= n) return;   // (the whole workgroup: no barrier is left waiting)
  const RowCells &C = cells[blockIdx.y];
  __shared__ int s_row[CELL_ROWS_TPB / 64][ROWCELL_MAXCAP];
  __shared__ int s_off[CELL_ROWS_TPB / 64][32], s_beg[CELL_ROWS_TPB / 64][32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cap = V.cap, capst = min(cap, ROWCELL_MAXCAP);
  const int nx = C.nc[0], ny = C.nc[1], nz = C.nc[2], ncells = C.ncells;
  const double rl2 = V.rlist * V.rlist;
  const double h0 = wave_uniform(V.h[0]), h1 = wave_uniform(V.h[1]), h2 = wave_uniform(V.h[2]), h3 = wave_uniform(V.h[3]), h4 = wave_uniform(V.h[4]),
               h5 = wave_uniform(V.h[5]);
  const double ih0 = 1.0 / h0, ih1 = 1.0 / h1, ih2 = 1.0 / h2;
  const int slot0 = blockIdx.x * CELL_WG_ROWS + wave * CELL_RPW;
  bool full = false;
  int most = 0;
  for (int g = 0; g < CELL_RPW; g++) {
    const bool live = slot0 + g < n;   // (wave-uniform; a wave without a row still waits at the barriers)
    const int i = live ? clampi(__builtin_amdgcn_readfirstlane(C.clist[slot0 + g]), 0, n - 1) : 0;
    const int ci = clampi(__builtin_amdgcn_readfirstlane(C.cellof[i]), 0, ncells - 1);
    const int cx = ci % nx, cy = (ci / nx) % ny, cz = ci / (nx * ny);
    int beg = 0, len = 0;
    if (live && lane < 27) {
      int sx = cx + lane % 3 - 1, sy = cy + (lane / 3) % 3 - 1, sz = cz + lane / 9 - 1;
      sx += sx < 0 ? nx : (sx >= nx ? -nx : 0);
      sy += sy < 0 ? ny : (sy >= ny ? -ny : 0);
      sz += sz < 0 ? nz : (sz >= nz ? -nz : 0);
      const int cc = clampi(sx + nx * (sy + ny * sz), 0, ncells - 1);
      beg = clampi(C.cstart[cc], 0, n);
      len = clampi(C.cstart[cc + 1] - beg, 0, n - beg);
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const int up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    const int total = __shfl(incl, 31);   // (lanes 27 .. 31 add nothing)
    if (lane < 32) { s_off[wave][lane] = incl - len; s_beg[wave][lane] = beg; }
    __syncthreads();
    const double xi = wave_uniform(S.x[3 * i]), yi = wave_uniform(S.x[3 * i + 1]), zi = wave_uniform(S.x[3 * i + 2]);
    int rowlen = 0;
    for (int t0 = 0; t0 < total; t0 += 64) {
      const int t = t0 + lane;
      const bool jl = t < total;
      int r = 0;   // the last range that starts at or before t: empty ranges share their successor's offset, ranges 27 .. 31 start at `total`
#pragma unroll
      for (int step = 16; step >= 1; step >>= 1) r += s_off[wave][r + step] <= t ? step : 0;
      const int j = jl ? clampi(C.clist[clampi(s_beg[wave][r] + (t - s_off[wave][r]), 0, n - 1)], 0, n - 1) : 0;
      const double xj = S.x[3 * j], yj = S.x[3 * j + 1], zj = S.x[3 * j + 2];
      double dx = xj - xi, dy = yj - yi, dz = zj - zi;
      const double n2 = rint(dz * ih2);
      dz -= n2 * h2; dy -= n2 * h3; dx -= n2 * h4;
      const double n1 = rint(dy * ih1);
      dy -= n1 * h1; dx -= n1 * h5;
      const double n0 = rint(dx * ih0);
      dx -= n0 * h0;
      const double r2 = dx * dx + dy * dy + dz * dz;
      const int c0i = 2 - (int)n0, c1i = 2 - (int)n1, c2i = 2 - (int)n2;
      const bool coded = (unsigned)c0i < 5u && (unsigned)c1i < 5u && (unsigned)c2i < 5u;   // (atoms are wrapped at a build: |n| <= 1)
      const bool ok = jl && coded && j != i && !(r2 > rl2);
      const unsigned long long m = __ballot(ok);
      const int pos = rowlen + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
      if (ok && pos < capst) s_row[wave][pos] = j | ((c0i + 5 * c1i + 25 * c2i) << 24);
      rowlen += __popcll(m);
    }
    __syncthreads();
    const int L = min(rowlen, capst);
    for (int e = lane; e < L; e += 64) {
      const int ent = s_row[wave][e], key = ent & ROW_JMASK;
      int rank = 0;
      for (int k = 0; k < L; k++) rank += (s_row[wave][k] & ROW_JMASK) < key ? 1 : 0;
      V.rows[(size_t)i * cap + rank] = ent;
    }
    if (live) {
      full |= rowlen > cap;
      most = max(most, rowlen);
      if (lane == 0) V.cnt[i] = min(rowlen, cap);
    }
  }
  if (lane == 0 && slot0 < n) {
    if (full) atomicOr(&V.stat[0], 1);
    atomicMax(&V.stat[1], most);
    atomicMax(&S.sc->maxneigh_seen, most);
  }
}

static inline int cdv(int a, int b) { return (a + b - 1) / b; }

void mdk_rowcells_build(hipStream_t st, const SimDev *d, const RowView *v, const RowCells *c, int ns, int maxatoms) {
  if (ns <= 0 || maxatoms <= 0) return;
  hipLaunchKernelGGL(k_cell_bin, dim3(1, (unsigned)ns, 1), dim3(CELL_BIN_TPB), 0, st, d, v, c);
  hipLaunchKernelGGL(k_cell_rows, dim3((unsigned)cdv(maxatoms, CELL_WG_ROWS), (unsigned)ns, 1), dim3(CELL_ROWS_TPB), 0, st, d, v, c);
}
