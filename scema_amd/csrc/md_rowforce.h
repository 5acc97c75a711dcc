// md_rowforce.h -- what the force kernels on the rows of mdk_rows_build share.  Device code.
//   the list kernels (k_sw_force, k_ts_force, k_vs_force, k_edip_force, k_ms_density): the image shifts, the table of the replica's
//     forces in LDS, the filter of one atom's row (rowf_filter) and the end of a workgroup (rowf_finish)
//   the gather kernels, which walk a whole row and take no atomic on a force (k_eam_*, k_adp_*, k_bd_force, k_bl_force, k_ms_force): the
//     image shifts, the copy of a table into LDS (rowf_to_lds), the walk of one atom's row (rowf_walk) and the half-pair virial (rowf_virial)
// md_rows.hip includes it for the launch shape.  No helper holds a barrier: a kernel's barriers stand in its own body.
#pragma once
#include "md_device.h"
#include "md_rows.h"
#include "md_types.h"

#define ROW_FORCE_TPB 256    /* force kernels: 16 groups of 16 lanes, a group per central atom */
#define ROW_NGRP (ROW_FORCE_TPB / 16)
static_assert(ROW_TILE % ROW_NGRP == 0 && ROW_MAXIN <= 32, "tile shapes of the force kernels");

extern __shared__ double s_rowf[];   // LACC: [3][npad]

// shift of every image code: code . h
__device__ __forceinline__ void rowf_shifts(const RowView &V, double *s_sh) {
  for (int code = threadIdx.x; code < ROW_NSHIFT; code += ROW_FORCE_TPB) {
    const int sx = code % 5 - 2, sy = (code / 5) % 5 - 2, sz = code / 25 - 2;
    s_sh[3 * code] = sx * V.h[0] + sy * V.h[5] + sz * V.h[4];
    s_sh[3 * code + 1] = sy * V.h[1] + sz * V.h[3];
    s_sh[3 * code + 2] = sz * V.h[2];
  }
}

// a table (or its first `words` words) from global memory into LDS, by the whole workgroup, in words of the width the table is made of
template <class Word, class T>
__device__ __forceinline__ void rowf_to_lds(T *dst, const void ROW_G *src, int words = (int)(sizeof(T) / sizeof(Word))) {
  static_assert(sizeof(T) % sizeof(Word) == 0, "a table is copied in whole words");
  for (int k = threadIdx.x; k < words; k += ROW_FORCE_TPB) ((Word *)dst)[k] = ((const Word ROW_G *)src)[k];
}

// A group of 16 lanes walks the row of atom i, a lane per entry: every entry goes to term(j, d0, d1, d2, r2), d = x_j - x_i with the
// entry's image shift.  Index and image code are clamped to what the builder can have written.  No cutoff is applied here: the kernel's
// own acceptance test is the first statement of its term, and so is any clamp of an element.  A group past the replica's last atom
// (i >= n) walks nothing; no lane leaves, so the group sums that follow see whole waves.
template <class Term>
__device__ __forceinline__ void rowf_walk(const RowView &V, const double *s_sh, int i, int l16, Term term) {
  const int n = V.n, cap = V.cap;
  const bool valid = i < n;
  const int ic = valid ? i : n - 1;
  const int cnt = valid ? min(V.cnt[ic], cap) : 0;
  const double xi0 = V.x[3 * ic], xi1 = V.x[3 * ic + 1], xi2 = V.x[3 * ic + 2];
  const size_t base = (size_t)ic * cap;
  for (int c = l16; c < cnt; c += 16) {
    const int ent = V.rows[base + c];
    const int j = min(ent & ROW_JMASK, n - 1), code = min((ent >> 24) & 0x7F, ROW_NSHIFT - 1);
    const double *sh = s_sh + 3 * code;
    const double d0 = V.x[3 * j] - xi0 + sh[0], d1 = V.x[3 * j + 1] - xi1 + sh[1], d2 = V.x[3 * j + 2] - xi2 + sh[2];
    term(j, d0, d1, d2, d0 * d0 + d1 * d1 + d2 * d2);
  }
}

// w += h d (x) d (xx, yy, zz, xy, xz, yz): the share of one end of a pair in its virial, h = half the force factor
__device__ __forceinline__ void rowf_virial(double (&w)[6], double h, double d0, double d1, double d2) {
  w[0] += h * d0 * d0; w[1] += h * d1 * d1; w[2] += h * d2 * d2; w[3] += h * d0 * d1; w[4] += h * d0 * d2; w[5] += h * d1 * d2;
}

// LDS FP64 atomic add without return value (ds_add_f64)
__device__ __forceinline__ void rowf_lds_add(double *p, double v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// Forces on partners go into a table of the replica's forces in LDS (LACC; ds_add_f64), flushed with one global FP64 atomic per touched
// atom and component; replicas beyond ROW_LDS_MAXPAD atoms add to global memory directly.
template <bool LACC>
__device__ __forceinline__ void rowf_zero(size_t np) {
  if (LACC)
    for (int k = threadIdx.x; k < 3 * (int)np; k += ROW_FORCE_TPB) s_rowf[k] = 0.0;
}
template <bool LACC>
__device__ __forceinline__ void rowf_add(double ROW_G *f, size_t np, int a, double g0, double g1, double g2) {
  if (LACC) { rowf_lds_add(&s_rowf[a], g0); rowf_lds_add(&s_rowf[np + a], g1); rowf_lds_add(&s_rowf[2 * np + a], g2); }
  else { atomicAdd((double *)&f[3 * a], g0); atomicAdd((double *)&f[3 * a + 1], g1); atomicAdd((double *)&f[3 * a + 2], g2); }
}

// One group of 16 lanes filters the row of atom i (element ti) to the entries INSIDE their cutoff, in the row's order (ballot order): an
// accepted entry goes to keep(pos, ent, tj, d0, d1, d2, r) with pos < ROW_MAXIN, cut(ti, tj) is the cutoff of a pair of elements.  Returns
// the entries kept; more than ROW_MAXIN inside set `crowded`.  A group past the replica's last atom (i >= n) filters nothing.
template <class Cut, class Keep>
__device__ __forceinline__ int rowf_filter(const RowView &V, const double *s_sh, int i, int ti, int l16, int shift16, bool &crowded, Cut cut, Keep keep) {
  const int n = V.n, cap = V.cap;
  const bool valid = i < n;
  const int ic = valid ? i : n - 1;
  const int cnt = valid ? min(V.cnt[ic], cap) : 0;
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
      const int j = min(ent & ROW_JMASK, n - 1), code = min((ent >> 24) & 0x7F, ROW_NSHIFT - 1);
      ent = j | (code << 24);   // (what the builder wrote; nothing else is ever used as an index)
      const double *sh = s_sh + 3 * code;
      d0 = V.x[3 * j] - xi0 + sh[0]; d1 = V.x[3 * j + 1] - xi1 + sh[1]; d2 = V.x[3 * j + 2] - xi2 + sh[2];
      tj = V.stype[j];
      const double r2 = d0 * d0 + d1 * d1 + d2 * d2, rc = cut(ti, tj);
      in = r2 < rc * rc && r2 > 0.0;
      r = sqrt(r2);
      in = in && r < rc;   // (the test the physics relies on: a pair at or beyond its cutoff never reaches an exponential)
    }
    const unsigned m16 = (unsigned)(__ballot(in) >> shift16) & 0xFFFFu;
    const int pos = nn + __popc(m16 & ((1u << l16) - 1u));
    if (in && pos < ROW_MAXIN) keep(pos, ent, tj, d0, d1, d2, r);
    nn += __popc(m16);
  }
  if (nn > ROW_MAXIN) { crowded = true; nn = ROW_MAXIN; }
  return nn;
}

// the central atom's own force: the sum over its group (a row of 16 lanes), added by the group's first lane
template <bool LACC>
__device__ __forceinline__ void rowf_add_own(const RowView &V, size_t np, int i, int l16, double fi0, double fi1, double fi2) {
  fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
  if (i < V.n && l16 == 0 && (fi0 != 0.0 || fi1 != 0.0 || fi2 != 0.0)) rowf_add<LACC>(V.f, np, i, fi0, fi1, fi2);
}

// end of a workgroup, after the last round's closing barrier: the LDS table to global memory (zeros skipped), the crowded bit, and the
// step's sums (esum -> eacc, wa -> virial part P_LJ, wb -> P_ANGLE), one atomic per value and workgroup
template <bool LACC>
__device__ __forceinline__ void rowf_finish(const RowView &V, SimScalars &sc, size_t np, bool crowded, double (&esum)[4], double (&wa)[6], double (&wb)[6], double *s_red) {
  if (LACC) {
    for (int k = threadIdx.x; k < 3 * V.n; k += ROW_FORCE_TPB) {
      const int a = k / 3, c = k - 3 * a;
      const double v = s_rowf[(size_t)c * np + a];
      if (v != 0.0) atomicAdd((double *)&V.f[k], v);
    }
  }
  if (crowded) atomicOr(&V.stat[0], 2);
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wa, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_ANGLE * 6], s_red);
}
