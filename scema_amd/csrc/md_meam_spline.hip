// md_meam_spline.hip -- gfx950 kernels of the spline-MEAM force stage (`pair_style meam/spline`: Ti, Zr, Nb, Mo, Si, Ti-O).  The neighbour
// rows, k_row_finish (energies and fault bits into the engine's scalars) and the launch shape are those of the row part (md_rows.hip).
// One launch per pass covers every replica of the batch (blockIdx.y).
//   k_ms_density ... rho_i = sum_j rho(r_ij) over every entry inside rho's range + the triplets f f g(cos) over the few inside f's range
//                    (meam_spline/ms_core.h); U(rho_i) - U(0) into the step's energy, U'(rho_i) into fp[i]; the three-body forces, which
//                    need U' of the central atom alone, in the same launch (skeleton: md_rowforce.h)
//   k_ms_force ..... the pair gather of k_eam_force, on the gather skeleton of md_rowforce.h: with every U' written, each end of a pair
//                    sums its own phi' + U'_i rho'_tj + U'_j rho'_ti; no atomic
// The potential has two ranges, as Vashishta has: phi and rho reach their last knots (cutmax, the rows' range), f a clearly shorter one.
// The list of ROW_MAXIN entries in LDS holds the entries inside f's range alone; the pair terms are taken in place, at any count.
// Engine parts: phi and the virial of phi' go to P_LJ, the embedding energy, the virial of the U' rho' terms and of the triplets to
// P_ANGLE; scema_md_meam_spline_debug_compute reports the two energies as e_pair and e_embed.
#include <hip/hip_runtime.h>

#include "md_kernels.h"
#include "md_meam_spline.h"
#include "md_rowforce.h"

static_assert(ROW_TILE == 64, "tile shape of md_meam_spline.hip");

// the lane's entry c of atom ic's row: partner, its element, d = x_j - x_i with the entry's image shift, r^2.  Index and image code are
// clamped to what the builder can have written, the element to the ne elements of the table.
struct MsEntry { int j, tj; double d0, d1, d2, r2; };
__device__ __forceinline__ MsEntry ms_entry(const RowView &V, const double *s_sh, int ne, size_t base, int c, double xi0, double xi1, double xi2) {
  const int ent = V.rows[base + c];
  MsEntry E;
  E.j = min(ent & ROW_JMASK, V.n - 1);
  const int code = min((ent >> 24) & 0x7F, ROW_NSHIFT - 1);
  const double *sh = s_sh + 3 * code;
  E.d0 = V.x[3 * E.j] - xi0 + sh[0]; E.d1 = V.x[3 * E.j + 1] - xi1 + sh[1]; E.d2 = V.x[3 * E.j + 2] - xi2 + sh[2];
  E.tj = min(V.stype[E.j], ne - 1);
  E.r2 = E.d0 * E.d0 + E.d1 * E.d1 + E.d2 * E.d2;
  return E;
}

// t -> (a, b), a < b: t = b (b - 1) / 2 + a
__device__ __forceinline__ void ms_pair_of(int t, int &a, int &b) {
  b = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)t)) * 0.5f);
  while (b * (b - 1) / 2 > t) b--;
  while ((b + 1) * b / 2 <= t) b++;
  a = t - b * (b - 1) / 2;
}

// Densities and three-body forces.  A workgroup owns ROW_TILE consecutive central atoms of one replica, a group of 16 lanes one of them
// at a time.
//   1. The group walks the atom's row once, a lane per entry.  An entry inside rho's last knot adds to the lane's density where it
//      stands, at any count (rho from the table in memory).  An entry inside f's last knot goes to the group's list in LDS in the row's
//      order (ballot order) with vector, distance, f and f'; more than ROW_MAXIN set the crowded bit.
//   2. The lanes take the triplets (a < b) of the list: f_a f_b g(cos) joins the density.  After the group's sum U and U' are taken:
//      U - U(0) into the embedding energy, U' into fp[i] for k_ms_force.
//   3. The lanes take the triplets again for the forces -U'_i grad(f f g): partners through the LDS table or global memory (LACC,
//      md_rowforce.h), the central atom's share through the group's sum, the virial into P_ANGLE.  g is evaluated a second time: the
//      values of up to 31 triplets a lane would need a runtime-indexed register array (scratch) or 127 KB of LDS.
// Only f and g, which the triplet loops read, are staged in LDS; rho and U are read where they stand.
template <bool LACC>
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_ms_density(const SimDev *sims, const RowView *views, const EamView *aux) {
  const RowView V = views[blockIdx.y];
  const int n = V.n, cap = V.cap;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const MsTable ROW_G *tab = (const MsTable ROW_G *)V.tab;
  double ROW_G *fp = aux[blockIdx.y].fp;
  SimScalars &sc = *sims[blockIdx.y].sc;
  const size_t np = (size_t)V.npad;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ MsFn s_f[MS_MAXEL], s_g[MS_NPAIR];
  __shared__ double s_nb[6][ROW_NGRP][ROW_MAXIN];   // d (3), r, f, f'
  __shared__ int s_jt[ROW_NGRP][ROW_MAXIN];         // partner (ROW_JMASK) and its element (from bit 24)
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  static_assert(sizeof(s_sh) + sizeof(s_f) + sizeof(s_g) + sizeof(s_nb) + sizeof(s_jt) + sizeof(s_red) + 3 * ROW_LDS_MAXPAD * 8 < 65536,
                "LDS of k_ms_density with the force table of ROW_LDS_MAXPAD atoms");
  static_assert(sizeof(MsFn) % 8 == 0, "MsFn is copied as doubles");
  const int ne = min(max(tab->nelem, 1), MS_MAXEL);
  const int off_rho = ne * (ne + 1) / 2, off_u = off_rho + ne, off_f = off_u + ne, off_g = off_f + ne;
  rowf_shifts(V, s_sh);
  for (int k = threadIdx.x; k < ne * (int)(sizeof(MsFn) / 8); k += ROW_FORCE_TPB) ((double *)s_f)[k] = ((const double ROW_G *)&tab->fn[off_f])[k];
  for (int k = threadIdx.x; k < off_rho * (int)(sizeof(MsFn) / 8); k += ROW_FORCE_TPB) ((double *)s_g)[k] = ((const double ROW_G *)&tab->fn[off_g])[k];
  rowf_zero<LACC>(np);
  __syncthreads();
  const MsFn *fn = (const MsFn *)&tab->fn[0];   // rho and U, from memory
  const double cutmax = tab->cutmax;
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int shift16 = 16 * (grp & 3);
  double esum[4] = {0.0, 0.0, 0.0, 0.0};   // pair energy (k_ms_force), embedding energy, ordered pairs inside cutmax, triplets
  double w0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w3[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool crowded = false;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup: the barriers and the group sums below are reached by every lane)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    const int ti = min(V.stype[ic], ne - 1);
    const int cnt = valid ? min(V.cnt[ic], cap) : 0;   // (a group past the replica's last atom walks nothing)
    const double xi0 = V.x[3 * ic], xi1 = V.x[3 * ic + 1], xi2 = V.x[3 * ic + 2];
    const size_t base = (size_t)ic * cap;
    double rho = 0.0;
    int nn = 0;
    for (int c0 = 0; c0 < cnt; c0 += 16) {
      const int c = c0 + l16;
      bool arm = false;
      MsEntry E = {0, 0, 0.0, 0.0, 0.0, 0.0};
      double r = 1.0;
      if (c < cnt) {
        E = ms_entry(V, s_sh, ne, base, c, xi0, xi1, xi2);
        r = sqrt(E.r2);
        if (E.r2 > 0.0 && r < cutmax) {
          esum[2] += 1.0;
          const MsFn &R = fn[off_rho + E.tj];
          double dr;
          if (r < R.x[R.n - 1]) rho += ms_eval(R, r, &dr);
          arm = r < s_f[E.tj].x[s_f[E.tj].n - 1];   // (the strict test: an arm at or beyond f's last knot is no arm)
        }
      }
      const unsigned m16 = (unsigned)(__ballot(arm) >> shift16) & 0xFFFFu;
      const int pos = nn + __popc(m16 & ((1u << l16) - 1u));
      if (arm && pos < ROW_MAXIN) {
        double fv, df;
        ms_arm(s_f[E.tj], r, &fv, &df);
        s_nb[0][grp][pos] = E.d0; s_nb[1][grp][pos] = E.d1; s_nb[2][grp][pos] = E.d2; s_nb[3][grp][pos] = r; s_nb[4][grp][pos] = fv; s_nb[5][grp][pos] = df;
        s_jt[grp][pos] = E.j | (E.tj << 24);
      }
      nn += __popc(m16);
    }
    if (nn > ROW_MAXIN) { crowded = true; nn = ROW_MAXIN; }
    __syncthreads();   // the groups' lists are complete
    const int ntrip = nn * (nn - 1) / 2;
    for (int t = l16; t < ntrip; t += 16) {
      int a, b;
      ms_pair_of(t, a, b);
      const double da_[3] = {s_nb[0][grp][a], s_nb[1][grp][a], s_nb[2][grp][a]}, db_[3] = {s_nb[0][grp][b], s_nb[1][grp][b], s_nb[2][grp][b]};
      double dg;
      const MsFn &G = s_g[ms_pair_index(ne, s_jt[grp][a] >> 24, s_jt[grp][b] >> 24)];
      rho += s_nb[4][grp][a] * s_nb[4][grp][b] * ms_eval(G, ms_cos(da_, s_nb[3][grp][a], db_, s_nb[3][grp][b]), &dg);
      esum[3] += 1.0;
    }
    rho = row_sum(rho);   // rho_i, in every lane of the group
    double up;
    const double u = ms_eval(fn[off_u + ti], rho, &up);
    if (valid && l16 == 0) {
      fp[i] = up;
      esum[1] += u - tab->u0[ti];
    }
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    for (int t = l16; t < ntrip; t += 16) {
      int a, b;
      ms_pair_of(t, a, b);
      const int ja = s_jt[grp][a], jb = s_jt[grp][b];
      const double da_[3] = {s_nb[0][grp][a], s_nb[1][grp][a], s_nb[2][grp][a]}, db_[3] = {s_nb[0][grp][b], s_nb[1][grp][b], s_nb[2][grp][b]};
      double gj[3], gk[3];
      (void)ms_three(s_g[ms_pair_index(ne, ja >> 24, jb >> 24)], da_, s_nb[3][grp][a], s_nb[4][grp][a], s_nb[5][grp][a], db_, s_nb[3][grp][b], s_nb[4][grp][b],
                     s_nb[5][grp][b], gj, gk);
      const double fj[3] = {-up * gj[0], -up * gj[1], -up * gj[2]}, fk[3] = {-up * gk[0], -up * gk[1], -up * gk[2]};
      rowf_add<LACC>(V.f, np, ja & ROW_JMASK, fj[0], fj[1], fj[2]);
      rowf_add<LACC>(V.f, np, jb & ROW_JMASK, fk[0], fk[1], fk[2]);
      fi0 -= fj[0] + fk[0]; fi1 -= fj[1] + fk[1]; fi2 -= fj[2] + fk[2];
      w3[0] += da_[0] * fj[0] + db_[0] * fk[0]; w3[1] += da_[1] * fj[1] + db_[1] * fk[1]; w3[2] += da_[2] * fj[2] + db_[2] * fk[2];
      w3[3] += da_[0] * fj[1] + db_[0] * fk[1]; w3[4] += da_[0] * fj[2] + db_[0] * fk[2]; w3[5] += da_[1] * fj[2] + db_[1] * fk[2];
    }
    rowf_add_own<LACC>(V, np, i, l16, fi0, fi1, fi2);
    __syncthreads();   // the lists have been read: the next atoms may overwrite them
  }
  rowf_finish<LACC>(V, sc, np, crowded, esum, w0, w3, s_red);
}

// Pair forces: the walk of k_eam_force (rowf_walk, md_rowforce.h).  A lane's entry inside cutmax takes phi' and the two density slopes
// (each inside its own last knot; phi and rho staged in LDS: three evaluations an entry, a bisection of dependent loads each where the knots are not equidistant)
// with U' of both ends; the group's sum joins what k_ms_density left in the atom's force -- this launch follows it on the stream
// and one lane alone touches f[i], so the addition needs no atomic.  Half of a pair's phi and half of its virial go to each end.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_ms_force(const SimDev *sims, const RowView *views, const EamView *aux) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const MsTable ROW_G *tab = (const MsTable ROW_G *)V.tab;
  const double ROW_G *fp = aux[blockIdx.y].fp;
  SimScalars &sc = *sims[blockIdx.y].sc;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ MsFn fn[MS_NPAIR + MS_MAXEL];   // phi and rho, the first two families of the table: this kernel has no force table, so they fit
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  const int ne = min(max(tab->nelem, 1), MS_MAXEL);
  const int off_rho = ne * (ne + 1) / 2;
  rowf_shifts(V, s_sh);
  rowf_to_lds<double>(fn, &tab->fn[0], (off_rho + ne) * (int)(sizeof(MsFn) / 8));
  __syncthreads();
  const double cutmax = tab->cutmax;
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};
  double wa[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ic = min(i, n - 1);
    const int ti = min(V.stype[ic], ne - 1);
    const double upi = fp[ic];
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      const double r = sqrt(r2);
      if (!(r2 > 0.0 && r < cutmax)) return;   // (r against cutmax, as k_ms_density decides it: not the squares)
      const int tj = min(V.stype[j], ne - 1);
      double phi, fa, fb;
      ms_pair(fn[ms_pair_index(ne, ti, tj)], fn[off_rho + tj], fn[off_rho + ti], r, upi, fp[j], &phi, &fa, &fb);
      const double fpair = fa + fb;
      fi0 += d0 * fpair; fi1 += d1 * fpair; fi2 += d2 * fpair;   // (the force on i points along d where the slope is positive)
      esum[0] += 0.5 * phi;
      rowf_virial(wa, -0.5 * fa, d0, d1, d2);   // d (x) (force on j), half at each end
      rowf_virial(wb, -0.5 * fb, d0, d1, d2);
    });
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (i < n && l16 == 0) { V.f[3 * i] += fi0; V.f[3 * i + 1] += fi1; V.f[3 * i + 2] += fi2; }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wa, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_ANGLE * 6], s_red);
}

void mdk_ms_forces(hipStream_t st, const SimDev *d, RowView *v, const EamView *a, int ns, int maxatoms) {
  mdk_row_stage(st, d, v, ns, maxatoms, [&](dim3 gt) {
    const int maxpad = (maxatoms + 63) / 64 * 64;
    if (maxpad <= ROW_LDS_MAXPAD) hipLaunchKernelGGL(k_ms_density<true>, gt, dim3(ROW_FORCE_TPB), 3 * (size_t)maxpad * sizeof(double), st, d, v, a);
    else hipLaunchKernelGGL(k_ms_density<false>, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
    hipLaunchKernelGGL(k_ms_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
  });
}
