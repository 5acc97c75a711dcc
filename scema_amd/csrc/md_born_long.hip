// md_born_long.hip -- gfx950 kernels of the Ewald ionic force stage (`pair_style born/coul/long`, `buck/coul/long` with `kspace_style
// ewald <accuracy>`; `pppm` is honoured as the Ewald sum it approximates).  Row replicas are small (8 to a few thousand ions), where a
// plain Ewald sum is the right solver; the neighbour rows, the integrator, fix deform and the batch machinery are those of the other row
// stages.  One launch covers every replica of the batch (blockIdx.y), padded to the largest atom count and the largest k list.
//   k_bl_force ..... real space: the Born term and K q_i q_j erfc(g r)/r over every entry of an atom's row inside cutmax, in the shape of
//                    k_bd_force (md_born_dsf.hip): the body both share (ionic_force, md_ionic_force.h); stores f
//   k_bl_sfac ...... S(k) = sum_i q_i exp(i k.r_i): a workgroup owns BL_SF_TPB k-vectors of one replica, a thread one of them, and walks
//                    every atom of the replica in atom order, BL_SF_ATOMS at a time staged in LDS as phase tables exp(2 pi i m u_d),
//                    m = 0 .. kmax_d.  One writer and a fixed order per S(k), no atomic.  The same thread turns S(k) into c_k S(k) for the
//                    box of the step and adds the reciprocal energy and virial; the first workgroup adds the self and background terms
//   k_bl_recip ..... adds -2 q_i sum_k c_k k Im(S(k) exp(-i k.r_i)) to f: 16 lanes per atom, a lane every 16th k-vector in ascending
//                    order, row_sum, one writer per atom
// between the row part and k_row_finish.  No atomic touches a force or S(k), and every sum has a fixed order: two evaluations of one state
// give the same forces bit for bit.  (The energies and the virial are summed with one atomic per workgroup, as in every row stage.)
// The integer triples are those of the run's start box and stay; the Cartesian k of a step comes from them and the box of the step
// (RowView::h, set by k_row_prepare from SimScalars::box), so fix deform moves the k-vectors with the lattice.  A box flip changes the
// basis and not the lattice: with a2 = a2(start) + A a1 and a3 = a3(start) + C a1 (BlView::shift) the triple of a vector in the basis of
// the step is (n1, n2 + A n1, n3 + C n1), and k.r = 2 pi (n1 u1 + n2 u2 + n3 u3) with u = (s1 + A s2 + C s3, s2, s3) of the step's
// fractional coordinates s, so the phase tables keep the index range of the set-up.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "md_born_long.h"
#include "md_ionic_force.h"

#define BL_SF_TPB 128        /* k-vectors of one workgroup of k_bl_sfac */
#define BL_SF_ATOMS 32       /* atoms staged per pass */
#define BL_PHD (BL_MAXKD + 1)
#define BL_PHROW (3 * BL_PHD) /* phase-table entries of one atom */
static_assert(3 * BL_SF_ATOMS <= BL_SF_TPB, "a thread per atom and dimension fills the phase tables");

// what the kernels take from a BlView, clamped to what the buffers and the LDS tables hold
struct BlShape { int nk, km0, km1, km2, a, c; };
__device__ __forceinline__ BlShape bl_shape(const BlView &B) {
  BlShape s;
  s.nk = min(max(B.nk, 0), min(B.nkcap, BL_MAXK));
  s.km0 = min(max(B.kmax[0], 0), BL_MAXKD); s.km1 = min(max(B.kmax[1], 0), BL_MAXKD); s.km2 = min(max(B.kmax[2], 0), BL_MAXKD);
  s.a = B.shift[0]; s.c = B.shift[1];
  return s;
}

// u of an atom: its fractional coordinates in the basis the triples were set up in (above)
__device__ __forceinline__ void bl_ucoord(const RowView &V, const BlShape &s, int i, double *u) {
  const double x[3] = {V.x[3 * i], V.x[3 * i + 1], V.x[3 * i + 2]};
  double f[3];
  bl_frac(V.h, x, f);
  u[0] = f[0] + s.a * f[1] + s.c * f[2]; u[1] = f[1]; u[2] = f[2];
}

// exp(2 pi i m u), m = 0 .. mmax
__device__ __forceinline__ void bl_phase_row(double u, int mmax, double2 *p) {
  double sn, cs;
  sincospi(2.0 * u, &sn, &cs);
  double re = 1.0, im = 0.0;
  p[0] = make_double2(1.0, 0.0);
  for (int m = 1; m <= mmax; m++) {
    const double t = re * cs - im * sn;
    im = re * sn + im * cs;
    re = t;
    p[m] = make_double2(re, im);
  }
}

// exp(i k.r) of a triple from one atom's tables
__device__ __forceinline__ double2 bl_phase(const double2 *p, int n1, int n2, int n3) {
  const double2 a = p[abs(n1)], b = p[BL_PHD + abs(n2)], c = p[2 * BL_PHD + abs(n3)];
  const double ai = n1 < 0 ? -a.y : a.y, bi = n2 < 0 ? -b.y : b.y, ci = n3 < 0 ? -c.y : c.y;
  const double re = a.x * b.x - ai * bi, im = a.x * bi + ai * b.x;
  return make_double2(re * c.x - im * ci, re * ci + im * c.x);
}

// Real space: the ionic body (md_ionic_force.h) with bl_pair at the replica's g; the self and background terms are k_bl_sfac's.
struct BlTerms {
  double g;
  __device__ __forceinline__ const BdTable &bd(const BlTable &T) const { return T.bd; }
  __device__ __forceinline__ void pair(const BlTable &T, const BdPairP &P, double qi, double qj, double r2, double *eb, double *ec, double *fb, double *fc) const {
    bl_pair(T, P, g, qi, qj, r2, eb, ec, fb, fc);
  }
  __device__ __forceinline__ void self(const BlTable &, double, double &) const {}
};
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_bl_force(const SimDev *sims, const RowView *views, const BlView *bls) {
  ionic_force<BlTable>(sims, views, BlTerms{bls[blockIdx.y].g});
}

// Structure factors.  No thread leaves before the last barrier: a thread past the replica's last k-vector sums a zero triple and stores
// nothing.  A workgroup whose whole chunk lies past the list leaves at the top, the first one excepted (the self and background terms).
__global__ __launch_bounds__(BL_SF_TPB) void k_bl_sfac(const SimDev *sims, const RowView *views, const BlView *bls) {
  const RowView V = views[blockIdx.y];
  const BlView B = bls[blockIdx.y];
  if (B.mesh) return;   // (the whole workgroup: a mesh replica's reciprocal part, self and background terms are k_blm_poisson's)
  const BlShape sh = bl_shape(B);
  if (blockIdx.x > 0 && (int)(blockIdx.x * BL_SF_TPB) >= sh.nk) return;   // (the whole workgroup)
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  const double MD_G *q = S.q;
  const int n = V.n;
  __shared__ double2 s_ph[BL_SF_ATOMS][BL_PHROW];
  __shared__ double s_q[BL_SF_ATOMS];
  __shared__ double s_red[8 * (BL_SF_TPB / 64)];
  const int k = blockIdx.x * BL_SF_TPB + threadIdx.x;
  const bool valid = k < sh.nk;
  const int n1 = valid ? min(max(B.kn[3 * k], -sh.km0), sh.km0) : 0, n2 = valid ? min(max(B.kn[3 * k + 1], -sh.km1), sh.km1) : 0,
            n3 = valid ? min(max(B.kn[3 * k + 2], -sh.km2), sh.km2) : 0;
  double sre = 0.0, sim = 0.0;
  for (int a0 = 0; a0 < n; a0 += BL_SF_ATOMS) {   // (uniform over the workgroup)
    __syncthreads();
    const int na = min(BL_SF_ATOMS, n - a0);
    if ((int)threadIdx.x < 3 * na) {
      const int a = threadIdx.x / 3, d = threadIdx.x - 3 * a;
      double u[3];
      bl_ucoord(V, sh, a0 + a, u);
      bl_phase_row(u[d], d == 0 ? sh.km0 : (d == 1 ? sh.km1 : sh.km2), &s_ph[a][d * BL_PHD]);
      if (d == 0) s_q[a] = q[a0 + a];
    }
    __syncthreads();
    for (int a = 0; a < na; a++) {
      const double2 p = bl_phase(s_ph[a], n1, n2, n3);
      const double qa = s_q[a];
      sre += qa * p.x; sim += qa * p.y;
    }
  }
  const double kc = ((const BlTable ROW_G *)V.tab)->bd.k, g = B.g, vol = V.h[0] * V.h[1] * V.h[2];
  double esum[1] = {0.0}, w[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (valid && g > 0.0) {
    double kv[3];
    const double h[6] = {V.h[0], V.h[1], V.h[2], V.h[3], V.h[4], V.h[5]};
    bl_kvec(h, n1, n2 + sh.a * n1, n3 + sh.c * n1, kv);
    const double k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    const double ck = bl_coef(kc, g, vol, k2);
    const double ek = ck * (sre * sre + sim * sim);
    const double vf = -2.0 * (1.0 / k2 + 0.25 / (g * g)) * ek;
    esum[0] = ek;
    w[0] = ek + vf * kv[0] * kv[0]; w[1] = ek + vf * kv[1] * kv[1]; w[2] = ek + vf * kv[2] * kv[2];
    w[3] = vf * kv[0] * kv[1]; w[4] = vf * kv[0] * kv[2]; w[5] = vf * kv[1] * kv[2];
    double ROW_G *sk = B.sk;
    const size_t st = (size_t)B.nkcap;
    sk[k] = ck * sre; sk[st + k] = ck * sim; sk[2 * st + k] = kv[0]; sk[3 * st + k] = kv[1]; sk[4 * st + k] = kv[2];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && g > 0.0) {
    double ebg;
    esum[0] += bl_self(kc, g, vol, B.qsqsum, B.qsum, &ebg);
    w[0] += ebg; w[1] += ebg; w[2] += ebg;
  }
  block_atomic_add_n<1, BL_SF_TPB / 64>(esum, (double *)V.eacc + 1, s_red);
  block_atomic_add_n<6, BL_SF_TPB / 64>(w, &sc.vir[P_COUL * 6], s_red);
}

// Reciprocal forces.  The launch shape of k_bl_force: a group of 16 lanes per atom; lanes 0..2 fill the atom's phase tables (a row of the
// workgroup's LDS block per group), then lane l sums the k-vectors l, l + 16, ... in ascending order.  The round is uniform over the
// workgroup, so its two barriers stand in the loop body.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_bl_recip(const SimDev *sims, const RowView *views, const BlView *bls) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const BlView B = bls[blockIdx.y];
  const BlShape sh = bl_shape(B);
  if (sh.nk == 0 || !(B.g > 0.0)) return;
  const double MD_G *q = sims[blockIdx.y].q;
  __shared__ double2 s_pt[ROW_NGRP][BL_PHROW];
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const double ROW_G *sk = B.sk;
  const size_t st = (size_t)B.nkcap;
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const bool valid = i < n;
    const int ic = valid ? i : n - 1;
    __syncthreads();
    if (l16 < 3) {
      double u[3];
      bl_ucoord(V, sh, ic, u);
      bl_phase_row(u[l16], l16 == 0 ? sh.km0 : (l16 == 1 ? sh.km1 : sh.km2), &s_pt[grp][l16 * BL_PHD]);
    }
    __syncthreads();
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    for (int k = l16; k < (valid ? sh.nk : 0); k += 16) {
      const int n1 = min(max(B.kn[3 * k], -sh.km0), sh.km0), n2 = min(max(B.kn[3 * k + 1], -sh.km1), sh.km1), n3 = min(max(B.kn[3 * k + 2], -sh.km2), sh.km2);
      const double2 p = bl_phase(s_pt[grp], n1, n2, n3);
      const double t = sk[st + k] * p.x - sk[k] * p.y;   // c_k Im(S exp(-i k.r_i))
      f0 += t * sk[2 * st + k]; f1 += t * sk[3 * st + k]; f2 += t * sk[4 * st + k];
    }
    f0 = row_sum(f0); f1 = row_sum(f1); f2 = row_sum(f2);
    if (valid && l16 == 0) {
      const double m2q = -2.0 * q[i];
      V.f[3 * i] += m2q * f0; V.f[3 * i + 1] += m2q * f1; V.f[3 * i + 2] += m2q * f2;
    }
  }
}

__global__ void k_bl_flip(const BlView *b, int fxy, int fxz) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { b->shift[0] += fxy; b->shift[1] += fxz; }
}

void mdk_bl_forces(hipStream_t st, const SimDev *d, RowView *v, const BlView *b, int ns, int maxatoms, int maxnk, bool ewald,
                   const std::function<void(dim3)> *mesh, const std::function<void(dim3)> *real) {
  mdk_row_stage(st, d, v, ns, maxatoms, [&](dim3 gt) {
    const dim3 gk((unsigned)std::max(1, (maxnk + BL_SF_TPB - 1) / BL_SF_TPB), (unsigned)ns, 1);
    if (real) (*real)(gt);
    else hipLaunchKernelGGL(k_bl_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, b);
    if (ewald) {
      hipLaunchKernelGGL(k_bl_sfac, gk, dim3(BL_SF_TPB), 0, st, d, v, b);
      hipLaunchKernelGGL(k_bl_recip, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, b);
    }
    if (mesh) (*mesh)(gt);
  });
}

void mdk_bl_flip(hipStream_t st, const BlView *b, int fxy, int fxz) { hipLaunchKernelGGL(k_bl_flip, dim3(1), dim3(64), 0, st, b, fxy, fxz); }
