// md_kernels.hip -- hand-written gfx950 kernels of the batched MD micro-solver.
//
// Every kernel runs on a 2-D grid: blockIdx.y = simulation (quadrature-point replica),
// blockIdx.x = tile of that simulation, so one launch advances the whole batch one stage.
// Nothing here synchronises with the host: neighbour rebuilds are decided on the device
// (sc->rebuild) and the rebuild kernels return immediately when the flag is clear.
//
// What each kernel implements (reference: the LAMMPS styles chosen by
// lammps_scripts_opls/in.set.lammps:27-57, in.strain.lammps:71-100,
// ELASTIC/in.homogenization.lammps:57-64):
//   k_pre / k_initial_integrate / k_final_integrate / k_post ... fix nvt (NH chain) + Verlet (K9)
//   k_bin / k_cell_scan / k_cell_fill / k_cell_sort / k_pack / k_neigh_build ... K1
//   (md_pair.hip)   k_neigh_build, k_pair ... K1, K2 (the roofline kernel)
//   (md_bonded.hip) k_bonded ................ K4-K7, S4
//   k_ewald_* ............ reciprocal Ewald sum (K3)
//   k_shake .............. fix shake (K8)
//   k_remap .............. fix deform ... remap x (K10)
//   pressure sample in k_post ... compute pressure + fix ave/time (K11)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "md_device.h"
#include "md_env.h"
#include "md_kernels.h"
#include "md_types.h"


// ------------------------------------------------------------------------------------------
// k_phase_init : start of a "run": thermostat reset, accumulators, forced rebuild
// ------------------------------------------------------------------------------------------
__global__ void k_phase_init(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  if (threadIdx.x == 0) {
    if (!sc.keep_nh)   // a fresh fix starts from zero; a run issued in segments (md_equil.hip) keeps its thermostat
      for (int k = 0; k <= MD_MAXCHAIN; k++) sc.eta[k] = sc.eta_dot[k] = sc.eta_dotdot[k] = sc.eta_mass[k] = 0.0;
    for (int k = 0; k < 9; k++) { sc.box0[k] = sc.box[k]; sc.box_prev[k] = sc.box[k]; }
    for (int k = 0; k < 6; k++) { sc.psum[k] = 0.0; sc.ke[k] = 0.0; }
    for (int k = 0; k < MD_NPART * 6; k++) sc.vir[k] = 0.0;
    for (int k = 0; k < MD_NPART; k++) sc.eng[k] = 0.0;
    sc.vscale = 1.0;
    sc.nsamples = 0;
    sc.step = 0;
    // A LAMMPS run begins with a list build (Verlet::setup), and so does a run here -- unless it continues one that has just ended on
    // this slot with the same cell grid (the sampling run behind the straining run of an evaluation): positions and box are those of
    // the last force evaluation but for the last remap of fix deform (k_post moves the box once more, k_remap carries the atoms along: 3e-3 A
    // per step at the reference's strain rate, 0.3 A at a rate of 1e-2 per fs), so they stand where the list's own test says so for the
    // positions and the box the run starts from -- the same test as for rows kept from the update before (below), with the rows' age and
    // reference positions.  (Until round 6 they stood unchecked: a sheared replica at a rate of 1e-2 lost pairs in the set-up evaluation
    // of its sampling run, 1e-7 of the stress.)  The set-up evaluation walks whole rows (walk_all: the displacement bounds of the skin bands are only taken from step 1 on).  A box flip that
    // is still pending forces the build as it would between two steps.  Results do not depend on when a list is built.
    int keep = S.keep_list && !sc.force_rebuild;
    sc.deltasq = 0.0;
    if (keep) {
      // rows from the run or the update before: they stand only if the list's own test says so -- every atom within half the skin (less the motion of
      // the box corners) of the position the rows were built for.  The box part here, the atoms in k_keep_validate.  A slot that last
      // served another state arrives with zeroed reference corners: the corner motion then exceeds any skin and the build is made.
      double c[24];
      box_corners(sc.box, c);
      double d1 = 0.0, d2 = 0.0;
      for (int k = 0; k < 8; k++) {
        const double dx = c[3 * k] - sc.corners_hold[3 * k], dy = c[3 * k + 1] - sc.corners_hold[3 * k + 1], dz = c[3 * k + 2] - sc.corners_hold[3 * k + 2];
        const double d = sqrt(dx * dx + dy * dy + dz * dz);
        if (d > d1) { d2 = d1; d1 = d; }
        else if (d > d2) d2 = d;
      }
      const double delta = 0.5 * (S.skin - (d1 + d2));
      if (delta > 0.0) sc.deltasq = delta * delta;
      else keep = 0;
    }
    if (!keep) sc.ago = 0;
    sc.check = 1;
    sc.rebuild = keep ? 0 : 1;
    sc.force_rebuild = 0;
    sc.corner = 0.0;
    sc.walk_all = keep ? 1 : 0;   // (a build clears it again: a fresh row is walked as far as segment B)
#if defined(PAIR_TIMING) || defined(PAIR_COUNT)
    for (int k = 0; k < 20; k++) sc.dbg[k] = 0;
    for (int k = 0; k < 8; k++) sc.dbg2[k] = 0;
#endif
  }
  for (int k = threadIdx.x; k < 2 * S.nk; k += blockDim.x) S.sfac[k] = 0.0;
  for (int k = threadIdx.x; k < S.ncells; k += blockDim.x) S.cell_count[k] = 0;
}

// k_keep_validate : rows kept from the run or the update before (SimDev::keep_list != 0) stand only while every atom is within the list's displacement
// bound of its reference position -- the test k_initial_integrate makes every step, here for the positions the run starts from
__global__ __launch_bounds__(TPB) void k_keep_validate(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.keep_list) return;
  SimScalars &sc = *S.sc;
  if (sc.rebuild) return;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  const double dx = S.x[3 * i] - S.xhold[3 * i], dy = S.x[3 * i + 1] - S.xhold[3 * i + 1], dz = S.x[3 * i + 2] - S.xhold[3 * i + 2];
  if (!(dx * dx + dy * dy + dz * dz <= sc.deltasq)) sc.rebuild = 1;   // (NaN-safe)
}

// k_setup_post : after the step-0 force evaluation: fix nvt setup (t_current, chain masses)
__global__ void k_setup_post(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  if (threadIdx.x == 0) {
    sc.t_current = (sc.ke[0] + sc.ke[1] + sc.ke[2]) / (S.tdof * MD_BOLTZ);
    if (S.nvt) {
      const double tf2 = S.t_freq * S.t_freq;
      sc.eta_mass[0] = S.tdof * MD_BOLTZ * S.t_target / tf2;
      for (int k = 1; k < S.t_chain; k++) sc.eta_mass[k] = MD_BOLTZ * S.t_target / tf2;
      for (int k = 1; k < S.t_chain; k++)
        sc.eta_dotdot[k] = (sc.eta_mass[k - 1] * sc.eta_dot[k - 1] * sc.eta_dot[k - 1] - MD_BOLTZ * S.t_target) / sc.eta_mass[k];
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_pre : beginning of a step (tiny, one block per simulation)
// ------------------------------------------------------------------------------------------
// the scalar part (one thread per simulation)
// displacement of box corner k (ix = k & 1, iy = k >> 1 & 1, iz = k >> 2: the order of box_corners) since the rows were built
__device__ __forceinline__ double corner_disp(const SimScalars &sc, int k) {
  BoxD b;
  box_derive(sc.box, b);
  const int ix = k & 1, iy = (k >> 1) & 1, iz = k >> 2;
  const double dx = b.h[0] * ix + b.h[5] * iy + b.h[4] * iz + b.lo[0] - sc.corners_hold[3 * k];
  const double dy = b.h[1] * iy + b.h[3] * iz + b.lo[1] - sc.corners_hold[3 * k + 1];
  const double dz = b.h[2] * iz + b.lo[2] - sc.corners_hold[3 * k + 2];
  return sqrt(dx * dx + dy * dy + dz * dz);
}
// the two LARGEST of the eight: LAMMPS' Neighbor::check_distance drops the old maximum when a new one arrives -- `if (d > d1) d1 = d; else
// if (d > d2) d2 = d;` -- and so underestimates the corner motion of a box whose corners move by different amounts, by up to half.  A list
// may be built earlier than LAMMPS builds its own, never later than its validity: results do not depend on when a valid list is built.
__device__ __forceinline__ void two_largest(const double *d, double &d1, double &d2) {
  d1 = 0.0; d2 = 0.0;
  for (int k = 0; k < 8; k++) {
    if (d[k] > d1) { d2 = d1; d1 = d[k]; }
    else if (d[k] > d2) d2 = d[k];
  }
}
// d1, d2: the two largest corner displacements (k_post has eight lanes compute the eight; the overload below does it alone)
__device__ __forceinline__ void pre_scalars(const SimDev &S, SimScalars &sc, double d1, double d2) {
  {
    sc.step += 1;
    sc.ago += 1;
    sc.rebuild = sc.force_rebuild;   // a box flip between two steps forces the rebuild (fix deform: next_reneighbor)
    sc.force_rebuild = 0;
    sc.check = (sc.ago >= S.neigh_delay) ? 1 : 0;
    // neighbour trigger threshold with a deforming triclinic box: the two largest box-corner
    // displacements since the last build are taken off the skin (corners that have moved by the whole skin: every displacement
    // triggers -- LAMMPS squares the negative difference and tests against that)
    const double delta = 0.5 * (S.skin - (d1 + d2));
    sc.deltasq = delta > 0.0 ? delta * delta : 0.0;
    // skin bands (md_skin_bands.h): the box term of the rule; the displacement bounds come from k_initial_integrate
    sc.corner = d1 + d2;
    sc.walk_all = 0;
    if (S.nvt) sc.vscale *= nhc_half(S, sc);
    for (int k = 0; k < 6; k++) sc.ke[k] = 0.0;
    for (int k = 0; k < MD_NPART * 6; k++) sc.vir[k] = 0.0;
    for (int k = 0; k < MD_NPART; k++) sc.eng[k] = 0.0;
  }
}
__device__ __forceinline__ void pre_scalars(const SimDev &S, SimScalars &sc) {
  double d[8], d1, d2;
  for (int k = 0; k < 8; k++) d[k] = corner_disp(sc, k);
  two_largest(d, d1, d2);
  pre_scalars(S, sc, d1, d2);
}
__global__ void k_pre(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.x];
  if (threadIdx.x == 0) pre_scalars(S, *S.sc);
  for (int k = threadIdx.x; k < 2 * S.nk; k += blockDim.x) S.sfac[k] = 0.0;
  for (int k = threadIdx.x; k < S.ncells; k += blockDim.x) S.cell_count[k] = 0;
}

// ------------------------------------------------------------------------------------------
// k_initial_integrate : v = v*vscale + dt/2 f/m ; x += dt v ; displacement check
// ------------------------------------------------------------------------------------------
// PACK: also write the atom's slot-ordered record for k_pair (the flows with the cell / cluster lists of md_pair.hip; not ReaxFF, which
// keeps its own lists and has no slots)
template <bool PACK>
__global__ __launch_bounds__(TPB) void k_initial_integrate(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  SimScalars &sc = *S.sc;
  const double vs = sc.vscale;
  const double dtfm = 0.5 * S.dt * MD_FTM2V / S.mass[i];
  double dsq = 0.0;
  double vn[3], xn[3];
  bool sane = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    vn[k] = S.v[3 * i + k] * vs + dtfm * S.f[3 * i + k];
    xn[k] = S.x[3 * i + k] + S.dt * vn[k];
    sane = sane && fabs(xn[k]) < 1.0e8;   // false for NaN and for atoms flung out of any box
  }
  if (!sane) {
    // A replica that blew up (overlapping atoms, absurd time step).  Positions index memory (cells, tables), so a
    // non-finite one must never be stored: the atom is frozen where it was, the replica is flagged (bit 16) and the
    // host reports it instead of a stress.
    atomicOr(&sc.overflow, 16);
#pragma unroll
    for (int k = 0; k < 3; k++) { vn[k] = 0.0; xn[k] = S.x[3 * i + k]; }
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    S.v[3 * i + k] = vn[k];
    S.x[3 * i + k] = xn[k];
    double d = xn[k] - S.xhold[3 * i + k];
    dsq += d * d;
  }
  if (sc.check && dsq > sc.deltasq) sc.rebuild = 1;
  // Skin bands: the atom's displacement as an FP32 upper bound at its slot, and the replica's level flag of it (a plain store of the same
  // value by whoever gets there, like the rebuild flag; the flag is read first, so that a level is written by its first few atoms only).
  // On a step that rebuilds, the kernels that deal the slots anew clear both.
  if (S.dslot) {
    const float dup = sqrtf((float)dsq) * 1.00001f;
    S.dslot[S.slot_of[i]] = dup;
    const int lev = skin_level(dup, S.dquant_inv);
    if (sc.dflag[lev] == 0) sc.dflag[lev] = 1;
  }
  // The slot-ordered record of the atom for k_pair (what k_pack does for the flows without this kernel): wrapped position at the
  // atom's slot, its pair-force accumulator cleared.  On a step that rebuilds, the slots are dealt anew afterwards and k_cell_sort
  // writes all records of its cell, so what is stored here is then simply overwritten.
  if (PACK) {
    BoxD b;
    box_derive(sc.box, b);
    const size_t s = (size_t)S.slot_of[i], np = (size_t)S.npad;
    const int w0 = S.wrapn[3 * i], w1 = S.wrapn[3 * i + 1], w2 = S.wrapn[3 * i + 2];
    double *xy = (double *)S.xq + 2 * s, *zq = (double *)S.xq + 2 * np + 2 * s;
    xy[0] = xn[0] - (b.h[0] * w0 + b.h[5] * w1 + b.h[4] * w2);
    xy[1] = xn[1] - (b.h[1] * w1 + b.h[3] * w2);
    zq[0] = xn[2] - (b.h[2] * w2);
    S.fs[s] = 0.0; S.fs[np + s] = 0.0; S.fs[2 * np + s] = 0.0;
  }
}

// ------------------------------------------------------------------------------------------
// neighbour build pipeline (all early-exit unless sc->rebuild)
// ------------------------------------------------------------------------------------------
// A workgroup bins BIN_APT * TPB consecutive atoms and counts them per cell in LDS first: the per-cell counters of a replica are
// hit by 86 atoms each, and global atomics on one address serialise at the memory side (0.65 ms per 576-replica rebuild with
// one global atomic per atom).  Grids of more than BIN_MAXCELLS cells count in global memory directly.
#define BIN_APT 4
#define BIN_MAXCELLS 2048
__global__ __launch_bounds__(TPB) void k_bin(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  if (!sc.rebuild) return;
  if ((int)(blockIdx.x * TPB * BIN_APT) >= S.natoms) return;
  __shared__ int s_cnt[BIN_MAXCELLS];
  const bool in_lds = S.ncells <= BIN_MAXCELLS;
  if (in_lds) {
    for (int k = threadIdx.x; k < S.ncells; k += TPB) s_cnt[k] = 0;
    __syncthreads();
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    box_corners(sc.box, sc.corners_hold);
    sc.force_rebuild = 0;
    sc.corner = 0.0;   // fresh list: every listed skin pair is outside the cutoff (no band open until something has moved)
    sc.walk_all = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x < MD_DLEVELS) sc.dflag[threadIdx.x] = 0;
  BoxD b;
  box_derive(sc.box, b);
  int nsub[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    // position inside the cell on a grid of ~1.1 A sub-cells (isotropic in Angstrom whatever the shape of the
    // cell, at most 16 per edge) -> Morton key: consecutive slots of a cell are spatial neighbours, which keeps the
    // 4-atom i-clusters of k_pair compact
    const double edge = (d == 0 ? b.h[0] : d == 1 ? b.h[1] : b.h[2]) / S.nc[d];
    const int n = (int)ceil(edge / 1.1);
    nsub[d] = n < 2 ? 2 : (n > 16 ? 16 : n);
  }
  for (int u = 0; u < BIN_APT; u++) {
    const int i = (blockIdx.x * BIN_APT + u) * TPB + threadIdx.x;
    if (i >= S.natoms) break;
    double x0 = S.x[3 * i], x1 = S.x[3 * i + 1], x2 = S.x[3 * i + 2];
    S.xhold[3 * i] = x0; S.xhold[3 * i + 1] = x1; S.xhold[3 * i + 2] = x2;
    double d0 = x0 - b.lo[0], d1 = x1 - b.lo[1], d2 = x2 - b.lo[2];
    double l[3];
    l[0] = b.hinv[0] * d0 + b.hinv[5] * d1 + b.hinv[4] * d2;
    l[1] = b.hinv[1] * d1 + b.hinv[3] * d2;
    l[2] = b.hinv[2] * d2;
    int c[3];
    int key = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      double fl = floor(l[d]);
      double w = l[d] - fl;
      if (w >= 1.0) { w = 0.0; fl += 1.0; }   // l = -1e-17: l - floor(l) rounds to 1.  The image that belongs to cell 0 is the one just below the low face
      S.wrapn[3 * i + d] = (int)fl;
      int cc = (int)(w * S.nc[d]);
      if (cc >= S.nc[d]) cc = S.nc[d] - 1;
      if (cc < 0) cc = 0;
      c[d] = cc;
      int sub = (int)((w * S.nc[d] - cc) * nsub[d]);
      sub = sub < 0 ? 0 : (sub > nsub[d] - 1 ? nsub[d] - 1 : sub);
      key |= ((sub & 1) << d) | ((sub & 2) << (d + 2)) | ((sub & 4) << (d + 4)) | ((sub & 8) << (d + 6));
    }
    S.ckey[i] = key;
    const int cell = (c[2] * S.nc[1] + c[1]) * S.nc[0] + c[0];
    S.cell_of[i] = cell;
    if (in_lds) atomicAdd(&s_cnt[cell], 1);
    else atomicAdd(&S.cell_count[cell], 1);
  }
  if (in_lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < S.ncells; k += TPB) {
      const int n = s_cnt[k];
      if (n) atomicAdd(&S.cell_count[k], n);
    }
  }
}

__global__ __launch_bounds__(TPB) void k_cell_scan(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  if (!sc.rebuild) return;
  __shared__ int s_part[TPB];
  __shared__ int s_base;
  if (threadIdx.x == 0) s_base = 0;
  __syncthreads();
  // every slot is a pad slot until k_cell_sort places an atom there
  for (int s = threadIdx.x; s < S.npad; s += TPB) S.perm[s] = -1;
  for (int start = 0; start < S.ncells; start += TPB) {
    int idx = start + threadIdx.x;
    // cells are padded to a multiple of MD_CLUSTER slots so that a cluster of MD_CLUSTER
    // consecutive slots never straddles two cells (k_pair works on such clusters)
    int v = (idx < S.ncells) ? (S.cell_count[idx] + MD_CLUSTER - 1) / MD_CLUSTER * MD_CLUSTER : 0;
    s_part[threadIdx.x] = v;
    __syncthreads();
    // Hillis-Steele inclusive scan
    for (int o = 1; o < TPB; o <<= 1) {
      int t = (threadIdx.x >= o) ? s_part[threadIdx.x - o] : 0;
      __syncthreads();
      s_part[threadIdx.x] += t;
      __syncthreads();
    }
    int incl = s_part[threadIdx.x];
    int base = s_base;
    if (idx < S.ncells) {
      S.cell_start[idx] = base + incl - v;
      S.cell_fill[idx] = 0;
    }
    __syncthreads();
    if (threadIdx.x == TPB - 1) s_base = base + incl;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    S.cell_start[S.ncells] = s_base;
    sc.ago = 0;
    sc.nbuilds += 1;
    sc.nentries = 0ull;
    if (!(S.rlist_ref2 < S.rlist2) || sc.step == 0) sc.nentries_ref = 0ull;   // (a wider list counts the reference's pairs at the first build of a run only)
    sc.nrowent = 0ull;
  }
}

// slots of the cell's range are handed out in any order (k_cell_sort fixes the order afterwards): a workgroup counts its
// BIN_APT * TPB atoms per cell in LDS, reserves one range per cell with a single global atomic, and numbers its atoms inside
__global__ __launch_bounds__(TPB) void k_cell_fill(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  if ((int)(blockIdx.x * TPB * BIN_APT) >= S.natoms) return;
  __shared__ int s_cnt[BIN_MAXCELLS];
  const bool in_lds = S.ncells <= BIN_MAXCELLS;
  int cell[BIN_APT], rank[BIN_APT];
  if (in_lds) {
    for (int k = threadIdx.x; k < S.ncells; k += TPB) s_cnt[k] = 0;
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < BIN_APT; u++) {
    const int i = (blockIdx.x * BIN_APT + u) * TPB + threadIdx.x;
    cell[u] = -1; rank[u] = 0;
    if (i < S.natoms) {
      cell[u] = S.cell_of[i];
      rank[u] = in_lds ? atomicAdd(&s_cnt[cell[u]], 1) : atomicAdd(&S.cell_fill[cell[u]], 1);
    }
  }
  if (in_lds) {
    __syncthreads();
    for (int k = threadIdx.x; k < S.ncells; k += TPB) {
      const int n = s_cnt[k];
      s_cnt[k] = n ? atomicAdd(&S.cell_fill[k], n) : 0;   // first slot of this workgroup's share of the cell
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < BIN_APT; u++) {
    const int i = (blockIdx.x * BIN_APT + u) * TPB + threadIdx.x;
    if (cell[u] >= 0) S.slot_tmp[S.cell_start[cell[u]] + (in_lds ? s_cnt[cell[u]] : 0) + rank[u]] = i;
  }
}

// slot-ordered record of one slot: wrapped position + charge as two 16-byte halves, (x,y)[npad] then (z,q)[npad] (see md_pair.hip),
// type, cleared pair-force accumulator.  a < 0: a pad slot -- a record no real atom is ever within the list cutoff of, every pad at
// its own place, 10^6 A from the next (two pads of one cell must not list each other either: the whole-table walk of
// k_neigh_build, taken when a group list overflows, tests pads against pads)
__device__ __forceinline__ void pack_slot(const SimDev &S, int s, int a, double x, double y, double z) {
  double *xy = (double *)S.xq + 2 * (size_t)s, *zq = (double *)S.xq + 2 * (size_t)S.npad + 2 * (size_t)s;
  if (a < 0) { xy[0] = 1.0e15 + 1.0e6 * (double)s; xy[1] = 1.0e15; zq[0] = 1.0e15; zq[1] = 0.0; S.stype[s] = 0; }
  else { xy[0] = x; xy[1] = y; zq[0] = z; zq[1] = S.q[a]; S.stype[s] = S.type[a]; }
  S.fs[s] = 0.0; S.fs[(size_t)S.npad + s] = 0.0; S.fs[2 * (size_t)S.npad + s] = 0.0;
  if (S.dslot) S.dslot[s] = 0.0f;   // (skin bands: nothing has moved since this build; a pad never does)
}

// k_cell_build : k_bin + k_cell_scan + k_cell_fill in ONE launch for replicas of up to CB_MAXATOMS atoms and BIN_MAXCELLS cells: one
// workgroup per replica, the cell counters and starts in LDS, no global atomics.  A step that does not rebuild pays one empty launch
// instead of three (a single replica is launch-bound: VERDICT r2 item 7), and a rebuild is three passes of one workgroup over its
// atoms.  Larger replicas keep the three kernels above (mdk_neighbor decides; SCEMA_MD_CELL_BUILD=0 forces them).
#define CB_TPB 1024
#define CB_MAXATOMS 65536
// coord > 0 (small launch groups that run whole, run_phase): the replicas of the launch rebuild TOGETHER -- as soon as one of them asks for
// it, all do.  A lone replica's rebuild keeps a quarter of the chip busy at the speed of its latencies (110-140 us for PE-10k) while the rest
// of the group waits: at 9 replicas that was 70 us of every 330-us step; nine rebuilds in one set of launches take little longer than one.
// Building a list before its displacement test asks for it is always valid: results do not depend on when a list is built -- as long as no
// list is ever used past its validity, which `neigh_modify delay 5` (the reference's setting: no test for five steps after a build) only
// guarantees while no atom covers half the skin in five steps.  Where one does (LAMMPS' "dangerous builds": a skin of 1 A on a hot or fast
// sheared system, never the reference's 2 A at 300 K) LAMMPS' own result depends on the step its lists were built at, and so does this one.
__global__ __launch_bounds__(CB_TPB) void k_cell_build(const SimDev *sims, int coord) {
  const SimDev &S = sims[blockIdx.x];
  SimScalars &sc = *S.sc;
  if (coord > 0) {
    int any = 0;
    for (int j = threadIdx.x; j < coord; j += CB_TPB) any |= sims[j].sc->rebuild;   // (set by the kernels before this one; a flag raised below by another workgroup of this launch only confirms what its own scan found)
    any = __syncthreads_or(any);
    if (!any) return;
    if (threadIdx.x == 0) sc.rebuild = 1;   // for the kernels behind this one
  } else if (!sc.rebuild) return;
  __shared__ int s_cnt[BIN_MAXCELLS], s_start[BIN_MAXCELLS];
  __shared__ int s_wsum[CB_TPB / 64];
  const int ncells = S.ncells, natoms = S.natoms;
  for (int k = threadIdx.x; k < ncells; k += CB_TPB) s_cnt[k] = 0;
  if (threadIdx.x == 0) {
    box_corners(sc.box, sc.corners_hold);
    sc.force_rebuild = 0;
    sc.corner = 0.0;   // fresh list: every listed skin pair is outside the cutoff (no band open until something has moved)
    sc.walk_all = 0;
  }
  if (threadIdx.x < MD_DLEVELS) sc.dflag[threadIdx.x] = 0;
  BoxD b;
  box_derive(sc.box, b);
  int nsub[3];
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double edge = (d == 0 ? b.h[0] : d == 1 ? b.h[1] : b.h[2]) / S.nc[d];
    const int n = (int)ceil(edge / 1.1);
    nsub[d] = n < 2 ? 2 : (n > 16 ? 16 : n);
  }
  __syncthreads();
  // pass 1: cell, sub-cell key and periodic image of every atom (as k_bin); its place among the atoms of its cell = the old value of the
  // cell's LDS counter (any order: k_cell_sort fixes the order afterwards), kept in slot_of until pass 3
  for (int i = threadIdx.x; i < natoms; i += CB_TPB) {
    const double x0 = S.x[3 * i], x1 = S.x[3 * i + 1], x2 = S.x[3 * i + 2];
    S.xhold[3 * i] = x0; S.xhold[3 * i + 1] = x1; S.xhold[3 * i + 2] = x2;
    const double d0 = x0 - b.lo[0], d1 = x1 - b.lo[1], d2 = x2 - b.lo[2];
    double l[3];
    l[0] = b.hinv[0] * d0 + b.hinv[5] * d1 + b.hinv[4] * d2;
    l[1] = b.hinv[1] * d1 + b.hinv[3] * d2;
    l[2] = b.hinv[2] * d2;
    int c[3];
    int key = 0;
#pragma unroll
    for (int d = 0; d < 3; d++) {
      double fl = floor(l[d]);
      double w = l[d] - fl;
      if (w >= 1.0) { w = 0.0; fl += 1.0; }   // (as in k_bin: the image count goes with the cell)
      S.wrapn[3 * i + d] = (int)fl;
      int cc = (int)(w * S.nc[d]);
      if (cc >= S.nc[d]) cc = S.nc[d] - 1;
      if (cc < 0) cc = 0;
      c[d] = cc;
      int sub = (int)((w * S.nc[d] - cc) * nsub[d]);
      sub = sub < 0 ? 0 : (sub > nsub[d] - 1 ? nsub[d] - 1 : sub);
      key |= ((sub & 1) << d) | ((sub & 2) << (d + 2)) | ((sub & 4) << (d + 4)) | ((sub & 8) << (d + 6));
    }
    S.ckey[i] = key;
    const int cell = (c[2] * S.nc[1] + c[1]) * S.nc[0] + c[0];
    S.cell_of[i] = cell;
    S.slot_of[i] = atomicAdd(&s_cnt[cell], 1);
  }
  __syncthreads();
#ifdef PAIR_WHATIF_TILE_ORDER
  // what-if: the tiles of k_pair in descending order of their atoms (= rows), so that the last workgroups of a launch
  // are the cheapest ones; the permutation lives in cell_fill, which this path does not use otherwise
  for (int c = threadIdx.x; c < ncells; c += CB_TPB) {
    const int mine = s_cnt[c];
    int rank = 0;
    for (int o = 0; o < ncells; o++) rank += (s_cnt[o] > mine || (s_cnt[o] == mine && o < c)) ? 1 : 0;
    S.cell_fill[rank] = c;
  }
#endif
  // pass 2: cell starts = exclusive scan of the counts padded to whole clusters (a cluster of MD_CLUSTER consecutive slots never
  // straddles two cells); every slot is a pad slot until k_cell_sort places an atom there
  {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = 2 * (int)threadIdx.x, i1 = i0 + 1;   // BIN_MAXCELLS = 2 * CB_TPB
    const int n0 = (i0 < ncells) ? s_cnt[i0] : 0, n1 = (i1 < ncells) ? s_cnt[i1] : 0;
    const int v0 = (n0 + MD_CLUSTER - 1) / MD_CLUSTER * MD_CLUSTER, v1 = (n1 + MD_CLUSTER - 1) / MD_CLUSTER * MD_CLUSTER;
    int incl = v0 + v1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += s_wsum[w];
    const int e0 = base + incl - (v0 + v1);
    if (i0 < ncells) { s_start[i0] = e0; S.cell_start[i0] = e0; S.cell_count[i0] = n0; }
    if (i1 < ncells) { s_start[i1] = e0 + v0; S.cell_start[i1] = e0 + v0; S.cell_count[i1] = n1; }
    if (threadIdx.x == CB_TPB - 1) {
      S.cell_start[ncells] = base + incl;
      sc.ago = 0;
      sc.nbuilds += 1;
      sc.nentries = 0ull;
      if (!(S.rlist_ref2 < S.rlist2) || sc.step == 0) sc.nentries_ref = 0ull;
      sc.nrowent = 0ull;
    }
    for (int sl = threadIdx.x; sl < S.npad; sl += CB_TPB) S.perm[sl] = -1;
  }
  __syncthreads();
  // pass 3: atoms to their places
  for (int i = threadIdx.x; i < natoms; i += CB_TPB) S.slot_tmp[s_start[S.cell_of[i]] + S.slot_of[i]] = i;
}

// Deterministic order inside each cell, chosen so that 4 consecutive slots (one i-cluster of k_pair) are spatial
// neighbours: a k-d ordering.  The cell's atoms are split recursively at the median of the longest extent of the
// current group (left part = half of the group's clusters, a multiple of 4 atoms) until the groups are single
// clusters; ties by atom index, so the result does not depend on the atomic fill order.  One wave per cell, O(n^2)
// rank counting per level in LDS (n <= KD_MAX; larger cells fall back to the Morton key of k_bin).
// KD_MAX = 128 or 256 (the launch picks by the mean cell population: the smaller one doubles the waves a CU holds, and this kernel
// is bound by the latency of its LDS loops); a cell beyond KD_MAX atoms takes the Morton order
template <int KD_MAX>
__global__ __launch_bounds__(64) void k_cell_sort(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.sc->rebuild) return;
  const int c = blockIdx.x;
  if (c >= S.ncells) return;
  const int b = S.cell_start[c], n = S.cell_count[c];  // the rest of the cell's range stays pad (-1)
  if (n > KD_MAX) {
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + (int)threadIdx.x;
      const int a = (i < n) ? S.slot_tmp[b + i] : 0;
      const int ka = (i < n) ? S.ckey[a] : 0;
      int r = 0;
      for (int j0 = 0; j0 < n; j0 += 64) {
        const int j = j0 + (int)threadIdx.x;
        const int o_l = (j < n) ? S.slot_tmp[b + j] : 0x7fffffff;
        const int ko_l = (j < n) ? S.ckey[o_l] : 0x7fffffff;
        const int m = min(64, n - j0);
        for (int t = 0; t < m; t++) {
          const int o = __shfl(o_l, t, 64), ko = __shfl(ko_l, t, 64);
          r += (ko < ka || (ko == ka && o < a)) ? 1 : 0;
        }
      }
      if (i < n) {
        S.perm[b + r] = a;
        S.slot_of[a] = b + r;
        BoxD bx;
        box_derive(S.sc->box, bx);
        const int w0 = S.wrapn[3 * a], w1 = S.wrapn[3 * a + 1], w2 = S.wrapn[3 * a + 2];
        pack_slot(S, b + r, a, S.x[3 * a] - (bx.h[0] * w0 + bx.h[5] * w1 + bx.h[4] * w2), S.x[3 * a + 1] - (bx.h[1] * w1 + bx.h[3] * w2), S.x[3 * a + 2] - (bx.h[2] * w2));
      }
    }
    for (int s = b + n + (int)threadIdx.x; s < S.cell_start[c + 1]; s += 64) pack_slot(S, s, -1, 0.0, 0.0, 0.0);
    return;
  }
  // coordinates and atom ids travel with the order (two buffers, swapped per level): the loops over a group read consecutive LDS
  // entries without a dependent index load in between (with an index array they waited for two LDS latencies per element:
  // 2.5 ms per 576-replica rebuild)
  __shared__ double s_x[2][KD_MAX][3];
  __shared__ int s_gid[2][KD_MAX];
  __shared__ int s_s[2][KD_MAX], s_e[2][KD_MAX];
  {
    BoxD bx;
    box_derive(S.sc->box, bx);
    for (int k = threadIdx.x; k < n; k += 64) {
      const int a = S.slot_tmp[b + k];
      const int w0 = S.wrapn[3 * a], w1 = S.wrapn[3 * a + 1], w2 = S.wrapn[3 * a + 2];
      s_x[0][k][0] = S.x[3 * a] - (bx.h[0] * w0 + bx.h[5] * w1 + bx.h[4] * w2);
      s_x[0][k][1] = S.x[3 * a + 1] - (bx.h[1] * w1 + bx.h[3] * w2);
      s_x[0][k][2] = S.x[3 * a + 2] - (bx.h[2] * w2);
      s_gid[0][k] = a;
      s_s[0][k] = 0; s_e[0][k] = n;
    }
  }
  int cur = 0;
  for (int level = 0; level < 10; level++) {
    __syncthreads();
    bool split_any = false;
    for (int p = threadIdx.x; p < n; p += 64) {
      const int s0 = s_s[cur][p], e0 = s_e[cur][p], cnt = e0 - s0;
      const double xp[3] = {s_x[cur][p][0], s_x[cur][p][1], s_x[cur][p][2]};
      const int gp = s_gid[cur][p];
      int np = p, ns = s0, ne = e0;
      if (cnt > 4) {
        split_any = true;
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
#pragma unroll 4
        for (int q = s0; q < e0; q++)
#pragma unroll
          for (int d = 0; d < 3; d++) { const double xv = s_x[cur][q][d]; lo[d] = fmin(lo[d], xv); hi[d] = fmax(hi[d], xv); }
        const double ex0 = hi[0] - lo[0], ex1 = hi[1] - lo[1], ex2 = hi[2] - lo[2];
        const int axis = (ex0 >= ex1 && ex0 >= ex2) ? 0 : (ex1 >= ex2 ? 1 : 2);
        const double xpa = axis == 0 ? xp[0] : (axis == 1 ? xp[1] : xp[2]);
        int rank = 0;
#pragma unroll 4
        for (int q = s0; q < e0; q++) {
          const double xq_ = s_x[cur][q][axis];
          rank += (xq_ < xpa || (xq_ == xpa && s_gid[cur][q] < gp)) ? 1 : 0;
        }
        const int nclus = (cnt + 3) / 4;
        const int left = ((nclus + 1) / 2) * 4;   // half of the group's clusters (rounded up), always < cnt
        np = s0 + rank;
        if (rank < left) { ns = s0; ne = s0 + left; } else { ns = s0 + left; ne = e0; }
      }
      s_x[1 - cur][np][0] = xp[0]; s_x[1 - cur][np][1] = xp[1]; s_x[1 - cur][np][2] = xp[2];
      s_gid[1 - cur][np] = gp; s_s[1 - cur][np] = ns; s_e[1 - cur][np] = ne;
    }
    cur = 1 - cur;
    if (!__any(split_any)) break;
  }
  __syncthreads();
  // the new order, and with it the slot-ordered records that k_pair and the list build read (the wrapped positions are at hand)
  for (int p = threadIdx.x; p < n; p += 64) {
    const int a = s_gid[cur][p];
    S.perm[b + p] = a;
    S.slot_of[a] = b + p;
    pack_slot(S, b + p, a, s_x[cur][p][0], s_x[cur][p][1], s_x[cur][p][2]);
  }
  for (int s = b + n + (int)threadIdx.x; s < S.cell_start[c + 1]; s += 64) pack_slot(S, s, -1, 0.0, 0.0, 0.0);
}

// k_pack : every step of the flows whose integrator does not write the records itself (Nose-Hoover / barostat runs, the minimiser,
// the set-up evaluation): slot-ordered wrapped coordinates, cleared pair-force accumulators
__global__ __launch_bounds__(TPB) void k_pack(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int s = blockIdx.x * TPB + threadIdx.x;
  if (s >= S.npad) return;
  // k_pair accumulates into the slot-ordered pair forces with atomics
  S.fs[s] = 0.0; S.fs[(size_t)S.npad + s] = 0.0; S.fs[2 * (size_t)S.npad + s] = 0.0;   // (fb needs no zeroing: k_bonded stores every entry)
  const int a = S.perm[s];
  if (a < 0) return;   // pad slot (its record was written when the slots were dealt: k_cell_sort)
  BoxD b;
  box_derive(S.sc->box, b);
  const int w0 = S.wrapn[3 * a], w1 = S.wrapn[3 * a + 1], w2 = S.wrapn[3 * a + 2];
  double4 r;
  r.x = S.x[3 * a] - (b.h[0] * w0 + b.h[5] * w1 + b.h[4] * w2);
  r.y = S.x[3 * a + 1] - (b.h[1] * w1 + b.h[3] * w2);
  r.z = S.x[3 * a + 2] - (b.h[2] * w2);
  // two arrays of 16-byte halves: (x,y)[npad], (z,q)[npad]  (see md_pair.hip)
  double *xy = (double *)S.xq + 2 * (size_t)s, *zq = (double *)S.xq + 2 * (size_t)S.npad + 2 * (size_t)s;
  xy[0] = r.x; xy[1] = r.y; zq[0] = r.z;   // (charge and type of a slot change only when the slots are dealt anew: k_cell_sort)
}

// k_neigh_build and k_pair live in md_pair.hip, the bonded terms in md_bonded.hip

__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void vt(double *v, double ax, double ay, double az, double fx, double fy, double fz) {
  v[0] += ax * fx; v[1] += ay * fy; v[2] += az * fz; v[3] += ax * fy; v[4] += ax * fz; v[5] += ay * fz;
}

// ------------------------------------------------------------------------------------------
// reciprocal Ewald sum
// ------------------------------------------------------------------------------------------
#define EW_ATOMS 64        // atoms staged per block in k_ewald_sfac
extern __shared__ double2 s_dyn[];  // phase tables, sized by the launch (3*Mmax entries per atom)

// fractional coordinates of atom a in [0,1): the phase angles of the Ewald sums are 2 pi times these, taken with
// sincospi (exact argument reduction, a fraction of the cost of sincos)
__device__ __forceinline__ void atom_phase(const SimDev &S, const BoxD &b, int a, double &t0, double &t1, double &t2) {
  const double d0 = S.x[3 * a] - b.lo[0], d1 = S.x[3 * a + 1] - b.lo[1], d2 = S.x[3 * a + 2] - b.lo[2];
  double l0 = b.hinv[0] * d0 + b.hinv[5] * d1 + b.hinv[4] * d2;
  double l1 = b.hinv[1] * d1 + b.hinv[3] * d2;
  double l2 = b.hinv[2] * d2;
  t0 = l0 - floor(l0);
  t1 = l1 - floor(l1);
  t2 = l2 - floor(l2);
}

// S(k) = sum_i q_i exp(i k.r_i): threads own GROUPS of k-vectors (n1, +-n2, +-n3), atoms are staged
// through LDS as per-atom tables exp(i m theta_d), m = 0..kmax_d (layout [atom][d][m] keeps lanes on
// consecutive 16-byte slots).  The up to four members of a group share the three table reads and the
// products of the phase factors: 3 LDS reads and ~32 FP64 operations per (atom, group) instead of
// 12 reads and ~48 operations (the kernel was LDS-bandwidth bound with one k-vector per thread).
// Blocks of one simulation add into the same S(k) with global atomics, which execute at the memory side and
// serialise per address: the atoms of a simulation are therefore spread over only EW_PARTS blocks, each walking
// its share of the atoms in chunks of EW_ATOMS and keeping the partial sums in registers.
#define EW_PARTS 16
// NR = rounds of groups per thread: thread gi owns the groups gi, gi + gthreads, ... (NR of them), so that k sets of up to
// NR * 256 groups (replicas of a few 10^4 atoms at the reference's accuracy) stay on the table path
template <int NR>
__global__ __launch_bounds__(256) void k_ewald_sfac(const SimDev *sims, int EW_MAXM, int gthreads, int nparts) {
  const SimDev &S = sims[blockIdx.y];
  if (S.nk == 0) return;
  double2 *s_tab = s_dyn;  // [EW_ATOMS][3][EW_MAXM]
  const int M0 = S.kmaxd[0] + 1, M1 = S.kmaxd[1] + 1, M2 = S.kmaxd[2] + 1;
  const int MS = 3 * EW_MAXM;
  const int nchunk = (S.natoms + EW_ATOMS - 1) / EW_ATOMS;
  // gthreads threads span the groups; the block's nsplit = blockDim / gthreads thread sets interleave the atoms
  const int nsplit = blockDim.x / gthreads, part = threadIdx.x / gthreads;
  const int gi = threadIdx.x % gthreads;
  int n1[NR], m2[NR], m3[NR], kpp[NR], kmp[NR], kpm[NR], kmm[NR];
  // exp(i(t1 +- t2 +- t3)) of the up to four members of a group are linear combinations of the eight real products
  // {cos,sin}(t1) {cos,sin}(t2) {cos,sin}(t3): those are what is summed over the atoms (4 products + 8 FMAs per atom and
  // group, the charge folded into the first table), and combined once at the end
  double T[NR][8];   // ccc ccs csc css scc scs ssc sss
#pragma unroll
  for (int r = 0; r < NR; r++) {
    n1[r] = 0; m2[r] = 0; m3[r] = 0; kpp[r] = -1; kmp[r] = -1; kpm[r] = -1; kmm[r] = -1;
    const int g = r * gthreads + gi;
    if (g < S.ngrp) {
      const int4 Ga = ((const int4 *)S.kgrp)[2 * g], Gb = ((const int4 *)S.kgrp)[2 * g + 1];
      n1[r] = Ga.x; m2[r] = Ga.y; m3[r] = Ga.z;
      kpp[r] = Ga.w; kmp[r] = Gb.x; kpm[r] = Gb.y; kmm[r] = Gb.z;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) T[r][q] = 0.0;
  }
  BoxD b;
  box_derive(S.sc->box, b);
  for (int ch = blockIdx.x; ch < nchunk; ch += nparts) {
    const int a0 = ch * EW_ATOMS;
    const int na = min(EW_ATOMS, S.natoms - a0);
    __syncthreads();
    for (int idx = threadIdx.x; idx < 3 * EW_ATOMS; idx += blockDim.x) {
      const int la = idx / 3, d = idx % 3;
      if (la < na) {
        double t[3];
        atom_phase(S, b, a0 + la, t[0], t[1], t[2]);
        double s1, c1;
        sincospi(2.0 * t[d], &s1, &c1);
        const int M = (d == 0) ? M0 : (d == 1) ? M1 : M2;
        const double qa = (d == 0) ? S.q[a0 + la] : 1.0;
        double cr = 1.0, ci = 0.0;
        double2 *tab = s_tab + la * MS + d * EW_MAXM;
        for (int m = 0; m < M; m++) {
          tab[m] = make_double2(qa * cr, qa * ci);
          const double nr = cr * c1 - ci * s1, ni = ci * c1 + cr * s1;
          cr = nr; ci = ni;
        }
      }
    }
    __syncthreads();
    if (gi < S.ngrp)
      for (int la = part; la < na; la += nsplit) {
#pragma unroll
        for (int r = 0; r < NR; r++) {
          const double2 e1 = s_tab[la * MS + n1[r]];
          const double2 e2 = s_tab[la * MS + EW_MAXM + m2[r]];
          const double2 e3 = s_tab[la * MS + 2 * EW_MAXM + m3[r]];
          const double cc = e1.x * e2.x, cs = e1.x * e2.y, sc_ = e1.y * e2.x, ss = e1.y * e2.y;
          T[r][0] = fma(cc, e3.x, T[r][0]); T[r][1] = fma(cc, e3.y, T[r][1]); T[r][2] = fma(cs, e3.x, T[r][2]); T[r][3] = fma(cs, e3.y, T[r][3]);
          T[r][4] = fma(sc_, e3.x, T[r][4]); T[r][5] = fma(sc_, e3.y, T[r][5]); T[r][6] = fma(ss, e3.x, T[r][6]); T[r][7] = fma(ss, e3.y, T[r][7]);
        }
      }
  }
  // Re = ccc - s2 s3 css - s2 ssc - s3 scs ; Im = scc + s2 csc + s3 ccs - s2 s3 sss  (s2, s3 = signs of n2, n3)
  // all indices are in registers: the atomics go out back to back
  double *sf = S.sfac;
#pragma unroll
  for (int r = 0; r < NR; r++) {
    const double T0 = T[r][0], T1 = T[r][1], T2 = T[r][2], T3 = T[r][3], T4 = T[r][4], T5 = T[r][5], T6 = T[r][6], T7 = T[r][7];
    if (kpp[r] >= 0) { atomicAdd(&sf[2 * kpp[r]], T0 - T3 - T6 - T5); atomicAdd(&sf[2 * kpp[r] + 1], T4 + T2 + T1 - T7); }
    if (kmp[r] >= 0) { atomicAdd(&sf[2 * kmp[r]], T0 + T3 + T6 - T5); atomicAdd(&sf[2 * kmp[r] + 1], T4 - T2 + T1 + T7); }
    if (kpm[r] >= 0) { atomicAdd(&sf[2 * kpm[r]], T0 + T3 - T6 + T5); atomicAdd(&sf[2 * kpm[r] + 1], T4 + T2 - T1 + T7); }
    if (kmm[r] >= 0) { atomicAdd(&sf[2 * kmm[r]], T0 - T3 + T6 + T5); atomicAdd(&sf[2 * kmm[r] + 1], T4 - T2 - T1 - T7); }
  }
  // more groups than NR * gthreads (huge k sets): the rest one group at a time, phases recomputed per atom
  for (int g2 = NR * gthreads + (int)threadIdx.x; g2 < S.ngrp; g2 += blockDim.x) {
    const int *G = S.kgrp + 8 * g2;
    for (int mm = 0; mm < 4; mm++) {
      const int k = G[3 + mm];
      if (k < 0) continue;
      const int a1 = S.kn[3 * k], a2 = S.kn[3 * k + 1], a3 = S.kn[3 * k + 2];
      double sr = 0.0, si = 0.0;
      for (int ch = blockIdx.x; ch < nchunk; ch += nparts)
        for (int la = 0; la < EW_ATOMS && ch * EW_ATOMS + la < S.natoms; la++) {
          double t[3];
          atom_phase(S, b, ch * EW_ATOMS + la, t[0], t[1], t[2]);
          double s1, c1;
          sincospi(2.0 * (a1 * t[0] + a2 * t[1] + a3 * t[2]), &s1, &c1);
          sr += S.q[ch * EW_ATOMS + la] * c1; si += S.q[ch * EW_ATOMS + la] * s1;
        }
      atomicAdd(&sf[2 * k], sr);
      atomicAdd(&sf[2 * k + 1], si);
    }
  }
}

// per-k coefficients for the current box + energy / virial of the reciprocal sum
__global__ __launch_bounds__(TPB) void k_ewald_post(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  if (S.nk == 0) return;
  __shared__ double s_red[8 * (TPB / 64)];
  if ((int)(blockIdx.x * TPB) >= S.nk) return;
  const int k = blockIdx.x * TPB + threadIdx.x;
  double v[6] = {0, 0, 0, 0, 0, 0}, e[1] = {0};
  if (k < S.nk) {
    BoxD b;
    box_derive(sc.box, b);
    const int n1 = S.kn[3 * k], n2 = S.kn[3 * k + 1], n3 = S.kn[3 * k + 2];
    const double kx = 2.0 * MD_PI * (b.hinv[0] * n1);
    const double ky = 2.0 * MD_PI * (b.hinv[5] * n1 + b.hinv[1] * n2);
    const double kz = 2.0 * MD_PI * (b.hinv[4] * n1 + b.hinv[3] * n2 + b.hinv[2] * n3);
    const double sqk = kx * kx + ky * ky + kz * kz;
    const double g2inv = 1.0 / (S.g_ewald * S.g_ewald);
    const double ug = 4.0 * MD_PI / b.vol * exp(-0.25 * sqk * g2inv) / sqk;
    S.kvec[4 * k] = kx; S.kvec[4 * k + 1] = ky; S.kvec[4 * k + 2] = kz; S.kvec[4 * k + 3] = ug;
    const double Sr = S.sfac[2 * k], Si = S.sfac[2 * k + 1];
    const double uk = MD_QQRD2E * ug * (Sr * Sr + Si * Si);
    const double vterm = -2.0 * (1.0 / sqk + 0.25 * g2inv);
    e[0] = uk;
    v[0] = uk * (1.0 + vterm * kx * kx); v[1] = uk * (1.0 + vterm * ky * ky); v[2] = uk * (1.0 + vterm * kz * kz);
    v[3] = uk * vterm * kx * ky; v[4] = uk * vterm * kx * kz; v[5] = uk * vterm * ky * kz;
    if (k == 0) {
      // self energy and neutralising background
      e[0] -= MD_QQRD2E * (S.g_ewald * S.qsqsum / sqrt(MD_PI) + 0.5 * MD_PI * S.qsum * S.qsum / (S.g_ewald * S.g_ewald * b.vol));
    }
  }
  block_atomic_add<6>(v, sc.vir + P_KSPACE * 6, s_red);
  block_atomic_add<1>(e, sc.eng + P_KSPACE, s_red);
}

// F_i = 2 q_i sum_k ug k (sin_i Sr - cos_i Si), one thread per atom.  The phase exp(i k.r_i) =
// e1^n1 e2^n2 e3^n3 is carried as a cursor over the k list (lexicographic in (n1,n2,n3), so the
// usual move is n3 -> n3+1 = one complex multiplication by e3; row and slab changes are re-derived
// from the running power of e1).  No per-atom tables: nothing in LDS but the per-k data (indices,
// ug*S(k), k vector), staged in chunks and read as broadcasts.
#define EWF_TPB 256
#define EWF_KC 64
struct __attribute__((aligned(16))) EwK {
  double pr, pi;   // ug * Re S, ug * Im S
  double kx, ky;
  double kz;
  int n1, n23;     // n1 ; (n2 + 128) | (n3 + 128) << 8
};
__device__ __forceinline__ void cmul(double &pr, double &pi, double c, double s) {
  const double nr = pr * c - pi * s, ni = pi * c + pr * s;
  pr = nr; pi = ni;
}
#define EWF_APT 2          // atoms per thread: two independent recurrences per lane, half the per-k LDS reads and scalar work per atom
// EWF_T threads per block: 256 for batches, 64 for small ones (a single replica then spreads over 81 instead of 21 blocks)
template <int EWF_T>
__global__ __launch_bounds__(EWF_T) void k_ewald_force(const SimDev *sims, int pairvir, int fkeep) {
  const SimDev &S = sims[blockIdx.y];
  if ((int)(blockIdx.x * EWF_T * EWF_APT) >= S.natoms) return;
  __shared__ EwK s_k[EWF_KC];
  __shared__ int s_run[EWF_KC];
  __shared__ double s_red[8 * (EWF_T / 64)];
  int at[EWF_APT];
  bool act[EWF_APT];
  double c1[EWF_APT], s1[EWF_APT], c2[EWF_APT], s2[EWF_APT], c3[EWF_APT], s3[EWF_APT];
  {
    BoxD b;
    box_derive(S.sc->box, b);
#pragma unroll
    for (int u = 0; u < EWF_APT; u++) {
      const int ai = (blockIdx.x * EWF_APT + u) * EWF_T + threadIdx.x;
      act[u] = ai < S.natoms;
      at[u] = min(ai, S.natoms - 1);
      double t[3];
      atom_phase(S, b, at[u], t[0], t[1], t[2]);
      sincospi(2.0 * t[0], &s1[u], &c1[u]); sincospi(2.0 * t[1], &s2[u], &c2[u]); sincospi(2.0 * t[2], &s3[u], &c3[u]);
    }
  }
  double e1r[EWF_APT], e1i[EWF_APT];   // e1^m1
  double pr[EWF_APT], pi[EWF_APT];     // e1^m1 e2^m2 e3^m3
  double fx[EWF_APT], fy[EWF_APT], fz[EWF_APT];
#pragma unroll
  for (int u = 0; u < EWF_APT; u++) { e1r[u] = 1.0; e1i[u] = 0.0; pr[u] = 1.0; pi[u] = 0.0; fx[u] = fy[u] = fz[u] = 0.0; }
  int m1 = 0, m2 = 0, m3 = 0;    // cursor (wave-uniform)
  for (int kb = 0; kb < S.nk; kb += EWF_KC) {
    __syncthreads();
    if (threadIdx.x < EWF_KC && kb + threadIdx.x < S.nk) {
      const int k = kb + threadIdx.x;
      EwK e;
      const double ug = S.kvec[4 * k + 3];
      e.pr = ug * S.sfac[2 * k]; e.pi = ug * S.sfac[2 * k + 1];
      e.kx = S.kvec[4 * k]; e.ky = S.kvec[4 * k + 1]; e.kz = S.kvec[4 * k + 2];
      e.n1 = S.kn[3 * k];
      e.n23 = (S.kn[3 * k + 1] + 128) | ((S.kn[3 * k + 2] + 128) << 8);
      s_k[threadIdx.x] = e;
    }
    if (threadIdx.x < EWF_KC && kb + threadIdx.x < S.nk) s_run[threadIdx.x] = S.krun[kb + threadIdx.x];
    __syncthreads();
    const int kc = min(EWF_KC, S.nk - kb);
    for (int kk = 0; kk < kc;) {
      // head of a row (or of a chunk): general move of the cursor
      const EwK e = s_k[kk];
      const int n1 = __builtin_amdgcn_readfirstlane(e.n1), n23 = __builtin_amdgcn_readfirstlane(e.n23);
      const int n2 = (n23 & 0xFF) - 128, n3 = ((n23 >> 8) & 0xFF) - 128;
#pragma unroll
      for (int u = 0; u < EWF_APT; u++) {
        if (n1 != m1) {   // next slab: restart from the running power of e1 (bounds the length of the recurrences)
          for (int m = m1; m < n1; m++) cmul(e1r[u], e1i[u], c1[u], s1[u]);
          pr[u] = e1r[u]; pi[u] = e1i[u];
        }
        const int f2 = (n1 != m1) ? 0 : m2, f3 = (n1 != m1) ? 0 : m3;
        for (int m = f2; m < n2; m++) cmul(pr[u], pi[u], c2[u], s2[u]);
        for (int m = f2; m > n2; m--) cmul(pr[u], pi[u], c2[u], -s2[u]);
        for (int m = f3; m < n3; m++) cmul(pr[u], pi[u], c3[u], s3[u]);
        for (int m = f3; m > n3; m--) cmul(pr[u], pi[u], c3[u], -s3[u]);
        const double pf = pi[u] * e.pr - pr[u] * e.pi;
        fx[u] = fma(pf, e.kx, fx[u]); fy[u] = fma(pf, e.ky, fy[u]); fz[u] = fma(pf, e.kz, fz[u]);
      }
      m1 = n1; m2 = n2; m3 = n3;
      // rest of the row: n3 -> n3 +- 1 = one complex multiplication each, no scalar control; the row's direction is the
      // sign of its run length (snake order of the k list, engine/engine_kspace.cpp ewald_tables)
      const int srun = __builtin_amdgcn_readfirstlane(s_run[kk]);
      const int run = min(srun < 0 ? -srun : srun, kc - 1 - kk);   // rows are cut at chunk ends
      double s3d[EWF_APT];
#pragma unroll
      for (int u = 0; u < EWF_APT; u++) s3d[u] = (srun < 0) ? -s3[u] : s3[u];
      for (int r = 1; r <= run; r++) {
        const EwK g = s_k[kk + r];
#pragma unroll
        for (int u = 0; u < EWF_APT; u++) {
          cmul(pr[u], pi[u], c3[u], s3d[u]);
          const double pf = pi[u] * g.pr - pr[u] * g.pi;
          fx[u] = fma(pf, g.kx, fx[u]); fy[u] = fma(pf, g.ky, fy[u]); fz[u] = fma(pf, g.kz, fz[u]);
        }
      }
      m3 += (srun < 0) ? -run : run;
      kk += run + 1;
    }
  }
  double pv[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int u = 0; u < EWF_APT; u++)
    if (act[u]) {
      // f (atom order) = pair forces (slot order, k_pair) + bonded forces (rank order, k_bonded) + reciprocal part;
      // every atom is owned by exactly one thread and the kernels of a step are stream-ordered
      const int a = at[u];
      const double pq = 2.0 * MD_QQRD2E * S.q[a];
      const size_t sl = (size_t)S.slot_of[a], np = (size_t)S.npad, r = (size_t)S.bt_rank[a];
      const double px = S.fs[sl], py = S.fs[np + sl], pz = S.fs[2 * np + sl];
      // fkeep: the PPPM chain of this step (side stream, joined before this launch) has left its forces in f
      const bool keep = fkeep && S.pg[0] > 0;
      const double k0 = keep ? S.f[3 * a] : 0.0, k1 = keep ? S.f[3 * a + 1] : 0.0, k2 = keep ? S.f[3 * a + 2] : 0.0;
      S.f[3 * a] = px + S.fb[3 * r] + pq * fx[u] + k0;
      S.f[3 * a + 1] = py + S.fb[3 * r + 1] + pq * fy[u] + k1;
      S.f[3 * a + 2] = pz + S.fb[3 * r + 2] + pq * fz[u] + k2;
      if (pairvir) {
        // pair virial, part 1: wrapped slot position (x) total pair force of the slot (part 2 = k_pair's partials)
        const double *xy = (const double *)S.xq + 2 * sl, *zq = (const double *)S.xq + 2 * np + 2 * sl;
        const double x = xy[0], y = xy[1], z = zq[0];
        pv[0] += x * px; pv[1] += y * py; pv[2] += z * pz; pv[3] += x * py; pv[4] += x * pz; pv[5] += y * pz;
      }
    }
  if (pairvir) {
    const int nrows = S.ncells * MD_TILE_WAVES;   // one row of 6 per cell and wave of k_pair
    const int nblk = (S.natoms + EWF_T * EWF_APT - 1) / (EWF_T * EWF_APT);   // blocks of this simulation that got this far
    for (int r = blockIdx.x * EWF_T + threadIdx.x; r < nrows; r += nblk * EWF_T) {
      const double *vp = S.virp + (size_t)r * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) pv[k] += vp[k];
    }
    // the lumped bonded virial: one row of 6 per bonded tile (k_bonded)
    for (int r = blockIdx.x * EWF_T + threadIdx.x; r < S.bt_ntile; r += nblk * EWF_T) {
      const double *vp = S.virb + (size_t)r * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) pv[k] += vp[k];
    }
    block_atomic_add_n<6, EWF_T / 64>(pv, S.sc->vir + P_LJ * 6, s_red);
  }
}

// ------------------------------------------------------------------------------------------
// k_shake : fix shake, one thread per star cluster (central atom + 1..3 satellites)
// ------------------------------------------------------------------------------------------
// One star cluster with NB satellites (NB a compile-time constant: every array below lives in registers, every loop is
// unrolled; the generic form with run-time bounds put its arrays into scratch memory and ran at 192 VGPRs).
// shake_lambda: the multipliers of the NB constraints.  xc = positions at the start of the step (constraint directions), xs = the
// unconstrained positions after it, dist = bond lengths; r[k] = xc[0] - xc[k+1] by minimum image is returned with them.
template <int NB>
__device__ __forceinline__ void shake_lambda(const SimDev &S, const BoxD &b, const double *dist, const double (&invm)[NB + 1], const double (&xc)[NB + 1][3],
                                             const double (&xs)[NB + 1][3], double (&lam)[NB], double (&r)[NB][3]) {
  double sv[NB][3];
#pragma unroll
  for (int k = 0; k < NB; k++) {
#pragma unroll
    for (int c = 0; c < 3; c++) { r[k][c] = xc[0][c] - xc[k + 1][c]; sv[k][c] = xs[0][c] - xs[k + 1][c]; }
    minimg(b, r[k][0], r[k][1], r[k][2]);
    minimg(b, sv[k][0], sv[k][1], sv[k][2]);
  }
#pragma unroll
  for (int k = 0; k < NB; k++) lam[k] = 0.0;
  if (NB == 1) {
    const double m01 = invm[0] + invm[1];
    const double r01sq = dot3(r[0], r[0]), s01sq = dot3(sv[0], sv[0]);
    const double a = m01 * m01 * r01sq, bb = 2.0 * m01 * dot3(sv[0], r[0]), c = s01sq - dist[0] * dist[0];
    double determ = bb * bb - 4.0 * a * c;
    if (determ < 0.0) determ = 0.0;
    const double l1 = (-bb + sqrt(determ)) / (2.0 * a), l2 = (-bb - sqrt(determ)) / (2.0 * a);
    lam[0] = (fabs(l1) <= fabs(l2)) ? l1 : l2;
  } else {
    double A[NB][NB], Ai[NB][NB], M[NB][NB];
#pragma unroll
    for (int k = 0; k < NB; k++)
#pragma unroll
      for (int j = 0; j < NB; j++) {
        M[k][j] = invm[0] + (k == j ? invm[k + 1] : 0.0);
        A[k][j] = 2.0 * M[k][j] * dot3(sv[k], r[j]);
        Ai[k][j] = 0.0;
      }
    if (NB == 2) {
      const double det = A[0][0] * A[1][1] - A[0][1] * A[1][0];
      Ai[0][0] = A[1][1] / det; Ai[0][1] = -A[0][1] / det; Ai[1][0] = -A[1][0] / det; Ai[1][1] = A[0][0] / det;
    } else {
      constexpr int Z = NB > 2 ? 2 : 0;   // (keeps the indices in range for the instantiations that never take this branch)
      const double det = A[0][0] * (A[1 % NB][1 % NB] * A[Z][Z] - A[1 % NB][Z] * A[Z][1 % NB]) - A[0][1 % NB] * (A[1 % NB][0] * A[Z][Z] - A[1 % NB][Z] * A[Z][0]) +
                         A[0][Z] * (A[1 % NB][0] * A[Z][1 % NB] - A[1 % NB][1 % NB] * A[Z][0]);
      const double id = 1.0 / det;
      Ai[0][0] = id * (A[1 % NB][1 % NB] * A[Z][Z] - A[1 % NB][Z] * A[Z][1 % NB]);
      Ai[0][1 % NB] = -id * (A[0][1 % NB] * A[Z][Z] - A[0][Z] * A[Z][1 % NB]);
      Ai[0][Z] = id * (A[0][1 % NB] * A[1 % NB][Z] - A[0][Z] * A[1 % NB][1 % NB]);
      Ai[1 % NB][0] = -id * (A[1 % NB][0] * A[Z][Z] - A[1 % NB][Z] * A[Z][0]);
      Ai[1 % NB][1 % NB] = id * (A[0][0] * A[Z][Z] - A[0][Z] * A[Z][0]);
      Ai[1 % NB][Z] = -id * (A[0][0] * A[1 % NB][Z] - A[0][Z] * A[1 % NB][0]);
      Ai[Z][0] = id * (A[1 % NB][0] * A[Z][1 % NB] - A[1 % NB][1 % NB] * A[Z][0]);
      Ai[Z][1 % NB] = -id * (A[0][0] * A[Z][1 % NB] - A[0][1 % NB] * A[Z][0]);
      Ai[Z][Z] = id * (A[0][0] * A[1 % NB][1 % NB] - A[0][1 % NB] * A[1 % NB][0]);
    }
    double ssq[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) ssq[k] = dot3(sv[k], sv[k]);
    bool done = false;
    int iter = 0;
    while (!done && iter < S.shake_maxiter) {
      double rhs[NB];
#pragma unroll
      for (int k = 0; k < NB; k++) {
        double w[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < NB; j++)
#pragma unroll
          for (int c = 0; c < 3; c++) w[c] += M[k][j] * lam[j] * r[j][c];
        rhs[k] = dist[k] * dist[k] - ssq[k] - dot3(w, w);
      }
      double ln[NB];
      done = true;
#pragma unroll
      for (int k = 0; k < NB; k++) {
        ln[k] = 0.0;
#pragma unroll
        for (int j = 0; j < NB; j++) ln[k] += Ai[k][j] * rhs[j];
        if (fabs(ln[k] - lam[k]) > S.shake_tol) done = false;
      }
#pragma unroll
      for (int k = 0; k < NB; k++) lam[k] = ln[k];
#pragma unroll
      for (int k = 0; k < NB; k++)
        if (isnan(lam[k])) done = true;
      iter++;
    }
  }
}

template <int NB>
__device__ __forceinline__ void shake_cluster(const SimDev &S, const BoxD &b, int cl, double dtfsq_scale, double (&v)[6]) {
  const double dtv = S.dt, dtfsq = dtfsq_scale * S.dt * S.dt * MD_FTM2V;
  const int *at = S.clus_at + 4 * cl;
  const double *dist = S.clus_d + 3 * cl;
  int ia[NB + 1];
  double invm[NB + 1], xs[NB + 1][3], xc[NB + 1][3];
  // v is exact here: k_initial_integrate folded the deferred NH factor in before the drift
#pragma unroll
  for (int a = 0; a <= NB; a++) {
    const int i = at[a];
    ia[a] = i;
    invm[a] = 1.0 / S.mass[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      xc[a][k] = S.x[3 * i + k];
      xs[a][k] = xc[a][k] + dtv * S.v[3 * i + k] + dtfsq * invm[a] * S.f[3 * i + k];
    }
  }
  double lam[NB], r[NB][3];
  shake_lambda<NB>(S, b, dist, invm, xc, xs, lam, r);
  double f0[3] = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const double l = lam[k] / dtfsq;
    const double ff[3] = {l * r[k][0], l * r[k][1], l * r[k][2]};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      f0[c] += ff[c];
      S.f[3 * ia[k + 1] + c] -= ff[c];
    }
    vt(v, r[k][0], r[k][1], r[k][2], ff[0], ff[1], ff[2]);
  }
#pragma unroll
  for (int c = 0; c < 3; c++) S.f[3 * ia[0] + c] += f0[c];
}

__global__ __launch_bounds__(TPB, 4) void k_shake(const SimDev *sims, double dtfsq_scale) {
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  if (!S.use_shake || S.nclus == 0) return;
  if ((int)(blockIdx.x * TPB) >= S.nclus) return;
  __shared__ double s_red[6 * (TPB / 64)];
  const int cl = blockIdx.x * TPB + threadIdx.x;
  double v[6] = {0, 0, 0, 0, 0, 0};
  if (cl < S.nclus) {
    BoxD b;
    box_derive(sc.box, b);
    box_uniform(b);
    const int nb = S.clus_n[cl] - 1;
    if (nb == 2) shake_cluster<2>(S, b, cl, dtfsq_scale, v);        // CH2
    else if (nb == 1) shake_cluster<1>(S, b, cl, dtfsq_scale, v);
    else if (nb == 3) shake_cluster<3>(S, b, cl, dtfsq_scale, v);   // CH3
  }
  block_atomic_add<6>(v, sc.vir + P_SHAKE * 6, s_red);
}

// ------------------------------------------------------------------------------------------
// k_final_integrate : v += dt/2 f/m ; kinetic tensor
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_final_integrate(const SimDev *sims, int kick) {
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  __shared__ double s_red[6 * (TPB / 64)];
  const int i = blockIdx.x * TPB + threadIdx.x;
  double ke[6] = {0, 0, 0, 0, 0, 0};
  if (i < S.natoms) {
    const double m = S.mass[i];
    const double dtfm = kick ? 0.5 * S.dt * MD_FTM2V / m : 0.0;
    double v[3];
    for (int k = 0; k < 3; k++) {
      v[k] = S.v[3 * i + k];
      if (kick) { v[k] += dtfm * S.f[3 * i + k]; S.v[3 * i + k] = v[k]; }
    }
    const double mm = m * MD_MVV2E;
    ke[0] = mm * v[0] * v[0]; ke[1] = mm * v[1] * v[1]; ke[2] = mm * v[2] * v[2];
    ke[3] = mm * v[0] * v[1]; ke[4] = mm * v[0] * v[2]; ke[5] = mm * v[1] * v[2];
  }
  block_atomic_add<6>(ke, sc.ke, s_red);
}

// ------------------------------------------------------------------------------------------
// k_finish : end of the force stage of a step in ONE pass over the atoms, for the steps that need no per-atom reciprocal sum (PPPM or no
// k-space; Verlet / fix nvt): what k_ewald_force (assembly of f from the slot-ordered pair forces, the rank-ordered bonded forces
// and the PPPM forces left in f; pair virial), k_shake and k_final_integrate do in three.  One thread per SHAKE cluster, then one
// per atom outside the clusters (all atoms of a replica that runs without fix shake).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void assemble_atom(const SimDev &S, int a, bool keep, int pairvir, double (&f)[3], double (&pv)[6]) {
  const size_t sl = (size_t)S.slot_of[a], np = (size_t)S.npad, r = (size_t)S.bt_rank[a];
  const double px = S.fs[sl], py = S.fs[np + sl], pz = S.fs[2 * np + sl];
  f[0] = px + S.fb[3 * r] + (keep ? S.f[3 * a] : 0.0);
  f[1] = py + S.fb[3 * r + 1] + (keep ? S.f[3 * a + 1] : 0.0);
  f[2] = pz + S.fb[3 * r + 2] + (keep ? S.f[3 * a + 2] : 0.0);
  if (pairvir) {
    // pair virial, part 1: wrapped slot position (x) total pair force of the slot (part 2 = k_pair's partials)
    const double *xy = (const double *)S.xq + 2 * sl, *zq = (const double *)S.xq + 2 * np + 2 * sl;
    const double x = xy[0], y = xy[1], z = zq[0];
    pv[0] += x * px; pv[1] += y * py; pv[2] += z * pz; pv[3] += x * py; pv[4] += x * pz; pv[5] += y * pz;
  }
}
__device__ __forceinline__ void kick_atom(const SimDev &S, int a, double invm, const double (&f)[3], const double (&v0)[3], double (&ke)[6]) {
  const double dtfm = 0.5 * S.dt * MD_FTM2V * invm;
  double v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    v[k] = v0[k] + dtfm * f[k];
    S.v[3 * a + k] = v[k];
    S.f[3 * a + k] = f[k];
  }
  const double mm = MD_MVV2E / invm;
  ke[0] += mm * v[0] * v[0]; ke[1] += mm * v[1] * v[1]; ke[2] += mm * v[2] * v[2];
  ke[3] += mm * v[0] * v[1]; ke[4] += mm * v[0] * v[2]; ke[5] += mm * v[1] * v[2];
}
template <int NB>
__device__ __forceinline__ void finish_cluster(const SimDev &S, const BoxD &b, int cl, bool keep, int pairvir, double (&pv)[6], double (&sv)[6], double (&ke)[6]) {
  const double dtv = S.dt, dtfsq = S.dt * S.dt * MD_FTM2V;
  const int *at = S.clus_at + 4 * cl;
  const double *dist = S.clus_d + 3 * cl;
  int ia[NB + 1];
  double invm[NB + 1], xs[NB + 1][3], xc[NB + 1][3], f[NB + 1][3], v0[NB + 1][3];
#pragma unroll
  for (int a = 0; a <= NB; a++) {
    const int i = at[a];
    ia[a] = i;
    invm[a] = 1.0 / S.mass[i];
    assemble_atom(S, i, keep, pairvir, f[a], pv);
#pragma unroll
    for (int k = 0; k < 3; k++) {
      xc[a][k] = S.x[3 * i + k];
      v0[a][k] = S.v[3 * i + k];
      xs[a][k] = xc[a][k] + dtv * v0[a][k] + dtfsq * invm[a] * f[a][k];
    }
  }
  double lam[NB], r[NB][3];
  shake_lambda<NB>(S, b, dist, invm, xc, xs, lam, r);
#pragma unroll
  for (int k = 0; k < NB; k++) {
    const double l = lam[k] / dtfsq;
    const double ff[3] = {l * r[k][0], l * r[k][1], l * r[k][2]};
#pragma unroll
    for (int c = 0; c < 3; c++) { f[0][c] += ff[c]; f[k + 1][c] -= ff[c]; }
    vt(sv, r[k][0], r[k][1], r[k][2], ff[0], ff[1], ff[2]);
  }
#pragma unroll
  for (int a = 0; a <= NB; a++) kick_atom(S, ia[a], invm[a], f[a], v0[a], ke);
}
__global__ __launch_bounds__(TPB, 2) void k_finish(const SimDev *sims, int pairvir, int fkeep) {
  const SimDev &S = sims[blockIdx.y];
  SimScalars &sc = *S.sc;
  const int nunits = S.use_shake ? S.nclus + S.nfree : S.natoms;
  if ((int)(blockIdx.x * TPB) >= nunits) return;
  __shared__ double s_red[6 * (TPB / 64)];
  const int u = blockIdx.x * TPB + threadIdx.x;
  const bool keep = fkeep && S.pg[0] > 0;
  double pv[6] = {0, 0, 0, 0, 0, 0}, sv[6] = {0, 0, 0, 0, 0, 0}, ke[6] = {0, 0, 0, 0, 0, 0};
  if (u < nunits) {
    if (S.use_shake && u < S.nclus) {
      BoxD b;
      box_derive(sc.box, b);
      box_uniform(b);
      const int nb = S.clus_n[u] - 1;
      if (nb == 2) finish_cluster<2>(S, b, u, keep, pairvir, pv, sv, ke);        // CH2
      else if (nb == 1) finish_cluster<1>(S, b, u, keep, pairvir, pv, sv, ke);
      else if (nb == 3) finish_cluster<3>(S, b, u, keep, pairvir, pv, sv, ke);   // CH3
    } else {
      const int a = S.use_shake ? S.free_at[u - S.nclus] : u;
      double f[3];
      assemble_atom(S, a, keep, pairvir, f, pv);
      const double v0[3] = {S.v[3 * a], S.v[3 * a + 1], S.v[3 * a + 2]};
      kick_atom(S, a, 1.0 / S.mass[a], f, v0, ke);
    }
  }
  if (pairvir) {
    const int nblk = (nunits + TPB - 1) / TPB;   // blocks of this simulation that got this far
    const int nrows = S.ncells * MD_TILE_WAVES;  // one row of 6 per cell and wave of k_pair
    for (int r = blockIdx.x * TPB + threadIdx.x; r < nrows; r += nblk * TPB) {
      const double *vp = S.virp + (size_t)r * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) pv[k] += vp[k];
    }
    for (int r = blockIdx.x * TPB + threadIdx.x; r < S.bt_ntile; r += nblk * TPB) {   // the lumped bonded virial: one row of 6 per bonded tile
      const double *vp = S.virb + (size_t)r * 6;
#pragma unroll
      for (int k = 0; k < 6; k++) pv[k] += vp[k];
    }
    block_atomic_add<6>(pv, sc.vir + P_LJ * 6, s_red);
  }
  if (S.use_shake) block_atomic_add<6>(sv, sc.vir + P_SHAKE * 6, s_red);
  block_atomic_add<6>(ke, sc.ke, s_red);
}

// ------------------------------------------------------------------------------------------
// k_post : end of step (tiny): thermostat second half, pressure sample, fix deform box update
// ------------------------------------------------------------------------------------------
// next_pre: a simulation with steps left also does the k_pre of its next step here (one launch less per step; the first step of a run
// has its own k_pre)
__device__ __forceinline__ void post_scalars(const SimDev &S, SimScalars &sc);
// The scalars of the replica are staged through LDS: one thread walking SimScalars in global memory is a chain of dependent round trips to
// the L2 (the kernels before it wrote those lines on other CUs) -- 11 us for a lone replica, whose step is 120 us of dependent launches.  The
// wave reads the structure with coalesced loads, thread 0 works on the copy, the wave writes back the part the two functions may change
// (everything up to keep_nh; nothing else touches a replica's scalars while its k_post runs: the side stream has joined before k_finish).
__global__ void k_post(const SimDev *sims, int next_pre) {
  const SimDev &S = sims[blockIdx.x];
  __shared__ SimScalars s_sc;
  __shared__ int s_more;
  static_assert(sizeof(SimScalars) % 8 == 0 && offsetof(SimScalars, keep_nh) % 4 == 0, "SimScalars is copied in 8- and 4-byte words");
  {
    const unsigned long long *src = (const unsigned long long *)S.sc;
    unsigned long long *dst = (unsigned long long *)&s_sc;
    for (int k = threadIdx.x; k < (int)(sizeof(SimScalars) / 8); k += blockDim.x) dst[k] = src[k];
  }
  __syncthreads();
  __shared__ double s_d[8];
  if (threadIdx.x == 0) {
    post_scalars(S, s_sc);
    s_more = next_pre && s_sc.step < S.nsteps;
  }
  __syncthreads();
  if (s_more) {   // (the eight corner displacements -- a box_derive and a square root each -- on eight lanes instead of one after the other)
    if (threadIdx.x < 8) s_d[threadIdx.x] = corner_disp(s_sc, threadIdx.x);
    __syncthreads();
    if (threadIdx.x == 0) {
      double d1, d2;
      two_largest(s_d, d1, d2);
      pre_scalars(S, s_sc, d1, d2);
    }
  }
  __syncthreads();
  {
    const int *src = (const int *)&s_sc;
    int *dst = (int *)S.sc;
    for (int k = threadIdx.x; k < (int)(offsetof(SimScalars, keep_nh) / 4); k += blockDim.x) dst[k] = src[k];
  }
  if (!s_more) return;
  for (int k = threadIdx.x; k < 2 * S.nk; k += blockDim.x) S.sfac[k] = 0.0;
  for (int k = threadIdx.x; k < S.ncells; k += blockDim.x) S.cell_count[k] = 0;
}
__device__ __forceinline__ void post_scalars(const SimDev &S, SimScalars &sc) {
  sc.t_current = (sc.ke[0] + sc.ke[1] + sc.ke[2]) / (S.tdof * MD_BOLTZ);
  double f2 = 1.0;
  if (S.nvt) f2 = nhc_half(S, sc);
  sc.vscale = f2;
  for (int k = 0; k < 6; k++) sc.ke[k] *= f2 * f2;
  // fix ave/time 1 nav nav c_thermo_press[*] ave running
  if (S.nav > 0 && sc.step <= S.nwin * S.nav) {
    BoxD b;
    box_derive(sc.box, b);
    for (int k = 0; k < 6; k++) {
      double w = 0.0;
      for (int p = 0; p < MD_NPART; p++) w += sc.vir[p * 6 + k];
      sc.psum[k] += (sc.ke[k] + w) / b.vol * MD_NKTV2P;
    }
    sc.nsamples += 1;
  }
  // fix deform 1 ... erate ... : box(t) linear in t about the box centre, raw tilt targets by Ly0/Lz0, then moved by whole
  // box lengths to the value closest to the current tilt ratio (LAMMPS fix_deform end_of_step; after a flip the tilt
  // continues from the flipped value).  The flip itself is decided and enqueued by the host (engine/engine_run.cpp run_phase).
  if (S.deform) {
    for (int k = 0; k < 9; k++) sc.box_prev[k] = sc.box[k];
    const double t = sc.step * S.dt;
    double nb[9];
    for (int d = 0; d < 3; d++) {
      const double L0 = sc.box0[3 + d] - sc.box0[d];
      nb[d] = sc.box0[d] - 0.5 * L0 * S.rates[d] * t;
      nb[3 + d] = sc.box0[3 + d] + 0.5 * L0 * S.rates[d] * t;
    }
    double tilt[3] = {sc.box0[6] + S.rates[3] * (sc.box0[4] - sc.box0[1]) * t, sc.box0[7] + S.rates[4] * (sc.box0[5] - sc.box0[2]) * t,
                      sc.box0[8] + S.rates[5] * (sc.box0[5] - sc.box0[2]) * t};
    const double xprd_n = nb[3] - nb[0], yprd_n = nb[4] - nb[1];
    const double xprd = sc.box[3] - sc.box[0], yprd = sc.box[4] - sc.box[1];
    const double denom[3] = {xprd_n, xprd_n, yprd_n};
    const double current[3] = {sc.box[6] / xprd, sc.box[7] / xprd, sc.box[8] / yprd};
    for (int i = 0; i < 3; i++) {
      int guard = 0;
      while (tilt[i] / denom[i] - current[i] > 0.0 && guard++ < 64) tilt[i] -= denom[i];
      while (tilt[i] / denom[i] - current[i] < 0.0 && guard++ < 128) tilt[i] += denom[i];
      if (fabs(tilt[i] / denom[i] - 1.0 - current[i]) < fabs(tilt[i] / denom[i] - current[i])) tilt[i] -= denom[i];
    }
    for (int k = 0; k < 6; k++) sc.box[k] = nb[k];
    sc.box[6] = tilt[0]; sc.box[7] = tilt[1]; sc.box[8] = tilt[2];
  }
}

// k_flip : triclinic box flip between two steps: only the representation of the lattice changes (positions are
// unwrapped and stay); the next step rebuilds cells, wraps and lists in the new box
__global__ void k_flip(const SimDev *sim, double xy, double xz, double yz) {
  SimScalars &sc = *sim->sc;
  if (threadIdx.x == 0) {
    sc.box[6] = xy; sc.box[7] = xz; sc.box[8] = yz;
    sc.force_rebuild = 1;   // for the k_pre of the next step ...
    sc.rebuild = 1;         // ... or directly, where that k_pre has already run at the end of the last step (k_post); k_bin clears the request
  }
}

// k_remap : fix deform ... remap x : x -> lamda(old box) -> x(new box)
__global__ __launch_bounds__(TPB) void k_remap(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  if (!S.deform) return;
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  BoxD bo, bn;
  box_derive(S.sc->box_prev, bo);
  box_derive(S.sc->box, bn);
  const double d0 = S.x[3 * i] - bo.lo[0], d1 = S.x[3 * i + 1] - bo.lo[1], d2 = S.x[3 * i + 2] - bo.lo[2];
  const double l0 = bo.hinv[0] * d0 + bo.hinv[5] * d1 + bo.hinv[4] * d2;
  const double l1 = bo.hinv[1] * d1 + bo.hinv[3] * d2;
  const double l2 = bo.hinv[2] * d2;
  S.x[3 * i] = bn.h[0] * l0 + bn.h[5] * l1 + bn.h[4] * l2 + bn.lo[0];
  S.x[3 * i + 1] = bn.h[1] * l1 + bn.h[3] * l2 + bn.lo[1];
  S.x[3 * i + 2] = bn.h[2] * l2 + bn.lo[2];
}

// k_scale_v : apply the deferred thermostat factor at the end of a run
__global__ __launch_bounds__(TPB) void k_scale_v(const SimDev *sims) {
  const SimDev &S = sims[blockIdx.y];
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S.natoms) return;
  const double vs = S.sc->vscale;
  for (int k = 0; k < 3; k++) S.v[3 * i + k] *= vs;
}
__global__ void k_phase_end(const SimDev *sims) {
  if (threadIdx.x == 0) sims[blockIdx.x].sc->vscale = 1.0;
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
static inline dim3 grid2(int nx, int ns) { return dim3((unsigned)nx, (unsigned)ns, 1); }
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

void mdk_phase_init(hipStream_t st, const SimDev *d, int ns) { hipLaunchKernelGGL(k_phase_init, dim3(ns), dim3(64), 0, st, d); }
void mdk_keep_validate(hipStream_t st, const SimDev *d, int ns, int maxatoms) { hipLaunchKernelGGL(k_keep_validate, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d); }
void mdk_setup_post(hipStream_t st, const SimDev *d, int ns) { hipLaunchKernelGGL(k_setup_post, dim3(ns), dim3(64), 0, st, d); }
void mdk_pre(hipStream_t st, const SimDev *d, int ns) { hipLaunchKernelGGL(k_pre, dim3(ns), dim3(64), 0, st, d); }
void mdk_initial_integrate(hipStream_t st, const SimDev *d, int ns, int maxatoms, bool pack) {
  if (pack) hipLaunchKernelGGL(k_initial_integrate<true>, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d);
  else hipLaunchKernelGGL(k_initial_integrate<false>, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d);
}
void mdk_neighbor(hipStream_t st, const SimDev *d, int ns, int maxatoms, int maxpad, int maxcells, int maxrow, int capj, bool pack, bool together) {
  static const bool one_launch = !(scema_env("SCEMA_MD_CELL_BUILD") && atoi(scema_env("SCEMA_MD_CELL_BUILD")) == 0);
  if (one_launch && maxatoms <= CB_MAXATOMS && maxcells <= BIN_MAXCELLS) hipLaunchKernelGGL(k_cell_build, dim3(ns), dim3(CB_TPB), 0, st, d, together ? ns : 0);
  else {
    hipLaunchKernelGGL(k_bin, grid2(cdiv(maxatoms, TPB * BIN_APT), ns), dim3(TPB), 0, st, d);
    hipLaunchKernelGGL(k_cell_scan, dim3(ns), dim3(TPB), 0, st, d);
    hipLaunchKernelGGL(k_cell_fill, grid2(cdiv(maxatoms, TPB * BIN_APT), ns), dim3(TPB), 0, st, d);
  }
  if (maxatoms <= 100 * maxcells) hipLaunchKernelGGL(k_cell_sort<128>, grid2(maxcells, ns), dim3(64), 0, st, d);
  else hipLaunchKernelGGL(k_cell_sort<256>, grid2(maxcells, ns), dim3(64), 0, st, d);
  if (pack) hipLaunchKernelGGL(k_pack, grid2(cdiv(maxpad, TPB), ns), dim3(TPB), 0, st, d);   // (not behind k_initial_integrate, which has done it)
  mdk_neigh_build(st, d, ns, maxcells, maxrow, capj);
}
// reciprocal sum, part 1 (structure factors + per-k coefficients): depends only on the positions
void mdk_ewald_recip(hipStream_t st, const SimDev *d, int ns, int maxk, int mmax, int maxgrp) {
  if (maxk <= 0) return;
  const size_t lds_s = (size_t)EW_ATOMS * 3 * mmax * sizeof(double2);
  // more than 64 KB of dynamic LDS needs an explicit opt-in (large k ranges: small cut_coul or tight accuracy)
  static size_t optin_tab[16] = {0};
  size_t &optin_s = lds_optin_slot(optin_tab);
  // threads own groups of k-vectors: the block size that wastes the fewest lanes; beyond 256 groups several per thread
  const int gthreads = maxgrp <= 64 ? 64 : (maxgrp <= 128 ? 128 : 256);
  const int rounds = maxgrp <= 256 ? 1 : (maxgrp <= 512 ? 2 : 4);
  const void *fn = rounds == 1 ? (const void *)k_ewald_sfac<1> : rounds == 2 ? (const void *)k_ewald_sfac<2> : (const void *)k_ewald_sfac<4>;
  static size_t optin_tab2[16] = {0}, optin_tab4[16] = {0};
  size_t &optin_r = rounds == 1 ? optin_s : lds_optin_slot(rounds == 2 ? optin_tab2 : optin_tab4);
  if (lds_s > 64 * 1024 && lds_s > optin_r) { (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_s); optin_r = lds_s; }
  // small batches: more blocks per simulation (a single replica would otherwise run on 16 of 256 CUs); the same-address atomics
  // at the end of the kernel grow with the parts, which is why large batches stay at EW_PARTS
  const int nparts = (ns * EW_PARTS >= 256) ? EW_PARTS : std::min(64, std::max(EW_PARTS, 256 / std::max(ns, 1)));
  if (rounds == 1) hipLaunchKernelGGL(k_ewald_sfac<1>, grid2(nparts, ns), dim3(256), lds_s, st, d, mmax, gthreads, nparts);
  else if (rounds == 2) hipLaunchKernelGGL(k_ewald_sfac<2>, grid2(nparts, ns), dim3(256), lds_s, st, d, mmax, gthreads, nparts);
  else hipLaunchKernelGGL(k_ewald_sfac<4>, grid2(nparts, ns), dim3(256), lds_s, st, d, mmax, gthreads, nparts);
  hipLaunchKernelGGL(k_ewald_post, grid2(cdiv(maxk, TPB), ns), dim3(TPB), 0, st, d);
}
// part 2: per-atom reciprocal force; also assembles f from the pair and bonded forces (runs even without charges)
void mdk_ewald_force(hipStream_t st, const SimDev *d, int ns, int maxatoms, int pairvir, int fkeep) {
  if (ns * cdiv(maxatoms, EWF_TPB * EWF_APT) >= 512) hipLaunchKernelGGL(k_ewald_force<EWF_TPB>, grid2(cdiv(maxatoms, EWF_TPB * EWF_APT), ns), dim3(EWF_TPB), 0, st, d, pairvir, fkeep);
  else hipLaunchKernelGGL(k_ewald_force<64>, grid2(cdiv(maxatoms, 64 * EWF_APT), ns), dim3(64), 0, st, d, pairvir, fkeep);
}
void mdk_shake(hipStream_t st, const SimDev *d, int ns, int maxclus, double dtfsq_scale) {
  if (maxclus <= 0) return;
  hipLaunchKernelGGL(k_shake, grid2(cdiv(maxclus, TPB), ns), dim3(TPB), 0, st, d, dtfsq_scale);
}
void mdk_finish(hipStream_t st, const SimDev *d, int ns, int maxunits, int pairvir, int fkeep) {
  hipLaunchKernelGGL(k_finish, grid2(cdiv(maxunits, TPB), ns), dim3(TPB), 0, st, d, pairvir, fkeep);
}
void mdk_final_integrate(hipStream_t st, const SimDev *d, int ns, int maxatoms, int kick) {
  hipLaunchKernelGGL(k_final_integrate, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d, kick);
}
void mdk_post(hipStream_t st, const SimDev *d, int ns, int next_pre) { hipLaunchKernelGGL(k_post, dim3(ns), dim3(64), 0, st, d, next_pre); }
void mdk_flip(hipStream_t st, const SimDev *sim, double xy, double xz, double yz) { hipLaunchKernelGGL(k_flip, dim3(1), dim3(64), 0, st, sim, xy, xz, yz); }
void mdk_remap(hipStream_t st, const SimDev *d, int ns, int maxatoms) {
  hipLaunchKernelGGL(k_remap, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d);
}
// many device-to-device copies in one launch (the x / v backups of a batch: 2 x 576 separate copy calls cost 13 ms of
// launch gaps per update); block row y serves descriptor y
__global__ __launch_bounds__(256) void k_copy_many(const MdkCopy *tab) {
  const MdkCopy c = tab[blockIdx.y];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < c.n; i += (long long)gridDim.x * 256) c.dst[i] = c.src[i];
}
void mdk_copy_many(hipStream_t st, const MdkCopy *tab, int ncopies, long long maxn) {
  if (ncopies <= 0 || maxn <= 0) return;
  const int bx = (int)std::min<long long>(cdiv((int)std::min<long long>(maxn, 1 << 30), 256 * 4), 64);
  hipLaunchKernelGGL(k_copy_many, grid2(std::max(bx, 1), ncopies), dim3(256), 0, st, tab);
}

__global__ __launch_bounds__(256) void k_zero_many(const MdkZero *tab) {
  const MdkZero c = tab[blockIdx.y];
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < c.n; i += (long long)gridDim.x * 256) c.p[i] = 0;
}
void mdk_zero_many(hipStream_t st, const MdkZero *tab, int nfills, long long maxn) {
  if (nfills <= 0 || maxn <= 0) return;
  const int bx = (int)std::min<long long>(cdiv((int)std::min<long long>(maxn, 1 << 30), 256 * 4), 64);
  hipLaunchKernelGGL(k_zero_many, grid2(std::max(bx, 1), nfills), dim3(256), 0, st, tab);
}

void mdk_phase_end(hipStream_t st, const SimDev *d, int ns, int maxatoms) {
  hipLaunchKernelGGL(k_scale_v, grid2(cdiv(maxatoms, TPB), ns), dim3(TPB), 0, st, d);
  hipLaunchKernelGGL(k_phase_end, dim3(ns), dim3(64), 0, st, d);
}
