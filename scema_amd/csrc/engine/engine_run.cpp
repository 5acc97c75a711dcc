// engine_run.cpp -- one "run" of a batch with the OPLS force stage: slots, launch policy, launch sequence of the MD steps, what comes back
// (the batch skeleton it shares with the other force stages is in engine_rows.cpp)
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// -------------------------------------------------------------------------------------------
// one "run" of a batch
// -------------------------------------------------------------------------------------------
// slots: every cell is padded to a multiple of MD_CLUSTER slots (i-clusters never straddle cells)
static int padded_slots(int natoms, int ncells) { return (natoms + (MD_CLUSTER - 1) * ncells + 255) / 256 * 256; }

int ensure_slot(scema_md_engine *e, Slot &sl, int natoms, int maxneigh, int ncells, int nk, int capj) {
  const int npad = padded_slots(natoms, ncells);
  if (natoms > sl.cap_atoms || npad > sl.cap_pad) {
    HIPCHK(sl.f.ensure(3 * (size_t)natoms * 8));
    HIPCHK(sl.slot_of.ensure((size_t)natoms * 4));
    HIPCHK(sl.fs.ensure(3 * (size_t)npad * 8));
    HIPCHK(sl.fb.ensure(3 * (size_t)npad * 8));
    HIPCHK(sl.virb.ensure(((size_t)natoms / BT_OWNERS + 2) * 6 * 8));
    HIPCHK(sl.tile_order.ensure((size_t)npad * 4));
    HIPCHK(sl.wrapn.ensure(3 * (size_t)natoms * 4));
    HIPCHK(sl.xhold.ensure(3 * (size_t)natoms * 8));
    HIPCHK(sl.cell_of.ensure((size_t)natoms * 4));
    HIPCHK(sl.ckey.ensure((size_t)natoms * 4));
    HIPCHK(sl.slot_tmp.ensure((size_t)npad * 4));   // indexed by (padded) slot
    HIPCHK(sl.xbak.ensure(3 * (size_t)natoms * 8));
    HIPCHK(sl.vbak.ensure(3 * (size_t)natoms * 8));
    HIPCHK(sl.xq.ensure((size_t)npad * 32));
    HIPCHK(sl.stype.ensure((size_t)npad * 4));
    HIPCHK(sl.perm.ensure((size_t)npad * 4));
    HIPCHK(sl.numneigh.ensure((size_t)(npad / MD_CLUSTER) * MD_BAND_CNT * 2));   // 16-bit cumulative counts per cluster (md_skin_bands.h)
    HIPCHK(sl.dslot.ensure((size_t)npad * 4));
    sl.cap_atoms = natoms;
    sl.cap_pad = npad;
    sl.cap_neigh = 0;
  }
  if (maxneigh > sl.cap_neigh || sl.cap_neigh == 0) {
    // one row of maxneigh entries per cluster of MD_CLUSTER slots
    HIPCHK(sl.neigh.ensure((size_t)maxneigh * (npad / MD_CLUSTER) * 4 + 8192));
    sl.cap_neigh = maxneigh;
  }
  if (ncells + 1 > sl.cap_cells) {
    HIPCHK(sl.cell_count.ensure((size_t)(ncells + 1) * 4));
    HIPCHK(sl.cell_start.ensure((size_t)(ncells + 1) * 4));
    HIPCHK(sl.cell_fill.ensure((size_t)(ncells + 1) * 4));
    HIPCHK(sl.tile_nj.ensure((size_t)(ncells + 1) * 4));
    HIPCHK(sl.tile_wstart.ensure((size_t)(ncells + 1) * 9 * 4));
    HIPCHK(sl.virp.ensure((size_t)(ncells + 1) * MD_TILE_WAVES * 6 * 8));
    sl.cap_cells = ncells + 1;
  }
  if ((size_t)ncells * capj > sl.cap_jtab || sl.cap_jtab == 0) {
    HIPCHK(sl.tile_jtab.ensure((size_t)ncells * capj * 4 + 1024));
    sl.cap_jtab = (size_t)ncells * capj;
  }
  if (nk > sl.cap_k || sl.cap_k == 0) {
    const int kc = std::max(nk, 64);
    HIPCHK(sl.sfac.ensure((size_t)kc * 2 * 8));
    HIPCHK(sl.kvec.ensure((size_t)kc * 4 * 8));
    sl.cap_k = kc;
  }
  return SCEMA_MD_OK;
}

// -------------------------------------------------------------------------------------------
// launch policy of the OPLS run: every batch-shape decision, and the switches that force one
// -------------------------------------------------------------------------------------------
namespace {

constexpr int MAXP = 4;   // part batches at most (plan_launch)

// k_bonded on the tiles' grouped stream (md_bonded_groups.h) or on one descriptor per term: the environment, else the engine's setting
// (scema_md_bonded_grouping), else grouped at every launch size
int bonded_grouped(const scema_md_engine *e) {
  static const int env = scema_env("SCEMA_MD_BONDED_GROUPED") ? (atoi(scema_env("SCEMA_MD_BONDED_GROUPED")) != 0 ? 1 : 0) : -1;
  if (env >= 0) return env;
  return e->bonded_group_mode < 0 ? 1 : e->bonded_group_mode;
}

struct Policy {
  // by the batch size, the run and the engine's streams (plan_launch)
  int kspace_threads = 1;
  int nparts = 1;
  int launch = 0;   // replicas of the largest launch: the first part
  bool small_batch = false, nb_together = false, fuse_pack = false, keep_lists = true;
  // by the layout of the batch (plan_sides)
  bool pppm_in_lds = false, pppm_side = false, fused_tail = false, bonded_side = false, recip_side = false;
  // structure factors + per-k coefficients of a launch of na replicas on the side stream, next to the bonded kernel (force_stage)
  bool recip_side_for(int na) const { return recip_side && na >= 16; }   // small batches: the fork/join costs more than it hides
};

Policy plan_launch(const scema_md_engine *e, int ns) {
  static const int parts_env = [] { const char *s = scema_env("SCEMA_MD_PARTS"); return s ? std::min(4, std::max(2, atoi(s))) : 0; }();
  static const int small_max = scema_env("SCEMA_MD_SMALL_BATCH_MAX") ? atoi(scema_env("SCEMA_MD_SMALL_BATCH_MAX")) : -1;
  static const int together_env = scema_env("SCEMA_MD_REBUILD_TOGETHER") ? atoi(scema_env("SCEMA_MD_REBUILD_TOGETHER")) : -1;
  Policy pol;
  // The k-space set-up of every replica (engine_kspace.cpp) is a pure function of the box and by far the longest part of the layout (12 us
  // per PE-10k replica, 7 of 8 ms for 576 while the GPU waits), so large batches spread it over a few host threads.
  pol.kspace_threads = ns >= 64 ? std::max(1, std::min(8, (int)std::thread::hardware_concurrency())) : 1;
  // Part batches on streams of their own: every kernel but k_pair is latency bound and leaves most issue slots idle, while
  // k_pair saturates them and holds every wave slot of the chip; with independent parts in flight the small kernels of
  // one part fill in as the pair workgroups of another retire (the in-order streams fall out of phase by themselves).
  // How many parts is a measured table (profiles/r06_t_parts_ab.log, same-box A/B against the whole / two-half forms): under 9 replicas
  // the batch runs whole with its PPPM chain on the side stream (8 replicas: 289 whole, 285 / 281 as three / four parts);
  // 9 replicas as three parts of three (306 against 294); 10-63 replicas as four parts (with the largest cells, below:
  // +6..12 % at 10-30 replicas, +4..6 % at 36-60; three parts 1-2 % behind, two 4-7 %); from 64 on two halves (three or
  // four parts: -0.5..+0.7 %, the chip is full either way).  Four is the most: a process has four hardware queues and further streams share them.  Five to eight
  // parts were measured -- six parts of a 36-replica batch: -12 %; with GPU_MAX_HW_QUEUES=8 -29 % -- and removed.  (They
  // also showed a bug: the hipFFT plans of the PPPM path were shared by all part streams beyond the second, pppm_plan of engine_kspace.cpp.)
  // SCEMA_MD_PARTS (2-4) forces a count for batches of 2 replicas per part and more, SCEMA_MD_SPLIT=0 runs every batch whole.
  if (e->split_streams && e->stream3 != nullptr && ns >= 9) {
    pol.nparts = parts_env > 0 ? (ns >= 2 * parts_env ? parts_env : 2) : ns < 10 ? 3 : ns < 64 ? 4 : 2;
    if (e->stream2 == nullptr || e->rx_side1 == nullptr) pol.nparts = std::min(pol.nparts, 2);
    pol.nparts = std::max(1, std::min(pol.nparts, ns / 2));
  }
  pol.launch = (ns + pol.nparts - 1) / pol.nparts;
  // Cell grids: batches that fill the chip take the largest cells (per-tile phases amortised over more rows); small ones the most cells: a
  // single replica on 120 tiles leaves half of the 512 workgroup slots empty and waits for one tile.  Replicas up to which the most-cells grid is
  // taken: every launch group that runs whole (scanned again in round 6, profiles/r06_d_cells_scan.txt: 180 instead of 120 cells +5.4 % at 9
  // replicas, +2.4 % at 18; batches of 32 and more run as two half batches that fill the chip together and are fastest with the largest cells:
  // 120 against 180 cells 378 / 372 evaluations/s at 36, 422 / 417 at 72, 441 / 429 at 144).  (31: a large batch issued whole -- SCEMA_MD_SPLIT=0,
  // the chip-exclusive timing of bench.py -- keeps the grid it has as two halves; part batches fill the chip together, like the two halves of a
  // large batch: 120 against 180 cells 345 / 330 evaluations/s at 12 replicas, 370 / 361 at 18, 391 / 386 at 24, profiles/r06_t_parts_ab.log)
  pol.small_batch = small_max >= 0 ? ns <= small_max : (pol.nparts == 1 && ns <= 31);
  // The replicas of a launch (a half batch where the batch runs as two) rebuild their rows together (k_cell_build): same
  // box, own trigger / together, evaluations/s: 2 replicas 118.3 / 122.5, 4: 189.0 / 204.6, 9: 263.8 / 297.6, 18: 319.0 / 348.4, 24: 331.7 / 357.1,
  // 36: 378.3 / 405.7, 72: 425.4 / 438.2, 144: 447.8 / 450.3, 288: 458.4 / 458.6, 576: 462.8 / 463.3 (profiles/r06_g_ab.log, r06_h_ab.log).
  // A common trigger fires at the earliest of the launch's replicas: with 288 of them per launch a list lives 12.6 instead of 18.2 steps, and
  // the builds that adds (at full occupancy: +4 % list-build time) buy nothing where scattered rebuilds already find the chip full.  So: launches
  // of fewer than 128 replicas.  SCEMA_MD_REBUILD_TOGETHER = 0 / 1: every replica on its own trigger / together at every size.
  pol.nb_together = ns > 1 && (together_env < 0 ? pol.launch < 128 : together_env != 0);
  // Small batches are launch-bound (a single replica: ~20 launches of 5-35 us per step), so there k_initial_integrate also writes the
  // slot-ordered records that k_pack would (scattered 16-byte stores: for 576 replicas that costs what the separate, coalesced
  // k_pack costs -- 304 against 170 + 125 us -- so large batches keep k_pack)
  // (by the size of a LAUNCH instead -- the halves of a batch of 36 to 72 -- it loses 0.3-1 %: profiles/r06_s_fusepack_ab.log)
  pol.fuse_pack = ns <= 32;
  pol.keep_lists = keep_list_switch();
  return pol;
}

// what the launches of a batch need to know of all its replicas: the largest of each size
struct Layout {
  int maxbt = 1, maxloc = 1, maxcoef = 0, maxrow = 64, maxcapj = 64, maxpoly = 1, maxatoms = 0, maxpad = 0, maxcells = 0, maxk = 0, mmax = 1,
      maxgrp = 0, maxclus = 0, maxunits = 0, maxsteps = 0;
  int maxgrid = 0, maxgridp = 0, maxdims = 0;   // PPPM: largest grid of the batch, ... with five more points per x row, largest nx + ny + nz
  long long sum_charged = 0, sum_grid = 0;      // PPPM replicas: charged atoms and mesh points (binned charge assignment: atoms per point)
  bool padx_ok = true;                          // (the padded LDS copies of the spreading and interpolation kernels fold five distinct pad columns per row)
  PppmLaunch tl;                                // tiled PPPM kernels: budget, mode and the largest tile counts and LDS sizes of the batch (md_pppm_tile.h)
  bool tl_sp_fits = true, tl_fo_fits = true;    // no mesh of the batch whose smallest brick is beyond the budget
  bool any_validate = false;   // some simulation may keep the rows its slot holds (SimDev::keep_list: 1 from the run, 2 from the update before)
};

void plan_sides(Policy &pol, const scema_md_engine *e, int ns, const RunSpec &spec, const Layout &L) {
  static const int fused_tail_env = scema_env("SCEMA_MD_FUSED_TAIL") ? atoi(scema_env("SCEMA_MD_FUSED_TAIL")) : -1;
  static const bool bonded_side_on = !(scema_env("SCEMA_MD_BONDED_SIDE") && atoi(scema_env("SCEMA_MD_BONDED_SIDE")) == 0);
  // small PPPM grids: the whole solve in one launch, in LDS (md_pppm.hip k_pppm_solve); SCEMA_MD_PPPM_FFT: batched hipFFT for every grid
  pol.pppm_in_lds = L.maxgrid > 0 && L.maxgrid <= mdk_pppm_solve_max() && (3 * (size_t)L.maxgrid + (size_t)L.maxdims) * 16 <= 150 * 1024 &&
                    !scema_env("SCEMA_MD_PPPM_FFT");
  // With one launch group and the side stream, the whole PPPM chain of a step (it needs the positions only) runs next to
  // k_pair and the bonded kernel: its forces are stored in SimDev::f, and k_ewald_force, which assembles the force of the
  // step, adds them after the join.  Otherwise the chain follows the assembly and adds to it.  PE-10k, evaluations per second
  // with the chain on the side stream / inline: 8 replicas 210 / 183, 72: 336 / 333, 576: 369 / 368; a single replica 39.7 / 41.6
  // (round 2: its k_pair does not fill the chip and the fork/join is pure latency -- with round 5's kernels, where the chain is 67 us of
  // dependent launches beside 45 us of k_pair + k_bonded, 16.7 against 18.3 ms per evaluation).  So: batches of up to 255 replicas; a
  // batch that fills the chip many times over gains nothing, and inline its k_pair launches are timed and profiled undisturbed.
  pol.pppm_side = L.maxgrid > 0 && pol.nparts == 1 && e->stream2 != nullptr && ns < 256;
  // Likewise the tail of the force stage of steps without a per-atom reciprocal sum (PPPM or no k-space; Verlet / fix nvt, production
  // virial): one pass (k_finish) instead of k_ewald_force + k_shake + k_final_integrate -- two launches less for a small batch
  // (a single replica: 14.2 against 17.4 us); a thread per SHAKE cluster gathers less well than the three kernels stream, so large
  // batches keep them (576 replicas: 452 against 426 us).  SCEMA_MD_FUSED_TAIL = 0 / 1 forces either.
  // (by the size of a launch: a batch of 36 as two halves +0.9 %, of 72 +-0, of 144 -0.3 %, profiles/r06_i_ab.log)
  pol.fused_tail = (fused_tail_env < 0 ? pol.launch <= 32 : fused_tail_env != 0) && !spec.nh && L.maxk == 0 && !spec.ev_always;
  // The bonded kernel behind the PPPM chain on the side stream on steps whose chain is short (no new influence function), for batches of 8
  // replicas and more, where the pair kernel is the longer of the step's two chains of dependent launches: +4 % at 9 replicas, +2 % at 18;
  // below 8 the PPPM chain is the longer one and the move costs 4-8 % (profiles/r06_d_ab.log).  SCEMA_MD_BONDED_SIDE = 0: off.
  // (k_post's work inside k_finish -- the replica's last workgroup, found by a ticket, does the end of the step -- was built and measured in
  // the same series: nothing at 1-4 replicas, where k_finish, k_post, k_remap and k_initial_integrate already run back to back without a gap,
  // and -2.5 / -3.6 % at 9 / 18 replicas, where the device-scope release and acquire around the ticket write back and invalidate the XCD's L2
  // with the replica's freshly stored velocities and forces in it.  Removed.)
  // (The bonded tiles of such a batch as extra workgroups of the k_pair launch -- on the CUs its 180 pair tiles leave idle -- take the kernel and
  // its launch gap off the main stream, 89 -> 72 us per step, and leave the PPPM chain beside it, fork 11 + 54 + join 11 us, the longer one:
  // 76.6 against 76.2 evaluations/s for one replica, 208 / 204 for four, 257 / 259 for seven.  profiles/r06_w_bonded_in_pair_ab.log.  Removed.)
  // (The bonded kernel of a batch under 8 replicas on a THIRD stream, beside both k_pair and the PPPM chain -- on paper 17 us off a lone replica's
  // 127 us step -- lost: 66.5 against 77.1 evaluations/s for one replica, 188.7 / 201.2 for four, 290.2 / 294.2 for nine.  A second fork and join
  // per step costs more than the 11 us kernel it hides.  profiles/r06_v_bonded_third_ab.log.  Removed.)
  pol.bonded_side = bonded_side_on && pol.pppm_side && pol.fused_tail && ns >= 8 && !(spec.deform || (spec.nh && spec.npt));
  // After k_pair: bonded terms on the main stream, structure factors + per-k coefficients on the side stream (both are small,
  // latency-bound kernels that need only the positions), joined before the per-atom reciprocal force
  pol.recip_side = pol.nparts == 1 && L.maxk > 0 && e->stream2 != nullptr;
}

// -------------------------------------------------------------------------------------------
// the stages of an OPLS run
// -------------------------------------------------------------------------------------------
using Clock = std::chrono::steady_clock;
double ms_between(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

struct OplsRun {
  scema_md_engine *e;
  std::vector<ActiveSim> &sims;
  const RunSpec &spec;
  const scema_md_params &P;
  const int ns;
  const double cutmax_all;
  const bool cle;   // cut_coul <= cut_lj
  const int ev;     // the pair kernel sums the virial (the barostat needs it on every step)
  Policy pol;
  std::vector<int> order;
  std::vector<Part> parts;
  std::vector<EwaldSetup> ews;                 // by position
  std::vector<std::vector<FlipEvent>> flips;   // by position: the box flips of this run (fix deform, flip yes)
  std::vector<size_t> koff;                    // by position: offset of the k-vector tables in e->h_kpack
  Layout L;
  std::vector<std::pair<int, int>> pppm_runs;  // (first position, count) of neighbours in the launch order that share a grid; none crosses a part
  bool pppm_clean[MAXP] = {};                  // per part: the charge grids hold zeros (the buffer is laid out anew for every run)
  const SimDev *D = nullptr;
  size_t ev_used = 0;
  std::vector<std::pair<int, int>> launch_sims;   // per timed pair launch: (first position, simulations)
  std::vector<std::unique_ptr<DevBuf>> flip_bufs;   // k-vector tables in the new reciprocal basis, alive until the run has drained
  std::vector<std::unique_ptr<std::vector<int>>> flip_host;
  std::vector<std::unique_ptr<SimDev>> flip_desc;
  // host time (SCEMA_MD_TIMING): the layout before the first launch, of which the k-space set-up, and per replica box range, cell grid, the rest
  double t_layout = 0, t_kspace = 0, t_box = 0, t_grid = 0, t_rest = 0;

  OplsRun(scema_md_engine *e_, std::vector<ActiveSim> &sims_, const RunSpec &spec_)
      : e(e_), sims(sims_), spec(spec_), P(e_->p), ns((int)sims_.size()), cutmax_all(std::max(P.cut_lj, P.cut_coul)), cle(P.cut_coul <= P.cut_lj),
        ev((spec_.sample || spec_.ev_always || (spec_.nh && spec_.npt)) ? 1 : 0), pol(plan_launch(e_, (int)sims_.size())), flips(sims_.size()),
        koff(sims_.size(), 0) {
    L.tl.budget = e->pppm_lds_bytes > 0 ? e->pppm_lds_bytes : (int)mdk_pppm_lds_limit();
    L.tl.mode = e->pppm_tile_mode;
  }

  void kspace_setup();
  int make_parts();
  int lay_out_sim(int pos);
  int lay_out_kspace();
  int pppm_stage(hipStream_t st, int pos0, int na, bool new_box, int add = 1);
  int pppm_fork(hipStream_t st, int pos0, int na, bool new_box, bool with_bonded = false);
  hipError_t force_stage(hipStream_t st, const SimDev *Dh, int na, bool side, int bparts, int pairvir, bool pppm_ahead);
  int setup_step();
  int minimise();
  int launch_step(const Part &pt, int na, bool timed);
  int apply_flip(int pos, const FlipEvent &fe);
  int run_steps();
  int finish();
};

// k-space set-up of every simulation first (by simulation index, before the launch order exists): g_ewald with the k list of the Ewald
// sum, or with the PPPM grid; ews by position once the order exists
void OplsRun::kspace_setup() {
  std::vector<EwaldSetup> ews_i(ns);
  auto kspace_one = [&](int i) {
    const Topo &T = *sims[i].st->topo;
    const SimScalars &hsc = e->h_sc[i];
    EwaldSetup &ew = ews_i[i];
    const bool kept = spec.ew_keep && spec.keep;
    const bool pppm = P.kspace_style == 1 && T.qsqsum > 0.0 && !kept;
    if (kept && (int)spec.ew_keep->size() == ns) ew = (*spec.ew_keep)[i];   // a run keeps the k-space setup of its start
    else ewald_setup(P, T, hsc.box, ew, pppm);
    if (pppm) {
      // PPPM: the Ewald k list is not used; g_ewald is adjusted to the grid (and with it the real-space part)
      int pgd[3];
      double gp = ew.g;
      pppm_setup_host(P, T, hsc.box, gp, pgd);
      ew = EwaldSetup();
      ew.g = gp;
      for (int d = 0; d < 3; d++) ew.kmaxd[d] = -pgd[d];   // the grid travels in the set-up record (negative: not a k range)
    }
  };
  const int nthr = pol.kspace_threads;
  if (nthr == 1) {
    for (int i = 0; i < ns; i++) kspace_one(i);
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < nthr; t++)
      pool.emplace_back([&, t] { for (int i = t; i < ns; i += nthr) kspace_one(i); });
    for (auto &th : pool) th.join();
  }
  if (spec.ew_keep && !spec.keep) *spec.ew_keep = ews_i;
  // order: among equally long runs the simulations that share a PPPM grid stand together (one batched transform per such group; a strained
  // batch can straddle a grid size)
  order = batch_order(sims, pol.nparts, [&](int i) {
    const int *k = ews_i[i].kmaxd;
    return k[0] < 0 ? ((long)(-k[0]) << 40) | ((long)(-k[1]) << 20) | (long)(-k[2]) : 0L;
  });
  ews.resize(ns);
  for (int pos = 0; pos < ns; pos++) ews[pos] = std::move(ews_i[order[pos]]);
}

int OplsRun::make_parts() {
  while ((int)e->md_part_done.size() < pol.nparts - 1) {
    hipEvent_t pe = nullptr;
    HIPCHK(hipEventCreateWithFlags(&pe, hipEventDisableTiming));
    e->md_part_done.push_back(pe);
  }
  const hipStream_t streams[MAXP] = {e->stream, e->stream3, e->stream2, e->rx_side1};
  parts = split_parts(ns, pol.nparts);
  for (int h = 0; h < pol.nparts; h++) parts[h].st = streams[h];
  e->h_sims.assign(ns, SimDev());
  e->h_kpack.clear();
  return SCEMA_MD_OK;
}

// Cell grid = tiling of k_pair (one workgroup per cell): the number of cells per dimension nc, the stencil reach mst and the capacities of
// the tables.  False if the estimated j table does not fit the LDS of the pair kernel.
static bool size_grid(const scema_md_engine *e, int natoms, const BoxRange &R, double rlist, const int nc[3], int mst[3], int &cj_out, int &mn_out) {
  int ncells = 1;
  for (int d = 0; d < 3; d++) {
    mst[d] = (int)std::ceil(rlist / (R.w[d] / nc[d]) - 1e-12);
    ncells *= nc[d];
  }
  // Cartesian extents of one cell (bounding box of its edge vectors), the largest over the run's boxes
  double ext[3] = {0, 0, 0};
  for (const HostBox &hb : R.boxes) {
    ext[0] = std::max(ext[0], std::fabs(hb.h[0]) / nc[0] + std::fabs(hb.h[5]) / nc[1] + std::fabs(hb.h[4]) / nc[2]);
    ext[1] = std::max(ext[1], std::fabs(hb.h[1]) / nc[1] + std::fabs(hb.h[3]) / nc[2]);
    ext[2] = std::max(ext[2], std::fabs(hb.h[2]) / nc[2]);
  }
  const double r = rlist;
  // volume of (cell (+) ball of rlist); the table holds the half stencil: half of it plus half of the own cell.
  // Calibrated on PE-10k grids from 6x6x5 to 4x5x4: estimate = 1.15-1.17 x the largest table seen.
  const double vmink = ext[0] * ext[1] * ext[2] + 2.0 * r * (ext[0] * ext[1] + ext[1] * ext[2] + ext[0] * ext[2]) +
                       MD_PI * r * r * (ext[0] + ext[1] + ext[2]) + 4.0 / 3.0 * MD_PI * r * r * r;
  const double rho_slots = (natoms + 1.5 * ncells) / R.vol_min;
  const double cellvol = R.vol_max / ncells;
  double cj = rho_slots * (0.5 * vmink + 0.5 * cellvol) * 1.13 * e->jtab_grow;
  cj = std::min(cj, (double)padded_slots(natoms, ncells) * 14.0);
  cj_out = std::max(64, ((int)std::ceil(cj) + 63) / 64 * 64);
  // row capacity of one i-cluster: the union of 4 half neighbour spheres whose centres are within a cell, plus
  // headroom; regrown on overflow
  const double rho = natoms / R.vol_min;
  mn_out = (int)std::ceil(rho * 4.0 / 3.0 * MD_PI * rlist * rlist * rlist * 1.25 * e->neigh_grow) + 128;
  mn_out = (std::min(mn_out, cj_out) + 63) / 64 * 64 + 64;   // (+ 64: the last 64 words of a row's capacity are k_neigh_build's dump zone, md_pair.hip)
  return cj_out <= MD_MAXJTAB && mdk_pair_lds_bytes(cj_out) <= 74 * 1024 && mdk_neigh_lds_bytes(cj_out, mn_out) <= 150 * 1024;
}

// The cell grid of a replica (S.nc, S.mst) and its capacities.  The per-tile phases of k_pair (table load, barrier, flush) are amortised
// over the tile's rows, so cells are made as LARGE as the LDS allows: of all grids with cell edges between rlist/2 and rlist, the one with
// the largest cells whose estimated j table (the images of the half stencil within rlist of the cell, 28 B of LDS each) still fits two
// workgroups per CU (small batches: the one with the most cells, plan_launch).  PE-10k: 5x6x4 cells of 8.9 x 7.4 x 10.1 A (22 clusters,
// 2 280 table entries) instead of 6x6x5 (14 clusters, 2 040): k_pair -3.5 %, build +8 %, step -2.4 %.  If no such grid fits, among edges
// down to rlist/4 (so that a slightly denser system degrades gradually), then uniform cells of rlist/5 ... rlist/8.
// `prev`: the grid of the run before on the same slot, kept (`keep`) where it is a valid one for this run's boxes -- and with it the
// neighbour rows on the device.  False if no grid fits; capj then holds the last table tried.
static bool choose_grid(const scema_md_engine *e, int natoms, const BoxRange &R, double rlist, bool small_batch, const ListSig *prev, SimDev &S,
                        int &capj, int &maxneigh, bool &keep) {
  keep = false;
  if (prev) {
    int mst[3], cj = 0, mn = 0;
    if (size_grid(e, natoms, R, rlist, prev->nc, mst, cj, mn) && cj <= prev->capj && mn <= prev->maxneigh &&
        padded_slots(natoms, prev->nc[0] * prev->nc[1] * prev->nc[2]) == prev->npad) {
      keep = true;
      capj = prev->capj; maxneigh = prev->maxneigh;
      for (int d = 0; d < 3; d++) { S.nc[d] = prev->nc[d]; S.mst[d] = mst[d]; }
      return true;
    }
  }
  bool fits = false;
  for (int pass = 0; pass < 2 && !fits; pass++) {
    int lo[3], hi[3];
    for (int d = 0; d < 3; d++) {
      lo[d] = std::max(2, std::min(64, (int)std::floor(R.w[d] / (rlist * 1.0001))));
      hi[d] = std::max(lo[d], std::min(64, (int)std::floor(R.w[d] / ((pass == 0 ? 0.5 : 0.25) * rlist * 1.0001))));
    }
    double best = -1.0e300;
    for (int n0 = lo[0]; n0 <= hi[0]; n0++)
      for (int n1 = lo[1]; n1 <= hi[1]; n1++)
        for (int n2 = lo[2]; n2 <= hi[2]; n2++) {
          const int nc[3] = {n0, n1, n2};
          int mst[3], cj, mn;
          if (!size_grid(e, natoms, R, rlist, nc, mst, cj, mn)) continue;
          const double score = small_batch ? (double)n0 * n1 * n2 : 1.0 / ((double)n0 * n1 * n2);
          if (score > best) {
            best = score;
            fits = true;
            capj = cj; maxneigh = mn;
            for (int d = 0; d < 3; d++) { S.nc[d] = nc[d]; S.mst[d] = mst[d]; }
          }
        }
  }
  for (int k = 5; k <= 8 && !fits; k++) {
    int nc[3], mst[3];
    for (int d = 0; d < 3; d++) nc[d] = std::max(1, std::min((int)std::floor(R.w[d] / (rlist / k * 1.0001)), 64));
    fits = size_grid(e, natoms, R, rlist, nc, mst, capj, maxneigh);
    for (int d = 0; d < 3; d++) { S.nc[d] = nc[d]; S.mst[d] = mst[d]; }
  }
  return fits;
}

// The replica at position pos of the launch order: its box range, list radius, cell grid, the capacities of its slot, its SimDev, and what
// it adds to the batch's maxima.  NOTE: slot index == position in `sims` (not in `order`): scalars stay attached to their slot.
int OplsRun::lay_out_sim(int pos) {
  const int i = order[pos];
  ActiveSim &A = sims[i];
  Topo &T = *A.st->topo;
  const SimScalars &hsc = e->h_sc[i];
  const auto tl0 = Clock::now();
  // box range over this run -> cell grid that stays valid while the box deforms and flips
  BoxRange R;
  if (!box_range(spec, A, hsc.box, R, flips[pos]))
    return fail(e, SCEMA_MD_ERR_BOX, "fix deform is changing yz too much with xy: the strain would tilt yz past half the box (a yz flip changes xz by xy, "
                "which LAMMPS refuses while xy is deformed too, as in.strain.lammps always does)");
  SimDev S;
  std::memset(&S, 0, sizeof S);
  // list skin of this simulation = the reference's neighbour skin + the state's performance extra (dropped where the
  // box is too small for it)
  if (!e->skin_adapt) A.st->skin_extra = e->skin_extra_fixed;
  for (int d = 0; d < 3; d++)
    if (R.w[d] < 2.0 * (cutmax_all + P.skin + A.st->skin_extra)) A.st->skin_extra = 0.0;
  const double skin_i = P.skin + A.st->skin_extra;
  const double rlist = cutmax_all + skin_i;
  for (int d = 0; d < 3; d++)
    if (R.w[d] < 2.0 * rlist) return fail(e, SCEMA_MD_ERR_BOX, "box width %.3f < 2*(cutoff+skin) = %.3f in dim %d", R.w[d], 2 * rlist, d);
  const auto tl1 = Clock::now();
  // A run that follows another one on the same slot (the sampling run of an evaluation behind its straining run) keeps that run's
  // cell grid where it is a valid one for the new box, and with it the neighbour rows on the device: one list build in seven of an
  // evaluation less.  (Capacities are strides of the stored tables: they stay what they were.)
  Slot &sl = *e->slots[i];
  const ListSig &g = sl.sig;
  const bool may_keep = spec.keep_list && pol.keep_lists && g.valid && g.kind == RowKind::Opls && g.topo == T.id && g.rlist == rlist && g.cut_lj == P.cut_lj &&
                        g.cut_coul == P.cut_coul && (spec.keep_list == 1 || g.state == A.st->id) && !hsc.force_rebuild && !hsc.overflow;
  int capj = 0, maxneigh = 0;
  bool keep = false;
  if (!choose_grid(e, T.natoms, R, rlist, pol.small_batch, may_keep ? &g : nullptr, S, capj, maxneigh, keep))
    return fail(e, SCEMA_MD_ERR_ARG, "the j table of a cell tile (%d entries) does not fit the LDS of the pair kernel (system too dense for the cutoff)", capj);
  S.keep_list = keep ? spec.keep_list : 0;
  L.any_validate = L.any_validate || S.keep_list != 0;
  S.ncells = S.nc[0] * S.nc[1] * S.nc[2];
  const auto tl2 = Clock::now();
  const EwaldSetup &ew = ews[pos];
  if (P.kspace_style == 1 && T.qsqsum > 0.0) {
    for (int d = 0; d < 3; d++) S.pg[d] = -ew.kmaxd[d];
    L.maxgrid = std::max(L.maxgrid, S.pg[0] * S.pg[1] * S.pg[2]);
    if (S.pg[0] < 5) L.padx_ok = false;
    L.sum_charged += T.ncharged; L.sum_grid += (long long)S.pg[0] * S.pg[1] * S.pg[2];
    L.maxgridp = std::max(L.maxgridp, (S.pg[0] + 5) * S.pg[1] * S.pg[2]);
    L.tl.fs_lds = std::max(L.tl.fs_lds, (size_t)pppm_fstride(S.pg[0], S.pg[1], S.pg[2], L.tl.budget).bytes);   // (the staged interpolation's padded copy)
    for (int which = 0; which < 2; which++) {
      const PppmTile t = pppm_tile_shape(S.pg[0], S.pg[1], S.pg[2], L.tl.budget, which);
      bool &fits = which ? L.tl_fo_fits : L.tl_sp_fits;
      if (t.ty == 0) { fits = false; continue; }
      int &my = which ? L.tl.fo_ty : L.tl.sp_ty, &mz = which ? L.tl.fo_tz : L.tl.sp_tz, &mt = which ? L.tl.fo_tiles : L.tl.sp_tiles;
      size_t &ml = which ? L.tl.fo_lds : L.tl.sp_lds;
      my = std::max(my, t.ty); mz = std::max(mz, t.tz); mt = std::max(mt, t.ty * t.tz);
      ml = std::max(ml, (size_t)pppm_tile_bytes(S.pg[0], S.pg[1], S.pg[2], t.by, t.bz, which));
    }
  }
  S.nk = (int)ew.kn.size() / 3;
  for (int d = 0; d < 3; d++) S.kmaxd[d] = std::max(ew.kmaxd[d], 0);
  S.g_ewald = ew.g;
  {
    // H depends on u only: fit once per (rounded-up) range and share it between simulations
    const double perr = cached_coul_poly(e, ew.g, P.cut_coul, S.coul_poly, &S.coul_npoly, &S.coul_uscale);
    if (perr > 1e-12 && !scema_env("SCEMA_MD_POLY_TOL")) return fail(e, SCEMA_MD_ERR_ARG, "real-space Ewald polynomial fit error %.3e too large (g*rc = %.3f)", perr, ew.g * P.cut_coul);
    for (int m = 0; m < MD_MAXPOLY; m++) S.coul_poly_g[m] = S.coul_poly[m] * ew.g;
  }
  {
    const double m = 0.1 * P.skin;   // margin of the row segments over the cutoffs (scan 0 .. 0.6 skin: flat optimum at 0.05-0.15)
    S.seg_a2 = (P.cut_coul + m) * (P.cut_coul + m);
    S.seg_b2 = (P.cut_lj + m) * (P.cut_lj + m);
    // the skin pairs -- listed beyond cutmax + m -- sit at the back of the rows in MD_SKIN_BANDS bands of equal width by build-time distance; a row is
    // walked into band b only once its cluster's and the replica's displacement bounds and the corner motion add up to w[b] (md_skin_bands.h)
    const double cmax = std::max(P.cut_coul, P.cut_lj);
    for (int b = 0; b < MD_SKIN_BANDS; b++) {
      const double w = m + b * (skin_i - m) / MD_SKIN_BANDS;
      S.band_e2[b] = (cmax + w) * (cmax + w);
      S.band_w[b] = skin_down(w);
    }
    S.dquant = (float)(skin_i / MD_DLEVELS);
    S.dquant_inv = (float)(MD_DLEVELS / skin_i);
    S.skin_bands = skin_bands_switch() ? 1 : 0;
  }
  S.natoms = T.natoms;
  S.npad = padded_slots(T.natoms, S.ncells);
  S.ntypes = T.ntypes;
  int rc = ensure_slot(e, sl, T.natoms, maxneigh, S.ncells, S.nk, capj);
  if (rc) return rc;
  S.maxneigh = maxneigh;
  S.capj = capj;
  {
    ListSig &gs = sl.sig;   // what this run's rows are built for; valid once the run has ended without a fault
    gs.valid = false;
    gs.kind = RowKind::Opls;
    gs.topo = T.id;
    for (int d = 0; d < 3; d++) gs.nc[d] = S.nc[d];
    gs.capj = capj; gs.maxneigh = maxneigh; gs.npad = S.npad;
    gs.rlist = rlist; gs.cut_lj = P.cut_lj; gs.cut_coul = P.cut_coul;
  }
  sim_common(S, P, spec, A, sl, e->d_sc.as<SimScalars>() + i);
  S.nbonds = T.nbonds; S.nbonds_noshake = T.nbonds_noshake; S.nangles = T.nangles; S.ndihedrals = T.ndihedrals;
  S.nimpropers = T.nimpropers; S.nspecial = T.nspecial; S.nclus = T.nclus;
  S.use_shake = (spec.use_shake && T.nclus > 0) ? 1 : 0;
  S.neigh_delay = P.neigh_delay;
  S.shake_maxiter = P.shake_maxiter;
  S.tdof = 3.0 * T.natoms - 3.0 - (S.use_shake ? T.ncons : 0);
  S.qsqsum = T.qsqsum; S.qsum = T.qsum;
  S.cut_lj2 = P.cut_lj * P.cut_lj; S.cut_coul2 = P.cut_coul * P.cut_coul; S.rlist2 = rlist * rlist;
  S.skin = skin_i;
  S.rlist_ref2 = (cutmax_all + P.skin) * (cutmax_all + P.skin);   // the reference's list, for the roofline accounting
  S.excl_cut2 = std::min(T.excl_cut * T.excl_cut, S.rlist2);
  S.shake_tol = P.shake_tol;
  S.lj = T.d_lj.as<double>();
  S.bt_terms = T.d_bt_terms.as<unsigned long long>(); S.bt_coef = T.d_bt_coef.as<double>(); S.bt_ncoef = T.bt_ncoef;
  for (int k = 0; k < 4; k++) S.bt_cf_off[k] = T.bt_cf_off[k];
  for (int k = 0; k < 6; k++) S.sp_w[k] = T.sp_w[k];
  S.ex_start = T.d_ex_start.as<int>(); S.ex_list = T.d_ex_list.as<int>();
  S.bt_desc = T.d_bt_desc.as<int>(); S.bt_atoms = T.d_bt_atoms.as<int>(); S.bt_rank = T.d_bt_rank.as<int>(); S.bt_ntile = T.bt_ntile;
  S.clus_at = T.d_clus_at.as<int>(); S.clus_n = T.d_clus_n.as<int>(); S.clus_d = T.d_clus_d.as<double>();
  S.free_at = T.d_free_at.as<int>(); S.nfree = T.nfree;
  S.xq = sl.xq.as<double4>(); S.stype = sl.stype.as<int>(); S.perm = sl.perm.as<int>(); S.slot_tmp = sl.slot_tmp.as<int>();
  S.cell_of = sl.cell_of.as<int>(); S.ckey = sl.ckey.as<int>(); S.cell_start = sl.cell_start.as<int>();
  S.cell_fill = sl.cell_fill.as<int>(); S.numneigh = sl.numneigh.as<int>(); S.neigh = sl.neigh.as<int>(); S.dslot = sl.dslot.as<float>();
  S.fs = sl.fs.as<double>(); S.fb = sl.fb.as<double>(); S.slot_of = sl.slot_of.as<int>(); S.tile_nj = sl.tile_nj.as<int>(); S.tile_jtab = sl.tile_jtab.as<int>(); S.tile_order = sl.tile_order.as<int>(); S.tile_wstart = sl.tile_wstart.as<int>(); S.virp = sl.virp.as<double>(); S.virb = sl.virb.as<double>();
  S.kvec = sl.kvec.as<double>();
  if (S.nk > 0) {
    // layout per simulation: kn[3 nk] | krun[nk] | pad to 4 ints | kgrp[8 ngrp]
    std::vector<int> &kpack = e->h_kpack;
    koff[pos] = kpack.size();
    kpack.insert(kpack.end(), ew.kn.begin(), ew.kn.end());
    kpack.insert(kpack.end(), ew.krun.begin(), ew.krun.end());
    while (kpack.size() % 4) kpack.push_back(0);
    kpack.insert(kpack.end(), ew.kgrp.begin(), ew.kgrp.end());
    S.ngrp = (int)ew.kgrp.size() / 8;
    L.maxgrp = std::max(L.maxgrp, S.ngrp);
  }
  e->h_sims[pos] = S;
  t_box += ms_between(tl0, tl1); t_grid += ms_between(tl1, tl2); t_rest += ms_between(tl2, Clock::now());
  L.maxrow = std::max(L.maxrow, maxneigh); L.maxcapj = std::max(L.maxcapj, capj);
  L.maxbt = std::max(L.maxbt, T.bt_ntile); L.maxloc = std::max(L.maxloc, T.bt_maxloc); L.maxcoef = std::max(L.maxcoef, T.bt_ncoef);
  L.maxatoms = std::max(L.maxatoms, S.natoms); L.maxpad = std::max(L.maxpad, S.npad); L.maxcells = std::max(L.maxcells, S.ncells);
  L.maxk = std::max(L.maxk, S.nk);
  L.maxpoly = std::max(L.maxpoly, S.coul_npoly);
  for (int d = 0; d < 3; d++) L.mmax = std::max(L.mmax, S.kmaxd[d] + 1);
  L.maxclus = std::max(L.maxclus, S.use_shake ? S.nclus : 0);
  L.maxunits = std::max(L.maxunits, S.use_shake ? S.nclus + S.nfree : S.natoms);
  L.maxsteps = std::max(L.maxsteps, A.nsteps);
  return SCEMA_MD_OK;
}

// The k-vector tables of all simulations (indices, row run lengths, groups) in one upload; PPPM: four complex grids and the influence
// function per simulation.  The charge grids of the batch are contiguous, and so are the field grids (three per simulation, simulation-
// major): one batched transform forward and ONE back for a launch group whose simulations share the grid, which they do for one material.
int OplsRun::lay_out_kspace() {
  // (Round 6 measured three ways of giving a launch that does not fill the chip more, shorter workgroups of k_pair -- every tile as 2 / 4 / 8
  // workgroups with a part of every row each; only the last replicas of a launch split that way; and the list kernels on a stream of their own
  // beside a first pair launch for the replicas whose rows stand -- and all three LOST at every batch size from 1 to 144 replicas: DESIGN.md 5.4,
  // profiles/r06_a_pair_parts_ab.log, r06_k_pair_tail_ab.log, r06_b_ab.log.  They were removed again; commit 992bf45 holds the code.)
  if ((size_t)64 * 3 * L.mmax * 16 + 4096 > 160 * 1024)
    return fail(e, SCEMA_MD_ERR_ARG, "k-space index range (|n| up to %d) too large for the LDS phase tables; raise cut_coul or loosen kspace_accuracy", L.mmax - 1);
  const std::vector<int> &kpack = e->h_kpack;
  HIPCHK(e->d_kpack.ensure(kpack.size() * sizeof(int) + 64));
  if (!kpack.empty()) HIPCHK(hipMemcpyAsync(e->d_kpack.p, kpack.data(), kpack.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  for (int pos = 0; pos < ns; pos++) {
    SimDev &S = e->h_sims[pos];
    if (S.nk <= 0) continue;
    const int *base = e->d_kpack.as<int>() + koff[pos];
    S.kn = base;
    S.krun = base + 3 * (size_t)S.nk;
    S.kgrp = base + ((4 * (size_t)S.nk + 3) / 4) * 4;
  }
  if (!L.tl_sp_fits) L.tl.sp_tiles = 0;
  if (!L.tl_fo_fits) L.tl.fo_tiles = 0;
  if (L.maxgrid > 0) {
    const size_t mg = (size_t)L.maxgrid;
    // (behind the influence function of every simulation, pgstride doubles into its block: the home-tile keys of its atoms, one int each --
    // k_pppm_keys; md_types.h, whose text the pair kernel's counters are pinned to, keeps its SimDev -- or, in the same place, the lists of the
    // binned charge assignment: item count, an item of two ints per atom at most, the charged atoms by bin: k_pppm_bins.  A launch takes either.)
    const size_t gfs = mg + (3 * (size_t)L.maxatoms + 2 + 1) / 2;
    HIPCHK(e->d_pppm.ensure((size_t)ns * (mg * 4 * sizeof(double2) + gfs * sizeof(double))));
    double *gbase = e->d_pppm.as<double>(), *ebase = gbase + (size_t)ns * mg * 2, *fbase = gbase + (size_t)ns * mg * 8;
    for (int pos = 0; pos < ns; pos++) {
      SimDev &S = e->h_sims[pos];
      S.pgrid = gbase + (size_t)pos * mg * 2;
      S.pfield = ebase + (size_t)pos * mg * 6;
      S.pgstride = (long long)L.maxgrid;
      S.pgf = fbase + (size_t)pos * gfs;
      L.maxdims = std::max(L.maxdims, S.pg[0] + S.pg[1] + S.pg[2]);
      const bool same = pos > 0 && pos != parts[part_of(parts, pos)].off && std::memcmp(S.pg, e->h_sims[pos - 1].pg, sizeof S.pg) == 0;
      if (same) pppm_runs.back().second += 1;
      else pppm_runs.push_back({pos, 1});
    }
  }
  return SCEMA_MD_OK;
}

// ---- the PPPM chain ----
// reciprocal part by PPPM for the simulations [pos0, pos0 + na) of a launch group (md_pppm.hip); after force_stage
int OplsRun::pppm_stage(hipStream_t st, int pos0, int na, bool new_box, int add) {
  if (L.maxgrid <= 0 || na <= 0) return SCEMA_MD_OK;
  const SimDev *Dp = D + pos0;
  bool &clean = pppm_clean[part_of(parts, pos0)];
  const int maxgridp = L.padx_ok ? L.maxgridp : 0;
  const int sp_path = mdk_pppm_spread_path(L.maxgrid, maxgridp, &L.tl), fo_path = mdk_pppm_force_path(L.maxgrid, &L.tl);
  {
    const int paths[8] = {sp_path, fo_path, sp_path == 1 ? L.tl.sp_ty : 1, sp_path == 1 ? L.tl.sp_tz : 1, fo_path == 1 ? L.tl.fo_ty : 1,
                          fo_path == 1 ? L.tl.fo_tz : 1, L.tl.budget, L.tl.mode};
    std::memcpy(e->pppm_paths, paths, sizeof paths);
  }
  if (sp_path == 1 || fo_path == 1) mdk_pppm_keys(st, Dp, na, L.maxatoms);   // home tiles from the positions of this step
  // Binned charge assignment: one more launch on the chain, which a small launch waits for and a large one wins back several times over
  // (PppmBinPolicy; SCEMA_MD_PPPM_BINNED and scema_md_pppm_binning force either)
  static const int binned_env = scema_env("SCEMA_MD_PPPM_BINNED") ? (atoi(scema_env("SCEMA_MD_PPPM_BINNED")) != 0 ? 1 : 0) : -1;
  const int bin_mode = binned_env >= 0 ? binned_env : e->pppm_bin_mode;
  PppmLaunch tl = L.tl;
  if (bin_mode != 0 && mdk_pppm_binned_ok(L.maxgrid, maxgridp, &L.tl)) {
    const PppmBinPolicy bp;
    tl.binned = bin_mode == 1 || (na >= bp.min_replicas && (double)L.sum_charged >= bp.min_per_point * (double)L.sum_grid) ? 1 : 0;
  }
  if (tl.binned) e->pppm_binned_launches += 1;
  // Staged interpolation: the field grids at the plane stride of md_pppm_fstride.h (SCEMA_MD_PPPM_FLAYOUT and scema_md_pppm_force_layout
  // force the dense layout or the rule; the default is the rule at every launch size: profiles/pppm_fstride_size_scan.log)
  static const int flayout_env = scema_env("SCEMA_MD_PPPM_FLAYOUT") ? (atoi(scema_env("SCEMA_MD_PPPM_FLAYOUT")) != 0 ? 1 : 0) : -1;
  PppmLaunch tlf = L.tl;
  if ((flayout_env >= 0 ? flayout_env : e->pppm_flayout_mode) == 0) tlf.fs_lds = 0;
  mdk_pppm_spread(st, Dp, na, L.maxgrid, L.maxatoms, clean ? 1 : 0, maxgridp, &tl);   // (the tiled kernel stores every point: no zero launch)
  clean = false;
  if (pol.pppm_in_lds) {   // small grids: the whole solve in one launch, in LDS (md_pppm.hip k_pppm_solve); it leaves the charge grids zeroed
    if (new_box) mdk_pppm_gf(st, Dp, na, L.maxgrid);
    mdk_pppm_solve(st, Dp, na, L.maxgrid, L.maxdims);
    clean = true;
    mdk_pppm_force(st, Dp, na, L.maxgrid, L.maxatoms, add, 1, &tlf);
    return SCEMA_MD_OK;
  }
  auto transform = [&](bool fields, int dir) -> int {   // the charge grids forward, or the three field grids of every simulation back
    for (const auto &run : pppm_runs) {
      if (run.first + run.second <= pos0 || run.first >= pos0 + na) continue;   // outside this launch group, or none of it is active any more
      const SimDev &S0 = e->h_sims[run.first];
      if (S0.pg[0] == 0) continue;
      if (const int rc = pppm_exec(e, S0.pg, (fields ? 3 : 1) * run.second, st, L.maxgrid, fields ? S0.pfield : S0.pgrid, dir)) return rc;
    }
    return SCEMA_MD_OK;
  };
  int rc = transform(false, HIPFFT_FORWARD);
  if (rc) return rc;
  if (new_box) mdk_pppm_gf(st, Dp, na, L.maxgrid);
  mdk_pppm_poisson(st, Dp, na, L.maxgrid);
  if ((rc = transform(true, HIPFFT_BACKWARD))) return rc;
  mdk_pppm_force(st, Dp, na, L.maxgrid, L.maxatoms, add, 0, &tlf);
  return SCEMA_MD_OK;
}

// the PPPM chain of a step on the side stream (Policy::pppm_side), its forces left in SimDev::f; optionally the bonded kernel behind it
int OplsRun::pppm_fork(hipStream_t st, int pos0, int na, bool new_box, bool with_bonded) {
  if (!pol.pppm_side) return SCEMA_MD_OK;
  HIPCHK(hipEventRecord(e->ev_fork, st));
  HIPCHK(hipStreamWaitEvent(e->stream2, e->ev_fork, 0));
  const int rc = pppm_stage(e->stream2, pos0, na, new_box, 0);
  if (rc) return rc;
  if (with_bonded) mdk_bonded(e->stream2, D + pos0, na, L.maxbt, L.maxloc, L.maxcoef, 0, bonded_grouped(e));   // (needs the positions only, like the chain before it)
  HIPCHK(hipEventRecord(e->ev_join, e->stream2));
  return SCEMA_MD_OK;
}

// After k_pair: the bonded terms, the structure factors + per-k coefficients (on the side stream where `side`), the per-atom reciprocal force
hipError_t OplsRun::force_stage(hipStream_t st, const SimDev *Dh, int na, bool side, int bparts, int pairvir, bool pppm_ahead) {
  hipError_t rc;
  if (side) {
    if ((rc = hipEventRecord(e->ev_fork, st)) != hipSuccess) return rc;
    if ((rc = hipStreamWaitEvent(e->stream2, e->ev_fork, 0)) != hipSuccess) return rc;
    mdk_ewald_recip(e->stream2, Dh, na, L.maxk, L.mmax, L.maxgrp);
    if ((rc = hipEventRecord(e->ev_join, e->stream2)) != hipSuccess) return rc;
  }
  mdk_bonded(st, Dh, na, L.maxbt, L.maxloc, L.maxcoef, bparts, bonded_grouped(e));
  if (side) {
    if ((rc = hipStreamWaitEvent(st, e->ev_join, 0)) != hipSuccess) return rc;
  } else {
    mdk_ewald_recip(st, Dh, na, L.maxk, L.mmax, L.maxgrp);
  }
  if (pppm_ahead) {   // the PPPM chain of this step ran on the side stream and left its forces in SimDev::f
    if ((rc = hipStreamWaitEvent(st, e->ev_join, 0)) != hipSuccess) return rc;
  }
  mdk_ewald_force(st, Dh, na, L.maxatoms, pairvir, pppm_ahead ? 1 : 0);
  return hipSuccess;
}

// step 0 of every part: lists, forces, the constraint and half-kick set-up
int OplsRun::setup_step() {
  int rc = fork_parts(e, parts, e->ev_up);   // (the other streams start behind the uploads)
  if (rc) return rc;
  for (const Part &pt : parts) {
    hipStream_t st = pt.st;
    const SimDev *Dh = D + pt.off;
    const int nh = pt.n;
    mdk_phase_init(st, Dh, nh);
    if (L.any_validate) mdk_keep_validate(st, Dh, nh, L.maxatoms);
    mdk_neighbor(st, Dh, nh, L.maxatoms, L.maxpad, L.maxcells, L.maxrow, L.maxcapj, true, pol.nb_together);
    if ((rc = pppm_fork(st, pt.off, nh, true))) return rc;
    mdk_pair(st, Dh, nh, L.maxcells, L.maxcapj, ev, spec.ev_always, L.maxpoly, cle);
    HIPCHK(force_stage(st, Dh, nh, pol.recip_side_for(nh), spec.ev_always, (ev && !spec.ev_always) ? 1 : 0, pol.pppm_side));
    if (!pol.pppm_side && (rc = pppm_stage(st, pt.off, nh, true))) return rc;
    if (!spec.static_only) mdk_shake(st, Dh, nh, L.maxclus, 0.5);
    mdk_final_integrate(st, Dh, nh, L.maxatoms, 0);
    if (spec.nh) mdk_setup_post_nh(st, Dh, nh);
    else mdk_setup_post(st, Dh, nh);
  }
  return SCEMA_MD_OK;
}

int OplsRun::minimise() {
  hipStream_t st = e->stream;
  auto force = [&]() -> int {
    mdk_neighbor(st, D, ns, L.maxatoms, L.maxpad, L.maxcells, L.maxrow, L.maxcapj);
    mdk_pair(st, D, ns, L.maxcells, L.maxcapj, 1, 1, L.maxpoly, cle);
    HIPCHK(force_stage(st, D, ns, false, 1, 0, false));
    return pppm_stage(st, 0, ns, false);
  };
  auto map_fault = [&](int fault) {
    e->overflow_bits = (fault & 1) ? (fault & (4 | 8)) : 0;
    return (fault & 1) ? SCEMA_MD_ERR_OVERFLOW : SCEMA_MD_OK;
  };
  return run_minimiser(e, order, L.maxatoms, spec, true, force, map_fault);
}

// one MD step of the first `na` simulations of a part, as a sequence of launches on that part's stream
// (The pair kernel as PERSISTENT workgroups -- one 1 024-thread workgroup per CU for the whole launch, two tiles in LDS, rows taken off LDS
// counters, no barrier between a tile's rows and its flush -- was built in two forms in round 6 to recover the quarter of a wave's life that
// k_pair spends outside its row loop, and lost: 405 / 342 against 463 / 451 evaluations/s at 576 replicas.  k_pair sits at 120 of 128 vector
// registers; the persistent shell's dozen extra live scalars tip the allocation into scratch reloads inside the row loop, whose every wait then
// covers all loads in flight.  profiles/r06_q_persistent_pair.txt has the wave clocks and the ISA counts; commit 2371531 holds the code.)
int OplsRun::launch_step(const Part &pt, int na, bool timed) {
  hipStream_t st = pt.st;
  const SimDev *Dh = D + pt.off;
  int rc;
  if (spec.nh) { mdk_pre_nh(st, Dh, na); mdk_initial_integrate_nh(st, Dh, na, L.maxatoms); }
  else mdk_initial_integrate(st, Dh, na, L.maxatoms, pol.fuse_pack);   // (its k_pre: at the end of the step before, in k_post; for step 1 in run_steps)
  // the PPPM chain needs the new positions only: it leaves for its side stream before the list kernels are issued, not behind them
  if ((rc = pppm_fork(st, pt.off, na, spec.deform || (spec.nh && spec.npt), pol.bonded_side))) return rc;
  mdk_neighbor(st, Dh, na, L.maxatoms, L.maxpad, L.maxcells, L.maxrow, L.maxcapj, spec.nh != 0 || !pol.fuse_pack, pol.nb_together);
  if (timed) {
    if (ev_used + 2 > e->ev_pool.size()) {
      hipEvent_t a, b;
      HIPCHK(hipEventCreate(&a));
      HIPCHK(hipEventCreate(&b));
      e->ev_pool.push_back(a);
      e->ev_pool.push_back(b);
    }
    HIPCHK(hipEventRecord(e->ev_pool[ev_used], st));
  }
  mdk_pair(st, Dh, na, L.maxcells, L.maxcapj, ev, spec.ev_always, L.maxpoly, cle);
  if (timed) {
    HIPCHK(hipEventRecord(e->ev_pool[ev_used + 1], st));
    ev_used += 2;
    launch_sims.push_back({pt.off, na});
  }
  if (pol.fused_tail) {
    // no per-atom reciprocal sum: the bonded kernel, the PPPM chain (its forces stored in f, from the side stream or here), then
    // assembly of f, fix shake and the second half-kick in one pass (k_finish)
    if (!pol.bonded_side) mdk_bonded(st, Dh, na, L.maxbt, L.maxloc, L.maxcoef, 0, bonded_grouped(e));
    if (pol.pppm_side) HIPCHK(hipStreamWaitEvent(st, e->ev_join, 0));
    else if ((rc = pppm_stage(st, pt.off, na, spec.deform, 0))) return rc;
    mdk_finish(st, Dh, na, L.maxunits, ev, L.maxgrid > 0 ? 1 : 0);
  } else {
    HIPCHK(force_stage(st, Dh, na, pol.recip_side_for(na), spec.ev_always, (ev && !spec.ev_always) ? 1 : 0, pol.pppm_side));
    if (!pol.pppm_side && (rc = pppm_stage(st, pt.off, na, spec.deform || (spec.nh && spec.npt)))) return rc;
    mdk_shake(st, Dh, na, L.maxclus, 1.0);
    mdk_final_integrate(st, Dh, na, L.maxatoms, 1);
  }
  if (spec.nh) mdk_post_nh(st, Dh, na);
  else mdk_post(st, Dh, na, 1);
  if (spec.deform) mdk_remap(st, Dh, na, L.maxatoms);
  return SCEMA_MD_OK;
}

// A flip detected at the end of a step: before the next one the box takes its flipped tilts, the list rebuild of the next step is forced and
// the k-vector list is re-expressed in the new reciprocal basis (same vectors: n2 += f_xy n1, n3 += f_yz n2 + f_xz n1), all stream-ordered
// behind the launches of the step
int OplsRun::apply_flip(int pos, const FlipEvent &fe) {
  hipStream_t st = parts[part_of(parts, pos)].st;
  SimDev &S = e->h_sims[pos];
  EwaldSetup &ew = ews[pos];
  if (S.nk > 0) {
    for (int k = 0; k < S.nk; k++) {
      const int n1 = ew.kn[3 * k], n2 = ew.kn[3 * k + 1], n3 = ew.kn[3 * k + 2];
      ew.kn[3 * k + 1] = n2 + fe.nflip[0] * n1;
      ew.kn[3 * k + 2] = n3 + fe.nflip[2] * n2 + fe.nflip[1] * n1;
    }
    ewald_tables(ew);
    flip_host.emplace_back(new std::vector<int>());
    std::vector<int> &hk = *flip_host.back();
    hk.insert(hk.end(), ew.kn.begin(), ew.kn.end());
    hk.insert(hk.end(), ew.krun.begin(), ew.krun.end());
    while (hk.size() % 4) hk.push_back(0);
    const size_t goff = hk.size();
    hk.insert(hk.end(), ew.kgrp.begin(), ew.kgrp.end());
    flip_bufs.emplace_back(new DevBuf());
    HIPCHK(flip_bufs.back()->ensure(hk.size() * sizeof(int) + 64));
    HIPCHK(hipMemcpyAsync(flip_bufs.back()->p, hk.data(), hk.size() * sizeof(int), hipMemcpyHostToDevice, st));
    const int *base = flip_bufs.back()->as<int>();
    S.kn = base;
    S.krun = base + 3 * (size_t)S.nk;
    S.kgrp = base + goff;
    S.ngrp = (int)ew.kgrp.size() / 8;
    for (int d = 0; d < 3; d++) { S.kmaxd[d] = ew.kmaxd[d]; L.mmax = std::max(L.mmax, S.kmaxd[d] + 1); }
    L.maxgrp = std::max(L.maxgrp, S.ngrp);
    if ((size_t)64 * 3 * L.mmax * 16 + 4096 > 160 * 1024)
      return fail(e, SCEMA_MD_ERR_ARG, "k-space index range after a box flip (|n| up to %d) too large for the LDS phase tables", L.mmax - 1);
    flip_desc.emplace_back(new SimDev(S));   // the source of an asynchronous upload must not change under it
    HIPCHK(hipMemcpyAsync(e->d_sims.as<SimDev>() + pos, flip_desc.back().get(), sizeof(SimDev), hipMemcpyHostToDevice, st));
  }
  mdk_flip(st, D + pos, fe.tilt[0], fe.tilt[1], fe.tilt[2]);
  e->prof.box_flips += 1;
  return SCEMA_MD_OK;
}

// the steps: runs of steps with the same active prefix of every part, each run ending at the next flip
// (hipGraph replay of the steps that share an active count was measured on ROCm 7.2 / MI355X -- ms per update of 1 / 72 PE-10k
// replicas: plain launches 25.8 / 236.7, replay 26.4 / 236.9, with the side stream inside the graph 55.2 / 251.3 -- and removed in
// round 4: profiles/HISTORY.md)
int OplsRun::run_steps() {
  const bool prof = e->p.profile != 0;
  const FlipSchedule flip_at = flip_schedule(flips, e->h_sims);
  if (!spec.nh)   // the k_pre of step 1, for the simulations that have a step 1; every later one rides on the k_post of the step before
    for (const Part &pt : parts) {
      const int n1 = active_prefix(e->h_sims, pt, 1);
      if (n1 > 0) mdk_pre(pt.st, D + pt.off, n1);
    }
  for (int step = 1; step <= L.maxsteps;) {
    const int na = active_prefix(e->h_sims, parts[0], step);
    if (na == 0) break;
    int run_len = e->h_sims[na - 1].nsteps - step + 1;   // steps until the active prefix shrinks (sorted by nsteps)
    int nact[MAXP] = {na}, nsum = na;
    for (int h = 1; h < pol.nparts; h++) {
      nact[h] = active_prefix(e->h_sims, parts[h], step);
      nsum += nact[h];
      if (nact[h] > 0) run_len = std::min(run_len, e->h_sims[parts[h].off + nact[h] - 1].nsteps - step + 1);
    }
    auto nxt = flip_at.lower_bound(step);
    if (nxt != flip_at.end()) run_len = std::min(run_len, nxt->first - step + 1);   // the launch group ends with the flipping step
    for (int r = 0; r < run_len; r++)
      for (int h = 0; h < pol.nparts; h++) {
        if (nact[h] == 0) continue;
        const int rc = launch_step(parts[h], nact[h], prof);
        if (rc) return rc;
      }
    e->prof.md_steps += (long long)nsum * run_len;
    step += run_len;
    auto fl = flip_at.find(step - 1);   // flips detected at the end of step - 1
    if (fl != flip_at.end())
      for (const auto &pk : fl->second) {
        const int rc = apply_flip(pk.first, flips[pk.first][pk.second]);
        if (rc) return rc;
      }
  }
  return SCEMA_MD_OK;
}

// the end of the run: join, scalars back, profile, faults, and the signatures of the rows that stand
int OplsRun::finish() {
  for (const Part &pt : parts) mdk_phase_end(pt.st, D + pt.off, pt.n, L.maxatoms);
  int rc = join_parts(e, parts, e->md_part_done.data());
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(e->h_sc.data(), e->d_sc.p, (size_t)ns * sizeof(SimScalars), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  if (e->p.profile != 0) {
    // algorithmic bytes of one pair launch: per simulation N*(4*nbar + 56) + 48 with
    // nbar = stored neighbours per atom of the (full) list
    std::vector<double> simbytes(ns);
    for (int pos = 0; pos < ns; pos++)   // the reference's list radius, whatever the skin used
      simbytes[pos] = 4.0 * (double)e->h_sc[order[pos]].nentries_ref + 56.0 * e->h_sims[pos].natoms + 48.0;
    if ((rc = sum_timed_launches(e, launch_sims.size(), e->prof.pair_ms, e->prof.pair_launches, e->prof.pair_union_ms))) return rc;
    for (const auto &ls : launch_sims) {
      e->prof.pair_sims += ls.second;
      for (int pos = ls.first; pos < ls.first + ls.second; pos++) e->prof.pair_alg_bytes += simbytes[pos];
    }
  }
  print_run_timing(e, ns, t_layout, t_kspace, t_box, t_grid, t_rest);
  const int fault = collect_faults(e, ns);
  for (int i = 0; i < ns; i++) {
    e->prof.unique_pairs_sum += 0.5 * (double)e->h_sc[i].nentries_ref;
    e->prof.unique_pairs_n += 1;
  }
  // A capacity that overflowed comes first: the run went on with truncated rows or tables (nothing is written past a capacity, pairs are
  // missing), so an instability or a stretched special pair later in the same run is its consequence, not the caller's input -- the retry
  // with grown capacities starts from the backup and reports them if they are real.
  e->overflow_bits = fault;
  {   // (what the builds of this run saw -- a table's count runs on past its capacity, a row's stops a chunk beyond -- against the smallest capacity of the launch)
    int seen_j = 0, seen_row = 0, cap_j = 1 << 30, cap_row = 1 << 30;
    for (int i = 0; i < ns; i++) {
      seen_j = std::max(seen_j, e->h_sc[i].maxj_seen); seen_row = std::max(seen_row, e->h_sc[i].maxneigh_seen);
      cap_j = std::min(cap_j, std::max(1, e->h_sims[i].capj)); cap_row = std::min(cap_row, std::max(1, e->h_sims[i].maxneigh));
    }
    e->overflow_need_j = std::max(1.0, (double)seen_j / cap_j);
    e->overflow_need_row = std::max(1.0, (double)seen_row / cap_row);
  }
  if (fault & 1) return SCEMA_MD_ERR_OVERFLOW;
  if (fault & 16) return fail(e, SCEMA_MD_ERR_ARG, "a simulation became unstable (non-finite or runaway atom positions): overlapping atoms or parameters far from the replica's equilibrium");
  if (fault & 2) return fail(e, SCEMA_MD_ERR_ARG, "an excluded (special) pair stretched beyond the exclusion gate; topology or state is broken");
  if (fault & 64) return SCEMA_MD_ERR_OVERFLOW;   // the barostat took the box out of the range this segment was laid out for
  lists_hold(e, sims, true, true);
  return SCEMA_MD_OK;
}

}  // namespace

// Advance sims[0..ns) (already assigned to slots 0..ns-1, scalars' box valid on the device).
// On return the per-sim SimScalars are in e->h_sc.
int run_phase(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  e->rows_run_ns = 0;   // (scema_md_debug_rows describes the last run of a row potential that ended well)
  {   // simulations of a material with a Stillinger-Weber, Tersoff or EAM potential attached take that force stage, whichever entry point issued the run
    size_t n_pot[ROW_NPOT] = {};
    for (const ActiveSim &A : sims)
      if (const RowPot *P = row_pot_of(e, A.st->topo->matid.c_str())) n_pot[P - row_pots]++;
    for (int k = 0; k < ROW_NPOT; k++) {   // (the first kind of the table that is present takes the run or is named in the refusal)
      if (n_pot[k] == sims.size() && n_pot[k] > 0) return run_phase_rowpot(e, sims, spec, row_pots[k]);
      if (n_pot[k]) return fail(e, SCEMA_MD_ERR_ARG, "one run mixes %s materials (%zu of %zu simulations) with others", row_pots[k].name, n_pot[k], sims.size());
    }
  }
  if (e->reax_active) return run_phase_reax(e, sims, spec);
  const auto t_enter = Clock::now();
  OplsRun R(e, sims, spec);
  R.kspace_setup();
  R.t_kspace = ms_between(t_enter, Clock::now());
  int rc = R.make_parts();
  for (int pos = 0; pos < R.ns && !rc; pos++) rc = R.lay_out_sim(pos);
  if (rc || (rc = R.lay_out_kspace())) return rc;
  plan_sides(R.pol, e, R.ns, spec, R.L);
  HIPCHK(e->d_sims.ensure((size_t)R.ns * sizeof(SimDev)));
  HIPCHK(hipMemcpyAsync(e->d_sims.p, e->h_sims.data(), (size_t)R.ns * sizeof(SimDev), hipMemcpyHostToDevice, e->stream));
  R.t_layout = ms_between(t_enter, Clock::now());
  R.D = e->d_sims.as<SimDev>();
  if ((rc = R.setup_step())) return rc;
  if (spec.minimize) return R.minimise();
  if ((rc = R.run_steps())) return rc;
  return R.finish();
}

int prepare_slots(scema_md_engine *e, std::vector<ActiveSim> &sims) {
  const int ns = (int)sims.size();
  while ((int)e->slots.size() < ns) e->slots.emplace_back(new Slot());
  HIPCHK(e->d_sc.ensure((size_t)std::max(ns, 1) * sizeof(SimScalars)));
  e->h_sc.assign(ns, SimScalars());
  for (int i = 0; i < ns; i++) {
    std::memset(&e->h_sc[i], 0, sizeof(SimScalars));
    std::memcpy(e->h_sc[i].box, sims[i].st->box, 9 * sizeof(double));
    e->h_sc[i].vscale = 1.0;
    // the slot may still hold this state's neighbour rows from the update before: their scalars come back with them (run_phase and the
    // device decide whether the rows are kept; a slot that last served another state leaves the zeros, which force the build)
    const ListSig &g = e->slots[i]->sig;
    if (g.valid && g.state == sims[i].st->id) {
      std::memcpy(e->h_sc[i].corners_hold, g.corners_hold, sizeof g.corners_hold);
      e->h_sc[i].ago = g.ago; e->h_sc[i].maxj_seen = g.maxj_seen;
      e->h_sc[i].nentries = g.nentries; e->h_sc[i].nentries_ref = g.nentries_ref; e->h_sc[i].nrowent = g.nrowent;
    }
  }
  HIPCHK(hipMemcpyAsync(e->d_sc.p, e->h_sc.data(), (size_t)ns * sizeof(SimScalars), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return SCEMA_MD_OK;
}

// scalars that must not leak from one run into the next when h_sc is re-uploaded
int reupload_scalars(scema_md_engine *e, int ns) {
  for (int i = 0; i < ns; i++) {
    e->h_sc[i].overflow = 0;
    e->h_sc[i].nbuilds = 0;
    e->h_sc[i].maxneigh_seen = 0;
  }
  HIPCHK(hipMemcpyAsync(e->d_sc.p, e->h_sc.data(), (size_t)ns * sizeof(SimScalars), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return SCEMA_MD_OK;
}

}  // namespace scema_eng
