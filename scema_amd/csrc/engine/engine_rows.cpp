// engine_rows.cpp -- the batch skeleton every force stage shares (launch order, part batches, box range, minimiser, flips, what a run leaves
// behind), the growth rule after an overflow, and the run of a batch on per-atom neighbour rows that the ReaxFF stage and the row potentials' stages share
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// -------------------------------------------------------------------------------------------
// the batch skeleton of every force stage
// -------------------------------------------------------------------------------------------
// Launch order: longest run first, so the active simulations are always a prefix (ties broken by `tie`, ascending); dealt round-robin into
// nparts part batches at consecutive positions: part p takes the ranks p, p + nparts, ... of the length order, so each part is itself sorted
// longest first and the parts carry the same mix of run lengths
std::vector<int> batch_order(const std::vector<ActiveSim> &sims, int nparts, const std::function<long(int)> &tie) {
  const int ns = (int)sims.size();
  std::vector<int> by_len(ns), order;
  for (int i = 0; i < ns; i++) by_len[i] = i;
  std::stable_sort(by_len.begin(), by_len.end(), [&](int a, int b) {
    if (sims[a].nsteps != sims[b].nsteps) return sims[a].nsteps > sims[b].nsteps;
    return tie && tie(a) < tie(b);
  });
  order.reserve(ns);
  for (int p = 0; p < nparts; p++)
    for (int r = p; r < ns; r += nparts) order.push_back(by_len[r]);
  return order;
}
std::vector<Part> split_parts(int ns, int nparts) {
  std::vector<Part> parts(nparts);
  for (int p = 0, off = 0; p < nparts; p++) {
    parts[p].off = off;
    parts[p].n = (ns - p + nparts - 1) / nparts;
    off += parts[p].n;
  }
  return parts;
}
int part_of(const std::vector<Part> &parts, int pos) {
  int h = 0;
  while (h + 1 < (int)parts.size() && pos >= parts[h + 1].off) h++;
  return h;
}
int active_prefix(const std::vector<SimDev> &h_sims, const Part &p, int step) {   // (a part is sorted longest first)
  int na = 0;
  while (na < p.n && h_sims[p.off + na].nsteps >= step) na++;
  return na;
}
// the parts beyond the first start behind what the main stream has issued so far
int fork_parts(scema_md_engine *e, const std::vector<Part> &parts, hipEvent_t ev) {
  if (parts.size() < 2) return SCEMA_MD_OK;
  HIPCHK(hipEventRecord(ev, e->stream));
  for (size_t k = 1; k < parts.size(); k++) HIPCHK(hipStreamWaitEvent(parts[k].st, ev, 0));
  return SCEMA_MD_OK;
}
// the main stream waits for the end of every other part (an event of its own per part: done[k - 1] for part k)
int join_parts(scema_md_engine *e, const std::vector<Part> &parts, const hipEvent_t *done) {
  for (size_t k = 1; k < parts.size(); k++) {
    HIPCHK(hipEventRecord(done[k - 1], parts[k].st));
    HIPCHK(hipStreamWaitEvent(e->stream, done[k - 1], 0));
  }
  return SCEMA_MD_OK;
}

// The boxes a replica passes through in this run: start and end of fix deform's path, with the boxes just before each flip (where the tilt
// is largest) as extremes, and both ends of the range the barostat may dilate the box to (tilts with it).  False: the path cannot be run.
bool box_range(const RunSpec &spec, const ActiveSim &A, const double *box, BoxRange &R, std::vector<FlipEvent> &flips) {
  double box_end[9];
  std::memcpy(box_end, box, sizeof box_end);
  R.boxes.assign(2, HostBox());
  if (spec.deform) {
    std::vector<HostBox> extremes;
    if (!deform_trajectory(box, A.rates, A.dt, A.nsteps, box_end, flips, extremes)) return false;
    R.boxes.insert(R.boxes.end(), extremes.begin(), extremes.end());
  }
  box_derive(box, R.boxes[0]);
  box_derive(box_end, R.boxes[1]);
  if (spec.nh && spec.npt && spec.box_margin > 0.0)
    for (int sgn = -1; sgn <= 1; sgn += 2) {
      double bx[9];
      const double f = 1.0 + sgn * spec.box_margin;
      for (int d = 0; d < 3; d++) {
        const double c = 0.5 * (box[d] + box[3 + d]);
        bx[d] = c + (box[d] - c) * f;
        bx[3 + d] = c + (box[3 + d] - c) * f;
      }
      for (int k = 6; k < 9; k++) bx[k] = box[k] * f;
      HostBox hb;
      box_derive(bx, hb);
      R.boxes.push_back(hb);
    }
  for (const HostBox &hb : R.boxes) {
    double w[3];
    perp_widths(hb, w);
    for (int d = 0; d < 3; d++) R.w[d] = std::min(R.w[d], w[d]);
    R.vol_min = std::min(R.vol_min, hb.vol);
    R.vol_max = std::max(R.vol_max, hb.vol);
  }
  return true;
}

// the fields of SimDev that do not depend on the force field (call after the slot's buffers are sized)
void sim_common(SimDev &S, const scema_md_params &P, const RunSpec &spec, const ActiveSim &A, const Slot &sl, SimScalars *sc) {
  S.nsteps = A.nsteps;
  if (spec.sample) {
    // in.homogenization.lammps:57 (the reax copy is the same): nav = nss/10 (nss/1000 beyond 10000 steps); nss/nav windows
    S.nav = (A.nsteps > 10000) ? A.nsteps / 1000 : A.nsteps / 10;
    if (S.nav < 1) S.nav = 1;
    S.nwin = A.nsteps / S.nav;
  }
  S.nvt = spec.nvt;
  S.deform = spec.deform;
  if (spec.nh) {
    S.ramp = 1; S.npt = spec.npt; S.nh_total = std::max(spec.nh_total, 1); S.lavg_nav = spec.lavg_nav;
    S.t_start = spec.t_start; S.t_stop = spec.t_stop; S.p_target = spec.p_target; S.p_freq = 1.0 / spec.p_period; S.box_margin = spec.box_margin;
  }
  if (spec.minimize) {
    S.min_etol = spec.min_etol; S.min_ftol = spec.min_ftol; S.min_dmax = 0.1; S.min_maxiter = spec.min_maxiter; S.min_maxeval = spec.min_maxeval;
  }
  S.t_chain = std::min(P.t_chain, MD_MAXCHAIN);
  S.dt = A.dt; S.t_target = A.temperature; S.t_freq = 1.0 / P.t_period;
  for (int k = 0; k < 6; k++) S.rates[k] = A.rates[k];
  const Topo &T = *A.st->topo;
  S.type = T.d_type.as<int>(); S.q = T.d_q.as<double>(); S.mass = T.d_mass.as<double>();
  S.x = A.st->x.as<double>(); S.v = A.st->v.as<double>(); S.f = sl.f.as<double>();
  S.wrapn = sl.wrapn.as<int>(); S.xhold = sl.xhold.as<double>(); S.sfac = sl.sfac.as<double>(); S.cell_count = sl.cell_count.as<int>();
  S.sc = sc;
}

// min_style sd (md_equil.hip): every replica runs its own line search, decided on the device between two force evaluations (`force`); the
// host only looks every 16 evaluations whether the search is over -- stop_on_any_overflow: once a replica has overflowed or every one has
// stopped (OPLS); else once every replica has either stopped or overflowed (ReaxFF).  x0 and the search direction live in the slots'
// backup arrays.  `map_fault` turns the union of the replicas' fault bits into the caller's error (0: none).
int run_minimiser(scema_md_engine *e, const std::vector<int> &order, int maxatoms, const RunSpec &spec, bool stop_on_any_overflow,
                  const std::function<int()> &force, const std::function<int(int)> &map_fault) {
  const int ns = (int)order.size();
  hipStream_t st = e->stream;
  const SimDev *D = e->d_sims.as<SimDev>();
  std::vector<double *> ptrs(2 * (size_t)ns);
  for (int pos = 0; pos < ns; pos++) {
    Slot &sl = *e->slots[order[pos]];
    ptrs[pos] = sl.xbak.as<double>();
    ptrs[ns + pos] = sl.vbak.as<double>();
    HIPCHK(hipMemsetAsync(sl.vbak.p, 0, 3 * (size_t)e->h_sims[pos].natoms * 8, st));
  }
  HIPCHK(e->d_minptr.ensure(ptrs.size() * sizeof(double *)));
  HIPCHK(hipMemcpyAsync(e->d_minptr.p, ptrs.data(), ptrs.size() * sizeof(double *), hipMemcpyHostToDevice, st));
  double *const *x0s = e->d_minptr.as<double *>(), *const *hsd = e->d_minptr.as<double *>() + ns;
  mdk_min_reduce(st, D, ns, maxatoms, hsd);
  mdk_min_decide(st, D, ns);
  const long long cap = (long long)spec.min_maxeval + 2LL * spec.min_maxiter + 8;
  const auto stopped = [](const SimScalars &c) { return c.min_phase == 4; };
  const auto overflowed = [](const SimScalars &c) { return c.overflow != 0; };
  bool done = false;
  for (long long ev_n = 0; ev_n < cap && !done;) {
    for (int r = 0; r < 16; r++, ev_n++) {
      mdk_min_pre(st, D, ns);
      mdk_min_move(st, D, ns, maxatoms, x0s, hsd);
      const int rc = force();
      if (rc) return rc;
      mdk_min_reduce(st, D, ns, maxatoms, hsd);
      mdk_min_decide(st, D, ns);
    }
    HIPCHK(hipMemcpyAsync(e->h_sc.data(), e->d_sc.p, (size_t)ns * sizeof(SimScalars), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const auto first = e->h_sc.begin(), last = first + ns;
    done = stop_on_any_overflow ? std::any_of(first, last, overflowed) || std::all_of(first, last, stopped)
                                : std::all_of(first, last, [&](const SimScalars &c) { return overflowed(c) || stopped(c); });
  }
  HIPCHK(hipGetLastError());
  int fault = 0;
  for (int i = 0; i < ns; i++) fault |= e->h_sc[i].overflow;
  if (fault & 16) return fail(e, SCEMA_MD_ERR_ARG, "a simulation became unstable during the minimisation (non-finite positions)");
  e->overflow_need_j = e->overflow_need_row = 1.0;   // (the demand is not measured here: a retry grows by the fixed step, grow_after_overflow)
  if (const int rc = map_fault(fault)) return rc;
  if (!done) return fail(e, SCEMA_MD_ERR_ARG, "minimiser did not stop within its evaluation budget");
  return SCEMA_MD_OK;
}

// box flips of the run (fix deform, flip yes): step -> (position, flip of that position) that flip after it
FlipSchedule flip_schedule(const std::vector<std::vector<FlipEvent>> &flips, const std::vector<SimDev> &h_sims) {
  FlipSchedule at;
  for (size_t pos = 0; pos < flips.size(); pos++)
    for (size_t k = 0; k < flips[pos].size(); k++)
      if (flips[pos][k].step < h_sims[pos].nsteps) at[flips[pos][k].step].push_back({(int)pos, (int)k});
  return at;
}

// HIP-event times of the first n timed launches (e->ev_pool: launch l from 2 l to 2 l + 1) into `ms` and `launches`, and the time with at
// least one of them in flight (the launches of several part batches overlap) into `union_ms`
int sum_timed_launches(scema_md_engine *e, size_t n, double &ms, long long &launches, double &union_ms) {
  for (size_t l = 0; l < n; l++) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, e->ev_pool[2 * l], e->ev_pool[2 * l + 1]));
    ms += t;
    launches += 1;
  }
  union_ms += event_union_ms(e->ev_pool, n);
  return SCEMA_MD_OK;
}

// the union of the fault bits of the run's replicas; their list builds go to the profile
int collect_faults(scema_md_engine *e, int ns) {
  int fault = 0;
  for (int i = 0; i < ns; i++) {
    fault |= e->h_sc[i].overflow;
    e->prof.neigh_builds += e->h_sc[i].nbuilds;
  }
  return fault;
}

// the rows on the device hold for the positions this run ended at (`counts`: with the list's statistics of the OPLS rows)
void lists_hold(scema_md_engine *e, const std::vector<ActiveSim> &sims, bool valid, bool counts) {
  for (size_t i = 0; i < sims.size(); i++) {
    ListSig &g = e->slots[i]->sig;
    const SimScalars &c = e->h_sc[i];
    g.valid = valid;
    g.state = sims[i].st->id;
    std::memcpy(g.corners_hold, c.corners_hold, sizeof g.corners_hold);
    g.ago = c.ago;
    if (counts) { g.maxj_seen = c.maxj_seen; g.nentries = c.nentries; g.nentries_ref = c.nentries_ref; g.nrowent = c.nrowent; }
  }
}

// SCEMA_MD_KEEP_LIST=0: every run builds its neighbour rows anew at its start
bool keep_list_switch() {
  static const bool on = !(scema_env("SCEMA_MD_KEEP_LIST") && atoi(scema_env("SCEMA_MD_KEEP_LIST")) == 0);
  return on;
}

// SCEMA_MD_SKIN_BANDS=0: k_pair walks every listed entry of a row on every step (the reference behaviour of the skin bands, md_skin_bands.h)
bool skin_bands_switch() {
  static const bool on = !(scema_env("SCEMA_MD_SKIN_BANDS") && atoi(scema_env("SCEMA_MD_SKIN_BANDS")) == 0);
  return on;
}

// by the demand the failed run saw where that is more than the fixed step: a capacity far too small is found in one retry, not six
void grow_after_overflow(scema_md_engine *e) {
  if (e->overflow_bits & 4) e->jtab_grow *= std::max(1.25, std::min(8.0, 1.1 * e->overflow_need_j));
  if ((e->overflow_bits & 8) || !(e->overflow_bits & 4)) e->neigh_grow *= std::max(1.5, std::min(8.0, 1.1 * e->overflow_need_row));
}

// static evaluation of one state (the parity hooks): one run of no steps, repeated with grown capacities while they overflow
int eval_static(scema_md_engine *e, State *s, const RunSpec &spec) {
  std::vector<ActiveSim> sims(1);
  sims[0].st = s;
  sims[0].nsteps = 0;
  sims[0].dt = 1.0;
  sims[0].temperature = 300.0;
  int rc = SCEMA_MD_OK;
  for (int attempt = 0; attempt < 6; attempt++) {
    if ((rc = prepare_slots(e, sims))) return rc;
    rc = run_phase(e, sims, spec);
    if (rc != SCEMA_MD_ERR_OVERFLOW) break;
    grow_after_overflow(e);
  }
  return rc;
}

// -------------------------------------------------------------------------------------------
// the run of a batch on per-atom neighbour rows: run_phase with the ReaxFF force stage or a row potential's
// -------------------------------------------------------------------------------------------
// The same step sequence as the OPLS run (k_pre, k_initial_integrate, forces, k_final_integrate, k_post, k_remap), the same batch rules
// (longest run first, active prefix, part batches), the same box flips; no cells, no k-space, no SHAKE (neither lammps_scripts_reax nor
// lammps_scripts_sisw has a fix shake or a kspace_style).  What differs between the two stages is behind RowStage (engine.h).

// The replica at position pos of the launch order: box range, images, row capacities, its slot, its SimDev; the stage binds its view
int RowRun::lay_out_sim(int pos) {
  const int i = order[pos];
  ActiveSim &A = sims[i];
  Topo &T = *A.st->topo;
  const SimScalars &hsc = e->h_sc[i];
  BoxRange R;
  if (!box_range(spec, A, hsc.box, R, flips[pos]))
    return fail(e, SCEMA_MD_ERR_BOX, "fix deform is changing yz too much with xy: the strain would tilt yz past half the box");
  RowNeed N;
  int rc = stage.rows(T, R, N);
  if (rc) return rc;
  bool small = false;
  for (int d = 0; d < 3; d++) small = small || R.w[d] < 2.0 * N.rlist;
  for (int d = 0; d < 3; d++) {
    N.mimg[d] = small ? (int)std::ceil(N.rlist / R.w[d]) : 0;
    if (N.mimg[d] > 2) return fail(e, SCEMA_MD_ERR_BOX, "box width %.3f < (cutoff+skin)/2 = %.3f in dim %d", R.w[d], 0.5 * N.rlist, d);
  }
  const int n = T.natoms, npad = (n + 63) / 64 * 64;
  Slot &sl = *e->slots[i];
  ListSig &g = sl.sig;
  // A run that follows another run of the same stage and state on the same slot (the sampling run behind the straining run of an evaluation;
  // the straining run of the next update) keeps that run's neighbour rows, as the OPLS path does (run_phase): the rows and their reference
  // positions live in the slot, the list's scalars come back through the slot's signature (prepare_slots), and k_phase_init /
  // k_keep_validate decide on the device whether they still hold.  The rows keep the capacities they were built with.
  const bool keep = spec.keep_list && keep_list_switch() && g.valid && g.kind == stage.kind && g.stamp == N.stamp && g.topo == T.id && g.rlist == N.rlist &&
                    g.npad == npad && (spec.keep_list == 1 || g.state == A.st->id) && !hsc.force_rebuild && !hsc.overflow && N.cap[0] <= g.cap[0] &&
                    N.cap[1] <= g.cap[1] && g.mimg[0] == N.mimg[0] && g.mimg[1] == N.mimg[1] && g.mimg[2] == N.mimg[2];
  if (keep)
    for (int k = 0; k < 2; k++) N.cap[k] = g.cap[k];
  // what this run's rows are built for; valid once the run has ended without a fault
  g.valid = false;
  g.kind = stage.kind;
  g.stamp = N.stamp;
  g.topo = T.id;
  g.rlist = N.rlist; g.npad = npad;
  for (int k = 0; k < 2; k++) g.cap[k] = N.cap[k];
  for (int d = 0; d < 3; d++) g.mimg[d] = N.mimg[d];
  if ((rc = ensure_slot(e, sl, n, 64, 1, 0, 64))) return rc;
  SimDev S;
  std::memset(&S, 0, sizeof S);
  S.keep_list = keep ? spec.keep_list : 0;
  any_validate = any_validate || S.keep_list == 2;
  sim_common(S, e->p, spec, A, sl, e->d_sc.as<SimScalars>() + i);
  S.natoms = n; S.npad = npad; S.ntypes = T.ntypes;
  S.use_shake = 0;
  if (spec.minimize) S.min_incremental = 1;   // the neighbour rebuild wraps the atoms into the box: trial points by increments
  S.neigh_delay = 0;   // neigh_modify every 1 delay 0 check yes (in.set.lammps of both script sets); rebuilt when needed, same pairs inside the cutoff
  S.tdof = 3.0 * n - 3.0;
  S.skin = N.skin;
  e->h_zerotab.push_back(MdkZero{sl.wrapn.as<int>(), 3 * (long long)n});
  if ((rc = stage.bind(pos, A, sl, S, N))) return rc;
  e->h_sims[pos] = S;
  maxatoms = std::max(maxatoms, n); maxpad = std::max(maxpad, npad); maxsteps = std::max(maxsteps, A.nsteps);
  return SCEMA_MD_OK;
}

// every replica's layout, and its upload
int RowRun::lay_out() {
  e->h_sims.assign(ns, SimDev());
  e->h_zerotab.clear();
  for (int pos = 0; pos < ns; pos++)
    if (const int rc = lay_out_sim(pos)) return rc;
  HIPCHK(e->d_sims.ensure((size_t)ns * sizeof(SimDev)));
  HIPCHK(hipMemcpyAsync(e->d_sims.p, e->h_sims.data(), (size_t)ns * sizeof(SimDev), hipMemcpyHostToDevice, e->stream));
  D = e->d_sims.as<SimDev>();
  if (const int rc = stage.upload()) return rc;
  // the wrap counters of every replica, and what the stage sums over the steps, start from zero: one launch
  HIPCHK(e->d_zerotab.ensure(e->h_zerotab.size() * sizeof(MdkZero)));
  HIPCHK(hipMemcpyAsync(e->d_zerotab.p, e->h_zerotab.data(), e->h_zerotab.size() * sizeof(MdkZero), hipMemcpyHostToDevice, e->stream));
  mdk_zero_many(e->stream, e->d_zerotab.as<MdkZero>(), (int)e->h_zerotab.size(), 3 * (long long)maxatoms + stage.zero_extra);
  return SCEMA_MD_OK;
}

// step 0 of the whole batch on the main stream
int RowRun::setup_step() {
  hipStream_t st = e->stream;
  mdk_phase_init(st, D, ns);
  if (any_validate) mdk_keep_validate(st, D, ns, maxatoms);
  if (const int rc = stage.setup()) return rc;
  stage.forces(st, 0, ns, 0, 0);
  mdk_final_integrate(st, D, ns, maxatoms, 0);
  if (spec.nh) mdk_setup_post_nh(st, D, ns);
  else mdk_setup_post(st, D, ns);
  return SCEMA_MD_OK;
}

// min_style sd (md_equil.hip): the line search of every replica on the device, forces from the stage
int RowRun::minimise() {
  auto force = [&] {
    stage.forces(e->stream, 0, ns, 1, 0);
    return SCEMA_MD_OK;
  };
  auto map_fault = [&](int fault) {
    if (const int rc = stage.faults(fault)) return rc;
    e->overflow_bits = (fault & 1) ? (1 | 8) : 0;
    return (fault & 1) ? SCEMA_MD_ERR_OVERFLOW : SCEMA_MD_OK;
  };
  return run_minimiser(e, order, maxatoms, spec, false, force, map_fault);
}

// Part batches: part 0 on the engine's main stream, the others on the streams the stage names (replicas are independent: each part runs its
// own sequence of steps, and one part's launch gaps, tails and latency-bound kernels are filled by the other's work)
int RowRun::make_parts(int nparts) {
  parts = split_parts(ns, nparts);
  parts[0].st = e->stream;
  if (nparts > 1) {
    if (const int rc = stage.part_streams(parts, done)) return rc;
    if (!e->row_fork) HIPCHK(hipEventCreateWithFlags(&e->row_fork, hipEventDisableTiming));
  }
  return fork_parts(e, parts, e->row_fork);
}

void RowRun::run_steps() {
  const FlipSchedule flip_at = flip_schedule(flips, e->h_sims);
  for (int step = 1; step <= maxsteps; step++) {
    bool any = false;
    for (size_t k = 0; k < parts.size(); k++) {
      const Part &pt = parts[k];
      const int na = active_prefix(e->h_sims, pt, step);
      if (na == 0) continue;
      any = true;
      const SimDev *Dh = D + pt.off;
      hipStream_t sh = pt.st;
      if (spec.nh) { mdk_pre_nh(sh, Dh, na); mdk_initial_integrate_nh(sh, Dh, na, maxatoms); }
      else { mdk_pre(sh, Dh, na); mdk_initial_integrate(sh, Dh, na, maxatoms); }
      stage.forces(sh, pt.off, na, step, (int)k);
      mdk_final_integrate(sh, Dh, na, maxatoms, 1);
      if (spec.nh) mdk_post_nh(sh, Dh, na);
      else mdk_post(sh, Dh, na);
      if (spec.deform) mdk_remap(sh, Dh, na, maxatoms);
      e->prof.md_steps += na;
    }
    if (!any) break;
    auto fl = flip_at.find(step);
    if (fl != flip_at.end())
      for (const auto &pk : fl->second) {
        const FlipEvent &fe = flips[pk.first][pk.second];
        hipStream_t fs = parts[part_of(parts, pk.first)].st;
        mdk_flip(fs, D + pk.first, fe.tilt[0], fe.tilt[1], fe.tilt[2]);
        stage.flipped(fs, pk.first, fe);
        e->prof.box_flips += 1;
      }
  }
}

int RowRun::read_scalars() {
  HIPCHK(hipMemcpyAsync(e->h_sc.data(), e->d_sc.p, (size_t)ns * sizeof(SimScalars), hipMemcpyDeviceToHost, e->stream));
  return SCEMA_MD_OK;
}

// the end of the run: join, scalars back, faults, the signatures of the rows that stand
int RowRun::finish() {
  hipStream_t st = e->stream;
  int rc = join_parts(e, parts, done.data());
  if (rc) return rc;
  mdk_phase_end(st, D, ns, maxatoms);
  if ((rc = stage.read_back())) return rc;
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  const int fault = collect_faults(e, ns);
  if (fault & 16) return fail(e, SCEMA_MD_ERR_ARG, "a simulation became unstable (non-finite or runaway atom positions): overlapping atoms or a time step too long");
  double need = 1.0;
  if ((rc = stage.after_read_back(fault, need))) return rc;
  e->overflow_need_j = 1.0;
  e->overflow_need_row = need;   // the largest demand / capacity the run saw: the retry grows by at least that (grow_after_overflow)
  e->overflow_bits = ((fault & 1) ? (1 | 8) : 0) | (fault & 64);
  if (fault & (1 | 64)) return SCEMA_MD_ERR_OVERFLOW;   // (64: the barostat took the box out of the range this segment was laid out for)
  lists_hold(e, sims, !spec.minimize, false);
  return SCEMA_MD_OK;
}

int run_rows(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec, RowStage &stage) {
  RowRun R(e, sims, spec, stage);
  const int nparts = stage.nparts();
  R.order = batch_order(sims, nparts);
  int rc;
  if ((rc = R.lay_out()) || (rc = R.setup_step())) return rc;
  if (spec.minimize) return R.minimise();
  if ((rc = R.make_parts(nparts))) return rc;
  R.run_steps();
  return R.finish();
}

}  // namespace scema_eng
