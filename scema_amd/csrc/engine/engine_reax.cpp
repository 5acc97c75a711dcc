// engine_reax.cpp -- host side of the ReaxFF path (force_field "reax"): run_phase_reax and the ReaxFF entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// run_phase_reax is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the ReaxFF force stage.

// (the pointers of RxView are qualified as global-memory pointers in device code, reax/rx_types.h: a cast in both passes of the compiler)
#define RXSET(dst, src) dst = (decltype(dst))(src)
static int ensure_rx_slot(scema_md_engine *e, RxSlot &r, int n, int npad, int maxnb, int maxbd, int maxnbn, bool col16) {
  if (npad > r.cap_pad) {
    HIPCHK(r.nb_cnt.ensure((size_t)npad * 4));
    HIPCHK(r.bd_cnt.ensure((size_t)npad * 4));
    HIPCHK(r.deltap.ensure((size_t)npad * 8));
    HIPCHK(r.total_bo.ensure((size_t)npad * 8));
    HIPCHK(r.cd_delta.ensure((size_t)npad * 8));
    HIPCHK(r.hd.ensure((size_t)npad * 8));
    HIPCHK(r.q.ensure((size_t)npad * 8));
    HIPCHK(r.s.ensure((size_t)npad * 8));
    HIPCHK(r.t.ensure((size_t)npad * 8));
    HIPCHK(r.s_hist.ensure(4 * (size_t)npad * 8));
    HIPCHK(r.t_hist.ensure(3 * (size_t)npad * 8));
    HIPCHK(r.qwork.ensure(10 * (size_t)npad * 8));
    HIPCHK(r.qpart.ensure((10 * (size_t)((npad + 255) / 256) + 2 * (size_t)(npad / RX_SWR + 1)) * 8));   // layout: md_reax.hip
    HIPCHK(r.pm_len.ensure((size_t)npad * 4));
    HIPCHK(r.pm_col.ensure((size_t)RX_PM_MAX * npad * 4));
    HIPCHK(r.pm_raw.ensure((size_t)RX_PM_MAX * npad * 8));
    HIPCHK(r.pm_val.ensure((size_t)RX_PM_MAX * npad * 8));
    HIPCHK(r.nbn_cnt.ensure((size_t)npad * 4));
    HIPCHK(r.hlen.ensure((size_t)npad * 4));
    HIPCHK(r.hownlen.ensure((size_t)npad * 4));
    HIPCHK(r.nb_own0.ensure((size_t)npad * 4));
    HIPCHK(r.misc.ensure(256));
    r.cap_pad = npad;
    r.cap_nb = 0;
    r.cap_bd = 0;
    r.cap_nbn = 0;
  }
  if (maxnbn > r.cap_nbn) {
    HIPCHK(r.nbn.ensure((size_t)maxnbn * npad * 4));
    HIPCHK(r.nbnT.ensure((size_t)maxnbn * npad * 4));
    r.cap_nbn = maxnbn;
  }
  if (maxnb > r.cap_nb) {
    HIPCHK(r.hval.ensure((size_t)maxnb * npad * 8));
    HIPCHK(r.nbT.ensure((size_t)maxnb * npad * 4));
    HIPCHK(r.hown.ensure((size_t)maxnb * npad * 4));
    r.cap_nb = maxnb;
  }
  if (!col16 && (size_t)r.cap_nb * npad > r.cap_col) {   // (32-bit columns beside the values: replicas of more than 65 536 atoms only)
    HIPCHK(r.hcol.ensure((size_t)r.cap_nb * npad * 4));
    r.cap_col = (size_t)r.cap_nb * npad;
  }
  if (maxbd > r.cap_bd) {
    const size_t plane = (size_t)maxbd * npad;
    HIPCHK(r.bd.ensure(plane * 4));
    HIPCHK(r.bd_rev.ensure(plane * 4));
    HIPCHK(r.bd_bop.ensure(4 * plane * 8));
    HIPCHK(r.bd_c.ensure(3 * plane * 8));
    HIPCHK(r.bd_bo.ensure(3 * plane * 8));
    HIPCHK(r.bd_g.ensure(3 * plane * 8));
    HIPCHK(r.bd_cb.ensure(plane * 8));
    r.cap_bd = maxbd;
  }
  (void)n;
  return SCEMA_MD_OK;
}

// force-field type of every atom of a replica: element of its LAMMPS type as pair_coeff names them
static int ensure_rtype(scema_md_engine *e, Topo &T) {
  if (T.rtype_stamp == e->rx_stamp && T.d_rtype.p) return SCEMA_MD_OK;
  std::vector<int> rt(T.natoms);
  for (int i = 0; i < T.natoms; i++) {
    const int ty = T.original.type[i];   // the registered LAMMPS type (Topo::type holds Lennard-Jones classes)
    if (ty < 0 || ty >= (int)e->rx_type_map.size())
      return fail(e, SCEMA_MD_ERR_ARG, "atom %d has type %d but the ReaxFF element list names %zu types (pair_coeff * * ffield ...)", i, ty + 1, e->rx_type_map.size());
    rt[i] = e->rx_type_map[ty];
  }
  int rc = upload(e, T.d_rtype, rt);
  if (rc) return rc;
  T.rtype_stamp = e->rx_stamp;
  return SCEMA_MD_OK;
}

namespace {

// many device-to-device copies in one launch, from a table that lives on the host only until the launch is issued
int copy_many(scema_md_engine *e, const std::vector<MdkCopy> &tab, long long maxn) {
  HIPCHK(e->d_copytab.ensure(tab.size() * sizeof(MdkCopy)));
  HIPCHK(hipMemcpyAsync(e->d_copytab.p, tab.data(), tab.size() * sizeof(MdkCopy), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));   // (the table is a local)
  mdk_copy_many(e->stream, e->d_copytab.as<MdkCopy>(), (int)tab.size(), maxn);
  return SCEMA_MD_OK;
}

struct RxStage : RowStage {
  scema_md_engine *e;
  const double rlist;
  double rnear = 0.0;   // the widest near row of the force field sizes the near rows
  bool col16 = true;    // columns of the charge-equilibration matrix as 16-bit atom indices (every replica of the batch has at most 65 536 atoms)
  bool all_sym = false, any_precond = false, any_cold = false, inject_precond_failure = false;
  RxView *VV = nullptr;
  const RxParams *RP = nullptr;
  std::vector<hipEvent_t> *evp = nullptr;
  size_t ev_used = 0;
  bool overlap = false;
  std::vector<RxSide> sides;     // per part: its side stream for the bond-order chain and the events around it

  RxStage(scema_md_engine *e_, const std::vector<ActiveSim> &sims) : RowStage(RowKind::Reax, 0), e(e_), rlist(e_->rx_host.swb + e_->rx_skin) {
    e->h_rxviews.assign(sims.size(), RxView());
    for (int k = 0; k < RX_MAXT * RX_MAXT; k++) rnear = std::max(rnear, std::sqrt(e->rx_host.rnear2[k]));
    col16 = !(scema_env("SCEMA_MD_RX_COL32") && atoi(scema_env("SCEMA_MD_RX_COL32")) != 0);   // (test switch: 32-bit columns for any size)
    for (const ActiveSim &A : sims) col16 = col16 && A.st->topo->natoms <= 65536;
    all_sym = col16 && e->rx_sym;
  }

  // (From six replicas per part on: 8 / 10 replicas whole 494 / 595 evaluations/s, as two parts 460 / 564; 12 / 16 / 18 replicas 617 / 776 / 847
  // whole, 661 / 852 / 910 as two.  Three and four parts lose at every size -- each part has a side stream too, and a process has four hardware
  // queues: 36 replicas 1 171 as two parts, 902 as three.  profiles/r06_x_reax_parts_ab.log)
  int nparts() const override { return (e->rx_halves >= 2 && run->ns >= 6 * e->rx_halves && !run->spec.minimize) ? e->rx_halves : 1; }

  int rows(Topo &T, const BoxRange &R, RowNeed &need) override {
    if (const int rc = ensure_rtype(e, T)) return rc;
    const double rho = T.natoms / R.vol_min;
    const int maxnb = (int)std::ceil(rho * 4.0 / 3.0 * MD_PI * rlist * rlist * rlist * 1.2 * e->neigh_grow) + 32;
    const int maxnbn = (int)std::ceil(rho * 4.0 / 3.0 * MD_PI * rnear * rnear * rnear * 1.5 * e->neigh_grow) + 32;
    need.rlist = rlist; need.skin = e->rx_skin; need.stamp = e->rx_stamp;
    need.cap[0] = (maxnb + 7) / 8 * 8;
    need.cap[1] = (maxnbn + 7) / 8 * 8;
    return SCEMA_MD_OK;
  }

  // rows, near rows, reference positions and the preconditioner live in the slot
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    const Topo &T = *A.st->topo;
    const int n = S.natoms, npad = S.npad, maxnb = need.cap[0], maxnbn = need.cap[1];
    const int maxbd = (int)std::ceil(24 * e->neigh_grow);
    if (!sl.rx) sl.rx.reset(new RxSlot());
    RxSlot &Rs = *sl.rx;
    if (const int rc = ensure_rx_slot(e, Rs, n, npad, maxnb, maxbd, maxnbn, col16)) return rc;
    RxView V;
    std::memset(&V, 0, sizeof V);
    for (int d = 0; d < 3; d++) V.mimg[d] = need.mimg[d];
    V.n = n; V.npad = npad; V.maxnb = maxnb; V.maxbd = maxbd;
    RXSET(V.rtype, T.d_rtype.as<int>()); RXSET(V.x, S.x); RXSET(V.q, Rs.q.as<double>());
    RXSET(V.nbn_cnt, Rs.nbn_cnt.as<int>()); RXSET(V.nbn, Rs.nbn.as<int>()); RXSET(V.nbnT, Rs.nbnT.as<int>()); V.maxnbn = maxnbn; V.rnear2 = rnear * rnear;
    RXSET(V.qpart, Rs.qpart.as<double>());
    RXSET(V.nb_cnt, Rs.nb_cnt.as<int>()); RXSET(V.nb, (int *)nullptr); RXSET(V.bd_cnt, Rs.bd_cnt.as<int>()); RXSET(V.bd, Rs.bd.as<int>()); RXSET(V.bd_rev, Rs.bd_rev.as<int>());
    RXSET(V.bd_bop, Rs.bd_bop.as<double>()); RXSET(V.bd_c, Rs.bd_c.as<double>()); RXSET(V.bd_bo, Rs.bd_bo.as<double>()); RXSET(V.bd_g, Rs.bd_g.as<double>()); RXSET(V.bd_cb, Rs.bd_cb.as<double>());
    RXSET(V.deltap, Rs.deltap.as<double>()); RXSET(V.total_bo, Rs.total_bo.as<double>()); RXSET(V.cd_delta, Rs.cd_delta.as<double>()); RXSET(V.hd, Rs.hd.as<double>());
    RXSET(V.f, S.f); RXSET(V.hval, col16 ? nullptr : Rs.hval.as<double>()); RXSET(V.hpk, col16 ? Rs.hval.as<unsigned long long>() : nullptr); RXSET(V.s, Rs.s.as<double>()); RXSET(V.t, Rs.t.as<double>());
    V.warm = (run->spec.qeq_continue || A.st->qhist_valid) ? 1 : 0;
    RXSET(V.hcol16, (unsigned short *)nullptr); RXSET(V.hcol32, col16 ? nullptr : Rs.hcol.as<int>()); RXSET(V.hlen, Rs.hlen.as<int>()); RXSET(V.nbT, Rs.nbT.as<int>());
    RXSET(V.hown, Rs.hown.as<int>()); RXSET(V.hownlen, Rs.hownlen.as<int>()); RXSET(V.nb_own0, Rs.nb_own0.as<int>());
    RXSET(V.s_hist, Rs.s_hist.as<double>()); RXSET(V.t_hist, Rs.t_hist.as<double>()); RXSET(V.qwork, Rs.qwork.as<double>());
    // the bonded-pattern preconditioner needs one image per neighbour (boxes at least two list radii wide: every production replica)
    V.pm_on = (e->rx_precond && V.mimg[0] == 0 && V.mimg[1] == 0 && V.mimg[2] == 0) ? 1 : 0;
    if (V.pm_on && scema_env("SCEMA_MD_TEST_QEQ_PRECOND_FAILS")) inject_precond_failure = true;   // test hook: this run reports a solve that did not converge
    any_precond = any_precond || V.pm_on;
    // the symmetric form of the solve: rows sorted by partner (one image per neighbour), both vectors of the replica in a workgroup's LDS
    all_sym = all_sym && V.mimg[0] == 0 && V.mimg[1] == 0 && V.mimg[2] == 0 && 2 * (size_t)npad * 16 + 4096 <= 128 * 1024;
    RXSET(V.pm_len, Rs.pm_len.as<int>()); RXSET(V.pm_col, Rs.pm_col.as<int>()); RXSET(V.pm_raw, Rs.pm_raw.as<double>()); RXSET(V.pm_val, Rs.pm_val.as<double>());
    RXSET(V.eparts, Rs.misc.as<double>());                         // [0, 13) doubles
    RXSET(V.qstat, (int *)(Rs.misc.as<char>() + 128));             // 6 ints
    RXSET(V.overflow, (int *)(Rs.misc.as<char>() + 160));
    RXSET(V.sweep_acc, (long long *)(Rs.misc.as<char>() + 168));   // 2 x 8 bytes
    e->h_rxviews[pos] = V;
    return SCEMA_MD_OK;
  }

  int upload() override {
    const size_t bytes = e->h_rxviews.size() * sizeof(RxView);
    HIPCHK(e->d_rxviews.ensure(bytes));
    HIPCHK(hipMemcpyAsync(e->d_rxviews.p, e->h_rxviews.data(), bytes, hipMemcpyHostToDevice, e->stream));
    VV = e->d_rxviews.as<RxView>();
    RP = e->d_rxparams.as<RxParams>();
    return SCEMA_MD_OK;
  }

  // how a solve is issued (md_reax.h): as many iterations as the slowest solve of the last run took plus a margin; the first
  // solves of a run that has replicas without a history take longer
  RxQeqPlan plan_for(int step) const {
    RxQeqPlan pl;
    pl.launch = (step < 4 && any_cold) ? e->rx_qeq_launch_cold : e->rx_qeq_launch;
    pl.setup = step == 0 ? 1 : 0;
    pl.precond = any_precond ? 1 : 0;
    pl.sym = all_sym ? 1 : 0;
    return pl;
  }

  int setup() override {
    const int ns = run->ns;
    const RunSpec &spec = run->spec;
    evp = (e->p.profile != 0 && !spec.minimize) ? &e->ev_pool : nullptr;
    // Charge-equilibration history: kept in place when this run follows another one on the same slots; else a state that has run
    // before brings its own (one copy launch for the batch); the rest start from zeros like a new fix qeq/reax
    std::vector<MdkCopy> tab;
    long long maxn = 0;
    for (int pos = 0; pos < ns; pos++) {
      const ActiveSim &A = run->sims[run->order[pos]];
      const RxView &V = e->h_rxviews[pos];
      if (!V.warm) any_cold = true;
      if (spec.qeq_continue || !A.st->qhist_valid) continue;
      const long long np = V.npad;
      tab.push_back(MdkCopy{A.st->qhist.as<double>(), V.s_hist, 4 * np});
      tab.push_back(MdkCopy{A.st->qhist.as<double>() + 4 * np, V.t_hist, 3 * np});
      maxn = std::max(maxn, 4 * np);
    }
    if (!tab.empty())
      if (const int rc = copy_many(e, tab, maxn)) return rc;
    // the bond-order chain of the force stage on the engine's side stream, next to the charge chain (md_reax.hip); SCEMA_REAX_OVERLAP=0: one stream
    sides.assign(1, RxSide{e->stream2, e->ev_fork, e->ev_up, e->ev_join});
    overlap = e->stream2 && e->ev_up && e->rx_overlap;
    mdk_reax_phase_init(e->stream, VV, ns, run->maxpad);
    return SCEMA_MD_OK;
  }

  // (the first solves of a run start from an empty history: RX_QEQ_COLD in md_reax.hip, setup is solve 1)
  void forces(hipStream_t st, int pos0, int n, int step, int part) override {
    mdk_reax_forces(st, run->D + pos0, VV + pos0, RP, n, run->maxatoms, rlist, e->rx_qeq_tol, e->rx_qeq_maxiter, plan_for(step), e->rx_terms, col16, evp, &ev_used,
                    overlap ? &sides[part] : nullptr);
  }

  // Each part has its own side stream for the bond-order chain: part 0 on the engine's main and side streams, part 1 on stream3 and the
  // engine's fourth stream, further parts -- a measurement aid, two is the optimum -- on streams of their own (created once, kept).
  // SCEMA_REAX_HALVES=0: one.
  int part_streams(std::vector<Part> &parts, std::vector<hipEvent_t> &done) override {
    const int nparts = (int)parts.size();
    const int pool0 = (e->stream3 && e->rx_side1) ? 2 : 1;   // parts served without the pool
    while (nparts > pool0 && (int)e->rx_parts.size() < nparts - pool0) {
      scema_md_engine::RxPart pt;
      bool ok = hipStreamCreateWithFlags(&pt.main, hipStreamNonBlocking) == hipSuccess && hipStreamCreateWithFlags(&pt.side, hipStreamNonBlocking) == hipSuccess;
      for (int k = 0; k < 4 && ok; k++) ok = hipEventCreateWithFlags(&pt.ev[k], hipEventDisableTiming) == hipSuccess;
      if (!ok) return fail(e, SCEMA_MD_ERR_DEVICE, "could not create the streams of the ReaxFF part batches");
      e->rx_parts.push_back(pt);
    }
    sides.resize(nparts);
    for (int k = 1; k < nparts; k++) {
      if (k == 1 && pool0 == 2) {
        parts[k].st = e->stream3;
        sides[k] = RxSide{e->rx_side1, e->rx_side1_ev[0], e->rx_side1_ev[1], e->rx_side1_ev[2]};
        done.push_back(e->rx_side1_ev[3]);
      } else {
        const auto &pt = e->rx_parts[k - pool0];
        parts[k].st = pt.main;
        sides[k] = RxSide{pt.side, pt.ev[0], pt.ev[1], pt.ev[2]};
        done.push_back(pt.ev[3]);
      }
    }
    return SCEMA_MD_OK;
  }

  // charge history back to the states, the scalars, the solver statistics: in this order on the main stream
  int read_back() override {
    const int ns = run->ns;
    std::vector<MdkCopy> tab;   // the states keep the history for their next run (a failed update drops it: backup_states)
    long long maxn = 0;
    for (int pos = 0; pos < ns; pos++) {
      const ActiveSim &A = run->sims[run->order[pos]];
      const RxView &V = e->h_rxviews[pos];
      const long long np = V.npad;
      HIPCHK(A.st->qhist.ensure(7 * (size_t)np * 8));
      tab.push_back(MdkCopy{V.s_hist, A.st->qhist.as<double>(), 4 * np});
      tab.push_back(MdkCopy{V.t_hist, A.st->qhist.as<double>() + 4 * np, 3 * np});
      maxn = std::max(maxn, 4 * np);
      A.st->qhist_valid = true;
    }
    int rc;
    if ((rc = copy_many(e, tab, maxn)) || (rc = run->read_scalars())) return rc;
    // (the solver statistics of all replicas in ONE read-back: two small copies per replica were 2 x 72 launch gaps of 24 us per run)
    HIPCHK(e->d_rxstat.ensure(8 * (size_t)ns * sizeof(long long)));
    e->h_rxstat.assign(8 * (size_t)ns, 0);
    mdk_reax_collect_stats(e->stream, VV, ns, e->d_rxstat.as<long long>());
    HIPCHK(hipMemcpyAsync(e->h_rxstat.data(), e->d_rxstat.p, 8 * (size_t)ns * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    return SCEMA_MD_OK;
  }

  // (the rows' demand is not read back: need stays 1, the retry after an overflow grows by the fixed step)
  int after_read_back(int fault, double &) override {
    const int ns = run->ns;
    const long long *qs = e->h_rxstat.data();
    if (evp) {
      // the matrix sweep of the charge equilibration, the HBM-bound kernel of this path: HIP-event time of every launch, and what
      // the launches read by the algorithm: 8 bytes per stored matrix entry (value and 16-bit column in one word, RxView::hpk; 8 + 4 with 32-bit columns) and RX_SWEEP_ROW_BYTES per row,
      // for every replica and sweep it took part in (counted on the device, k_rx_qeq_finish)
      if (const int rc = sum_timed_launches(e, ev_used / 2, e->prof.rx_sweep_ms, e->prof.rx_sweep_launches, e->prof.rx_sweep_union_ms)) return rc;
      for (int pos = 0; pos < ns; pos++) {
        e->prof.rx_sweep_entries += (double)qs[8 * pos + 6];
        e->prof.rx_sweep_rows += (double)qs[8 * pos + 7];
      }
      e->prof.rx_sweep_col_bytes = col16 ? 0 : 4;   // (packed entries: the column rides in the value's word)
      e->prof.rx_sweep_symmetric = all_sym ? 1 : 0;
    }
    int most = 0, most_cold = 0;
    for (int i = 0; i < ns; i++) {
      e->rx_qeq_iters += (int)qs[8 * i];
      e->rx_qeq_solves += (int)qs[8 * i + 1] - (e->h_rxviews[i].warm ? RX_QEQ_COLD_SOLVES : 0);   // (a warm run starts its solve count past the cold ones)
      most = std::max(most, (int)qs[8 * i + 2]);
      most_cold = std::max(most_cold, (int)qs[8 * i + 5]);
      e->rx_qeq_slow += (int)qs[8 * i + 3];
    }
    // iterations issued as launches in the next run: what the slowest solve of this one needed (of all replicas and steps), plus one.  A launch
    // that finds every replica converged still costs its two kernels and their gaps (28 us); a replica that needs more than was issued
    // finishes in one workgroup (80 us per iteration).  Scan on the 72-replica set, slowest solve 15: 13 launches 543, 14: 591, 15: 603,
    // 16: 598, 18: 590 evaluations/s (tools/reax_launch_scan.sh, profiles/r04_zh_launch_scan.txt)
    if (!e->rx_qeq_launch_pinned) {
      // (the floor of 8 dated from the Jacobi preconditioner's 11 iterations per solve; with 3.9 per solve -- slowest 5 -- it issued 8: scan
      // with the round-5 preconditioner, 72 replicas: 3 launches 577, 4: 747, 5: 978, 6: 969, 7: 965, 8: 959 evaluations/s)
      if (most > 0) e->rx_qeq_launch = std::max(4, most + 1);
      if (most_cold > 0) e->rx_qeq_launch_cold = std::max(4, most_cold + 1);
    }
    return faults(fault | (inject_precond_failure ? 32 : 0));
  }

  int faults(int fault) override {
    if (fault & 32) {
      e->rx_qeq_failed = true;   // (eval_chunk retries once with the reference's Jacobi preconditioner if the approximate inverse was on)
      return fail(e, SCEMA_MD_ERR_ARG, "charge equilibration did not converge to %.1e in %d iterations", e->rx_qeq_tol, e->rx_qeq_maxiter);
    }
    return SCEMA_MD_OK;
  }
};

}  // namespace

int run_phase_reax(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  if (!e->rx_ready) return fail(e, SCEMA_MD_ERR_ARG, "force field 'reax' asked for but no ReaxFF force-field file is loaded (scema_md_reax_configure)");
  RxStage stage(e, sims);
  return run_rows(e, sims, spec, stage);
}

}  // namespace scema_eng

extern "C" {

// ---- ReaxFF path ----
// The reach of the uncorrected bond order of a type pair (rx_bond_prime_pair, reax/rx_core.h: three terms exp(p_a (r / r_x)^p_b) with p_a < 0 < p_b, each
// falling with r): the r at which it passes bo_cut, plus a margin that covers the difference between this libm evaluation and the kernels' own
// exp / log by orders of magnitude.  The exact test stays in the kernel; this only keeps hopeless candidates out of the near rows
// (a row of 105 candidates within 5 + 1 A of a polyethylene atom holds 30 within reach + 1 A).  Parameters that do not fall with r: no cut.
static double rx_bond_reach(const RxParams &P, int ti, int tj) {
  const RxSbp &si = P.sbp[ti], &sj = P.sbp[tj];
  const RxTbp &t = P.tbp[ti * RX_MAXT + tj];
  const bool on_s = si.r_s > 0.0 && sj.r_s > 0.0, on_p = si.r_pi > 0.0 && sj.r_pi > 0.0, on_pp = si.r_pi_pi > 0.0 && sj.r_pi_pi > 0.0;
  if ((on_s && !(t.p_bo1 < 0.0 && t.p_bo2 > 0.0)) || (on_p && !(t.p_bo3 < 0.0 && t.p_bo4 > 0.0)) || (on_pp && !(t.p_bo5 < 0.0 && t.p_bo6 > 0.0))) return RX_BOND_CUT;
  auto bo = [&](double r) {
    const double lr = std::log(r);
    double b = 0.0;
    if (on_s) b += (1.0 + P.bo_cut) * std::exp(t.p_bo1 * std::exp(t.p_bo2 * (lr - t.lr_s)));
    if (on_p) b += std::exp(t.p_bo3 * std::exp(t.p_bo4 * (lr - t.lr_p)));
    if (on_pp) b += std::exp(t.p_bo5 * std::exp(t.p_bo6 * (lr - t.lr_pp)));
    return b;
  };
  if (!(P.bo_cut > 0.0) || bo(RX_BOND_CUT) >= P.bo_cut) return RX_BOND_CUT;
  double lo = 1e-3, hi = RX_BOND_CUT;
  if (bo(lo) < P.bo_cut) return lo;
  for (int it = 0; it < 200 && hi - lo > 1e-12; it++) {
    const double mid = 0.5 * (lo + hi);
    (bo(mid) >= P.bo_cut ? lo : hi) = mid;
  }
  return std::min((double)RX_BOND_CUT, hi * (1.0 + 1e-6) + 1e-6);
}
static void rx_near_radii(RxParams &P, double skin) {
  const bool full = scema_env("SCEMA_MD_RX_NEAR_FULL") && atoi(scema_env("SCEMA_MD_RX_NEAR_FULL")) != 0;   // (test hook: every pair inside the bond cutoff)
  for (int a = 0; a < RX_MAXT; a++)
    for (int b = 0; b < RX_MAXT; b++) {
      const bool used = a < P.nt && b < P.nt;
      const double reach = !used ? 0.0 : full ? (double)RX_BOND_CUT : std::max(rx_bond_reach(P, a, b), rx_bond_reach(P, b, a));
      if (used && b >= a && scema_env("SCEMA_MD_TIMING")) fprintf(stderr, "[scema_md] reax types %d-%d: bond order below bo_cut beyond %.4f A\n", a, b, reach);
      P.rbond[a * RX_MAXT + b] = reach;
      const double rn = std::max(reach, (double)RX_PM_RADIUS) + skin;
      P.rnear2[a * RX_MAXT + b] = used ? rn * rn : 0.0;
    }
}

int scema_md_reax_configure(scema_md_engine *e, const char *ffield_path, const char *const *elements, int32_t n_elements, double qeq_tol, double skin) {
  if (!e || !ffield_path || !elements || n_elements <= 0) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  HIPCHK(hipSetDevice(e->p.device));
  std::vector<std::string> el(elements, elements + n_elements);
  std::string err;
  RxParams P;
  std::vector<int> map;
  if (!scema::read_reax_ffield(ffield_path, el, P, map, err)) return fail(e, SCEMA_MD_ERR_IO, "%s", err.c_str());
  if (const char *x = scema_env("SCEMA_REAX_DROP_DSBO2")) P.lammps_dsbo2 = atoi(x) ? 1 : 0;
  e->rx_host = P;
  e->rx_type_map = map;
  if (qeq_tol > 0.0) e->rx_qeq_tol = qeq_tol;
  if (skin >= 0.0) e->rx_skin = skin;
  if (const char *x = scema_env("SCEMA_REAX_SKIN")) e->rx_skin = atof(x);
  if (const char *x = scema_env("SCEMA_REAX_QEQ_LAUNCH")) { e->rx_qeq_launch = e->rx_qeq_launch_cold = std::max(0, atoi(x)); e->rx_qeq_launch_pinned = true; }
  rx_near_radii(e->rx_host, e->rx_skin);
  HIPCHK(e->d_rxparams.ensure(sizeof(RxParams)));
  HIPCHK(hipMemcpyAsync(e->d_rxparams.p, &e->rx_host, sizeof(RxParams), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->rx_ready = true;
  e->rx_stamp += 1;
  e->reax_active = true;
  return SCEMA_MD_OK;
}
int scema_md_reax_activate(scema_md_engine *e, int32_t on) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (on && !e->rx_ready) return fail(e, SCEMA_MD_ERR_ARG, "no ReaxFF force field loaded");
  e->reax_active = on != 0;
  return SCEMA_MD_OK;
}
int scema_md_reax_concurrency(scema_md_engine *e, int32_t halves, int32_t overlap) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (halves >= 0) e->rx_halves = std::min(halves, 8);
  if (overlap >= 0) e->rx_overlap = overlap != 0;
  return SCEMA_MD_OK;
}
int scema_md_batch_split(scema_md_engine *e, int32_t on) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (on >= 0) e->split_streams = on != 0;
  return SCEMA_MD_OK;
}
int scema_md_get_concurrency(const scema_md_engine *e, int32_t *out) {
  if (!e || !out) return SCEMA_MD_ERR_ARG;
  out[0] = e->split_streams ? 1 : 0;
  out[1] = e->rx_halves;
  out[2] = e->rx_overlap ? 1 : 0;
  return SCEMA_MD_OK;
}
int scema_md_pppm_tiling(scema_md_engine *e, int32_t mode, int32_t lds_bytes) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (mode < -1 || mode > 1) return fail(e, SCEMA_MD_ERR_ARG, "scema_md_pppm_tiling: mode %d (1 tiled kernels, 0 the kernels without LDS, -1 keeps)", mode);
  // the smallest brick there is: one x row of a mesh of two points (charge assignment)
  const int least = 2 * 8, most = 160 * 1024;
  if (lds_bytes < -1 || (lds_bytes > 0 && (lds_bytes < least || lds_bytes > most)))
    return fail(e, SCEMA_MD_ERR_ARG, "scema_md_pppm_tiling: an LDS budget of %d bytes (%d .. %d, 0 the device default, -1 keeps)", lds_bytes, least, most);
  if (mode >= 0) e->pppm_tile_mode = mode;
  if (lds_bytes >= 0) e->pppm_lds_bytes = lds_bytes;
  return SCEMA_MD_OK;
}
int scema_md_pppm_binning(scema_md_engine *e, int32_t mode) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (mode < -1 || mode > 2) return fail(e, SCEMA_MD_ERR_ARG, "scema_md_pppm_binning: mode %d (0 off, 1 wherever eligible, 2 by the launch policy, -1 keeps)", mode);
  if (mode >= 0) e->pppm_bin_mode = mode;
  return SCEMA_MD_OK;
}
int scema_md_bonded_grouping(scema_md_engine *e, int32_t mode) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (mode < -1 || mode > 1) return fail(e, SCEMA_MD_ERR_ARG, "scema_md_bonded_grouping: mode %d (0 one descriptor per term, 1 the grouped stream, -1 the default)", mode);
  e->bonded_group_mode = mode;
  return SCEMA_MD_OK;
}
int scema_md_pppm_force_layout(scema_md_engine *e, int32_t mode) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (mode < -1 || mode > 1) return fail(e, SCEMA_MD_ERR_ARG, "scema_md_pppm_force_layout: mode %d (0 the dense layout, 1 the stride rule, -1 the default)", mode);
  e->pppm_flayout_mode = mode < 0 ? 1 : mode;
  return SCEMA_MD_OK;
}
int scema_md_pppm_force_strides(const int32_t grid[3], int32_t lds_bytes, int32_t out[3]) {
  if (!grid || !out || grid[0] < 1 || grid[1] < 1 || grid[2] < 1 || lds_bytes < 0) return SCEMA_MD_ERR_ARG;
  const PppmFStride fs = pppm_fstride(grid[0], grid[1], grid[2], lds_bytes > 0 ? lds_bytes : (long long)mdk_pppm_lds_limit());
  if (fs.bytes > INT32_MAX) return SCEMA_MD_ERR_ARG;
  out[0] = fs.rs; out[1] = fs.ps; out[2] = (int32_t)fs.bytes;
  return SCEMA_MD_OK;
}
long long scema_md_pppm_binned_launches(const scema_md_engine *e) { return e ? e->pppm_binned_launches : -(long long)SCEMA_MD_ERR_ARG; }
int scema_md_pppm_paths(const scema_md_engine *e, int32_t out[8]) {
  if (!e || !out) return SCEMA_MD_ERR_ARG;
  for (int k = 0; k < 8; k++) out[k] = e->pppm_paths[k];
  return SCEMA_MD_OK;
}
int scema_md_pppm_tile_shape(const int32_t grid[3], int32_t lds_bytes, int32_t which, int32_t out[4]) {
  if (!grid || !out || grid[0] < 1 || grid[1] < 1 || grid[2] < 1 || lds_bytes < 0 || which < 0 || which > 1) return SCEMA_MD_ERR_ARG;
  const PppmTile t = pppm_tile_shape(grid[0], grid[1], grid[2], lds_bytes > 0 ? lds_bytes : (long long)mdk_pppm_lds_limit(), which);
  out[0] = t.by; out[1] = t.bz; out[2] = t.ty; out[3] = t.tz;
  return SCEMA_MD_OK;
}
int scema_md_pppm_plan_count(const scema_md_engine *e) { return e ? (int)e->pppm_plans.size() : -SCEMA_MD_ERR_ARG; }
int scema_md_reax_set(scema_md_engine *e, int32_t exact_gradient, int32_t terms, int32_t qeq_maxiter) {
  if (!e || !e->rx_ready) return fail(e, SCEMA_MD_ERR_ARG, "no ReaxFF force field loaded");
  HIPCHK(hipSetDevice(e->p.device));
  if (exact_gradient >= 0) {
    e->rx_host.lammps_dsbo2 = exact_gradient ? 0 : 1;
    HIPCHK(hipMemcpyAsync(e->d_rxparams.p, &e->rx_host, sizeof(RxParams), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if (terms >= 0) e->rx_terms = terms;
  if (qeq_maxiter > 0) e->rx_qeq_maxiter = qeq_maxiter;
  return SCEMA_MD_OK;
}
// static evaluation of a state (qp_id SCEMA_MD_QP_NONE: the registered replica): forces, the 13 energy parts, virial, charges
int scema_md_reax_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *eparts, double *virial,
                                double *q, double *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!e->rx_ready) return fail(e, SCEMA_MD_ERR_ARG, "no ReaxFF force field loaded");
  HIPCHK(hipSetDevice(e->p.device));
  State *s = nullptr;
  std::unique_ptr<State> tmp;
  int rc = debug_state(e, qp_id, matid, replica, &s, tmp);
  if (rc) return rc;
  const bool saved = e->reax_active;
  e->reax_active = true;
  const long long it0 = e->rx_qeq_iters;
  RunSpec R;
  R.nvt = 0;
  R.static_only = 1;
  rc = eval_static(e, s, R);
  e->reax_active = saved;
  if (rc) return rc;
  const int n = s->topo->natoms;
  const SimScalars &sc = e->h_sc[0];
  const RxView &V = e->h_rxviews[0];
  if (f) HIPCHK(hipMemcpy(f, e->slots[0]->f.p, 3 * (size_t)n * 8, hipMemcpyDeviceToHost));
  if (eparts) HIPCHK(hipMemcpy(eparts, V.eparts, RX_NPART * 8, hipMemcpyDeviceToHost));
  if (q) HIPCHK(hipMemcpy(q, V.q, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (virial)
    for (int k = 0; k < 6; k++) {
      virial[k] = 0.0;
      for (int p = 0; p < MD_NPART; p++) virial[k] += sc.vir[p * 6 + k];
    }
  if (info) {
    info[0] = sc.maxneigh_seen;
    info[1] = V.maxnb;
    info[2] = V.maxbd;
    info[3] = (double)(e->rx_qeq_iters - it0);
    info[4] = V.mimg[0] + V.mimg[1] + V.mimg[2];
    std::vector<int> bc(n);
    HIPCHK(hipMemcpy(bc.data(), V.bd_cnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    int mb = 0;
    for (int v : bc) mb = std::max(mb, v);
    info[5] = mb;
  }
  return SCEMA_MD_OK;
}
int scema_md_reax_stats(const scema_md_engine *e, double *out) {
  if (!e || !out) return SCEMA_MD_ERR_ARG;
  out[0] = (double)e->rx_qeq_iters;
  out[1] = (double)e->rx_qeq_solves;
  out[2] = e->rx_skin;
  out[3] = e->rx_qeq_tol;
  out[4] = (double)e->rx_qeq_slow;
  out[5] = (double)e->rx_qeq_launch;
  out[6] = (double)e->rx_precond_fallbacks;
  return SCEMA_MD_OK;
}

}  // extern "C"
