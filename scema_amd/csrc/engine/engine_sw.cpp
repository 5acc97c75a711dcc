// engine_sw.cpp -- host side of the Stillinger-Weber path (`pair_style sw`: the reference's examples/streched_polyhedron): run_phase_sw and
// the SW entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// run_phase_sw is run_phase with another force stage, as run_phase_reax is: the same step sequence (k_pre, k_initial_integrate, forces,
// k_final_integrate, k_post, k_remap), the same batch rules (longest run first, active prefix, part batches), the same box flips; no cells,
// no k-space, no SHAKE, no bonded terms (lammps_scripts_sisw/in.strain.lammps has none of them).

SwMaterial *sw_material(scema_md_engine *e, const std::string &matid) {
  auto it = e->sw_mats.find(matid);
  return it == e->sw_mats.end() ? nullptr : it->second.get();
}

bool sw_bare_replica(const Topo &t) {
  const scema_md_system &s = t.original.sys;
  if (s.nbonds || s.nangles || s.ndihedrals || s.nimpropers) return false;
  for (double q : t.original.q) if (q != 0.0) return false;
  for (double v : t.original.eps) if (v != 0.0) return false;
  return true;
}

#define SWSET(dst, src) dst = (decltype(dst))(src)

// element of every atom of a replica: the element pair_coeff names for its LAMMPS type
static int ensure_swtype(scema_md_engine *e, Topo &T, const SwMaterial &M) {
  if (T.swtype_stamp == M.stamp && T.d_swtype.p) return SCEMA_MD_OK;
  std::vector<int> st(T.natoms);
  for (int i = 0; i < T.natoms; i++) {
    const int ty = T.original.type[i];   // the registered LAMMPS type (Topo::type holds Lennard-Jones classes)
    if (ty < 0 || ty >= (int)M.type_map.size())
      return fail(e, SCEMA_MD_ERR_ARG, "atom %d has type %d but the Stillinger-Weber element list names %zu types (pair_coeff * * file ...)", i, ty + 1, M.type_map.size());
    st[i] = M.type_map[ty];
  }
  int rc = upload(e, T.d_swtype, st);
  if (rc) return rc;
  T.swtype_stamp = M.stamp;
  return SCEMA_MD_OK;
}

namespace {

struct SwRun {
  scema_md_engine *e;
  std::vector<ActiveSim> &sims;
  const RunSpec &spec;
  const int ns;
  std::vector<int> order;
  std::vector<std::vector<FlipEvent>> flips;   // by position
  int maxatoms = 0, maxsteps = 0;
  bool any_validate = false;
  const SimDev *D = nullptr;
  SwView *VV = nullptr;
  std::vector<Part> parts;

  SwRun(scema_md_engine *e_, std::vector<ActiveSim> &sims_, const RunSpec &spec_) : e(e_), sims(sims_), spec(spec_), ns((int)sims_.size()), flips(sims_.size()) {}

  int lay_out();
  int lay_out_sim(int pos);
  int setup_step();
  int minimise();
  int make_parts(int nparts);
  void run_steps();
  int finish();
};

// The replica at position pos of the launch order: box range, images, row capacity, its slot, its SimDev and SwView
int SwRun::lay_out_sim(int pos) {
  const int i = order[pos];
  ActiveSim &A = sims[i];
  Topo &T = *A.st->topo;
  SwMaterial &M = *sw_material(e, T.matid);
  int rc = ensure_swtype(e, T, M);
  if (rc) return rc;
  const SimScalars &hsc = e->h_sc[i];
  BoxRange R;
  if (!box_range(spec, A, hsc.box, R, flips[pos]))
    return fail(e, SCEMA_MD_ERR_BOX, "fix deform is changing yz too much with xy: the strain would tilt yz past half the box");
  const double rlist = M.tab.cutmax + M.skin;
  SimDev S;
  std::memset(&S, 0, sizeof S);
  SwView V;
  std::memset(&V, 0, sizeof V);
  bool small = false;
  for (int d = 0; d < 3; d++) small = small || R.w[d] < 2.0 * rlist;
  for (int d = 0; d < 3; d++) {
    V.mimg[d] = small ? (int)std::ceil(rlist / R.w[d]) : 0;
    if (V.mimg[d] > 2) return fail(e, SCEMA_MD_ERR_BOX, "box width %.3f < (cutoff+skin)/2 = %.3f in dim %d", R.w[d], 0.5 * rlist, d);
  }
  const int n = T.natoms, npad = (n + 63) / 64 * 64;
  if (n >= (1 << 24)) return fail(e, SCEMA_MD_ERR_ARG, "a Stillinger-Weber replica of %d atoms: row entries hold 24-bit atom indices", n);
  // row capacity: the mean count inside the list radius at the densest box of the run, with headroom (x 1.5 per overflow: eval_chunk)
  const double rho = n / R.vol_min;
  int cap = (int)std::ceil(rho * 4.0 / 3.0 * MD_PI * rlist * rlist * rlist * 1.5 * e->neigh_grow);
  cap = std::max(8, (cap + 7) / 8 * 8);
  Slot &sl = *e->slots[i];
  // a run that follows another SW run of the same state on the same slot keeps that run's rows, as the other two paths do (run_phase,
  // run_phase_reax): k_phase_init / k_keep_validate decide on the device whether they still hold.  The rows keep their capacity.
  bool keep = false;
  {
    const ListSig &g = sl.sig;
    if (spec.keep_list && keep_list_switch() && g.valid && g.sw_stamp != 0 && g.sw_stamp == M.stamp && g.topo == T.id && g.rlist == rlist && g.npad == npad &&
        (spec.keep_list == 1 || g.state == A.st->id) && !hsc.force_rebuild && !hsc.overflow && cap <= g.maxneigh && g.rx_mimg[0] == V.mimg[0] &&
        g.rx_mimg[1] == V.mimg[1] && g.rx_mimg[2] == V.mimg[2] && sl.sw) {
      keep = true;
      cap = g.maxneigh;
    }
  }
  S.keep_list = keep ? spec.keep_list : 0;
  any_validate = any_validate || S.keep_list == 2;
  {
    ListSig &g = sl.sig;   // what this run's rows are built for; valid once the run has ended without a fault
    g.valid = false;
    g.rx_stamp = -1;   // (neither OPLS rows, 0, nor rows of a ReaxFF stamp)
    g.sw_stamp = M.stamp;
    g.topo = T.id;
    g.rlist = rlist; g.npad = npad; g.maxneigh = cap; g.capj = 0;
    for (int d = 0; d < 3; d++) g.rx_mimg[d] = V.mimg[d];
  }
  rc = ensure_slot(e, sl, n, 64, 1, 0, 64);
  if (rc) return rc;
  if (!sl.sw) sl.sw.reset(new SwSlot());
  SwSlot &W = *sl.sw;
  if (npad > W.cap_pad) {
    HIPCHK(W.cnt.ensure((size_t)npad * 4));
    HIPCHK(W.misc.ensure(64));
    W.cap_pad = npad;
    W.cap_rows = 0;
  }
  if ((size_t)npad * cap > W.cap_rows) {
    HIPCHK(W.rows.ensure((size_t)npad * cap * 4));
    W.cap_rows = (size_t)npad * cap;
  }
  sim_common(S, e->p, spec, A, sl, e->d_sc.as<SimScalars>() + i);
  S.natoms = n; S.npad = npad; S.ntypes = T.ntypes;
  S.use_shake = 0;
  if (spec.minimize) S.min_incremental = 1;   // the neighbour rebuild wraps the atoms into the box: trial points by increments
  S.neigh_delay = 0;   // neigh_modify every 1 delay 0 check yes (lammps_scripts_sisw/in.set.lammps)
  S.tdof = 3.0 * n - 3.0;
  S.skin = M.skin;
  S.far_band = M.skin;
  V.n = n; V.npad = npad; V.cap = cap; V.rlist = rlist;
  SWSET(V.stype, T.d_swtype.as<int>()); SWSET(V.tab, M.d_tab.as<SwTable>()); SWSET(V.x, S.x); SWSET(V.f, S.f);
  SWSET(V.cnt, W.cnt.as<int>()); SWSET(V.rows, W.rows.as<int>());
  SWSET(V.eacc, W.misc.as<double>());                 // [0, 4) doubles
  SWSET(V.stat, (int *)(W.misc.as<char>() + 32));     // 2 ints
  e->h_zerotab.push_back(MdkZero{sl.wrapn.as<int>(), 3 * (long long)n});
  e->h_zerotab.push_back(MdkZero{W.misc.as<int>(), 16});
  e->h_sims[pos] = S;
  e->h_swviews[pos] = V;
  maxatoms = std::max(maxatoms, n); maxsteps = std::max(maxsteps, A.nsteps);
  return SCEMA_MD_OK;
}

int SwRun::lay_out() {
  e->h_sims.assign(ns, SimDev());
  e->h_swviews.assign(ns, SwView());
  e->h_zerotab.clear();
  for (int pos = 0; pos < ns; pos++)
    if (const int rc = lay_out_sim(pos)) return rc;
  HIPCHK(e->d_sims.ensure((size_t)ns * sizeof(SimDev)));
  HIPCHK(e->d_swviews.ensure((size_t)ns * sizeof(SwView)));
  HIPCHK(hipMemcpyAsync(e->d_sims.p, e->h_sims.data(), (size_t)ns * sizeof(SimDev), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->d_swviews.p, e->h_swviews.data(), (size_t)ns * sizeof(SwView), hipMemcpyHostToDevice, e->stream));
  // the wrap counters and the step sums of every replica start from zero: one launch
  HIPCHK(e->d_zerotab.ensure(e->h_zerotab.size() * sizeof(MdkZero)));
  HIPCHK(hipMemcpyAsync(e->d_zerotab.p, e->h_zerotab.data(), e->h_zerotab.size() * sizeof(MdkZero), hipMemcpyHostToDevice, e->stream));
  mdk_zero_many(e->stream, e->d_zerotab.as<MdkZero>(), (int)e->h_zerotab.size(), 3 * (long long)maxatoms + 16);
  D = e->d_sims.as<SimDev>();
  VV = e->d_swviews.as<SwView>();
  return SCEMA_MD_OK;
}

// step 0 of the whole batch on the main stream
int SwRun::setup_step() {
  hipStream_t st = e->stream;
  mdk_phase_init(st, D, ns);
  if (any_validate) mdk_keep_validate(st, D, ns, maxatoms);
  mdk_sw_forces(st, D, VV, ns, maxatoms);
  mdk_final_integrate(st, D, ns, maxatoms, 0);
  if (spec.nh) mdk_setup_post_nh(st, D, ns);
  else mdk_setup_post(st, D, ns);
  return SCEMA_MD_OK;
}

// min_style sd (md_equil.hip): the line search of every replica on the device, forces from the SW stage
int SwRun::minimise() {
  auto force = [&] {
    mdk_sw_forces(e->stream, D, VV, ns, maxatoms);
    return SCEMA_MD_OK;
  };
  auto map_fault = [&](int fault) {
    if (fault & 128) return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside the Stillinger-Weber cutoff", SW_MAXIN);
    e->overflow_bits = (fault & 1) ? (1 | 8) : 0;
    return (fault & 1) ? SCEMA_MD_ERR_OVERFLOW : SCEMA_MD_OK;
  };
  return run_minimiser(e, order, maxatoms, spec, false, force, map_fault);
}

// Part batches: part 0 on the engine's main stream, part 1 on its third (replicas are independent: one part's launch gaps and tails are
// filled by the other's work).  Not measured yet for this force stage: the split follows the other paths' shape, SCEMA_MD_SPLIT=0 /
// scema_md_batch_split(e, 0) runs the batch whole.
int SwRun::make_parts(int nparts) {
  parts = split_parts(ns, nparts);
  parts[0].st = e->stream;
  if (nparts > 1) {
    parts[1].st = e->stream3;
    if (!e->sw_fork) HIPCHK(hipEventCreateWithFlags(&e->sw_fork, hipEventDisableTiming));
    if (!e->sw_done) HIPCHK(hipEventCreateWithFlags(&e->sw_done, hipEventDisableTiming));
  }
  return fork_parts(e, parts, e->sw_fork);
}

void SwRun::run_steps() {
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
      mdk_sw_forces(sh, Dh, VV + pt.off, na, maxatoms);
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
        mdk_flip(parts[part_of(parts, pk.first)].st, D + pk.first, fe.tilt[0], fe.tilt[1], fe.tilt[2]);
        e->prof.box_flips += 1;
      }
  }
}

// the end of the run: join, scalars back, faults, the signatures of the rows that stand
int SwRun::finish() {
  hipStream_t st = e->stream;
  int rc = join_parts(e, parts, &e->sw_done);
  if (rc) return rc;
  mdk_phase_end(st, D, ns, maxatoms);
  HIPCHK(hipMemcpyAsync(e->h_sc.data(), e->d_sc.p, (size_t)ns * sizeof(SimScalars), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  const int fault = collect_faults(e, ns);
  if (fault & 16) return fail(e, SCEMA_MD_ERR_ARG, "a simulation became unstable (non-finite or runaway atom positions): overlapping atoms or a time step too long");
  if (fault & 128) return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside the Stillinger-Weber cutoff", SW_MAXIN);
  if (fault & 1) {
    // the largest demand / capacity the run saw: the retry grows by at least that (eval_chunk)
    double need = 1.0;
    for (int pos = 0; pos < ns; pos++) need = std::max(need, (double)e->h_sc[order[pos]].maxneigh_seen / (double)std::max(e->h_swviews[pos].cap, 1));
    e->overflow_need_row = need;
    e->overflow_bits = (1 | 8) | (fault & 64);
    return SCEMA_MD_ERR_OVERFLOW;
  }
  e->overflow_bits = fault & 64;
  if (fault & 64) return SCEMA_MD_ERR_OVERFLOW;   // the barostat took the box out of the range this segment was laid out for
  lists_hold(e, sims, !spec.minimize, false);
  return SCEMA_MD_OK;
}

}  // namespace

int run_phase_sw(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  SwRun R(e, sims, spec);
  const int nparts = (e->split_streams && e->stream3 && R.ns >= 8 && !spec.minimize) ? 2 : 1;
  R.order = batch_order(sims, nparts);
  int rc;
  if ((rc = R.lay_out()) || (rc = R.setup_step())) return rc;
  if (spec.minimize) return R.minimise();
  if ((rc = R.make_parts(nparts))) return rc;
  R.run_steps();
  return R.finish();
}

}  // namespace scema_eng

extern "C" {

int scema_md_sw_configure(scema_md_engine *e, const char *matid, const char *sw_path, const char *const *elements, int32_t n_elements,
                          int32_t energy_unit, double skin) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid || !*matid || !sw_path || !elements || n_elements <= 0) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  HIPCHK(hipSetDevice(e->p.device));
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  std::unique_ptr<SwMaterial> M(new SwMaterial());
  std::string err;
  if (!scema::read_sw_params(sw_path, el, energy_unit, M->tab, M->type_map, err)) return fail(e, SCEMA_MD_ERR_IO, "%s", err.c_str());
  M->skin = skin < 0.0 ? 1.0 : skin;
  M->stamp = ++e->sw_stamp;
  HIPCHK(M->d_tab.ensure(sizeof(SwTable)));
  HIPCHK(hipMemcpyAsync(M->d_tab.p, &M->tab, sizeof(SwTable), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->sw_mats[matid] = std::move(M);   // (a potential it replaces goes with its table: rows and element arrays carry its stamp and are rebuilt)
  return SCEMA_MD_OK;
}

// static evaluation of a state (qp_id SCEMA_MD_QP_NONE: the registered replica)
int scema_md_sw_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3, double *virial,
                              double *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  if (!sw_material(e, matid)) return fail(e, SCEMA_MD_ERR_ARG, "no Stillinger-Weber potential attached to material %s (scema_md_sw_configure)", matid);
  HIPCHK(hipSetDevice(e->p.device));
  State *s = nullptr;
  std::unique_ptr<State> tmp;
  int rc = debug_state(e, qp_id, matid, replica, &s, tmp);
  if (rc) return rc;
  std::vector<ActiveSim> sims(1);
  sims[0].st = s;
  sims[0].nsteps = 0;
  sims[0].dt = 1.0;
  sims[0].temperature = 300.0;
  for (int attempt = 0; attempt < 6; attempt++) {
    if ((rc = prepare_slots(e, sims))) break;
    RunSpec R;
    R.nvt = 0;
    R.static_only = 1;
    rc = run_phase(e, sims, R);
    if (rc != SCEMA_MD_ERR_OVERFLOW) break;
    e->neigh_grow *= std::max(1.5, std::min(8.0, 1.1 * e->overflow_need_row));
  }
  if (rc) return rc;
  const int n = s->topo->natoms;
  const SimScalars &sc = e->h_sc[0];
  const SwView &V = e->h_swviews[0];
  double acc[4];
  HIPCHK(hipMemcpy(acc, (const void *)V.eacc, sizeof acc, hipMemcpyDeviceToHost));
  if (f) HIPCHK(hipMemcpy(f, e->slots[0]->f.p, 3 * (size_t)n * 8, hipMemcpyDeviceToHost));
  if (e2) *e2 = acc[0];
  if (e3) *e3 = acc[1];
  if (virial)
    for (int k = 0; k < 6; k++) {
      virial[k] = 0.0;
      for (int p = 0; p < MD_NPART; p++) virial[k] += sc.vir[p * 6 + k];
    }
  if (info) {
    info[0] = sc.maxneigh_seen;
    info[1] = V.cap;
    info[2] = acc[2];
    info[3] = acc[3];
  }
  return SCEMA_MD_OK;
}

}  // extern "C"
