// engine_sw.cpp -- host side of the Stillinger-Weber path (`pair_style sw`: the reference's examples/streched_polyhedron): run_phase_sw and
// the SW entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// run_phase_sw is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the Stillinger-Weber force stage: no bonded terms either
// (lammps_scripts_sisw/in.strain.lammps has none).

RowMaterial *row_material(scema_md_engine *e, const std::string &matid, RowKind kind) {
  auto it = e->row_mats.find(matid);
  return it == e->row_mats.end() || it->second->kind != kind ? nullptr : it->second.get();
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
int ensure_swtype(scema_md_engine *e, Topo &T, const std::vector<int> &type_map, long long stamp, const char *what) {
  if (T.swtype_stamp == stamp && T.d_swtype.p) return SCEMA_MD_OK;
  std::vector<int> st(T.natoms);
  for (int i = 0; i < T.natoms; i++) {
    const int ty = T.original.type[i];   // the registered LAMMPS type (Topo::type holds Lennard-Jones classes)
    if (ty < 0 || ty >= (int)type_map.size())
      return fail(e, SCEMA_MD_ERR_ARG, "atom %d has type %d but the %s element list names %zu types (pair_coeff * * file ...)", i, ty + 1, what, type_map.size());
    st[i] = type_map[ty];
  }
  int rc = upload(e, T.d_swtype, st);
  if (rc) return rc;
  T.swtype_stamp = stamp;
  return SCEMA_MD_OK;
}

// ---- the row part the Stillinger-Weber, the Tersoff and the embedded-atom stage share (engine.h: SwRowsStage) ----

SwRowsStage::SwRowsStage(scema_md_engine *e_, int ns, RowKind kind_, const char *what_) : RowStage(kind_, 16), e(e_), what(what_) {
  e->h_swviews.assign(ns, SwView());
}

// Part batches: part 0 on the engine's main stream, part 1 on its third.  The split follows the other paths' shape, SCEMA_MD_SPLIT=0 /
// scema_md_batch_split(e, 0) runs the batch whole.
int SwRowsStage::nparts() const { return (e->split_streams && e->stream3 && run->ns >= 8 && !run->spec.minimize) ? 2 : 1; }

int SwRowsStage::rows(Topo &T, const BoxRange &R, RowNeed &need) {
  const RowMaterial &M = *row_material(e, T.matid, kind);
  if (const int rc = ensure_swtype(e, T, M.type_map, M.stamp, what)) return rc;
  const int n = T.natoms;
  if (n >= (1 << 24)) return fail(e, SCEMA_MD_ERR_ARG, "a %s replica of %d atoms: row entries hold 24-bit atom indices", what, n);
  const double rlist = M.cutmax + M.skin;
  // row capacity: the mean count inside the list radius at the densest box of the run, with headroom (grown after an overflow: grow_after_overflow)
  const double rho = n / R.vol_min;
  const int cap = (int)std::ceil(rho * 4.0 / 3.0 * MD_PI * rlist * rlist * rlist * 1.5 * e->neigh_grow);
  need.rlist = rlist; need.skin = M.skin; need.stamp = M.stamp;
  // (the floor of 8 entries grows with the same factor: a cluster in a large empty box has a mean density near zero, and a factor that
  // only multiplied `cap` would be swallowed by the floor -- 17 neighbours in a 30 A box were still not held after six attempts)
  const int floor8 = (int)std::ceil(8.0 * e->neigh_grow);
  need.cap[0] = std::max(8, (std::max(cap, floor8) + 7) / 8 * 8);
  return SCEMA_MD_OK;
}

int SwRowsStage::bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) {
  const Topo &T = *A.st->topo;
  const int npad = S.npad, cap = need.cap[0];
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
  SwView V;
  std::memset(&V, 0, sizeof V);
  for (int d = 0; d < 3; d++) V.mimg[d] = need.mimg[d];
  V.n = S.natoms; V.npad = npad; V.cap = cap; V.rlist = need.rlist;
  SWSET(V.stype, T.d_swtype.as<int>()); SWSET(V.x, S.x); SWSET(V.f, S.f);
  SWSET(V.cnt, W.cnt.as<int>()); SWSET(V.rows, W.rows.as<int>());
  SWSET(V.eacc, W.misc.as<double>());                 // [0, 4) doubles
  SWSET(V.stat, (int *)(W.misc.as<char>() + 32));     // 2 ints
  e->h_zerotab.push_back(MdkZero{W.misc.as<int>(), 16});   // (the step sums)
  SWSET(V.tab, row_material(e, T.matid, kind)->d_tab.p);
  e->h_swviews[pos] = V;
  return SCEMA_MD_OK;
}

int SwRowsStage::upload() {
  const size_t bytes = e->h_swviews.size() * sizeof(SwView);
  HIPCHK(e->d_swviews.ensure(bytes));
  HIPCHK(hipMemcpyAsync(e->d_swviews.p, e->h_swviews.data(), bytes, hipMemcpyHostToDevice, e->stream));
  VV = e->d_swviews.as<SwView>();
  return SCEMA_MD_OK;
}

int SwRowsStage::part_streams(std::vector<Part> &parts, std::vector<hipEvent_t> &done) {
  if (!e->sw_done) HIPCHK(hipEventCreateWithFlags(&e->sw_done, hipEventDisableTiming));
  parts[1].st = e->stream3;
  done.push_back(e->sw_done);
  return SCEMA_MD_OK;
}

int SwRowsStage::read_back() { return run->read_scalars(); }

int SwRowsStage::after_read_back(int fault, double &need) {
  for (int pos = 0; pos < run->ns; pos++)
    need = std::max(need, (double)e->h_sc[run->order[pos]].maxneigh_seen / (double)std::max(e->h_swviews[pos].cap, 1));
  return faults(fault);
}

int SwRowsStage::faults(int fault) {
  if (fault & 128) return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside the %s cutoff", SW_MAXIN, what);
  return SCEMA_MD_OK;
}

namespace {

struct SwStage : SwRowsStage {
  SwStage(scema_md_engine *e_, int ns) : SwRowsStage(e_, ns, RowKind::Sw, "Stillinger-Weber") {}
  void forces(hipStream_t st, int pos0, int n, int, int) override { mdk_sw_forces(st, run->D + pos0, VV + pos0, n, run->maxatoms); }
};

}  // namespace

int run_phase_sw(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  SwStage stage(e, (int)sims.size());
  return run_rows(e, sims, spec, stage);
}

// ---- the entry points of the C ABI the two potentials share ----

int row_configure(scema_md_engine *e, RowKind kind, const char *matid, const char *path, const char *const *elements, int32_t n_elements, double skin,
                  const RowTableReader &read) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid || !*matid || !path || !elements || n_elements <= 0) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  HIPCHK(hipSetDevice(e->p.device));
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  std::unique_ptr<RowMaterial> M(new RowMaterial());
  std::string err;
  RowTableBlock blk;
  if (!read(el, M->type_map, blk, err)) return fail(e, SCEMA_MD_ERR_IO, "%s", err.c_str());
  M->kind = kind;
  M->cutmax = blk.cutmax;
  M->skin = skin < 0.0 ? 1.0 : skin;
  M->stamp = ++e->sw_stamp;
  HIPCHK(M->d_tab.ensure(blk.bytes));
  HIPCHK(hipMemcpyAsync(M->d_tab.p, blk.p, blk.bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->row_mats[matid] = std::move(M);   // (the potential it replaces, of either kind, goes with its table: rows and element arrays carry its stamp and are rebuilt)
  return SCEMA_MD_OK;
}

// static evaluation of a state (qp_id SCEMA_MD_QP_NONE: the registered replica)
int row_debug_compute(scema_md_engine *e, RowKind kind, int32_t qp_id, const char *matid, int32_t replica, double *f, double *ea, double *eb,
                      double *virial, double *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  if (!row_material(e, matid, kind)) {
    if (kind == RowKind::Sw) return fail(e, SCEMA_MD_ERR_ARG, "no Stillinger-Weber potential attached to material %s (scema_md_sw_configure)", matid);
    if (kind == RowKind::Eam) return fail(e, SCEMA_MD_ERR_ARG, "no EAM potential attached to material %s (scema_md_eam_configure)", matid);
    return fail(e, SCEMA_MD_ERR_ARG, "no Tersoff potential attached to material %s (scema_md_tersoff_configure)", matid);
  }
  HIPCHK(hipSetDevice(e->p.device));
  State *s = nullptr;
  std::unique_ptr<State> tmp;
  int rc = debug_state(e, qp_id, matid, replica, &s, tmp);
  if (rc) return rc;
  RunSpec R;
  R.nvt = 0;
  R.static_only = 1;
  if ((rc = eval_static(e, s, R))) return rc;
  const int n = s->topo->natoms;
  const SimScalars &sc = e->h_sc[0];
  const SwView &V = e->h_swviews[0];
  double acc[4];
  HIPCHK(hipMemcpy(acc, (const void *)V.eacc, sizeof acc, hipMemcpyDeviceToHost));
  if (f) HIPCHK(hipMemcpy(f, e->slots[0]->f.p, 3 * (size_t)n * 8, hipMemcpyDeviceToHost));
  if (ea) *ea = acc[0];
  if (eb) *eb = acc[1];
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

}  // namespace scema_eng

extern "C" {

int scema_md_sw_configure(scema_md_engine *e, const char *matid, const char *sw_path, const char *const *elements, int32_t n_elements,
                          int32_t energy_unit, double skin) {
  SwTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_sw_params(sw_path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::Sw, matid, sw_path, elements, n_elements, skin, read);
}

int scema_md_sw_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3, double *virial,
                              double *info) {
  return row_debug_compute(e, RowKind::Sw, qp_id, matid, replica, f, e2, e3, virial, info);
}

}  // extern "C"
