// engine_tersoff.cpp -- host side of the Tersoff path (`pair_style tersoff`): run_phase_tersoff and the Tersoff entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

#include <fstream>
#include <sstream>

namespace scema_eng {

// run_phase_tersoff is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the Tersoff force stage.  The row part of a
// replica's work set is an SwView over the slot's SwSlot (SwRowsStage, shared with the Stillinger-Weber stage: the rows are mdk_sw_rows');
// rows built for the other potential are never kept, the slot's ListSig carries RowKind::Tersoff and the material's stamp.

TsMaterial *ts_material(scema_md_engine *e, const std::string &matid) {
  auto it = e->ts_mats.find(matid);
  return it == e->ts_mats.end() ? nullptr : it->second.get();
}

#define TSSET(dst, src) dst = (decltype(dst))(src)

namespace {

// the row part is SwRowsStage (engine_sw.cpp); the stage adds the TsView of every position and its launch
struct TsStage : SwRowsStage {
  const TsMaterial *mat = nullptr;
  TsView *TT = nullptr;

  TsStage(scema_md_engine *e_, int ns) : SwRowsStage(e_, ns, RowKind::Tersoff, "Tersoff") { e->h_tsviews.assign(ns, TsView()); }

  Mat material(const Topo &T) override {
    mat = ts_material(e, T.matid);
    Mat M;
    M.cutmax = mat->tab.cutmax; M.skin = mat->skin; M.stamp = mat->stamp; M.type_map = &mat->type_map;
    return M;
  }

  int bind_view(int pos, SwView &) override {
    TSSET(e->h_tsviews[pos].tab, mat->d_tab.as<TsTable>());
    return SCEMA_MD_OK;
  }

  int upload_views() override {
    const size_t bytes = e->h_tsviews.size() * sizeof(TsView);
    HIPCHK(e->d_tsviews.ensure(bytes));
    HIPCHK(hipMemcpyAsync(e->d_tsviews.p, e->h_tsviews.data(), bytes, hipMemcpyHostToDevice, e->stream));
    TT = e->d_tsviews.as<TsView>();
    return SCEMA_MD_OK;
  }

  void forces(hipStream_t st, int pos0, int n, int, int) override { mdk_ts_forces(st, run->D + pos0, VV + pos0, TT + pos0, n, run->maxatoms); }
};

}  // namespace

int run_phase_tersoff(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  TsStage stage(e, (int)sims.size());
  return run_rows(e, sims, spec, stage);
}

// The one line of in.strain.lammps that names a Tersoff file -- `pair_coeff * * ${locs}/<name>.tersoff <El> ...`, ${locs} being the scripts
// folder -- parsed as LAMMPS would: words separated by blanks, `#` starts a comment.  Nothing else of the script is read.
int tersoff_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  const std::string script = folder + "/in.strain.lammps";
  std::ifstream in(script);
  if (!in) return SCEMA_MD_OK;
  std::string line;
  for (int ln = 1; std::getline(in, line); ln++) {
    const size_t h = line.find('#');
    if (h != std::string::npos) line.resize(h);
    std::istringstream ss(line);
    std::vector<std::string> w;
    for (std::string s; ss >> s;) w.push_back(s);
    if (w.empty() || w[0] != "pair_coeff") continue;
    const std::string ext = ".tersoff", locs = "${locs}/";
    bool names = false;
    for (const std::string &s : w) names = names || (s.size() > ext.size() && s.compare(s.size() - ext.size(), ext.size(), ext) == 0);
    if (!names) continue;
    const bool ok = w.size() >= 5 && w[1] == "*" && w[2] == "*" && w[3].compare(0, locs.size(), locs) == 0 && w[3].size() > locs.size() + ext.size() &&
                    w[3].compare(w[3].size() - ext.size(), ext.size(), ext) == 0 && w[3].find('/', locs.size()) == std::string::npos;
    if (!ok)
      return fail(e, SCEMA_MD_ERR_ARG, "%s line %d: expected `pair_coeff * * ${locs}/<name>.tersoff <element> ...`", script.c_str(), ln);
    const std::string path = folder + "/" + w[3].substr(locs.size());
    std::vector<const char *> el;
    for (size_t k = 4; k < w.size(); k++) el.push_back(w[k].c_str());
    return scema_md_tersoff_configure(e, matid, path.c_str(), el.data(), (int32_t)el.size(), 0, -1.0);
  }
  return SCEMA_MD_OK;
}

}  // namespace scema_eng

extern "C" {

int scema_md_tersoff_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                               int32_t energy_unit, double skin) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid || !*matid || !path || !elements || n_elements <= 0) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  HIPCHK(hipSetDevice(e->p.device));
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  std::unique_ptr<TsMaterial> M(new TsMaterial());
  std::string err;
  if (!scema::read_tersoff_params(path, el, energy_unit, M->tab, M->type_map, err)) return fail(e, SCEMA_MD_ERR_IO, "%s", err.c_str());
  M->skin = skin < 0.0 ? 1.0 : skin;
  M->stamp = ++e->sw_stamp;
  HIPCHK(M->d_tab.ensure(sizeof(TsTable)));
  HIPCHK(hipMemcpyAsync(M->d_tab.p, &M->tab, sizeof(TsTable), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->ts_mats[matid] = std::move(M);   // (a potential it replaces goes with its table: rows and element arrays carry its stamp and are rebuilt)
  e->sw_mats.erase(matid);            // (a Stillinger-Weber potential included: a material holds one attachment)
  return SCEMA_MD_OK;
}

// static evaluation of a state (qp_id SCEMA_MD_QP_NONE: the registered replica)
int scema_md_tersoff_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep, double *e_att,
                                   double *virial, double *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  if (!ts_material(e, matid)) return fail(e, SCEMA_MD_ERR_ARG, "no Tersoff potential attached to material %s (scema_md_tersoff_configure)", matid);
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
  if (e_rep) *e_rep = acc[0];
  if (e_att) *e_att = acc[1];
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
