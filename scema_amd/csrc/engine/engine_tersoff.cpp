// engine_tersoff.cpp -- host side of the Tersoff path (`pair_style tersoff`): run_phase_tersoff and the Tersoff entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

#include <fstream>
#include <sstream>

namespace scema_eng {

// run_phase_tersoff is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the Tersoff force stage.  The row part of a
// replica's work set is an SwView over the slot's SwSlot (SwRowsStage, shared with the Stillinger-Weber stage: the rows are mdk_sw_rows');
// rows built for the other potential are never kept, the slot's ListSig carries RowKind::Tersoff and the material's stamp.

namespace {

struct TsStage : SwRowsStage {
  TsStage(scema_md_engine *e_, int ns) : SwRowsStage(e_, ns, RowKind::Tersoff, "Tersoff") {}
  void forces(hipStream_t st, int pos0, int n, int, int) override { mdk_ts_forces(st, run->D + pos0, VV + pos0, n, run->maxatoms); }
};

}  // namespace

int run_phase_tersoff(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  TsStage stage(e, (int)sims.size());
  return run_rows(e, sims, spec, stage);
}

// The one line of in.strain.lammps that names a potential file of extension `ext` -- `pair_coeff * * ${locs}/<name><ext> <El> ...`, ${locs}
// being the scripts folder -- parsed as LAMMPS would: words separated by blanks, `#` starts a comment.  Nothing else of the script is read.
int pair_coeff_from_scripts(scema_md_engine *e, const std::string &folder, const std::string &ext,
                            const std::function<int(const char *path, const char *const *elements, int32_t n)> &configure) {
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
    const std::string locs = "${locs}/";
    bool names = false;
    for (const std::string &s : w) names = names || (s.size() > ext.size() && s.compare(s.size() - ext.size(), ext.size(), ext) == 0);
    if (!names) continue;
    const bool ok = w.size() >= 5 && w[1] == "*" && w[2] == "*" && w[3].compare(0, locs.size(), locs) == 0 && w[3].size() > locs.size() + ext.size() &&
                    w[3].compare(w[3].size() - ext.size(), ext.size(), ext) == 0 && w[3].find('/', locs.size()) == std::string::npos;
    if (!ok)
      return fail(e, SCEMA_MD_ERR_ARG, "%s line %d: expected `pair_coeff * * ${locs}/<name>%s <element> ...`", script.c_str(), ln, ext.c_str());
    const std::string path = folder + "/" + w[3].substr(locs.size());
    std::vector<const char *> el;
    for (size_t k = 4; k < w.size(); k++) el.push_back(w[k].c_str());
    return configure(path.c_str(), el.data(), (int32_t)el.size());
  }
  return SCEMA_MD_OK;
}

int tersoff_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  return pair_coeff_from_scripts(e, folder, ".tersoff", [&](const char *path, const char *const *el, int32_t n) {
    return scema_md_tersoff_configure(e, matid, path, el, n, 0, -1.0);
  });
}

}  // namespace scema_eng

extern "C" {

int scema_md_tersoff_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                               int32_t energy_unit, double skin) {
  TsTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_tersoff_params(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::Tersoff, matid, path, elements, n_elements, skin, read);
}

int scema_md_tersoff_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep, double *e_att,
                                   double *virial, double *info) {
  return row_debug_compute(e, RowKind::Tersoff, qp_id, matid, replica, f, e_rep, e_att, virial, info);
}

}  // extern "C"
