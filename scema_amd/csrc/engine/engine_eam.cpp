// engine_eam.cpp -- host side of the embedded-atom path (`pair_style eam/alloy`): run_phase_eam and the EAM entry points of the C ABI
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// run_phase_eam is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the embedded-atom force stage.  The row part of a
// replica's work set is an SwView over the slot's SwSlot (SwRowsStage, shared with the Stillinger-Weber and the Tersoff stage: the rows are
// mdk_sw_rows'); what the two passes hand from one to the other, F'(rho) per atom, lives in the slot too and reaches the kernels through
// an array of EamView parallel to the views.  Rows built for another potential are never kept: the slot's ListSig carries RowKind::Eam and
// the material's stamp.

namespace {

struct EamStage : SwRowsStage {
  EamView *AA = nullptr;   // on the device (upload)
  EamStage(scema_md_engine *e_, int ns) : SwRowsStage(e_, ns, RowKind::Eam, "EAM") { e->h_eamviews.assign(ns, EamView()); }
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    if (const int rc = SwRowsStage::bind(pos, A, sl, S, need)) return rc;
    HIPCHK(sl.sw->fp.ensure((size_t)S.npad * sizeof(double)));
    e->h_eamviews[pos].fp = (decltype(EamView::fp))sl.sw->fp.as<double>();
    return SCEMA_MD_OK;
  }
  int upload() override {
    if (const int rc = SwRowsStage::upload()) return rc;
    const size_t bytes = e->h_eamviews.size() * sizeof(EamView);
    HIPCHK(e->d_eamviews.ensure(bytes));
    HIPCHK(hipMemcpyAsync(e->d_eamviews.p, e->h_eamviews.data(), bytes, hipMemcpyHostToDevice, e->stream));
    AA = e->d_eamviews.as<EamView>();
    return SCEMA_MD_OK;
  }
  void forces(hipStream_t st, int pos0, int n, int, int) override { mdk_eam_forces(st, run->D + pos0, VV + pos0, AA + pos0, n, run->maxatoms); }
  int faults(int) override { return SCEMA_MD_OK; }   // (its kernels keep no list of 32: they never raise the "too many neighbours" bit)
};

}  // namespace

int run_phase_eam(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec) {
  EamStage stage(e, (int)sims.size());
  return run_rows(e, sims, spec, stage);
}

int eam_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  return pair_coeff_from_scripts(e, folder, ".eam.alloy", [&](const char *path, const char *const *el, int32_t n) {
    return scema_md_eam_configure(e, matid, path, el, n, 0, -1.0);
  });
}

}  // namespace scema_eng

extern "C" {

int scema_md_eam_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                           int32_t energy_unit, double skin) {
  std::vector<double> block;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_eam_setfl(path, el, energy_unit, block, type_map, err)) return false;
    blk = RowTableBlock{block.data(), block.size() * sizeof(double), scema::eam_head(block).cutoff};
    return true;
  };
  return row_configure(e, RowKind::Eam, matid, path, elements, n_elements, skin, read);
}

int scema_md_eam_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair, double *e_embed,
                               double *virial, double *info) {
  return row_debug_compute(e, RowKind::Eam, qp_id, matid, replica, f, e_pair, e_embed, virial, info);
}

}  // extern "C"
