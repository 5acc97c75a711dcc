// engine_debug.cpp -- parity / measurement entry points: static evaluations and plain runs on a stored state; the timing printout of a run
#include "engine.h"
#include "../md_env.h"

namespace scema_eng {

// The skin bands of the replica at position pos of the last run, as its next pair launch would walk them (md_skin_bands.h): out[2 K + 3] =
// skin entries listed per band, walked per band, rows with skin entries, rows with a band open, rows with every band open.  A launch and a
// copy of its own: diagnostics, never part of a step.
int skin_band_stats(const scema_md_engine *e, int pos, unsigned long long *out) {
  const int n = 2 * MD_SKIN_BANDS + 3;
  unsigned long long *d = nullptr;
  if (hipMalloc(&d, n * sizeof *d) != hipSuccess) return SCEMA_MD_ERR_DEVICE;
  hipError_t err = hipMemsetAsync(d, 0, n * sizeof *d, e->stream);
  if (err == hipSuccess) {
    mdk_band_stats(e->stream, e->d_sims.as<SimDev>() + pos, d);
    err = hipMemcpyAsync(out, d, n * sizeof *d, hipMemcpyDeviceToHost, e->stream);
  }
  if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
  (void)hipFree(d);
  return err == hipSuccess ? SCEMA_MD_OK : SCEMA_MD_ERR_DEVICE;
}

// SCEMA_MD_TIMING: the lists of the first replica of the run that just ended, the host time of its layout, and the counters of a build
// with PAIR_COUNT / PAIR_TIMING
void print_run_timing(const scema_md_engine *e, int ns, double layout_ms, double kspace_ms, double box_ms, double grid_ms, double rest_ms) {
  if (!scema_env("SCEMA_MD_TIMING") || ns <= 0) return;
  const SimScalars &c = e->h_sc[0];
  const SimDev &S0 = e->h_sims[0];
  fprintf(stderr, "[scema_md] sim 0: cells %dx%dx%d, j table max %d of %d, row max %d of %d, row entries/cluster %.1f, listed pairs/atom %.1f, builds %d\n",
          S0.nc[0], S0.nc[1], S0.nc[2], c.maxj_seen, S0.capj, c.maxneigh_seen, S0.maxneigh, (double)c.nrowent / (S0.npad / MD_CLUSTER),
          (double)c.nentries / S0.natoms, c.nbuilds);
  fprintf(stderr, "[scema_md] host: %.2f ms laying out %d simulations before the first launch of this run (k-space set-up on host threads %.2f, box range %.2f, cell grid %.2f, rest of the loop %.2f)\n",
          layout_ms, ns, kspace_ms, box_ms, grid_ms, rest_ms);
  if (S0.dslot) {
    unsigned long long bs[2 * MD_SKIN_BANDS + 3];
    if (skin_band_stats(e, 0, bs) == SCEMA_MD_OK) {
      fprintf(stderr, "[scema_md] sim 0 after %d steps, list skin %.2f A: skin entries walked / listed per band:", c.step, S0.skin);
      for (int b = 0; b < MD_SKIN_BANDS; b++) fprintf(stderr, " %llu / %llu", bs[MD_SKIN_BANDS + b], bs[b]);
      fprintf(stderr, "; rows with skin entries %llu, with a band open %llu, with all open %llu\n", bs[2 * MD_SKIN_BANDS], bs[2 * MD_SKIN_BANDS + 1], bs[2 * MD_SKIN_BANDS + 2]);
    }
  }
#ifdef PAIR_COUNT
  fprintf(stderr, "[scema_md] k_pair lanes (sim 0, this run): %llu wave-chunks (%llu with work); atom blocks run %llu = %.2f per working chunk, %.1f lanes of 64 in them; "
          "LJ block run in %llu of them with %.1f lanes; coulomb block in %llu with %.1f lanes; pairs inside the LJ cutoff %llu, inside the coulomb cutoff %llu\n",
          c.dbg[0], c.dbg[1], c.dbg[2], (double)c.dbg[2] / std::max(1ull, c.dbg[1]), (double)c.dbg[3] / std::max(1ull, c.dbg[2]), c.dbg[5],
          (double)c.dbg[4] / std::max(1ull, c.dbg[5]), c.dbg[7], (double)c.dbg[6] / std::max(1ull, c.dbg[7]), c.dbg[4], c.dbg[6]);
#endif
#ifdef PAIR_TIMING
  if (c.dbg2[7])
    fprintf(stderr, "[scema_md] k_pppm_solve clocks (sim 0, thread 0, mean per launch): grid in %.0f, forward passes %.0f, spectra %.0f + %.0f, inverse passes %.0f + %.0f, out + sums %.0f\n",
            (double)c.dbg2[0] / c.dbg2[7], (double)c.dbg2[1] / c.dbg2[7], (double)c.dbg2[2] / c.dbg2[7], (double)c.dbg2[4] / c.dbg2[7], (double)c.dbg2[3] / c.dbg2[7],
            (double)c.dbg2[5] / c.dbg2[7], (double)c.dbg2[6] / c.dbg2[7]);
  fprintf(stderr, "[scema_md] k_pair wave clocks (sim 0, mean per wave): prologue %.0f, rows %.0f, barrier wait %.0f, flush %.0f (%llu waves)\n",
          (double)c.dbg[0] / c.dbg[4], (double)c.dbg[1] / c.dbg[4], (double)c.dbg[2] / c.dbg[4], (double)c.dbg[3] / c.dbg[4], c.dbg[4]);
  {   // (the same clocks summed over the whole batch)
    unsigned long long a[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ns; i++) for (int k = 0; k < 6; k++) a[k] += e->h_sc[i].dbg[k];
    if (a[4]) fprintf(stderr, "[scema_md] pair kernel wave clocks (whole batch, mean per wave and tile visit): prologue %.0f, rows %.0f, wait %.0f, flush %.0f (of which staging %.0f) (%llu visits)\n",
                      (double)a[0] / a[4], (double)a[1] / a[4], (double)a[2] / a[4], (double)a[3] / a[4], (double)a[5] / a[4], a[4]);
  }
  if (c.nbuilds > 0) {
    const double nw = (double)c.nbuilds * S0.ncells * MD_TILE_WAVES;
    fprintf(stderr, "[scema_md] k_neigh_build wave clocks (sim 0, mean per wave and build): table %.0f (boxes and runs %.0f, candidates %.0f), rows %.0f, schedule %.0f; %llu waves of %.0f; %.2f rows per wave of %.1f chunks\n",
            (double)c.dbg[5] / nw, (double)c.dbg[8] / nw, (double)(c.dbg[5] - c.dbg[8]) / nw, (double)c.dbg[6] / nw, (double)c.dbg[7] / nw, c.dbg[9], nw,
            (double)c.dbg[11] / nw, (double)c.dbg[10] / std::max(1ull, c.dbg[11]));
    const double nr = (double)std::max(1ull, c.dbg[11]);
    fprintf(stderr, "[scema_md] k_neigh_build per row (sim 0, cycles): set-up %.0f, chunk loop %.0f = %.0f per chunk, row end %.0f; of %.1f chunks %.2f walk exclusion lists, %.2f are own-cell chunks\n",
            (double)c.dbg[12] / nr, (double)c.dbg[13] / nr, (double)c.dbg[13] / std::max(1ull, c.dbg[10]), (double)c.dbg[14] / nr, (double)c.dbg[10] / nr,
            (double)c.dbg[15] / nr, (double)c.dbg[16] / nr);
  }
#endif
}

// ---- parity / measurement hooks ----
// qp_id == SCEMA_MD_QP_NONE: a temporary copy of the registered init state (held by `tmp`)
int debug_state(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, State **out, std::unique_ptr<State> &tmp) {
  Topo *t = find_topo(e, matid, replica);
  if (!t) return fail(e, SCEMA_MD_ERR_NOSTATE, "replica %s_%d not registered", matid, replica);
  if (qp_id == SCEMA_MD_QP_NONE) {
    int rc = make_state(e, t, t->init_box, t->init_x.data(), t->init_v.data(), false, tmp);
    if (rc) return rc;
    *out = tmp.get();
    return SCEMA_MD_OK;
  }
  State *s = find_state(e, qp_id, matid, replica);
  if (!s) return fail(e, SCEMA_MD_ERR_NOSTATE, "no state for qp %d", qp_id);
  *out = s;
  return SCEMA_MD_OK;
}

}  // namespace scema_eng

extern "C" {

int scema_md_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, int32_t use_shake, double *f,
                           double *energies, double *virials, double *info) {
  if (e) (void)settle_pending(e, false);   // an update that waits for its verdict (no communicator) stands once the engine is used for something else
  if (!e) return SCEMA_MD_ERR_ARG;
  HIPCHK(hipSetDevice(e->p.device));
  State *s = nullptr;
  std::unique_ptr<State> tmp;
  int rc = debug_state(e, qp_id, matid, replica, &s, tmp);
  if (rc) return rc;
  RunSpec R;
  R.use_shake = use_shake;
  R.ev_always = 1;
  R.static_only = 1;
  R.nvt = 0;
  if ((rc = eval_static(e, s, R))) return rc;
  const SimScalars &sc = e->h_sc[0];
  if (f) HIPCHK(hipMemcpy(f, e->slots[0]->f.p, 3 * (size_t)s->topo->natoms * 8, hipMemcpyDeviceToHost));
  if (energies) std::memcpy(energies, sc.eng, sizeof sc.eng);
  if (virials) std::memcpy(virials, sc.vir, sizeof sc.vir);
  if (info) {
    info[0] = e->h_sims[0].g_ewald;
    info[1] = e->h_sims[0].nk;
    info[2] = 0.5 * (double)sc.nentries;
    info[3] = e->h_sims[0].tdof;
    info[4] = sc.t_current;
    info[5] = sc.maxneigh_seen;
    info[4] = (double)sc.nrowent;  // row entries stored (t_current is not needed by the callers)
    info[6] = e->h_sims[0].maxneigh;
    info[7] = s->topo->nclus;
  }
  return SCEMA_MD_OK;
}

int scema_md_debug_skin_bands(scema_md_engine *e, int32_t pos, uint64_t *out, int32_t cap) {
  if (!e || !out || pos < 0 || pos >= (int)e->h_sims.size() || cap < 2 * MD_SKIN_BANDS + 4) return SCEMA_MD_ERR_ARG;
  if (!e->h_sims[pos].dslot) return fail(e, SCEMA_MD_ERR_ARG, "the last run kept no cluster rows with skin bands");
  HIPCHK(hipSetDevice(e->p.device));
  unsigned long long bs[2 * MD_SKIN_BANDS + 3];
  if (skin_band_stats(e, pos, bs)) return fail(e, SCEMA_MD_ERR_DEVICE, "the statistics launch of the skin bands failed");
  out[0] = MD_SKIN_BANDS;
  for (int k = 0; k < 2 * MD_SKIN_BANDS + 3; k++) out[1 + k] = bs[k];
  return SCEMA_MD_OK;
}

int scema_md_debug_run(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, int32_t nsteps, double dt,
                       double temperature, int32_t nvt, int32_t use_shake, const double *rates, double *press_avg) {
  if (e) (void)settle_pending(e, false);   // an update that waits for its verdict (no communicator) stands once the engine is used for something else
  if (!e || nsteps < 0) return SCEMA_MD_ERR_ARG;
  HIPCHK(hipSetDevice(e->p.device));
  if (qp_id == SCEMA_MD_QP_NONE) return fail(e, SCEMA_MD_ERR_ARG, "debug_run needs a stored state (scema_md_set_state first)");
  State *s = nullptr;
  std::unique_ptr<State> tmp;
  int rc = debug_state(e, qp_id, matid, replica, &s, tmp);
  if (rc) return rc;
  std::vector<ActiveSim> sims(1);
  sims[0].st = s;
  sims[0].nsteps = nsteps;
  sims[0].dt = dt;
  sims[0].temperature = temperature;
  if (rates) for (int k = 0; k < 6; k++) sims[0].rates[k] = rates[k];
  if ((rc = prepare_slots(e, sims))) return rc;
  RunSpec R;
  R.nvt = nvt;
  R.use_shake = use_shake;
  R.deform = rates ? 1 : 0;
  R.sample = press_avg ? 1 : 0;
  rc = run_phase(e, sims, R);
  if (rc) return rc;
  const SimScalars &sc = e->h_sc[0];
  std::memcpy(s->box, sc.box, 9 * sizeof(double));
  if (press_avg) for (int k = 0; k < 6; k++) press_avg[k] = sc.psum[k] / (double)std::max(sc.nsamples, 1);
  return SCEMA_MD_OK;
}

}  // extern "C"
