// engine_rowpot.cpp -- host side of the potentials on full neighbour rows (`pair_style sw`: the reference's examples/streched_polyhedron;
// `pair_style tersoff`; `pair_style eam/alloy`; `pair_style tersoff/mod`, `tersoff/mod/c`; `pair_style tersoff/zbl`; `pair_style vashishta`; `pair_style adp`; `pair_style edip`, `edip/multi`; `pair_style meam/spline`; `pair_style born/coul/dsf`; `pair_style born/coul/long`, `buck/coul/long`; `pair_style hybrid/overlay coul/long eam/alloy`): the stage they
// share, the table that tells them apart (row_pots), their stages and their entry points of the C ABI.  A further potential is one entry of the table, a reader for its configure entry point and a kernel.
#include "engine.h"
#include "../md_env.h"

#include <fstream>
#include <sstream>

namespace scema_eng {

// run_phase_rowpot is the run on per-atom neighbour rows (run_rows, engine_rows.cpp) with the force stage of one of these potentials: no
// bonded terms (lammps_scripts_sisw/in.strain.lammps has none).  The row part of a replica's work set is a RowView over the slot's RowSlot;
// rows built for another potential are never kept: the slot's ListSig carries the stage's RowKind and the material's stamp.

// the potential of a material id if it is of that kind, or null
static RowMaterial *row_material(scema_md_engine *e, const std::string &matid, RowKind kind) {
  auto it = e->row_mats.find(matid);
  return it == e->row_mats.end() || it->second->kind != kind ? nullptr : it->second.get();
}

const RowPot *row_pot_of(scema_md_engine *e, const char *matid) {
  if (!matid) return nullptr;
  auto it = e->row_mats.find(matid);
  if (it == e->row_mats.end()) return nullptr;
  for (const RowPot &P : row_pots)
    if (P.kind == it->second->kind) return &P;
  return nullptr;
}

bool bare_replica(const Topo &t) {
  const scema_md_system &s = t.original.sys;
  if (s.nbonds || s.nangles || s.ndihedrals || s.nimpropers) return false;
  for (double q : t.original.q) if (q != 0.0) return false;
  for (double v : t.original.eps) if (v != 0.0) return false;
  return true;
}

bool ionic_replica(const Topo &t) {
  const scema_md_system &s = t.original.sys;
  if (s.nbonds || s.nangles || s.ndihedrals || s.nimpropers) return false;
  for (double v : t.original.eps) if (v != 0.0) return false;
  for (double q : t.original.q) if (q != 0.0) return true;
  return false;
}

#define ROWSET(dst, src) dst = (decltype(dst))(src)

// element of every atom of a replica on the device (Topo::d_eltype): the element pair_coeff names for its LAMMPS type; `what` names the
// potential in the refusal
static int ensure_eltype(scema_md_engine *e, Topo &T, const std::vector<int> &type_map, long long stamp, const char *what) {
  if (T.eltype_stamp == stamp && T.d_eltype.p) return SCEMA_MD_OK;
  std::vector<int> st(T.natoms);
  for (int i = 0; i < T.natoms; i++) {
    const int ty = T.original.type[i];   // the registered LAMMPS type (Topo::type holds Lennard-Jones classes)
    if (ty < 0 || ty >= (int)type_map.size())
      return fail(e, SCEMA_MD_ERR_ARG, "atom %d has type %d but the %s element list names %zu types (pair_coeff * * file ...)", i, ty + 1, what, type_map.size());
    st[i] = type_map[ty];
  }
  int rc = upload(e, T.d_eltype, st);
  if (rc) return rc;
  T.eltype_stamp = stamp;
  return SCEMA_MD_OK;
}

// ---- the stage the potentials share: full neighbour rows inside the material's largest cutoff + skin in the slot's RowSlot, one
// RowView per position (e->h_rowviews / d_rowviews; `tab` is the material's table on the device, of the stage's own type), the row
// capacity and its growth, part batches on the main and the third stream, the "too many neighbours" fault ----

struct RowPotStage : RowStage {
  scema_md_engine *e;
  const char *what;             // the potential's name in messages
  RowView *VV = nullptr;        // the views on the device (upload)
  RowPotStage(scema_md_engine *e_, int ns, const RowPot &pot);
  int nparts() const override;
  int rows(Topo &T, const BoxRange &R, RowNeed &need) override;
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override;
  int upload() override;
  int setup() override { return SCEMA_MD_OK; }
  int part_streams(std::vector<Part> &parts, std::vector<hipEvent_t> &done) override;
  int read_back() override;
  int after_read_back(int fault, double &need) override;
  int faults(int fault) override;
  // the stage's kernels for the positions [pos0, pos0 + n) (every stage reaches the row build through mdk_rows_build), and its own
  // "too many neighbours" fault
  virtual void launch(hipStream_t st, int pos0, int n) = 0;
  virtual int crowded(int fault);
  void forces(hipStream_t st, int pos0, int n, int step, int part) override;
  long cells_missed = 0;        // launch groups whose cell launch did not match their replicas' paths (forces)
};

RowPotStage::RowPotStage(scema_md_engine *e_, int ns, const RowPot &pot) : RowStage(pot.kind, 16), e(e_), what(pot.name) {
  e->h_rowviews.assign(ns, RowView());
  e->h_rowcells.assign(ns, RowCells());
  e->h_rowcells_on.assign(ns, 0);
}

// Part batches: part 0 on the engine's main stream, part 1 on its third.  The split follows the other paths' shape, SCEMA_MD_SPLIT=0 /
// scema_md_batch_split(e, 0) runs the batch whole.
int RowPotStage::nparts() const { return (e->split_streams && e->stream3 && run->ns >= 8 && !run->spec.minimize) ? 2 : 1; }

int RowPotStage::rows(Topo &T, const BoxRange &R, RowNeed &need) {
  const RowMaterial &M = *row_material(e, T.matid, kind);
  if (const int rc = ensure_eltype(e, T, M.type_map, M.stamp, what)) return rc;
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
  for (int d = 0; d < 3; d++) need.w[d] = R.w[d];   // (the cell grid of the replica: bind, once the driver has set the image search)
  return SCEMA_MD_OK;
}

int RowPotStage::bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) {
  const Topo &T = *A.st->topo;
  const int npad = S.npad, cap = need.cap[0];
  if (!sl.row) sl.row.reset(new RowSlot());
  RowSlot &W = *sl.row;
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
  RowView V;
  std::memset(&V, 0, sizeof V);
  for (int d = 0; d < 3; d++) V.mimg[d] = need.mimg[d];
  V.n = S.natoms; V.npad = npad; V.cap = cap; V.rlist = need.rlist;
  ROWSET(V.stype, T.d_eltype.as<int>()); ROWSET(V.x, S.x); ROWSET(V.f, S.f);
  ROWSET(V.cnt, W.cnt.as<int>()); ROWSET(V.rows, W.rows.as<int>());
  ROWSET(V.eacc, W.misc.as<double>());                 // [0, 4) doubles
  ROWSET(V.stat, (int *)(W.misc.as<char>() + 32));     // 2 ints
  e->h_zerotab.push_back(MdkZero{W.misc.as<int>(), 16});   // (the step sums)
  ROWSET(V.tab, row_material(e, T.matid, kind)->d_tab.p);
  // Rows through cells (md_rowcells.h: minimum image, 3 cells and more per dimension over the whole run, a capacity the build kernel
  // stages, the size threshold or SCEMA_MD_ROW_CELLS).  The grid is this run's: it is rebuilt with the rows at every rebuild and nothing
  // of it outlives the run, and the rows are those of k_row_build entry for entry, so rows kept from a run on the other path hold
  // (the slot's ListSig has no field for the path).
  RowCells G;
  std::memset(&G, 0, sizeof G);
  if (rowcell_grid(need.w, need.rlist, need.mimg, cap, V.n, npad, e->row_cells_mode, G.nc)) {
    G.ncells = G.nc[0] * G.nc[1] * G.nc[2];
    if (npad > W.cap_cellpad) {
      HIPCHK(W.clist.ensure((size_t)npad * 4));
      HIPCHK(W.cellof.ensure((size_t)npad * 4));
      W.cap_cellpad = npad;
    }
    if (G.ncells > W.cap_ncells) {
      HIPCHK(W.cstart.ensure(((size_t)G.ncells + 1) * 4));
      HIPCHK(W.ccur.ensure((size_t)G.ncells * 4));
      W.cap_ncells = G.ncells;
    }
    ROWSET(G.cstart, W.cstart.as<int>()); ROWSET(G.ccur, W.ccur.as<int>());
    ROWSET(G.clist, W.clist.as<int>()); ROWSET(G.cellof, W.cellof.as<int>());
    V.cells = 1;
  }
  e->h_rowviews[pos] = V;
  e->h_rowcells[pos] = G;
  e->h_rowcells_on[pos] = V.cells ? 1 : 0;
  return SCEMA_MD_OK;
}

// a host vector of views (or of a stage's side array parallel to them) into its buffer on the device, on the engine's stream
template <class T>
static int upload_views(scema_md_engine *e, DevBuf &buf, const std::vector<T> &host, T *&dev) {
  const size_t bytes = host.size() * sizeof(T);
  HIPCHK(buf.ensure(bytes));
  HIPCHK(hipMemcpyAsync(buf.p, host.data(), bytes, hipMemcpyHostToDevice, e->stream));
  dev = buf.as<T>();
  return SCEMA_MD_OK;
}

int RowPotStage::upload() {
  if (const int rc = upload_views(e, e->d_rowviews, e->h_rowviews, VV)) return rc;
  // the cell arrays travel only where a replica uses them; the launches of this thread learn either way which positions do (md_rows.h)
  RowCells *cells = nullptr;
  if (std::any_of(e->h_rowcells_on.begin(), e->h_rowcells_on.end(), [](unsigned char c) { return c != 0; }))
    if (const int rc = upload_views(e, e->d_rowcells, e->h_rowcells, cells)) return rc;
  mdk_rows_cells(VV, cells, e->h_rowcells_on.data(), (int)e->h_rowcells_on.size());
  return SCEMA_MD_OK;
}

int RowPotStage::part_streams(std::vector<Part> &parts, std::vector<hipEvent_t> &done) {
  if (!e->row_part_done) HIPCHK(hipEventCreateWithFlags(&e->row_part_done, hipEventDisableTiming));
  parts[1].st = e->stream3;
  done.push_back(e->row_part_done);
  return SCEMA_MD_OK;
}

int RowPotStage::read_back() { return run->read_scalars(); }

int RowPotStage::after_read_back(int fault, double &need) {
  for (int pos = 0; pos < run->ns; pos++) {
    need = std::max(need, (double)e->h_sc[run->order[pos]].maxneigh_seen / (double)std::max(e->h_rowviews[pos].cap, 1));
    if (e->h_rowcells_on[pos]) e->prof.row_cell_builds += e->h_sc[run->order[pos]].nbuilds;
  }
  return faults(fault);
}

// A replica marked RowView::cells leaves k_row_build at its top, so a launch group that holds one must have got the cell kernels, and
// mdk_rows_build learns the paths from what upload() bound on this thread (md_rows.h): every launch is checked against the stage's own
// flags, and a run in which one did not match ends in an error instead of forces from rows that were never built.
void RowPotStage::forces(hipStream_t st, int pos0, int n, int, int) {
  const long before = mdk_rows_cell_groups();
  launch(st, pos0, n);
  bool want = false;
  for (int k = pos0; k < pos0 + n && k < (int)e->h_rowcells_on.size(); k++) want = want || e->h_rowcells_on[k] != 0;
  if (want != (mdk_rows_cell_groups() != before)) cells_missed += 1;
}

int RowPotStage::faults(int fault) {
  if (cells_missed)
    return fail(e, SCEMA_MD_ERR_DEVICE, "%ld launch groups of this %s run were issued without the row build their replicas are laid out for (cell path)", cells_missed, what);
  return crowded(fault);
}

int RowPotStage::crowded(int fault) {
  if (fault & 128) return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside the %s cutoff", ROW_MAXIN, what);
  return SCEMA_MD_OK;
}

// ---- the stages: each launches its kernels (mdk_row_forces for the list kernels of md_sw.h, md_tersoff.h, md_vashishta.h, md_edip.h;
// mdk_row_stage for the stages with launches of their own: md_eam.h, md_adp.h, md_meam_spline.h, md_born_dsf.h, md_born_long.h, md_eam_coul.h) ----

namespace {

struct SwStage : RowPotStage {
  using RowPotStage::RowPotStage;
  void launch(hipStream_t st, int pos0, int n) override { mdk_sw_forces(st, run->D + pos0, VV + pos0, n, run->maxatoms); }
};

// (Tersoff and its forms tersoff/mod(/c) and tersoff/zbl: one stage, the form's launch wrapper)
template <void (*Launch)(hipStream_t, const SimDev *, RowView *, int, int)>
struct TsStage : RowPotStage {
  using RowPotStage::RowPotStage;
  void launch(hipStream_t st, int pos0, int n) override { Launch(st, run->D + pos0, VV + pos0, n, run->maxatoms); }
};

// What the two passes of the embedded-atom stage hand from one to the other, F'(rho) per atom, lives in the slot too and reaches the
// kernels through an array of EamView parallel to the views.
struct EamStage : RowPotStage {
  EamView *AA = nullptr;   // on the device (upload)
  EamStage(scema_md_engine *e_, int ns, const RowPot &pot) : RowPotStage(e_, ns, pot) { e->h_eamviews.assign(ns, EamView()); }
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    if (const int rc = RowPotStage::bind(pos, A, sl, S, need)) return rc;
    HIPCHK(sl.row->fp.ensure((size_t)S.npad * sizeof(double)));
    e->h_eamviews[pos].fp = (decltype(EamView::fp))sl.row->fp.as<double>();
    return SCEMA_MD_OK;
  }
  int upload() override { const int rc = RowPotStage::upload(); return rc ? rc : upload_views(e, e->d_eamviews, e->h_eamviews, AA); }
  void launch(hipStream_t st, int pos0, int n) override { mdk_eam_forces(st, run->D + pos0, VV + pos0, AA + pos0, n, run->maxatoms); }
  int crowded(int) override { return SCEMA_MD_OK; }   // (its kernels keep no list of 32: they never raise the "too many neighbours" bit)
};

// The angular-dependent stage hands ten doubles per atom from its first pass to its second (md_adp.h AdpView): the slot's own array again
struct AdpStage : RowPotStage {
  AdpView *AA = nullptr;   // on the device (upload)
  AdpStage(scema_md_engine *e_, int ns, const RowPot &pot) : RowPotStage(e_, ns, pot) { e->h_adpviews.assign(ns, AdpView()); }
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    if (const int rc = RowPotStage::bind(pos, A, sl, S, need)) return rc;
    HIPCHK(sl.row->adp.ensure((size_t)S.npad * ADP_REC * sizeof(double)));
    e->h_adpviews[pos].rec = (decltype(AdpView::rec))sl.row->adp.as<double>();
    return SCEMA_MD_OK;
  }
  int upload() override { const int rc = RowPotStage::upload(); return rc ? rc : upload_views(e, e->d_adpviews, e->h_adpviews, AA); }
  void launch(hipStream_t st, int pos0, int n) override { mdk_adp_forces(st, run->D + pos0, VV + pos0, AA + pos0, n, run->maxatoms); }
  int crowded(int) override { return SCEMA_MD_OK; }   // (as for EAM: no list of 32)
};

// Vashishta: the list of ROW_MAXIN entries holds the neighbours inside r0, the three-body range, alone; the pair term takes any number
// inside rc (158 in SiC), so the refusal names r0
struct VsStage : TsStage<mdk_vs_forces> {
  using TsStage<mdk_vs_forces>::TsStage;
  int crowded(int fault) override {
    if (fault & 128)
      return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside r0, the three-body range of the %s potential (inside rc any number is taken)",
                  ROW_MAXIN, what);
    return SCEMA_MD_OK;
  }
};

// EDIP: one range, a of a pair, for the pair term, the arms and the coordination alike, so the refusal names a
struct EdipStage : TsStage<mdk_edip_forces> {
  using TsStage<mdk_edip_forces>::TsStage;
  int crowded(int fault) override {
    if (fault & 128)
      return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside a (cutoffA), the range of the %s potential", ROW_MAXIN, what);
    return SCEMA_MD_OK;
  }
};

// Spline MEAM: the two passes of the embedded-atom stage (it owns fp, here U'(rho)) around a list of ROW_MAXIN entries that holds the
// neighbours inside f's last knot, the three-body range, alone; rho and phi take any number inside cutmax, so the refusal names f's range
struct MsStage : EamStage {
  using EamStage::EamStage;
  void launch(hipStream_t st, int pos0, int n) override { mdk_ms_forces(st, run->D + pos0, VV + pos0, AA + pos0, n, run->maxatoms); }
  int crowded(int fault) override {
    if (fault & 128)
      return fail(e, SCEMA_MD_ERR_ARG, "an atom has more than %d neighbours inside the last knot of f, the three-body range of the %s potential (inside cutmax any number is taken)",
                  ROW_MAXIN, what);
    return SCEMA_MD_OK;
  }
};

// Born/DSF: the first stage that reads the replica's charges (SimDev::q, bound for every run by sim_common).  The type map is the
// identity: pair_coeff names types, not elements.  No list of ROW_MAXIN: any number of neighbours inside cutmax is taken
struct BdStage : RowPotStage {
  using RowPotStage::RowPotStage;
  void launch(hipStream_t st, int pos0, int n) override { mdk_bd_forces(st, run->D + pos0, VV + pos0, n, run->maxatoms); }
  int crowded(int) override { return SCEMA_MD_OK; }
};

// (the table's common signature: the style has no element list)
int born_dsf_configure_entry(scema_md_engine *e, const char *matid, const char *path, const char *const *, int32_t, int32_t energy_unit, double skin) {
  return scema_md_born_dsf_configure(e, matid, path, energy_unit, skin);
}

// Born/long: Born/DSF's real-space shape with the Ewald split, and a reciprocal sum of its own on the row layout (md_born_long.h).  The
// k-space set-up is the run's: g_ewald and the integer triples from the run's start box by ewald_setup (engine_kspace.cpp) with the
// material's cut_coul and accuracy and the replica's charges; the triples stay while fix deform moves the box, and a box flip re-expresses
// them on the device (flipped).  Triples, the step's S(k) and the flip counts live in the slot and grow like the rows.
void bl_setup(const scema_md_params &base, double cut_coul, double accuracy, const Topo &T, const double *box, EwaldSetup &ew) {
  scema_md_params p = base;
  p.cut_coul = cut_coul;
  p.kspace_accuracy = accuracy;
  ewald_setup(p, T, box, ew);
}

// The mesh set-up of a run: LAMMPS' initial g_ewald estimate (ewald_setup, g only), then the grid and the adjusted g of pppm_setup_host,
// with the material's cut_coul and accuracy as bl_setup takes them.  The accuracy is relative, so K cancels.
void bl_mesh_setup(const scema_md_params &base, double cut_coul, double accuracy, const Topo &T, const double *box, double &g, int pg[3]) {
  scema_md_params p = base;
  p.cut_coul = cut_coul;
  p.kspace_accuracy = accuracy;
  EwaldSetup ew;
  ewald_setup(p, T, box, ew, true);
  g = ew.g;
  pg[0] = pg[1] = pg[2] = 0;
  if (T.qsqsum > 0.0) pppm_setup_host(p, T, box, g, pg);
}

// what the mesh solver refuses, or an empty string
std::string bl_mesh_refusal(const char *what, int natoms, double accuracy, const int pg[3]) {
  char buf[512];
  buf[0] = 0;
  const long long ng = (long long)pg[0] * pg[1] * pg[2];
  if (pg[0] >= BLM_MAXDIM || pg[1] >= BLM_MAXDIM || pg[2] >= BLM_MAXDIM)
    snprintf(buf, sizeof buf, "a %s replica of %d atoms at accuracy %g: the mesh search reached its cap of %d points in a dimension (mesh %d x %d x %d)", what,
             natoms, accuracy, BLM_MAXDIM, pg[0], pg[1], pg[2]);
  else if (ng > BLM_MAXGRID)
    snprintf(buf, sizeof buf, "a %s replica of %d atoms needs a mesh of %d x %d x %d = %lld points at accuracy %g: the mesh solver of the row driver holds %d",
             what, natoms, pg[0], pg[1], pg[2], ng, accuracy, BLM_MAXGRID);
  return buf;
}

// Which reciprocal solver a replica gets is decided here, per replica and run (RowMaterial::kspace_mode, scema_md_born_long_kspace): mode 0
// is the Ewald sum wherever its k list fits, whatever the script's solver word, and the mesh for a `pppm` script beyond the limits; mode 1
// the mesh (md_born_long_mesh.h) for every replica; mode 2 the Ewald sum or its refusal.  A launch group may hold replicas of both.
struct BlStage : RowPotStage {
  BlView *BB = nullptr;    // on the device (upload)
  BlmView *MM = nullptr;   // the mesh views, parallel
  int cur_step = 0;        // the step of the force call being issued (forces)
  int fft_rc = 0;          // a hipFFT call of this run failed: nothing more of the run is enqueued (launch), and faults() reports it
  std::string fft_msg;
  BlStage(scema_md_engine *e_, int ns, const RowPot &pot) : RowPotStage(e_, ns, pot) {
    e->h_blviews.assign(ns, BlView());
    e->h_blmviews.assign(ns, BlmView());
  }
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    if (const int rc = RowPotStage::bind(pos, A, sl, S, need)) return rc;
    const Topo &T = *A.st->topo;
    const RowMaterial &M = *e->row_mats.find(T.matid)->second;
    const double *box = e->h_sc[run->order[pos]].box;
    EwaldSetup ew;
    bool mesh = M.kspace_mode == 1 && T.qsqsum > 0.0;
    if (!mesh) {
      bl_setup(e->p, M.kspace_cut, M.kspace_acc, T, box, ew);
      const int nk = (int)ew.kn.size() / 3;
      if (nk > BL_MAXK || ew.kmaxd[0] > BL_MAXKD || ew.kmaxd[1] > BL_MAXKD || ew.kmaxd[2] > BL_MAXKD) {
        if (M.kspace_mode == 0 && M.kspace_pppm) mesh = true;
        else
          return fail(e, SCEMA_MD_ERR_ARG,
                      "a %s replica of %d atoms needs %d k-vectors (indices up to %d %d %d) at accuracy %g: the Ewald sum of the row driver holds %d (indices up to %d); "
                      "PPPM on the row driver is the follow-up for replicas of that size",
                      what, T.natoms, nk, ew.kmaxd[0], ew.kmaxd[1], ew.kmaxd[2], M.kspace_acc, BL_MAXK, BL_MAXKD);
      }
    }
    BlmView G;
    std::memset(&G, 0, sizeof G);
    if (mesh) {
      ew = EwaldSetup();
      bl_mesh_setup(e->p, M.kspace_cut, M.kspace_acc, T, box, ew.g, G.n);
      const std::string no = bl_mesh_refusal(what, T.natoms, M.kspace_acc, G.n);
      if (!no.empty()) return fail(e, SCEMA_MD_ERR_ARG, "%s", no.c_str());
      G.g = ew.g;
    }
    const int nk = (int)ew.kn.size() / 3;
    RowSlot &W = *sl.row;
    const int nkcap = std::max(64, (nk + 63) / 64 * 64);
    HIPCHK(W.kn.ensure((size_t)nkcap * 3 * sizeof(int)));
    HIPCHK(W.sk.ensure((size_t)nkcap * 5 * sizeof(double)));
    HIPCHK(W.kshift.ensure(2 * sizeof(int)));
    if (nk) HIPCHK(hipMemcpy(W.kn.p, ew.kn.data(), (size_t)nk * 3 * sizeof(int), hipMemcpyHostToDevice));
    e->h_zerotab.push_back(MdkZero{W.kshift.as<int>(), 2});   // (the triples are those of this run's start box)
    BlView B;
    std::memset(&B, 0, sizeof B);
    B.nk = nk; B.nkcap = nkcap;
    for (int d = 0; d < 3; d++) B.kmax[d] = ew.kmaxd[d];
    B.mesh = mesh ? 1 : 0;
    B.g = ew.g;
    for (double q : T.q) { B.qsqsum += q * q; B.qsum += q; G.qabs += std::fabs(q); }
    G.qsqsum = B.qsqsum; G.qsum = B.qsum;
    ROWSET(B.kn, W.kn.as<int>()); ROWSET(B.sk, W.sk.as<double>()); ROWSET(B.shift, W.kshift.as<int>());
    e->h_blviews[pos] = B;
    e->h_blmviews[pos] = G;
    return SCEMA_MD_OK;
  }
  // the grids of the run's mesh replicas, position-major at the stride of the largest mesh, then the views
  int upload() override {
    if (const int rc = RowPotStage::upload()) return rc;
    const size_t ns = e->h_blmviews.size();
    size_t stride = 0;
    for (const BlmView &G : e->h_blmviews) stride = std::max(stride, (size_t)G.n[0] * G.n[1] * G.n[2]);
    if (stride) {
      HIPCHK(e->blm_igrid.ensure(ns * stride * sizeof(long long)));
      HIPCHK(e->blm_cgrid.ensure(ns * stride * 2 * sizeof(double)));
      HIPCHK(e->blm_field.ensure(ns * stride * 6 * sizeof(double)));
      HIPCHK(e->blm_gf.ensure(ns * stride * sizeof(double)));
      HIPCHK(hipMemsetAsync(e->blm_igrid.p, 0, ns * stride * sizeof(long long), e->stream));   // (k_blm_convert leaves it zeroed; a run that failed midway may not have)
      for (size_t pos = 0; pos < ns; pos++) {
        BlmView &G = e->h_blmviews[pos];
        G.gcap = (int)stride;
        ROWSET(G.igrid, e->blm_igrid.as<long long>() + pos * stride);
        ROWSET(G.cgrid, e->blm_cgrid.as<double>() + pos * stride * 2);
        ROWSET(G.field, e->blm_field.as<double>() + pos * stride * 6);
        ROWSET(G.gf, e->blm_gf.as<double>() + pos * stride);
      }
    }
    if (const int rc = upload_views(e, e->d_blviews, e->h_blviews, BB)) return rc;
    return upload_views(e, e->d_blmviews, e->h_blmviews, MM);
  }
  void forces(hipStream_t st, int pos0, int n, int step, int part) override {
    cur_step = step;
    RowPotStage::forces(st, pos0, n, step, part);
  }
  // the transforms of a launch group: one exec per run of consecutive positions with equal mesh, forward on the charge grids, backward
  // on 3 x run field grids
  struct FftCall { BlStage *stage; hipStream_t st; int pos0, n; };
  int transform(hipStream_t st, int pos0, int n, bool backward) {
    const int end = std::min(pos0 + n, (int)e->h_blmviews.size());
    for (int k = pos0; k < end;) {
      const BlmView &G = e->h_blmviews[k];
      int len = 1;
      while (k + len < end && std::memcmp(e->h_blmviews[k + len].n, G.n, sizeof G.n) == 0) len++;
      if (G.n[0] > 0)
        if (const int rc = pppm_exec(e, G.n, (backward ? 3 : 1) * len, st, G.gcap, backward ? (double *)G.field : (double *)G.cgrid,
                                     backward ? HIPFFT_BACKWARD : HIPFFT_FORWARD))
          return rc;
      k += len;
    }
    return SCEMA_MD_OK;
  }
  static int transform_entry(void *ctx, int backward) {
    const FftCall &c = *(const FftCall *)ctx;
    return c.stage->transform(c.st, c.pos0, c.n, backward != 0);
  }
  void launch(hipStream_t st, int pos0, int n) override { launch_real(st, pos0, n, nullptr); }
  // real: what a stage with a real-space part of its own enqueues in place of k_bl_force (md_born_long.h)
  void launch_real(hipStream_t st, int pos0, int n, const std::function<void(dim3)> *real) {
    if (fft_rc) return;
    int maxnk = 0, maxgrid = 0;
    bool ewald = false;
    for (int k = pos0; k < pos0 + n && k < (int)e->h_blviews.size(); k++) {
      const BlmView &G = e->h_blmviews[k];
      maxnk = std::max(maxnk, e->h_blviews[k].nk);
      maxgrid = std::max(maxgrid, G.n[0] * G.n[1] * G.n[2]);
      ewald = ewald || !e->h_blviews[k].mesh;
    }
    if (maxgrid == 0) {
      mdk_bl_forces(st, run->D + pos0, VV + pos0, BB + pos0, n, run->maxatoms, maxnk, true, nullptr, real);
      return;
    }
    // the influence function follows the box: every step of a run whose box moves (fix deform, the barostat), else the run's first call
    const RunSpec &sp = run->spec;
    const bool new_box = cur_step == 0 || sp.deform || (sp.nh && sp.npt);
    FftCall call{this, st, pos0, n};
    fft_rc = mdk_bl_mesh_forces(st, run->D + pos0, VV + pos0, BB + pos0, MM + pos0, n, run->maxatoms, maxnk, ewald, maxgrid, new_box, transform_entry, &call, real);
    if (fft_rc) fft_msg = e->err;
  }
  // (the mesh lives in the fractional coordinates of the step's box, and the box of the step after a flip is the flipped one)
  void flipped(hipStream_t st, int pos, const FlipEvent &fe) override {
    if (!e->h_blviews[pos].mesh) mdk_bl_flip(st, BB + pos, fe.nflip[0], fe.nflip[1]);
  }
  int faults(int fault) override {
    if (fft_rc) return fail(e, SCEMA_MD_ERR_DEVICE, "a mesh transform of this %s run failed: %s", what, fft_msg.c_str());
    return RowPotStage::faults(fault);
  }
  int crowded(int) override { return SCEMA_MD_OK; }
};

int born_long_configure_entry(scema_md_engine *e, const char *matid, const char *path, const char *const *, int32_t, int32_t energy_unit, double skin) {
  return scema_md_born_long_configure(e, matid, path, energy_unit, skin);
}

// EAM + long-range Coulomb (`pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`): the first stage made of two potentials.  The
// Born/long stage as it is -- the k-space set-up per run, the Ewald-or-mesh decision per replica, the transforms, the flips, the
// refusals beyond the limits -- with the side array of the embedded-atom stage (F' per atom) and the fused real-space kernels of
// md_eam_coul.h in the place of k_bl_force.  The element of an atom is that of the setfl tables (RowMaterial::type_map).
struct EcStage : BlStage {
  EamView *AA = nullptr;   // on the device (upload)
  EcStage(scema_md_engine *e_, int ns, const RowPot &pot) : BlStage(e_, ns, pot) { e->h_eamviews.assign(ns, EamView()); }
  int bind(int pos, const ActiveSim &A, Slot &sl, const SimDev &S, const RowNeed &need) override {
    if (const int rc = BlStage::bind(pos, A, sl, S, need)) return rc;
    HIPCHK(sl.row->fp.ensure((size_t)S.npad * sizeof(double)));
    e->h_eamviews[pos].fp = (decltype(EamView::fp))sl.row->fp.as<double>();
    return SCEMA_MD_OK;
  }
  int upload() override { const int rc = BlStage::upload(); return rc ? rc : upload_views(e, e->d_eamviews, e->h_eamviews, AA); }
  void launch(hipStream_t st, int pos0, int n) override {
    const std::function<void(dim3)> real = [&](dim3 gt) { mdk_ec_real(st, gt, run->D + pos0, VV + pos0, AA + pos0, BB + pos0); };
    launch_real(st, pos0, n, &real);
  }
};

int eam_coul_configure_entry(scema_md_engine *e, const char *matid, const char *path, const char *const *, int32_t, int32_t energy_unit, double skin) {
  return scema_md_eam_coul_configure(e, matid, path, energy_unit, skin);
}

template <class Stage>
RowStage *make_stage(scema_md_engine *e, int ns, const RowPot &pot) { return new Stage(e, ns, pot); }

}  // namespace

// the order is the precedence of the refusals (run_phase, scema_md_strain_batch) and of self-configuration (rowpot_from_scripts)
const RowPot row_pots[ROW_NPOT] = {
    {RowKind::Sw, "Stillinger-Weber", "scema_md_sw_configure", {nullptr, nullptr}, scema_md_sw_configure, make_stage<SwStage>},
    {RowKind::Tersoff, "Tersoff", "scema_md_tersoff_configure", {".tersoff", nullptr}, scema_md_tersoff_configure, make_stage<TsStage<mdk_ts_forces>>},
    {RowKind::Eam, "EAM", "scema_md_eam_configure", {".eam.alloy", nullptr}, scema_md_eam_configure, make_stage<EamStage>},
    {RowKind::TersoffMod, "Tersoff/mod", "scema_md_tersoff_mod_configure", {".tersoff.mod", ".tersoff.modc"}, scema_md_tersoff_mod_configure,
     make_stage<TsStage<mdk_ts_mod_forces>>},
    {RowKind::TersoffZbl, "Tersoff/ZBL", "scema_md_tersoff_zbl_configure", {".tersoff.zbl", nullptr}, scema_md_tersoff_zbl_configure,
     make_stage<TsStage<mdk_ts_zbl_forces>>},
    {RowKind::Vashishta, "Vashishta", "scema_md_vashishta_configure", {".vashishta", nullptr}, scema_md_vashishta_configure, make_stage<VsStage>},
    {RowKind::Adp, "ADP", "scema_md_adp_configure", {".adp", nullptr}, scema_md_adp_configure, make_stage<AdpStage>},
    {RowKind::Edip, "EDIP", "scema_md_edip_configure", {".edip", nullptr}, scema_md_edip_configure, make_stage<EdipStage>},
    {RowKind::MeamSpline, "MEAM/spline", "scema_md_meam_spline_configure", {".meam.spline", nullptr}, scema_md_meam_spline_configure, make_stage<MsStage>},
    {RowKind::BornDsf, "Born/DSF", "scema_md_born_dsf_configure", {nullptr, nullptr}, born_dsf_configure_entry, make_stage<BdStage>},
    {RowKind::BornLong, "Born/long", "scema_md_born_long_configure", {nullptr, nullptr}, born_long_configure_entry, make_stage<BlStage>},
    {RowKind::EamCoul, "EAM/coul", "scema_md_eam_coul_configure", {nullptr, nullptr}, eam_coul_configure_entry, make_stage<EcStage>},
};

int run_phase_rowpot(scema_md_engine *e, std::vector<ActiveSim> &sims, const RunSpec &spec, const RowPot &pot) {
  const std::unique_ptr<RowStage> stage(pot.stage(e, (int)sims.size(), pot));
  const int rc = run_rows(e, sims, spec, *stage);
  if (rc == SCEMA_MD_OK) e->rows_run_ns = (int)sims.size();
  return rc;
}

// The one line of in.strain.lammps that names a potential file of extension `ext` -- `pair_coeff * * ${locs}/<name><ext> <El> ...`, ${locs}
// being the scripts folder -- parsed as LAMMPS would: words separated by blanks, `#` starts a comment.  Nothing else of the script is read.
// The line goes to `configure` as (path, elements, n); no such file or line: nothing happens (0); a malformed line: an error
static int pair_coeff_from_scripts(scema_md_engine *e, const std::string &folder, const std::string &ext,
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

int rowpot_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  for (const RowPot &P : row_pots)
    for (const char *ext : P.ext) {
      if (!ext) break;
      const int rc = pair_coeff_from_scripts(e, folder, ext, [&](const char *path, const char *const *el, int32_t n) {
        return P.configure(e, matid, path, el, n, 0, -1.0);
      });
      if (rc || row_pot_of(e, matid)) return rc;
    }
  return SCEMA_MD_OK;
}

// Self-configuration of the ionic styles: a script with the pair_style line of `read`'s style attaches it to the material through
// `configure`, in the units the script names
static const BdTable &bd_of(const BdTable &T) { return T; }
static const BdTable &bd_of(const BlTable &T) { return T.bd; }

template <class Table>
static int ionic_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder,
                              bool (*read)(const std::string &, int, Table &, std::vector<int> &, std::string &, std::vector<double> *, bool *),
                              int (*configure)(scema_md_engine *, const char *, const char *, int32_t, double)) {
  const std::string script = folder + "/in.strain.lammps";
  if (!std::ifstream(script).good()) return SCEMA_MD_OK;
  Table T;
  std::vector<int> type_map;
  std::string err;
  bool has_style = false;
  const bool ok = read(script, -1, T, type_map, err, nullptr, &has_style);
  if (!has_style) return SCEMA_MD_OK;   // (another style's script, or none: nothing changes for the replica)
  if (!ok) return fail(e, SCEMA_MD_ERR_ARG, "%s", err.c_str());
  return configure(e, matid, script.c_str(), bd_of(T).k == BD_COULOMB_KCALMOL ? 1 : 0, -1.0);
}

int born_dsf_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  return ionic_from_scripts<BdTable>(e, matid, folder, scema::read_born_dsf_params, scema_md_born_dsf_configure);
}

int born_long_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  return ionic_from_scripts<BlTable>(e, matid, folder, scema::read_born_long_params, scema_md_born_long_configure);
}

// the same for `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`: the script names its own setfl file and elements
int eam_coul_from_scripts(scema_md_engine *e, const char *matid, const std::string &folder) {
  const std::string script = folder + "/in.strain.lammps";
  if (!std::ifstream(script).good()) return SCEMA_MD_OK;
  scema::EamCoulParams P;
  std::string err;
  bool has_style = false;
  const bool ok = scema::read_eam_coul_script(script, -1, P, err, &has_style);
  if (!has_style) return SCEMA_MD_OK;   // (another style's script, or none: nothing changes for the replica)
  if (!ok) return fail(e, SCEMA_MD_ERR_ARG, "%s", err.c_str());
  return scema_md_eam_coul_configure(e, matid, script.c_str(), P.unit, -1.0);
}

// ---- what the entry points of the C ABI share.  row_configure: `read` fills type_map from the file and says where its host table
// stands, how large it is (the reader decides) and its largest cutoff (blk), or err; row_debug_compute: ea, eb are the two energies of the
// stage ----

struct RowTableBlock { const void *p = nullptr; size_t bytes = 0; double cutmax = 0.0; };
typedef std::function<bool(const std::vector<std::string> &elements, std::vector<int> &type_map, RowTableBlock &blk, std::string &err)> RowTableReader;

static int row_configure(scema_md_engine *e, RowKind kind, const char *matid, const char *path, const char *const *elements, int32_t n_elements, double skin,
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
  M->stamp = ++e->row_stamp;
  HIPCHK(M->d_tab.ensure(blk.bytes));
  HIPCHK(hipMemcpyAsync(M->d_tab.p, blk.p, blk.bytes, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  e->row_mats[matid] = std::move(M);   // (the potential it replaces, of either kind, goes with its table: rows and element arrays carry its stamp and are rebuilt)
  return SCEMA_MD_OK;
}

// static evaluation of a state (qp_id SCEMA_MD_QP_NONE: the registered replica)
static int row_debug_compute(scema_md_engine *e, RowKind kind, int32_t qp_id, const char *matid, int32_t replica, double *f, double *ea, double *eb,
                             double *virial, double *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  (void)settle_pending(e, false);
  if (!row_material(e, matid, kind)) {
    for (const RowPot &P : row_pots)
      if (P.kind == kind) return fail(e, SCEMA_MD_ERR_ARG, "no %s potential attached to material %s (%s)", P.name, matid, P.configure_name);
    return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
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
  const RowView &V = e->h_rowviews[0];
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

int scema_md_debug_rows(scema_md_engine *e, int32_t pos, int32_t *cnt, int32_t *rows, int64_t rows_cap, int32_t *info) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (e->rows_run_ns <= 0) return fail(e, SCEMA_MD_ERR_ARG, "debug_rows: no run or static evaluation of a row potential has ended on this engine yet");
  if (pos < 0 || pos >= e->rows_run_ns || (size_t)pos >= e->h_rowviews.size())
    return fail(e, SCEMA_MD_ERR_ARG, "debug_rows: position %d of a run of %d replicas", pos, e->rows_run_ns);
  if (!info || (!cnt != !rows)) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  const RowView &V = e->h_rowviews[pos];
  const RowCells &G = e->h_rowcells[pos];
  info[0] = V.n; info[1] = V.cap; info[2] = V.cells;
  for (int d = 0; d < 3; d++) info[3 + d] = G.nc[d];
  if (!cnt) return SCEMA_MD_OK;
  const int64_t want = (int64_t)V.n * V.cap;
  if (rows_cap < want) return fail(e, SCEMA_MD_ERR_ARG, "debug_rows: rows_cap %lld < n * capacity = %d * %d", (long long)rows_cap, V.n, V.cap);
  HIPCHK(hipSetDevice(e->p.device));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(cnt, (const void *)V.cnt, (size_t)V.n * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rows, (const void *)V.rows, (size_t)want * 4, hipMemcpyDeviceToHost));
  return SCEMA_MD_OK;
}

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

int scema_md_tersoff_mod_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin) {
  TsModTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_tersoff_mod_params(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::TersoffMod, matid, path, elements, n_elements, skin, read);
}

int scema_md_tersoff_mod_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep, double *e_att,
                                       double *virial, double *info) {
  return row_debug_compute(e, RowKind::TersoffMod, qp_id, matid, replica, f, e_rep, e_att, virial, info);
}

int scema_md_tersoff_zbl_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin) {
  TsZblTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_tersoff_zbl_params(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::TersoffZbl, matid, path, elements, n_elements, skin, read);
}

int scema_md_tersoff_zbl_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_rep, double *e_att,
                                       double *virial, double *info) {
  return row_debug_compute(e, RowKind::TersoffZbl, qp_id, matid, replica, f, e_rep, e_att, virial, info);
}

int scema_md_vashishta_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                 int32_t energy_unit, double skin) {
  VsTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_vashishta_params(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::Vashishta, matid, path, elements, n_elements, skin, read);
}

int scema_md_vashishta_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3,
                                     double *virial, double *info) {
  return row_debug_compute(e, RowKind::Vashishta, qp_id, matid, replica, f, e2, e3, virial, info);
}

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

int scema_md_adp_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                           int32_t energy_unit, double skin) {
  std::vector<double> block;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_adp_setfl(path, el, energy_unit, block, type_map, err)) return false;
    blk = RowTableBlock{block.data(), block.size() * sizeof(double), scema::eam_head(block).cutoff};
    return true;
  };
  return row_configure(e, RowKind::Adp, matid, path, elements, n_elements, skin, read);
}

int scema_md_adp_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair, double *e_manybody,
                               double *virial, double *info) {
  return row_debug_compute(e, RowKind::Adp, qp_id, matid, replica, f, e_pair, e_manybody, virial, info);
}

int scema_md_edip_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                            int32_t energy_unit, double skin) {
  EdipTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_edip_params(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::Edip, matid, path, elements, n_elements, skin, read);
}

int scema_md_edip_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e2, double *e3,
                                double *virial, double *info) {
  return row_debug_compute(e, RowKind::Edip, qp_id, matid, replica, f, e2, e3, virial, info);
}

int scema_md_meam_spline_configure(scema_md_engine *e, const char *matid, const char *path, const char *const *elements, int32_t n_elements,
                                   int32_t energy_unit, double skin) {
  MsTable T;
  auto read = [&](const std::vector<std::string> &el, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_meam_spline(path, el, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  return row_configure(e, RowKind::MeamSpline, matid, path, elements, n_elements, skin, read);
}

int scema_md_meam_spline_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_pair, double *e_embed,
                                       double *virial, double *info) {
  return row_debug_compute(e, RowKind::MeamSpline, qp_id, matid, replica, f, e_pair, e_embed, virial, info);
}

int scema_md_born_dsf_configure(scema_md_engine *e, const char *matid, const char *path, int32_t energy_unit, double skin) {
  if (e && energy_unit != 0 && energy_unit != 1) return fail(e, SCEMA_MD_ERR_ARG, "energy unit %d (0: A, C and D eV-based, 1: in kcal/mol)", energy_unit);
  BdTable T;
  auto read = [&](const std::vector<std::string> &, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_born_dsf_params(path, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.cutmax};
    return true;
  };
  static const char *const no_elements[1] = {"*"};   // (pair_coeff names types: the type map is the identity over the fragment's types)
  return row_configure(e, RowKind::BornDsf, matid, path, no_elements, 1, skin, read);
}

int scema_md_born_dsf_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_born, double *e_coul,
                                    double *virial, double *info) {
  return row_debug_compute(e, RowKind::BornDsf, qp_id, matid, replica, f, e_born, e_coul, virial, info);
}

int scema_md_born_long_configure(scema_md_engine *e, const char *matid, const char *path, int32_t energy_unit, double skin) {
  if (e && energy_unit != 0 && energy_unit != 1) return fail(e, SCEMA_MD_ERR_ARG, "energy unit %d (0: A, C and D eV-based, 1: in kcal/mol)", energy_unit);
  BlTable T;
  auto read = [&](const std::vector<std::string> &, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::read_born_long_params(path, energy_unit, T, type_map, err)) return false;
    blk = RowTableBlock{&T, sizeof T, T.bd.cutmax};
    return true;
  };
  static const char *const no_elements[1] = {"*"};   // (pair_coeff names types: the type map is the identity over the fragment's types)
  const int rc = row_configure(e, RowKind::BornLong, matid, path, no_elements, 1, skin, read);
  if (rc) return rc;
  RowMaterial &M = *e->row_mats[matid];
  M.kspace_cut = T.bd.cut_coul;
  M.kspace_acc = T.accuracy;
  M.kspace_pppm = T.pppm;
  return SCEMA_MD_OK;
}

// the reciprocal solver mode of a material of that kind (scema_md_born_long_kspace, scema_md_eam_coul_kspace)
static int row_kspace_mode(scema_md_engine *e, RowKind kind, const char *matid, int32_t mode) {
  if (!e) return SCEMA_MD_ERR_ARG;
  if (!matid) return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  auto it = e->row_mats.find(matid);
  if (it == e->row_mats.end() || it->second->kind != kind) {
    for (const RowPot &P : row_pots)
      if (P.kind == kind) return fail(e, SCEMA_MD_ERR_ARG, "no %s potential attached to material %s (%s)", P.name, matid, P.configure_name);
    return fail(e, SCEMA_MD_ERR_ARG, "bad arguments");
  }
  if (mode < 0 || mode > 2) return fail(e, SCEMA_MD_ERR_ARG, "reciprocal solver mode %d (0: by the script and the Ewald limits, 1: the mesh, 2: the Ewald sum)", mode);
  it->second->kspace_mode = mode;
  return SCEMA_MD_OK;
}

// the static evaluation of a stage with a reciprocal part: info[6], and the mesh it ran on for *_last_mesh
static int row_kspace_debug_compute(scema_md_engine *e, RowKind kind, int32_t qp_id, const char *matid, int32_t replica, double *f, double *ea, double *eb,
                                    double *virial, double *info) {
  double info4[4] = {0.0, 0.0, 0.0, 0.0};
  if (e) e->blm_last_mesh[0] = e->blm_last_mesh[1] = e->blm_last_mesh[2] = 0;
  const int rc = row_debug_compute(e, kind, qp_id, matid, replica, f, ea, eb, virial, info4);
  if (rc) return rc;
  if (!e->h_blmviews.empty())
    for (int d = 0; d < 3; d++) e->blm_last_mesh[d] = e->h_blmviews[0].n[d];
  if (info) {
    for (int k = 0; k < 4; k++) info[k] = info4[k];
    info[4] = e->h_blviews.empty() ? 0.0 : e->h_blviews[0].nk;
    info[5] = e->h_blviews.empty() ? 0.0 : e->h_blviews[0].g;
  }
  return SCEMA_MD_OK;
}

int scema_md_born_long_kspace(scema_md_engine *e, const char *matid, int32_t mode) { return row_kspace_mode(e, RowKind::BornLong, matid, mode); }

int scema_md_eam_coul_configure(scema_md_engine *e, const char *matid, const char *path, int32_t energy_unit, double skin) {
  if (e && energy_unit != 0 && energy_unit != 1) return fail(e, SCEMA_MD_ERR_ARG, "energy unit %d (0: the setfl tables in eV, 1: in kcal/mol)", energy_unit);
  std::vector<double> block;
  scema::EamCoulParams P;
  auto read = [&](const std::vector<std::string> &, std::vector<int> &type_map, RowTableBlock &blk, std::string &err) {
    if (!scema::build_eam_coul_block(path, energy_unit, block, type_map, P, err)) return false;
    blk = RowTableBlock{block.data(), block.size() * sizeof(double), scema::eam_coul_table(block).bd.cutmax};
    return true;
  };
  static const char *const no_elements[1] = {"*"};   // (the script's eam/alloy line names the elements)
  const int rc = row_configure(e, RowKind::EamCoul, matid, path, no_elements, 1, skin, read);
  if (rc) return rc;
  RowMaterial &M = *e->row_mats[matid];
  M.kspace_cut = P.cut_coul;
  M.kspace_acc = P.accuracy;
  M.kspace_pppm = P.pppm;
  return SCEMA_MD_OK;
}

int scema_md_eam_coul_kspace(scema_md_engine *e, const char *matid, int32_t mode) { return row_kspace_mode(e, RowKind::EamCoul, matid, mode); }

int scema_md_eam_coul_last_mesh(scema_md_engine *e, int32_t *grid) { return scema_md_born_long_last_mesh(e, grid); }

int scema_md_eam_coul_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_eam, double *e_coul,
                                    double *virial, double *info) {
  return row_kspace_debug_compute(e, RowKind::EamCoul, qp_id, matid, replica, f, e_eam, e_coul, virial, info);
}

int scema_md_born_long_last_mesh(scema_md_engine *e, int32_t *grid) {
  if (!e || !grid) return SCEMA_MD_ERR_ARG;
  for (int d = 0; d < 3; d++) grid[d] = e->blm_last_mesh[d];
  return SCEMA_MD_OK;
}

int scema_md_born_long_debug_compute(scema_md_engine *e, int32_t qp_id, const char *matid, int32_t replica, double *f, double *e_born, double *e_coul,
                                     double *virial, double *info) {
  return row_kspace_debug_compute(e, RowKind::BornLong, qp_id, matid, replica, f, e_born, e_coul, virial, info);
}

// what the two pure host entries below open with: the message buffer emptied, the common argument rules beside the entry's own
// (args_ok), the table of the file, a run's default parameters and a Topo of the two numbers the k-space set-up reads
struct BlHostCase { BlTable T; scema_md_params p; Topo t; };
static void bl_host_say(char *errbuf, int32_t errcap, const std::string &m) {
  if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
}
static int bl_host_case(const char *path, int32_t energy_unit, const double *box, int32_t natoms, double qsqsum, bool args_ok, char *errbuf, int32_t errcap,
                        BlHostCase &C) {
  bl_host_say(errbuf, errcap, "");
  if (!path || !box || natoms <= 0 || !args_ok || (energy_unit != 0 && energy_unit != 1)) { bl_host_say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<int> map;
  std::string err;
  if (!scema::read_born_long_params(path, energy_unit, C.T, map, err)) { bl_host_say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  scema_md_default_params(&C.p);
  C.t.natoms = natoms;
  C.t.qsqsum = qsqsum;
  return SCEMA_MD_OK;
}

int scema_md_born_long_kvectors(const char *path, int32_t energy_unit, const double *box, int32_t natoms, double qsqsum, double *g_ewald, int32_t *kmax,
                                int32_t *nk, int32_t *triples, int32_t triples_cap, char *errbuf, int32_t errcap) {
  BlHostCase C;
  if (const int rc = bl_host_case(path, energy_unit, box, natoms, qsqsum, qsqsum >= 0.0 && triples_cap >= 0, errbuf, errcap, C)) return rc;
  EwaldSetup ew;
  bl_setup(C.p, C.T.bd.cut_coul, C.T.accuracy, C.t, box, ew);
  const int n = (int)ew.kn.size() / 3;
  if (g_ewald) *g_ewald = ew.g;
  if (kmax) for (int d = 0; d < 3; d++) kmax[d] = ew.kmaxd[d];
  if (nk) *nk = n;
  if (triples) {
    if (triples_cap < n) { bl_host_say(errbuf, errcap, "triples_cap " + std::to_string(triples_cap) + " < nk = " + std::to_string(n)); return SCEMA_MD_ERR_ARG; }
    for (int k = 0; k < 3 * n; k++) triples[k] = ew.kn[k];
  }
  return SCEMA_MD_OK;
}

int scema_md_born_long_mesh(const char *path, int32_t energy_unit, const double *box, int32_t natoms, double qsqsum, double *g_ewald, int32_t *grid,
                            char *errbuf, int32_t errcap) {
  BlHostCase C;
  if (const int rc = bl_host_case(path, energy_unit, box, natoms, qsqsum, qsqsum > 0.0, errbuf, errcap, C)) return rc;
  double g = 0.0;
  int pg[3] = {0, 0, 0};
  bl_mesh_setup(C.p, C.T.bd.cut_coul, C.T.accuracy, C.t, box, g, pg);
  if (g_ewald) *g_ewald = g;
  if (grid) for (int d = 0; d < 3; d++) grid[d] = pg[d];
  const std::string no = bl_mesh_refusal("Born/long", natoms, C.T.accuracy, pg);
  if (!no.empty()) { bl_host_say(errbuf, errcap, no); return SCEMA_MD_ERR_ARG; }
  return SCEMA_MD_OK;
}

}  // extern "C"
