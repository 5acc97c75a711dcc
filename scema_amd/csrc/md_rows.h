// md_rows.h -- the row part every force stage on full neighbour rows shares (md_rows.hip; the Stillinger-Weber, the Tersoff and the
// embedded-atom stage: md_sw.hip, md_tersoff.hip, md_eam.hip): one replica's work set and the host-callable launch wrappers
#pragma once
#include <hip/hip_runtime.h>

#include "md_row_entry.h"
struct SimDev;

#if defined(__HIP_DEVICE_COMPILE__)
#define ROW_G __attribute__((address_space(1)))
#else
#define ROW_G
#endif

#define ROW_MAXIN 32         /* neighbours of one atom INSIDE the cutoff that a force kernel keeps (diamond silicon: 4; compressed 10 %: 16); more raise fault bit 2 */
#define ROW_LDS_MAXPAD 1024  /* replicas up to this many (padded) atoms sum their forces in a workgroup's LDS table; larger ones add to global memory directly */
#define ROW_TILE 64          /* central atoms of one workgroup of a force kernel, rows of one workgroup of the row build */

// one replica's work set.  Every pointer points to global memory and says so in device code (md_types.h)
typedef struct {
  int n, npad;               // atoms, n rounded up to 64
  int cap;                   // capacity (entries) of one neighbour row
  int cells;                 // 1: the rows are built through cells (k_cell_bin, k_cell_rows: md_rowcells.hip; RowCells) and k_row_build returns at its top
  double rlist;              // radius the rows cover: the material's largest cutoff + list skin
  int mimg[3], pad2_;        // neighbour search: 0 0 0 = minimum image (box at least two list radii wide), else images up to mimg[d] boxes away
  double h[6], lo[3];        // box of the step: lx, ly, lz, yz, xz, xy and origin (k_row_prepare)
  const int ROW_G *stype;    // [n] element of every atom (index into the material's tables)
  const void ROW_G *tab;     // the material's parameter tables: the stage's own type (SwTable, TsTable, an EamHead block), cast once by its kernels
  const double ROW_G *x;     // [n][3]
  double ROW_G *f;           // [n][3]
  int ROW_G *cnt;            // [npad] entries of a row (clamped to cap)
  int ROW_G *rows;           // [npad][cap] full rows inside cutoff + skin: atom | image code << 24, sorted by atom (md_row_entry.h)
  double ROW_G *eacc;        // [4] of the step: the stage's two energies and two counts
  int ROW_G *stat;           // [2] fault bits of the step (1: a row was full at the last build, 2: more than ROW_MAXIN neighbours inside the cutoff),
                             //     longest row the last build asked for (unclamped)
} RowView;
static_assert(sizeof(double ROW_G *) == sizeof(double *), "the qualified pointers of RowView have the size of plain ones: host and device passes see one layout");

// the cell arrays of a replica whose rows are built through cells (md_rowcells.h has the grid rule), parallel to the views; all zero for
// a replica on the N^2 build
typedef struct {
  int nc[3], ncells;         // cells along each box vector (fractional coordinates of the step's box), their number
  int ROW_G *cstart;         // [ncells + 1] first entry of a cell in clist
  int ROW_G *ccur;           // [ncells] atoms of a cell while they are counted, then the fill cursor
  int ROW_G *clist;          // [npad] atoms by cell; inside a cell in no fixed order
  int ROW_G *cellof;         // [npad] cell of every atom
} RowCells;

// the row part of a step for the first ns replicas (k_row_prepare, k_row_wrap, k_row_build): neighbour rows where the rebuild flag of the
// step is set; the rows cover RowView::rlist and read nothing of RowView::tab.  mdk_rows_finish is the last launch of a stage on them
// (k_row_finish: eacc[0], eacc[1] and the fault bits into the engine's scalars).
// mdk_rows_cells names, for the calling thread's launches from now on, the view array whose replicas `on` marks as built through cells and
// the RowCells parallel to it (both on the device; `on` on the host, copied): mdk_rows_build puts the cell kernels (mdk_rowcells_build)
// between k_row_wrap and k_row_build for a group v .. v + ns of that array that holds such a replica, and issues exactly the three launches
// above for every other group
void mdk_rows_cells(const RowView *views, const RowCells *cells, const unsigned char *on, int ns);
long mdk_rows_cell_groups();   // launch groups of the calling thread that mdk_rows_build has given the cell kernels so far (the stage checks every launch against it)
void mdk_rowcells_build(hipStream_t st, const SimDev *d, const RowView *v, const RowCells *c, int ns, int maxatoms);
void mdk_rows_build(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
void mdk_rows_finish(hipStream_t st, const SimDev *d, RowView *v, int ns);
// a force stage on those rows: the row part, then `lacc` (replicas up to ROW_LDS_MAXPAD atoms, with the LDS force table) or `direct`, then
// k_row_finish.  mdk_sw_forces (md_sw.h) and mdk_ts_forces (md_tersoff.h) are this with their kernels
typedef void (*RowForceKernel)(const SimDev *, const RowView *);
void mdk_row_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms, RowForceKernel lacc, RowForceKernel direct);
// the same sequence for a stage with launches of its own (two passes, a side array, a k-space part): `launches(gt)` issues them on `st`,
// gt being the grid of a tile of ROW_TILE central atoms per workgroup and a replica per blockIdx.y
template <class Launches>
inline void mdk_row_stage(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms, Launches launches) {
  if (ns <= 0 || maxatoms <= 0) return;
  mdk_rows_build(st, d, v, ns, maxatoms);
  launches(dim3((unsigned)((maxatoms + ROW_TILE - 1) / ROW_TILE), (unsigned)ns, 1));
  mdk_rows_finish(st, d, v, ns);
}
