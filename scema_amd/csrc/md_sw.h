// md_sw.h -- the Stillinger-Weber force stage (md_sw.hip): one replica's work set and the host-callable launch wrappers
#pragma once
#include <hip/hip_runtime.h>

#include "sw/sw_core.h"
struct SimDev;

#if defined(__HIP_DEVICE_COMPILE__)
#define SW_G __attribute__((address_space(1)))
#else
#define SW_G
#endif

#define SW_MAXIN 32          /* neighbours of one atom INSIDE the cutoff that the force kernel keeps (diamond silicon: 4; compressed 10 %: 16); more raise fault bit 2 */
#define SW_LDS_MAXPAD 1024   /* replicas up to this many (padded) atoms sum their forces in a workgroup's LDS table; larger ones add to global memory directly */
#define SW_TILE 64           /* central atoms of one workgroup of the force kernel, rows of one workgroup of the row build */

// one replica's work set.  Every pointer points to global memory and says so in device code (md_types.h)
typedef struct {
  int n, npad;               // atoms, n rounded up to 64
  int cap;                   // capacity (entries) of one neighbour row
  int pad_;
  double rlist;              // radius the rows cover: the material's largest a sigma + list skin
  int mimg[3], pad2_;        // neighbour search: 0 0 0 = minimum image (box at least two list radii wide), else images up to mimg[d] boxes away
  double h[6], lo[3];        // box of the step: lx, ly, lz, yz, xz, xy and origin (k_sw_prepare)
  const int SW_G *stype;     // [n] element of every atom (index into the material's SwTable)
  const void SW_G *tab;      // the material's parameter tables: the stage's own type (SwTable, TsTable, an EamHead block), cast once by its kernels
  const double SW_G *x;      // [n][3]
  double SW_G *f;            // [n][3]
  int SW_G *cnt;             // [npad] entries of a row (clamped to cap)
  int SW_G *rows;            // [npad][cap] full rows inside cutoff + skin: atom | image code << 24, sorted by atom
  double SW_G *eacc;         // [4] of the step: two-body energy, three-body energy, pairs inside the cutoff, triplets evaluated
  int SW_G *stat;            // [2] fault bits of the step (1: a row was full at the last build, 2: more than SW_MAXIN neighbours inside the cutoff),
                             //     longest row the last build asked for (unclamped)
} SwView;
static_assert(sizeof(double SW_G *) == sizeof(double *), "the qualified pointers of SwView have the size of plain ones: host and device passes see one layout");

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set, pair and triplet
// terms, forces into SimDev::f, virial (parts P_LJ, P_ANGLE) and energies into SimScalars
void mdk_sw_forces(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms);
// its first three launches alone (k_sw_prepare, k_sw_wrap, k_sw_rows): the row part of a step, which the Tersoff and the embedded-atom
// force stage share (md_tersoff.hip, md_eam.hip); the rows cover SwView::rlist and read nothing of SwView::tab.  mdk_sw_finish is the last
// launch of a stage on them (k_sw_finish: eacc[0], eacc[1] and the fault bits into the engine's scalars)
void mdk_sw_rows(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms);
void mdk_sw_finish(hipStream_t st, const SimDev *d, SwView *v, int ns);
// a force stage on those rows: the row part, then `lacc` (replicas up to SW_LDS_MAXPAD atoms, with the LDS force table) or `direct`, then
// k_sw_finish.  mdk_sw_forces and mdk_ts_forces (md_tersoff.h) are this with their kernels
typedef void (*SwForceKernel)(const SimDev *, const SwView *);
void mdk_row_forces(hipStream_t st, const SimDev *d, SwView *v, int ns, int maxatoms, SwForceKernel lacc, SwForceKernel direct);
