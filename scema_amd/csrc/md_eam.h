// md_eam.h -- the embedded-atom force stage (md_eam.hip): what its kernels need beyond the row part's view, and the launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "eam/eam_core.h"
#include "md_rows.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to
// the material's block -- an EamHead and its spline tables, eam/eam_core.h -- `stype` indexes it, `eacc` holds the pair energy, the
// embedding energy, the ordered pairs inside the cutoff and the atoms whose density lies above rhomax) and, parallel to the views, an
// EamView: the stage's own per-slot arrays.  The kernels keep no list of an atom's neighbours: an atom may have any number inside the cutoff.
typedef struct {
  double ROW_G *fp;           // [npad] F'(rho_i) of the step: written by the density pass, read by the force pass
} EamView;

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), the
// density pass, the force pass, forces into SimDev::f, virial (parts P_LJ: the pair term, P_ANGLE: the embedding terms) and energies into
// SimScalars
void mdk_eam_forces(hipStream_t st, const SimDev *d, RowView *v, const EamView *a, int ns, int maxatoms);
