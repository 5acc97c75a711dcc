// md_meam_spline.h -- the spline-MEAM force stage (md_meam_spline.hip): its launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "md_eam.h"
#include "md_rows.h"
#include "meam_spline/ms_core.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to
// the material's MsTable, `stype` indexes it, `eacc` holds the pair energy, the embedding energy, the ordered pairs inside cutmax and the
// triplets of the lists inside f's range) and, parallel to the views, the EamView of the embedded-atom stage (md_eam.h): fp[i] = U'(rho_i)
// of the step, written by the density pass and read by the force pass.

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), the
// density pass with the three-body forces, the pair pass, forces into SimDev::f, virial (parts P_LJ: phi, P_ANGLE: the embedding terms)
// and energies into SimScalars
void mdk_ms_forces(hipStream_t st, const SimDev *d, RowView *v, const EamView *a, int ns, int maxatoms);
