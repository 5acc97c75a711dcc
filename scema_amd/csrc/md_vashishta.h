// md_vashishta.h -- the Vashishta force stage (md_vashishta.hip): its launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "md_rows.h"
#include "vashishta/vs_core.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to
// the material's VsTable, `stype` indexes it, `eacc` holds two-body energy, three-body energy, ordered pairs inside rc, pairs (a, b) of
// the lists inside r0).

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), pair
// and triplet terms, forces into SimDev::f, virial (parts P_LJ, P_ANGLE) and energies into SimScalars
void mdk_vs_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
