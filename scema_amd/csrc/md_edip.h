// md_edip.h -- the EDIP force stage (md_edip.hip): its launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "md_rows.h"
#include "edip/edip_core.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to
// the material's EdipTable, `stype` indexes it, `eacc` holds two-body energy, three-body energy, ordered pairs inside a, triplets).

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), pair,
// triplet and coordination terms, forces into SimDev::f, virial (parts P_LJ, P_ANGLE) and energies into SimScalars
void mdk_edip_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
