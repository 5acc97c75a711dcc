// md_born_dsf.h -- the ionic force stage (md_born_dsf.hip, `pair_style born/coul/dsf`): its launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "ionic/bd_core.h"
#include "md_rows.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to
// the material's BdTable, `stype` holds the atom types that index it, `eacc` holds the Born energy, the Coulomb energy with the self term,
// ordered pairs inside cutmax, ordered pairs inside cut_coul).  The charges are those of the replica (SimDev::q).

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), the
// pair terms, forces into SimDev::f, virial (parts P_LJ for the Born term, P_COUL for the Coulomb term) and energies into SimScalars
void mdk_bd_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
