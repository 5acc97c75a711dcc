// md_tersoff.h -- the Tersoff force stage (md_tersoff.hip): its launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "md_rows.h"
#include "tersoff/ts_core.h"

// One replica's work set is the RowView of the row part (md_rows.h: box, positions, forces, rows, step sums and fault bits; `tab` points to the
// material's TsTable, `stype` indexes it, `eacc` holds repulsive energy, bond-order energy, ordered pairs inside the cutoff, ordered (j, k)
// evaluated).  More than ROW_MAXIN neighbours of one atom INSIDE the cutoff (diamond: 4; scaled by 0.75: 16) raise stat bit 2 -> fault bit 128.

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), pair
// terms and bond orders, forces into SimDev::f, virial (parts P_LJ: the repulsive term, P_ANGLE: everything that carries b_ij) and
// energies into SimScalars
void mdk_ts_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
// the same stage for `pair_style tersoff/mod` and `tersoff/mod/c` (`tab` points to a TsModTable) and for `tersoff/zbl` (a TsZblTable): the
// kernel's instances for those forms
void mdk_ts_mod_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
void mdk_ts_zbl_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms);
