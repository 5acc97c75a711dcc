// md_tersoff.h -- the Tersoff force stage (md_tersoff.hip): what a replica's work set holds beyond the row part, and the launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "md_sw.h"
#include "tersoff/ts_core.h"

#define TS_MAXIN SW_MAXIN    /* neighbours of one atom INSIDE the cutoff that the force kernel keeps (diamond: 4; scaled by 0.75: 16); more raise stat bit 2 -> fault bit 128 */

// One replica's work set is the SwView of the row part (md_sw.h: box, positions, forces, rows, step sums and fault bits; its `tab` stays
// null, `stype` indexes the TsTable, `eacc` holds repulsive energy, bond-order energy, ordered pairs inside the cutoff, ordered (j, k)
// evaluated) and this
typedef struct {
  const TsTable SW_G *tab;   // the material's parameter tables
} TsView;

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_sw_rows), pair
// terms and bond orders, forces into SimDev::f, virial (parts P_LJ: the repulsive term, P_ANGLE: everything that carries b_ij) and
// energies into SimScalars
void mdk_ts_forces(hipStream_t st, const SimDev *d, SwView *v, const TsView *t, int ns, int maxatoms);
