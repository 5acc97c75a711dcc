// md_adp.h -- the force stage of the angular-dependent potential (md_adp.hip): what its kernels need beyond the row part's view, and the
// launch wrapper
#pragma once
#include <hip/hip_runtime.h>

#include "eam/adp_core.h"
#include "md_rows.h"

// One replica's work set is the RowView of the row part (md_rows.h; `tab` points to the material's block -- an AdpHead and its spline
// tables, eam/adp_core.h -- `eacc` holds the pair energy, the embedding plus the angular energy, the ordered pairs inside the cutoff and
// the atoms whose density lies above rhomax) and, parallel to the views, an AdpView: the stage's own per-slot array.
typedef struct {
  double ROW_G *rec;          // [npad][ADP_REC] {F'(rho_i), mu_i x y z, lam_i xx yy zz yz xz xy} of the step: written by the density pass,
                              // read by the force pass.  One record of 80 bytes per atom, 16-byte aligned: what the force pass gathers per entry
} AdpView;

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build), the
// density pass, the force pass, forces into SimDev::f, virial (parts P_LJ: phi, P_ANGLE: everything else) and energies into SimScalars
void mdk_adp_forces(hipStream_t st, const SimDev *d, RowView *v, const AdpView *a, int ns, int maxatoms);
