// md_eam_coul.h -- the real-space part of the EAM + long-range Coulomb stage (md_eam_coul.hip, `pair_style hybrid/overlay coul/long
// <cut_coul> eam/alloy`): the launcher that takes the place of k_bl_force in mdk_bl_forces / mdk_bl_mesh_forces (md_born_long.h,
// md_born_long_mesh.h).  The reciprocal part, Ewald sum or mesh, is that of the Born/long stage, unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "eam/ec_core.h"
#include "md_born_long.h"
#include "md_eam.h"

// One replica's work set is the RowView of the row part (`tab` points to the material's block, eam/ec_core.h: a BlTable, then the EAM
// block at EC_EAM_OFF; `stype` holds the element of the setfl tables; `eacc` holds the whole EAM energy, the whole Coulomb energy, the
// ordered pairs inside the setfl cutoff, the ordered pairs inside cut_coul), the EamView of the embedded-atom stage (F' per atom) and the
// BlView of the Born/long stage (g_ewald of the run).  The charges are those of the replica (SimDev::q).
// The density pass, then the fused force pass, on the grid gt of the row force kernels (mdk_row_stage): forces are stored into SimDev::f,
// the EAM virial goes to P_LJ, the real-space Coulomb virial to P_COUL.
void mdk_ec_real(hipStream_t st, dim3 gt, const SimDev *d, const RowView *v, const EamView *a, const BlView *b);
