// ec_core.h -- the table block of the EAM + long-range Coulomb stage (`pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`): where
// its two parts stand.  Compiled by hipcc for the kernels of md_eam_coul.hip and by plain g++ for the host (host/eam_coul_params.cpp
// builds the block, tests/eam_coul_host_driver.cpp holds the offsets against what the kernels assume).
//
// One material is one flat block of doubles:
//   [0, EC_EAM_OFF)      a BlTable (ionic/bl_core.h) whose Born pairs are all zero (cut_lj2 = 0: no pair ever reaches the Born term);
//                        cut_coul, K, cutmax = max(setfl cutoff, cut_coul), accuracy and the solver word are set.  The reciprocal
//                        kernels of md_born_long.hip and md_born_long_mesh.hip read K through ((const BlTable *)tab)->bd.k and run
//                        unchanged on this block
//   [EC_EAM_OFF, ...)    the EAM block of eam_core.h: an EamHead and its records, offsets counted from EC_EAM_OFF.  A record is 32 bytes
//                        and stays 32-byte aligned: EC_EAM_OFF is a multiple of 4 doubles
#pragma once
#include "../ionic/bl_core.h"
#include "eam_core.h"

#define EC_EAM_OFF ((int)((sizeof(BlTable) + 31) / 32 * 4))   /* in doubles */
static_assert(EC_EAM_OFF % 4 == 0 && EC_EAM_OFF * sizeof(double) >= sizeof(BlTable), "the EAM block follows the BlTable at a 32-byte boundary");
