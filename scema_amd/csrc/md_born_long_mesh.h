// md_born_long_mesh.h -- the mesh reciprocal solver of the Ewald ionic force stage (md_born_long_mesh.hip): PPPM on the row layout for
// the replicas whose k list the Ewald sum of md_born_long.hip does not hold, or whose material asks for the mesh
// (scema_md_born_long_kspace).  The mesh view of a replica and the launch wrapper.
#pragma once
#include <hip/hip_runtime.h>

#include "ionic/blm_core.h"
#include "md_born_long.h"

// Parallel to the RowView and the BlView of a replica.  The mesh and g_ewald are those of the RUN (scema_eng::pppm_setup_host on the run's
// start box) and stay; the mesh lives in the fractional coordinates of the step's box (RowView::h, lo), so fix deform and a box flip
// need nothing but the influence function of the new box.  The grids belong to the engine, not to the slot: hipFFT wants the grids of a
// batch at one stride, `gcap` points, the largest mesh of the run.  An Ewald replica has n = 0 0 0 and every mesh kernel leaves it alone;
// a mesh replica has BlView::mesh = 1, nk = 0, and the Ewald kernels leave it alone.
typedef struct {
  int n[3], gcap;              // mesh points per dimension; points each of the replica's grids holds (n0 n1 n2 <= gcap)
  double g;                    // g_ewald of the run, adjusted to the mesh
  double qsqsum, qsum, qabs;   // sum q_i^2, sum q_i, sum |q_i| of the replica (the last sets the fixed-point scale: blm_fixed_shift)
  long long ROW_G *igrid;      // [gcap] the charge grid in fixed point: k_blm_assign adds, k_blm_convert reads and zeroes
  double ROW_G *cgrid;         // [gcap][2] the complex charge grid, transformed in place
  double ROW_G *field;         // [3][gcap][2] the three complex field grids, transformed in place
  double ROW_G *gf;            // [gcap] the influence function of the last box k_blm_gf was launched for
} BlmView;

// transforms of the mesh replicas among the ns positions of a launch, enqueued on its stream: the charge grids forward (backward 0) or
// the field grids backward (1); not 0: a failure, after which the chain enqueues nothing more
typedef int (*BlmTransform)(void *ctx, int backward);

// The force stage of one step for the first ns replicas, Ewald and mesh replicas alike: the row part, k_bl_force, the Ewald pair where
// `ewald` (a replica of the group runs the Ewald sum), then for the mesh replicas (maxgrid: their largest mesh, 0 for none) k_blm_assign,
// k_blm_convert, the forward transform, k_blm_gf where new_box, k_blm_poisson, the backward transforms, k_blm_interp; k_row_finish.
// Returns what a transform returned (0: all enqueued).  real: as for mdk_bl_forces, what takes the place of k_bl_force.
int mdk_bl_mesh_forces(hipStream_t st, const SimDev *d, RowView *v, const BlView *b, const BlmView *m, int ns, int maxatoms, int maxnk, bool ewald,
                       int maxgrid, bool new_box, BlmTransform transform, void *ctx, const std::function<void(dim3)> *real = nullptr);
