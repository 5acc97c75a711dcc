// md_born_long.h -- the Ewald ionic force stage (md_born_long.hip, `pair_style born/coul/long` and `buck/coul/long`): the k-space view of
// a replica and the launch wrappers
#pragma once
#include <hip/hip_runtime.h>

#include <functional>

#include "ionic/bl_core.h"
#include "md_rows.h"

// One replica's work set is the RowView of the row part (md_rows.h; `tab` points to the material's BlTable, `stype` holds the atom types
// that index it, `eacc` holds the Born energy, the whole Coulomb energy (real space, reciprocal space, self and background), ordered pairs
// inside cutmax, ordered pairs inside cut_coul) and, parallel to it, the k-space set-up of the RUN: g_ewald and the integer triples from
// the run's start box (scema_eng::ewald_setup), fixed over the run.  The charges are those of the replica (SimDev::q).
typedef struct {
  int nk, nkcap;             // k-vectors of the half space (at most BL_MAXK); stride of `sk`
  int kmax[3], mesh;         // largest |n_d| of the triples (at most BL_MAXKD each); 1: the replica's reciprocal part runs on the mesh
                             // (md_born_long_mesh.h: nk is 0, the Ewald pair leaves the replica alone, its self energy included)
  double g;                  // g_ewald of the run
  double qsqsum, qsum;       // sum q_i^2, sum q_i of the replica
  const int ROW_G *kn;       // [nk][3] the triples in the reciprocal basis of the run's start box
  double ROW_G *sk;          // [5][nkcap] of the step: c_k Re S(k), c_k Im S(k), k_x, k_y, k_z (k_bl_sfac writes, k_bl_recip reads)
  int ROW_G *shift;          // [2] box flips of the run so far, summed: a2 = a2(start) + shift[0] a1, a3 = a3(start) + shift[1] a1
} BlView;

// the force stage of one step for the first ns replicas: neighbour rows where the rebuild flag of the step is set (mdk_rows_build),
// k_bl_force (real space, stores SimDev::f), k_bl_sfac (S(k), reciprocal energy and virial, self energy), k_bl_recip (adds the reciprocal
// force), k_row_finish.  maxnk: the largest BlView::nk of the ns replicas.  Virial parts: P_LJ for the Born term, P_COUL for everything
// Coulomb.  ewald false: no replica of the group runs the Ewald sum and the pair of reciprocal kernels is not launched; mesh: what the
// mesh solver enqueues for its replicas between the Ewald pair and k_row_finish (md_born_long_mesh.h), given the grid of k_bl_force.
// real: what a stage with a real-space part of its own enqueues in place of k_bl_force, given that grid (md_eam_coul.h: the density pass,
// then the fused force pass); it stores SimDev::f and adds the real-space Coulomb energy to eacc[1].  Absent: k_bl_force.
void mdk_bl_forces(hipStream_t st, const SimDev *d, RowView *v, const BlView *b, int ns, int maxatoms, int maxnk, bool ewald = true,
                   const std::function<void(dim3)> *mesh = nullptr, const std::function<void(dim3)> *real = nullptr);
// a box flip of one replica by fxy, fxz lattice steps, after mdk_flip on the same stream: the triples keep their Cartesian vectors
void mdk_bl_flip(hipStream_t st, const BlView *b, int fxy, int fxz);
