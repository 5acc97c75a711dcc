// md_pppm.h -- host-callable launch wrappers of the PPPM kernels (md_pppm.hip); the transforms between them are hipFFT calls
// issued by the engine (engine/engine_run.cpp pppm_stage)
#pragma once
#include <hip/hip_runtime.h>
struct SimDev;
size_t mdk_pppm_lds_limit();
// What the tiled kernels of a launch need from the host (engine_run.cpp fills it from the meshes of the batch by md_pppm_tile.h):
// budget: LDS bytes of the tile rule and of the whole-mesh tests (> 0); mode 0: the kernels without LDS for meshes beyond it, as before;
// per kernel the largest tile counts of the batch (tiles: largest ty * tz = gridDim.x; 0: a mesh whose smallest brick does not fit, the
// launch keeps the kernel without LDS) and the largest brick / staged size in bytes.
struct PppmLaunch {
  int budget = 0, mode = 1;
  int sp_ty = 0, sp_tz = 0, sp_tiles = 0, fo_ty = 0, fo_tz = 0, fo_tiles = 0;
  size_t sp_lds = 0, fo_lds = 0;
  int binned = 0;   // this launch: the binned pair of spreading kernels where mdk_pppm_binned_ok (the engine decides: pppm_stage)
  // staged interpolation (force path 0): the largest LDS size of the batch's meshes in the layout of md_pppm_fstride.h, by pppm_fstride at
  // this budget -- the largest PADDED size, not the size of the largest mesh; 0: every replica keeps the dense layout (scema_md_pppm_force_layout)
  size_t fs_lds = 0;
};
// Binned charge assignment (k_pppm_bins + k_pppm_spread_binned): from how many replicas per launch, and from how many charged atoms per
// grid point in the mean, the pair of launches is taken when nothing forces it (scema_md_pppm_binning mode 2).  k_pppm_bins is one more
// launch on the chain, one workgroup per replica: PE-10k, evaluations/s off / on by batch (replicas per launch): 1: 75.9 / 66.0, 4: 206.1 /
// 193.5, 9 (3): 302.5 / 291.3, 36 (9): 436.5 / 430.8, 72 (36): 444.7 / 440.4, 144 (72): 455.7 / 462.8, 576 (288): 461.2 / 471.4
// (profiles/pppm_binned_size_scan.log, pppm_binned_headline_ab.log).  Below two atoms per point there is nothing to merge.
struct PppmBinPolicy { int min_replicas = 72; double min_per_point = 2.0; };
// 1: the launch may take the binned kernels -- the whole padded mesh in LDS (spread path 0, every nx >= 5), no tiled interpolation
int mdk_pppm_binned_ok(int maxgrid, int maxgridp, const PppmLaunch *tl);
// 0: the whole mesh in LDS, 1: tiled, 2: no LDS (global atomics / unstaged reads) -- what mdk_pppm_spread / mdk_pppm_force take and return
int mdk_pppm_spread_path(int maxgrid, int maxgridp, const PppmLaunch *tl);
int mdk_pppm_force_path(int maxgrid, const PppmLaunch *tl);
// home-tile keys of all atoms from the current positions (one int per atom behind SimDev::pgf, pgstride doubles in): before the first tiled kernel of a step
void mdk_pppm_keys(hipStream_t st, const SimDev *d, int ns, int maxatoms);
// charges -> grid 0 (complex, imaginary part 0); maxgrid = largest nx*ny*nz of the batch
// zeroed != 0: the charge grids are known to hold zeros (k_pppm_solve leaves them so)
int mdk_pppm_spread(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxatoms, int zeroed, int maxgridp = 0, const PppmLaunch *tl = nullptr);   // maxgridp: largest grid with 5 more points per x row (0: no padded LDS copy)
// small grids (maxgrid <= mdk_pppm_solve_max()): forward transform, energy / virial / field spectra and the three inverse transforms in one
// launch, in LDS (replaces the transforms of the engine and mdk_pppm_poisson); maxdims = largest nx + ny + nz of the batch
int mdk_pppm_solve_max();
void mdk_pppm_solve(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxdims);
// influence function of the current box into SimDev::pgf
void mdk_pppm_gf(hipStream_t st, const SimDev *d, int ns, int maxgrid);
// after the forward transform of grid 0: energy, virial, field spectra into grids 1..3
void mdk_pppm_poisson(hipStream_t st, const SimDev *d, int ns, int maxgrid);
// after the inverse transforms of the field grids: forces added to SimDev::f (add != 0) or stored there (the chain runs ahead of
// the kernel that assembles the force of the step, which then adds them: mdk_ewald_force fkeep)
int mdk_pppm_force(hipStream_t st, const SimDev *d, int ns, int maxgrid, int maxatoms, int add, int real_fields = 0, const PppmLaunch *tl = nullptr);   // real_fields: after mdk_pppm_solve
