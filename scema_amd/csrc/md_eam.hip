// md_eam.hip -- gfx950 kernels of the embedded-atom force stage (`pair_style eam/alloy`).  The neighbour rows are those of the
// row part (mdk_rows_build, md_rows.hip: full rows inside cutoff + skin, sorted by partner, image codes in the convention of the
// ReaxFF rows); the integrator, thermostat, fix deform, pressure sampling and the batch machinery are the ones of the OPLS path.  One
// launch covers every replica of the batch (blockIdx.y).
//   k_eam_density .. rho_i over the entries of atom i's row inside the cutoff, F(rho_i) into the step's energy, F'(rho_i) into fp[i]
//   k_eam_force .... the same walk (rowf_walk, md_rowforce.h) with the full pair term (eam/eam_core.h): every F' exists before any force is formed
// between the row part and k_row_finish (md_rows.hip).  With full rows every atom sums its own force: neither kernel has an atomic on a
// force or a density, rows are sorted and the sum over a group has a fixed order, so forces do not depend on the schedule.
// Engine parts: phi and the virial of phi' go to P_LJ, the embedding energy and the virial of the F' terms to P_ANGLE.  Only their sum
// enters the stress; the split is what scema_md_eam_debug_compute reports as e_pair and e_embed.
#include <hip/hip_runtime.h>

#include "md_eam.h"
#include "md_eam_body.h"

// Densities: the body both embedded-atom stages share (eam_density_body, md_eam_body.h): the embedding energy to eacc[1], the atoms above
// rhomax to eacc[3].
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_eam_density(const SimDev *sims, const RowView *views, const EamView *aux) {
  const RowView V = views[blockIdx.y];
  if ((int)(blockIdx.x * ROW_TILE) >= V.n) return;   // (the whole workgroup)
  eam_density_body<1, true>(V, (EamTab)V.tab, aux[blockIdx.y].fp);
}

// Forces: the same walk; a lane's entry takes the derivative records of the two densities and both records of r phi, and F' of both
// ends (eam_entry, md_eam_body.h).  The group's sum is the atom's force, stored once.  Half of a pair's phi and half of its virial go to each end.
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_eam_force(const SimDev *sims, const RowView *views, const EamView *aux) {
  const RowView V = views[blockIdx.y];
  const int n = V.n;
  if ((int)(blockIdx.x * ROW_TILE) >= n) return;   // (the whole workgroup)
  const EamTab blk = (EamTab)V.tab;
  const double ROW_G *fp = aux[blockIdx.y].fp;
  SimScalars &sc = *sims[blockIdx.y].sc;
  __shared__ double s_sh[3 * ROW_NSHIFT];
  __shared__ EamHead s_hd;
  __shared__ double s_red[8 * (ROW_FORCE_TPB / 64)];
  rowf_shifts(V, s_sh);
  rowf_to_lds<int>(&s_hd, blk);   // (offsets are read per lane, by the partner's element)
  __syncthreads();
  const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
  const int nr = s_hd.nr;
  const double rdr = s_hd.rdr, cut2 = s_hd.cut2;
  double esum[4] = {0.0, 0.0, 0.0, 0.0};
  double wa[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, wb[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int it = 0; it < ROW_TILE / ROW_NGRP; it++) {   // (uniform over the workgroup)
    const int i = blockIdx.x * ROW_TILE + it * ROW_NGRP + grp;
    const int ic = min(i, n - 1);
    const int ti = V.stype[ic];
    const double fpi = fp[ic];
    double fi0 = 0.0, fi1 = 0.0, fi2 = 0.0;
    rowf_walk(V, s_sh, i, l16, [&](int j, double d0, double d1, double d2, double r2) __attribute__((always_inline)) {
      if (!(r2 < cut2 && r2 > 0.0)) return;
      double phi, fa, fb;
      eam_entry(blk, s_hd, nr, rdr, ti, V.stype[j], sqrt(r2), fpi, fp[j], &phi, &fa, &fb);
      const double fpair = fa + fb;
      fi0 -= d0 * fpair; fi1 -= d1 * fpair; fi2 -= d2 * fpair;   // (x_i - x_j = -d)
      esum[0] += 0.5 * phi;
      rowf_virial(wa, 0.5 * fa, d0, d1, d2);
      rowf_virial(wb, 0.5 * fb, d0, d1, d2);
    });
    fi0 = row_sum(fi0); fi1 = row_sum(fi1); fi2 = row_sum(fi2);
    if (i < n && l16 == 0) { V.f[3 * i] = fi0; V.f[3 * i + 1] = fi1; V.f[3 * i + 2] = fi2; }
  }
  block_atomic_add_n<4, ROW_FORCE_TPB / 64>(esum, (double *)V.eacc, s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wa, &sc.vir[P_LJ * 6], s_red);
  block_atomic_add_n<6, ROW_FORCE_TPB / 64>(wb, &sc.vir[P_ANGLE * 6], s_red);
}

void mdk_eam_forces(hipStream_t st, const SimDev *d, RowView *v, const EamView *a, int ns, int maxatoms) {
  mdk_row_stage(st, d, v, ns, maxatoms, [&](dim3 gt) {
    hipLaunchKernelGGL(k_eam_density, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
    hipLaunchKernelGGL(k_eam_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v, a);
  });
}
