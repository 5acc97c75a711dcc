// md_born_dsf.hip -- gfx950 kernel of the ionic force stage (`pair_style born/coul/dsf`: rock-salt halides, MgO, UO2, Buckingham and
// Born-Mayer-Huggins models of oxides and glasses), the first row stage that reads a charge.  The neighbour rows are those of the row
// part (mdk_rows_build, md_rows.hip: full rows inside cutmax + skin, sorted by partner, image codes in the convention of the ReaxFF
// rows); the integrator, thermostat, fix deform, pressure sampling and the batch machinery are the ones of the OPLS path.  One launch
// covers every replica of the batch (blockIdx.y).
//   k_bd_force ..... the Born term and the damped-shifted-force Coulomb term (ionic/bd_core.h) over every entry of an atom's row inside
//                    cutmax: the body the ionic stages share (ionic_force, md_ionic_force.h) on the gather skeleton of md_rowforce.h
// between the row part and k_row_finish.  With full rows every atom sums its own force: no atomic on a force, rows are sorted and the
// sum over a group has a fixed order, so two evaluations of one state give the same forces bit for bit.  Nothing is kept in a list of
// ROW_MAXIN: any number of neighbours is taken (rock salt has about 190 inside 10 A).
// Engine parts: the virial of the Born term goes to P_LJ, that of the Coulomb term to P_COUL; the energies reach SimScalars through
// k_row_finish, which the row stages share (eacc[0] -> eng[P_LJ], eacc[1] -> eng[P_ANGLE]).  Only the sums enter the stress and the
// total energy; the split is what scema_md_born_dsf_debug_compute reports as e_born and e_coul.
#include <hip/hip_runtime.h>

#include "md_born_dsf.h"
#include "md_ionic_force.h"

// Forces: the ionic body with bd_pair; the group's first lane adds the atom's self energy.
struct BdTerms {
  __device__ __forceinline__ const BdTable &bd(const BdTable &T) const { return T; }
  __device__ __forceinline__ void pair(const BdTable &T, const BdPairP &P, double qi, double qj, double r2, double *eb, double *ec, double *fb, double *fc) const {
    bd_pair(T, P, qi, qj, r2, eb, ec, fb, fc);
  }
  __device__ __forceinline__ void self(const BdTable &T, double qi, double &ecoul) const { ecoul += bd_self(T, qi); }
};
__global__ __launch_bounds__(ROW_FORCE_TPB) void k_bd_force(const SimDev *sims, const RowView *views) { ionic_force<BdTable>(sims, views, BdTerms()); }

void mdk_bd_forces(hipStream_t st, const SimDev *d, RowView *v, int ns, int maxatoms) {
  mdk_row_stage(st, d, v, ns, maxatoms, [&](dim3 gt) { hipLaunchKernelGGL(k_bd_force, gt, dim3(ROW_FORCE_TPB), 0, st, d, v); });
}
