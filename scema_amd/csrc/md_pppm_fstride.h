// md_pppm_fstride.h -- where a field point lies in the LDS copy of k_pppm_force<true, *> (md_pppm.hip): one function for the host (the
// launch's LDS size, scema_md_pppm_force_strides) and the device (every workgroup derives the layout from the mesh of its replica).
// Point (gx, gy, gz) of field f lies at double f * ps * nz + gz * ps + gy * rs + gx.  The dense layout is rs = nx, ps = nx * ny.
//
// Why not dense: a ds_read_b64 is served per group of 32 lanes, and two doubles share a bank pair when their indices agree mod 32.
// Consecutive lanes hold consecutive atoms, which are neighbours in space: their stencil points differ by a few planes and a point or two
// within the plane.  With a plane stride of 144 (12 x 12 x 12) planes z, z + 2, z + 4 fall on the same banks and every read of PE-10k is
// served in three turns (tools/pppm_bank_model.py: 6.0 cycles per wave read against 2.0 without conflicts).
//
// The rule: rows stay dense (a padded row costs ny * nz doubles per point and buys nothing a plane stride does not: the model has
// (13, 158) at 2.43 and (12, 146) at 2.46 on PE-10k).  The plane stride is nx * ny + p, p = 0 .. 7, the p for which the fewest of the next
// five planes put a point within two steps in the plane, |dx| + |dy| <= 2, on the bank pair of the point itself; ties take the smaller p.
// The padded layout is taken only where
//   - it fits the budget and the dense copy does too (the 6 144-point rule that decides staged against tiled is about the dense size),
//   - it keeps every workgroup the dense copy has resident on a CU (checked for workgroups of 256 threads, up to five per CU; the kernel's
//     other block size, 512 threads, holds two at most and keeps them wherever 256 threads keep theirs), and
//   - every dimension of the mesh is longer than the stencil: with five points or fewer in a dimension a single atom's reads already
//     cover it and wrap; on such meshes (a few hundred atoms at most) the model finds the dense layout at or next to the best of all
//     plane strides on the test lattices, and no stride that is better on all of them.
// Everywhere else the dense strides come back.  Integer arithmetic only: host and device agree to the bit.
#pragma once
#if defined(__HIPCC__)
#define PPF_HD __host__ __device__
#else
#define PPF_HD
#endif

#define PP_FS_TPB 256              // the smaller block size of k_pppm_force<true, *>: the one with more workgroups per CU to lose
#define PP_FS_CU_LDS (160 * 1024)  // LDS of a CU
#define PP_FS_CU_WAVES 20          // waves a CU holds at the kernel's 95 VGPRs (5 per SIMD)
#define PP_FS_MAXPAD 7
#define PP_FS_PLANES 5

struct PppmFStride { int rs, ps; long long bytes; };   // row stride, plane stride (doubles); LDS bytes of the three fields

// workgroups of the kernel's block size a CU holds with `bytes` of LDS each (0 < bytes <= PP_FS_CU_LDS)
PPF_HD inline int pppm_fstride_resident(int bytes) {
  const int by_lds = PP_FS_CU_LDS / bytes, by_waves = PP_FS_CU_WAVES / (PP_FS_TPB / 64);
  return by_lds < by_waves ? by_lds : by_waves;
}

PPF_HD inline PppmFStride pppm_fstride_dense(int nx, int ny, int nz) {
  const PppmFStride d = {nx, nx * ny, 24LL * nx * ny * nz};
  return d;
}

PPF_HD inline PppmFStride pppm_fstride(int nx, int ny, int nz, long long budget) {
  const PppmFStride dense = pppm_fstride_dense(nx, ny, nz);
  if (nx <= 5 || ny <= 5 || nz <= 5 || dense.bytes > budget || dense.bytes > PP_FS_CU_LDS) return dense;
  // bank pairs (index mod 32) of the points within two steps of a point in its own plane (the set is its own mirror image: planes above
  // stand for planes below)
  unsigned near = 0u;
  for (int dy = -2; dy <= 2; dy++) {
    const int w = 2 - (dy < 0 ? -dy : dy);
    for (int dx = -w; dx <= w; dx++) near |= 1u << ((unsigned)(dy * nx + dx) & 31u);
  }
  const int cap = (int)(budget < PP_FS_CU_LDS ? budget : PP_FS_CU_LDS);   // (the dense copy fits it: all sizes below are ints)
  const int resident = pppm_fstride_resident((int)dense.bytes);
  int best_p = 0, best_hits = PP_FS_PLANES + 1;
  for (int p = 0; p <= PP_FS_MAXPAD; p++) {
    const int bytes = 24 * (dense.ps + p) * nz;
    if (bytes > cap || bytes * resident > PP_FS_CU_LDS) break;   // beyond the budget, or a resident workgroup fewer
    int hits = 0;
    for (int dz = 1; dz <= PP_FS_PLANES; dz++) hits += (int)((near >> ((unsigned)(dz * (dense.ps + p)) & 31u)) & 1u);
    if (hits < best_hits) { best_hits = hits; best_p = p; }
  }
  const PppmFStride out = {nx, dense.ps + best_p, 24LL * (dense.ps + best_p) * nz};
  return out;
}
