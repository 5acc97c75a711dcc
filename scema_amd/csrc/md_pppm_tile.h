// md_pppm_tile.h -- the tile rule of the tiled PPPM kernels (md_pppm.hip k_pppm_spread_tiled, k_pppm_force_tiled), one function for the host
// (launch shapes, scema_md_pppm_tile_shape) and the device (every workgroup derives its brick from the mesh of its replica).
// Tiles are bricks of by x bz mesh rows in (y, z) that span whole x rows; tile (ty_i, tz_i) owns the rows y0 = ty_i by .. , z0 = tz_i bz .. (the
// last tile of an axis may be shorter).  which = 0, charge assignment: the brick alone is kept, nx by bz doubles.  which = 1, interpolation:
// three field grids over the brick and a halo of two rows on each side of a tiled axis, 3 nx (by + 4)(bz + 4) doubles.
//   - a mesh that fits the budget whole is one tile;
//   - z-slabs (by = ny) while one plane (assignment) or five planes (interpolation) fit; y is tiled only beyond that;
//   - the tile counts follow from the largest brick that fits, the brick is then shrunk to the smallest that keeps those counts (even tiles);
//   - a mesh whose smallest brick -- one row, with its halo 5 x 5 rows -- does not fit: all zeros.
#pragma once
#if defined(__HIPCC__)
#define PPT_HD __host__ __device__
#else
#define PPT_HD
#endif

struct PppmTile { int by, bz, ty, tz; };

PPT_HD inline long long pppm_tile_bytes(int nx, int ny, int nz, int by, int bz, int which) {
  if (!which) return 8LL * nx * by * bz;
  return 24LL * nx * (by + (by < ny ? 4 : 0)) * (bz + (bz < nz ? 4 : 0));
}

PPT_HD inline PppmTile pppm_tile_shape(int nx, int ny, int nz, long long budget, int which) {
  PppmTile t = {0, 0, 0, 0};
  if (nx < 1 || ny < 1 || nz < 1 || budget <= 0) return t;
  const long long unit = (which ? 24LL : 8LL) * nx;   // one x row in every staged grid
  const int h = which ? 4 : 0;
  if (unit * ny * nz <= budget) { t.by = ny; t.bz = nz; t.ty = 1; t.tz = 1; return t; }
  long long by = ny, bz = budget / (unit * ny) - h;   // z-slabs (bz < nz: the mesh does not fit whole)
  if (bz < 1) {
    by = budget / (unit * (1 + h)) - h;   // rows of a brick one plane thick (by < ny: a slab that thick does not fit)
    if (by < 1) return t;
    t.ty = (int)((ny + by - 1) / by);
    by = (ny + t.ty - 1) / t.ty;
    bz = budget / (unit * (by + h)) - h;   // (what the evened-out rows leave)
    if (bz > nz) bz = nz;
  }
  t.ty = (int)((ny + by - 1) / by);
  t.tz = (int)((nz + bz - 1) / bz);
  bz = (nz + t.tz - 1) / t.tz;
  t.tz = (int)((nz + bz - 1) / bz);
  t.by = (int)by;
  t.bz = (int)bz;
  return t;
}
