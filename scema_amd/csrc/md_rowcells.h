// md_rowcells.h -- the grid rule of the cell-binned row build (md_rowcells.hip), for device and host code alike: plain
// inline functions, so that g++ compiles them for the CPU test of the rule (tests/rowcells_host_driver.cpp).
//   A replica's rows may be built through cells where every pair inside the list radius lies in cells that are periodic neighbours: the
//   grid lives in fractional coordinates of the step's box with ncell[d] = floor(w[d] / rlist) cells along box vector d, w[d] the
//   narrowest perpendicular width over the run.  Two atoms inside rlist differ by at most rlist / w_box[d] <= 1 / ncell[d] in fraction d
//   at every box of the run, so the 27-cell periodic stencil holds every partner; with 3 cells and more per dimension it meets each cell
//   once.
#pragma once

#if defined(__HIPCC__)
#define ROWCELL_HD __host__ __device__ inline
#else
#define ROWCELL_HD inline
#endif

#define ROWCELL_MAXCAP 1024        /* entries of one row the build kernel stages in LDS: a replica with a larger row capacity takes the N^2 build */
#define ROWCELL_CELLS_PER_PAD 2    /* cells of a grid <= this many times npad (a gas in a huge box): coarsened per dimension beyond it */
/* Replicas of fewer atoms take the N^2 build unless SCEMA_MD_ROW_CELLS=1.  The rule for it -- the smallest measured size from which the cell
 * path is no slower in the update time for SW and EAM alike -- gives no size up to 8 788 atoms (EAM is 1.3 % slower there and 3 % at 4 000:
 * one launch more per step, and a replica builds its rows once in some 660 steps), so the threshold stands at the first
 * atom count a row entry cannot hold (ROW_JMASK + 1): no replica takes the cell path by default, SCEMA_MD_ROW_CELLS=1 opts in. */
#define ROWCELL_MIN_ATOMS (1 << 24)

/* `mode` of rowcell_grid: SCEMA_MD_ROW_CELLS 0, 1, unset */
#define ROWCELL_OFF 0
#define ROWCELL_FORCE 1
#define ROWCELL_AUTO 2

// The grid of a replica of n atoms (npad: n rounded up to 64) with perpendicular widths w, list radius rlist, image search mimg and row
// capacity cap: 1 and nc[3] if its rows are built through cells, else 0 and nc = 0 0 0
ROWCELL_HD int rowcell_grid(const double w[3], double rlist, const int mimg[3], int cap, int n, int npad, int mode, int nc[3]) {
  nc[0] = nc[1] = nc[2] = 0;
  if (mode == ROWCELL_OFF) return 0;
  if (mimg[0] | mimg[1] | mimg[2]) return 0;
  if (cap > ROWCELL_MAXCAP) return 0;
  if (mode != ROWCELL_FORCE && n < ROWCELL_MIN_ATOMS) return 0;
  if (!(rlist > 0.0)) return 0;
  int c[3];
  for (int d = 0; d < 3; d++) {
    const double q = w[d] / rlist;
    if (!(q >= 3.0)) return 0;
    c[d] = q > 1024.0 ? 1024 : (int)q;   // (floor; 2^30 cells at the most)
  }
  // the cap: the dimension with the most cells gives one up, while it has more than 3 (27 cells never exceed 2 x 64)
  const long long most = (long long)ROWCELL_CELLS_PER_PAD * npad;
  while ((long long)c[0] * c[1] * c[2] > most) {
    int d = 0;
    if (c[1] > c[d]) d = 1;
    if (c[2] > c[d]) d = 2;
    if (c[d] <= 3) break;
    c[d] -= 1;
  }
  if ((long long)c[0] * c[1] * c[2] > most) return 0;
  nc[0] = c[0]; nc[1] = c[1]; nc[2] = c[2];
  return 1;
}

// the cell of a wrapped fractional coordinate along a dimension of nc cells: clamped, so that a fraction that rounds to 1.0 (or lies a
// rounding below 0) stays on the grid
ROWCELL_HD int rowcell_of(double frac, int nc) {
  const double s = frac * (double)nc;
  int c = s >= 0.0 ? (s < (double)nc ? (int)s : nc - 1) : 0;   // (a NaN lands in cell 0)
  if (c > nc - 1) c = nc - 1;
  return c;
}

// the fractional coordinates of a point in the box h (lx, ly, lz, yz, xz, xy) at lo: the arithmetic of k_row_wrap
ROWCELL_HD void rowcell_frac(const double x[3], const double h[6], const double lo[3], double l[3]) {
  l[2] = (x[2] - lo[2]) / h[2];
  l[1] = ((x[1] - lo[1]) - h[3] * l[2]) / h[1];
  l[0] = ((x[0] - lo[0]) - h[5] * l[1] - h[4] * l[2]) / h[0];
}

// the cell index of cell coordinates (x fastest)
ROWCELL_HD int rowcell_index(int cx, int cy, int cz, const int nc[3]) { return cx + nc[0] * (cy + nc[1] * cz); }
