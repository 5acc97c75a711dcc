// The grid rule of the cell-binned row build (scema_amd/csrc/md_rowcells.h) compiled for the host: tests/test_rowcells_rule.py calls it
// through ctypes.  The header is the one k_cell_bin, k_cell_rows and the engine's layout include.
#include "../scema_amd/csrc/md_rowcells.h"

extern "C" {
int rch_maxcap() { return ROWCELL_MAXCAP; }
int rch_cells_per_pad() { return ROWCELL_CELLS_PER_PAD; }
int rch_min_atoms() { return ROWCELL_MIN_ATOMS; }
int rch_grid(const double *w, double rlist, const int *mimg, int cap, int n, int npad, int mode, int *nc) {
  return rowcell_grid(w, rlist, mimg, cap, n, npad, mode, nc);
}
int rch_of(double frac, int nc) { return rowcell_of(frac, nc); }
// the cells of n points x[n][3] in the box h (lx ly lz yz xz xy) at lo on the grid nc: cell[n] (x fastest) and the coordinates c3[n][3]
void rch_cells(int n, const double *x, const double *h, const double *lo, const int *nc, int *cell, int *c3) {
  for (int i = 0; i < n; i++) {
    double l[3];
    rowcell_frac(x + 3 * i, h, lo, l);
    for (int d = 0; d < 3; d++) c3[3 * i + d] = rowcell_of(l[d], nc[d]);
    cell[i] = rowcell_index(c3[3 * i], c3[3 * i + 1], c3[3 * i + 2], nc);
  }
}
}
