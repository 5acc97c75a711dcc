// bonded_groups_host_driver.cpp -- the grouping of scema_amd/csrc/md_bonded_groups.h as a stand-alone program (no HIP): reads a topology as
// text, prints the dihedral groups, the left-over dihedrals, the hosts of the special pairs and, per group, the tiles that evaluate it,
// the tile that counts it and its two packed words (local index = atom & 1023).  tests/test_bonded_groups_host.py drives it; the same
// source is built once more with AddressSanitizer + UBSan.
//
// input:  natoms owners / rank[natoms] / ndih, then a b c d type per dihedral / npair, then a b / nbond, then a b / nangle, then a b c
// output: "G c2 c3 nk nm k0 k1 k2 m0 m1 m2 t0..t8 count_tile w0 w1 ntiles tiles..." per group, "L i" per left-over dihedral,
//         "P i kind host" per special pair, "B i pair" per bond, "A i pair" per angle
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../scema_amd/csrc/md_bonded_groups.h"

static int read_int(FILE *f) {
  int v;
  if (fscanf(f, "%d", &v) != 1) { fprintf(stderr, "bonded_groups_host_driver: short input\n"); exit(2); }
  return v;
}
static std::vector<int> read_rows(FILE *f, int width, int &n) {
  n = read_int(f);
  if (n < 0) { fprintf(stderr, "bonded_groups_host_driver: negative count\n"); exit(2); }
  std::vector<int> v((size_t)n * width);
  for (int &x : v) x = read_int(f);
  return v;
}

int main(int argc, char **argv) {
  FILE *f = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!f) { fprintf(stderr, "bonded_groups_host_driver: cannot open %s\n", argv[1]); return 2; }
  const int natoms = read_int(f), owners = read_int(f);
  std::vector<int> rank(natoms);
  for (int &r : rank) r = read_int(f);
  int ndih, npair, nbond, nangle;
  const std::vector<int> dih5 = read_rows(f, 5, ndih);
  const std::vector<int> pair = read_rows(f, 2, npair), bond = read_rows(f, 2, nbond), angle = read_rows(f, 3, nangle);
  if (f != stdin) fclose(f);
  std::vector<int> dih(4 * (size_t)ndih), type(ndih);
  for (int i = 0; i < ndih; i++) {
    for (int k = 0; k < 4; k++) dih[4 * i + k] = dih5[5 * i + k];
    type[i] = dih5[5 * i + 4];
  }
  const bonded_groups::DihedralGroups dg = bonded_groups::group_dihedrals(ndih, dih.data(), type.data());
  std::vector<int> tiles;
  for (const bonded_groups::Group &g : dg.groups) {
    int atoms[2 + 2 * BTG_SIDE];
    const int na = bonded_groups::group_atoms(g, atoms);
    bonded_groups::tiles_of(atoms, na, rank.data(), owners, tiles);
    const int ct = bonded_groups::group_count_tile(g, rank.data(), owners);
    unsigned long long w[2];
    bonded_groups::pack_group(g, [](int atom) { return atom & 1023; }, tiles[0] == ct, w);
    printf("G %d %d %d %d", g.c2, g.c3, g.nk, g.nm);
    for (int q = 0; q < BTG_SIDE; q++) printf(" %d", g.k[q]);
    for (int q = 0; q < BTG_SIDE; q++) printf(" %d", g.m[q]);
    for (int q = 0; q < BTG_SIDE * BTG_SIDE; q++) printf(" %d", g.type[q]);
    printf(" %d %llu %llu %zu", ct, w[0], w[1], tiles.size());
    for (int tl : tiles) printf(" %d", tl);
    printf("\n");
  }
  for (int i : dg.left) printf("L %d\n", i);
  const bonded_groups::SpecialHosts h = bonded_groups::attach_specials(npair, pair.data(), nbond, bond.data(), nangle, angle.data());
  for (int i = 0; i < npair; i++) printf("P %d %d %d\n", i, h.pair_host_kind[i], h.pair_host[i]);
  for (int i = 0; i < nbond; i++) printf("B %d %d\n", i, h.bond_pair[i]);
  for (int i = 0; i < nangle; i++) printf("A %d %d\n", i, h.angle_pair[i]);
  return 0;
}
