// vashishta_params.h -- reader of LAMMPS Vashishta parameter files (what `pair_style vashishta` + `pair_coeff * * SiC.vashishta Si C`
// does): the tables of the elements named, in the layout the kernel uses (vashishta/vs_core.h).
#pragma once
#include <string>
#include <vector>

#include "../vashishta/vs_core.h"

namespace scema {

#define VS_EV_TO_KCALMOL 23.060549
#define VS_COULOMB_EV 14.399645       /* K in eV A (units metal) */
#define VS_COULOMB_KCALMOL 332.06371  /* K in kcal/mol A (units real) */
#define VS_NFIELD 14   /* H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta0 */

// elements[k] = element symbol of LAMMPS atom type k + 1.  On success T holds the tables of the distinct elements (compact index =
// order of first appearance, at most VS_MAXEL), with the shift constants U(rc), U'(rc) of every pair, and type_map[k] the compact index
// of LAMMPS type k + 1.  raw, when given, receives the fourteen numbers of every triplet kept, [i][j][k][14], energies in kcal/mol.
// energy_unit 0: H, D, W and B are eV-based (units metal), K = 14.399645 eV A, everything converted to kcal/mol; 1: the numbers as
// written, K = 332.06371.
// False with a message in err: what read_triplet_file refuses (host/triplet_file.h); in an entry i j j: rc <= 0, eta <= 0 with H != 0, a
// negative lambda1, lambda4, gamma or r0, r0 > rc; a negative C in any entry; entries i j j and j i i whose rc or r0 differ (a pair has
// one cutoff at both ends: each end of a pair sums its own half).
bool read_vashishta_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, VsTable &T, std::vector<int> &type_map,
                           std::string &err, std::vector<double> *raw = nullptr);

}  // namespace scema
