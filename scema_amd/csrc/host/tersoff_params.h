// tersoff_params.h -- reader of LAMMPS Tersoff parameter files (what `pair_style tersoff` + `pair_coeff * * SiC.tersoff Si C` does): the
// tables of the elements named, in the layout the kernels use (tersoff/ts_core.h).
#pragma once
#include <string>
#include <vector>

#include "../tersoff/ts_core.h"

namespace scema {

#define TS_EV_TO_KCALMOL 23.060549
#define TS_NFIELD 14   /* m gamma lambda3 c d costheta0 n beta lambda2 B R D lambda1 A */

// elements[k] = element symbol of LAMMPS atom type k + 1.  On success T holds the tables of the distinct elements (compact index =
// order of first appearance, at most TS_MAXEL) and type_map[k] the compact index of LAMMPS type k + 1.  raw, when given, receives the
// fourteen numbers of every triplet kept, [i][j][k][14], A and B in kcal/mol.
// energy_unit 0: A and B are in eV (units metal, as the files LAMMPS ships) and are converted to kcal/mol; 1: kcal/mol as written.
// False with a message in err: unreadable file, non-numeric field, short or duplicate entry, a negative c, d, n, beta, lambda2, B, R, D,
// lambda1, A or gamma, D > R, m other than 1 or 3, n = 0 in an entry i j j (the switch points of b would not exist), a triplet of the named
// elements that the file lacks.
bool read_tersoff_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsTable &T, std::vector<int> &type_map,
                         std::string &err, std::vector<double> *raw = nullptr);

}  // namespace scema
