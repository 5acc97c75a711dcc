// sw_params.h -- reader of LAMMPS Stillinger-Weber parameter files (what `pair_coeff * * Si.sw Si` does in
// lammps_scripts_sisw/in.strain.lammps): the tables of the elements named, in the layout the kernels use (sw/sw_core.h).
#pragma once
#include <string>
#include <vector>

#include "../sw/sw_core.h"

namespace scema {

#define SW_EV_TO_KCALMOL 23.060549
#define SW_NFIELD 11   /* epsilon sigma a lambda gamma costheta0 A B p q tol */

// elements[k] = element symbol of LAMMPS atom type k + 1.  On success T holds the tables of the distinct elements (compact index =
// order of first appearance, at most SW_MAXEL) and type_map[k] the compact index of LAMMPS type k + 1.  raw, when given, receives the
// eleven numbers of every triplet kept as the file has them, [i][j][k][11].
// energy_unit 0: epsilon is in eV (the header of the reference's Si.sw) and is converted to kcal/mol; 1: epsilon is kcal/mol as written.
// False with a message in err: unreadable file, non-numeric field, short entry, a triplet of the named elements that the file lacks.
bool read_sw_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, SwTable &T, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *raw = nullptr);

}  // namespace scema
