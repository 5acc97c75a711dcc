// edip_params.h -- reader of LAMMPS EDIP parameter files (what `pair_style edip` + `pair_coeff * * Si.edip Si`, or `pair_style edip/multi`
// + `pair_coeff * * SiC.edip Si C`, does): the tables of the elements named, in the layout the kernel uses (edip/edip_core.h).
#pragma once
#include <string>
#include <vector>

#include "../edip/edip_core.h"

namespace scema {

#define EDIP_EV_TO_KCALMOL 23.060549
#define EDIP_NFIELD 17   /* A B cutoffA cutoffC alpha beta eta gamma lambda mu rho sigma Q0 u1 u2 u3 u4 */

// elements[k] = element symbol of LAMMPS atom type k + 1.  On success T holds the tables of the distinct elements (compact index =
// order of first appearance, at most EDIP_MAXEL) and type_map[k] the compact index of LAMMPS type k + 1.  raw, when given, receives the
// seventeen numbers of every triplet kept, [i][j][k][17], A and lambda in kcal/mol.  energy_unit 0: A and lambda are eV (units metal)
// and are converted to kcal/mol; 1: the numbers as written.
// False with a message in err: what read_triplet_file refuses (host/triplet_file.h); in an entry i j j: cutoffA <= 0, cutoffC < 0,
// cutoffC >= cutoffA, a negative alpha, sigma, gamma or rho (a message each), B <= 0 with A != 0; entries i j k and i k j whose eight triplet numbers
// (eta lambda mu Q0 u1 u2 u3 u4) differ (the sum over j < k must not depend on the order of a row); entries i j j and j i i whose
// cutoffA differ (a pair has one cutoff at both ends).
bool read_edip_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, EdipTable &T, std::vector<int> &type_map,
                      std::string &err, std::vector<double> *raw = nullptr);

}  // namespace scema
