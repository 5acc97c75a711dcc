// meam_spline_params.h -- reader of LAMMPS spline-MEAM files (what `pair_style meam/spline` + `pair_coeff * * Ti.meam.spline Ti`, or
// `pair_coeff * * TiO.meam.spline Ti O`, does): the splines of the elements named, in the layout the kernels use (meam_spline/ms_core.h).
#pragma once
#include <string>
#include <vector>

#include "../meam_spline/ms_core.h"

namespace scema {

#define MS_EV_TO_KCALMOL 23.060549

// elements[k] = element symbol of LAMMPS atom type k + 1.  Two formats:
//   old, one element .... a comment line, then phi, rho, U, f, g, each as: a line `N`, a line `d0 dN` (the end slopes), one line that is
//                         skipped, N lines `x y y2` (y2 is read and ignored: the second derivatives come from the solve here).  The file
//                         names no element: every name of `elements` maps to its one element.
//   new, n elements ..... a comment line, `meam/spline <n> <El1> .. <Eln>`, then the families phi, rho, U, f, g (pair families as the
//                         upper triangle, row-major), each spline as: a line `spline3eq`, `N`, `d0 dN`, N lines `x y y2`.
// On success T holds the splines of the distinct elements named (compact index = order of first appearance, at most MS_MAXEL) and
// type_map[k] the compact index of LAMMPS type k + 1.  energy_unit 0: phi and U are eV (units metal) and are converted to kcal/mol; 1:
// as written.  False with `path: message` in err, the line named: unreadable or truncated file, N < 2 or N > MS_MAXKNOT, knots not
// strictly ascending, a word that is no finite number, a missing `spline3eq`, an element count that disagrees with the header's list, more
// than MS_MAXEL elements kept, an empty name or a name the file lacks (NULL included), a phi, rho or f that does not end with value 0
// and slope 0 (the energy would jump at the cutoff).
bool read_meam_spline(const std::string &path, const std::vector<std::string> &elements, int energy_unit, MsTable &T, std::vector<int> &type_map,
                      std::string &err);

}  // namespace scema
