// born_long_params.h -- the parameters of `pair_style born/coul/long` and `buck/coul/long`.  As for born/coul/dsf (born_dsf_params.h)
// LAMMPS has no parameter file for these styles: the parameters are the script lines themselves, and this reader takes them from any text
// file (in.strain.lammps included) into the layout the kernels use (ionic/bl_core.h).
#pragma once
#include <string>
#include <vector>

#include "../ionic/bl_core.h"
#include "born_dsf_params.h"

namespace scema {

// Words are blank-separated, `#` starts a comment.  The lines read:
//   pair_style born/coul/long <cut_lj> [<cut_coul>]             (cut_coul defaults to cut_lj)
//   pair_coeff I J A rho sigma C D [cut_lj]                     (I <= J: numeric types from 1, or `*` alone for either: every type)
// or
//   pair_style buck/coul/long <cut_lj> [<cut_coul>]
//   pair_coeff I J A rho C [cut_lj]                             (sigma = 0, D = 0 of the same table)
// and
//   kspace_style ewald|pppm <accuracy>                          (required: LAMMPS refuses the pair style without one)
//   units real|metal                                            (optional)
// and every other command but kspace_modify is ignored.  Types, `*`, overriding, energy_unit (0, 1, -1) and raw are those of
// read_born_dsf_params; has_style, when given, says whether a pair_style line of one of the two styles was seen (also on failure).
// False with "<path> line <n>: <reason>" in err: what read_born_dsf_params refuses (alpha apart), and: no kspace_style line (line 0) or
// two of them; a solver that is neither ewald nor pppm; an accuracy <= 0 or >= 1; a kspace_modify line (none of its options is honoured);
// a pair_coeff line with the word count of the other style.
bool read_born_long_params(const std::string &path, int energy_unit, BlTable &T, std::vector<int> &type_map, std::string &err,
                           std::vector<double> *raw = nullptr, bool *has_style = nullptr);

}  // namespace scema
