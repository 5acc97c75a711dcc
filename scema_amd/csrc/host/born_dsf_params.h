// born_dsf_params.h -- the parameters of `pair_style born/coul/dsf`.  LAMMPS has no parameter file for this style: the parameters are the
// script lines themselves, and this reader takes them from any text file (in.strain.lammps included) into the layout the kernel uses
// (ionic/bd_core.h).
#pragma once
#include <string>
#include <vector>

#include "../ionic/bd_core.h"

namespace scema {

#define BD_EV_TO_KCALMOL 23.060549
#define BD_COULOMB_EV 14.399645       /* K in eV A (units metal) */
#define BD_COULOMB_KCALMOL 332.06371  /* K in kcal A/mol (units real, MD_QQRD2E) */
#define BD_NFIELD 6   /* A rho sigma C D cut_lj */

// Words are blank-separated, `#` starts a comment.  The lines read:
//   pair_style born/coul/dsf <alpha> <cut_lj> [<cut_coul>]      (cut_coul defaults to cut_lj)
//   pair_coeff I J A rho sigma C D [cut_lj]                     (I <= J: numeric types from 1, or `*` alone for either: every type)
//   units real|metal                                            (optional)
// and every other command is ignored.  The fragment's number of types is the largest type a pair_coeff line names (BD_MAXEL where every
// line says `*`); type_map becomes the identity over them.  A later pair_coeff line overrides an earlier one, as in LAMMPS.
// energy_unit 0: A, C and D are eV-based (units metal), K = 14.399645 eV A, everything converted to kcal/mol; 1: the numbers as written,
// K = 332.06371; -1: 1 iff the text says `units real`, else 0 (self-configuration).  raw, when given, receives A rho sigma C D cut_lj of
// every ordered pair, [n][n][6], energies in kcal/mol; has_style, when given, says whether a `pair_style born/coul/dsf` line was seen
// (also on failure).
// False with "<path> line <n>: <reason>" in err: no pair_style line (line 0) or two of them; another pair style; alpha <= 0, a cutoff <= 0,
// rho <= 0; a word that is not a finite number, a missing or surplus word; I > J, a range m*n, a type below 1 or above BD_MAXEL; a pair
// I <= J of the types present that is never set (there is no mixing rule); a units line that is neither real nor metal or that
// contradicts energy_unit 0 or 1.
bool read_born_dsf_params(const std::string &path, int energy_unit, BdTable &T, std::vector<int> &type_map, std::string &err,
                          std::vector<double> *raw = nullptr, bool *has_style = nullptr);

}  // namespace scema
