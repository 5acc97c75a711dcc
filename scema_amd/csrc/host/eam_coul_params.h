// eam_coul_params.h -- the parameters of `pair_style hybrid/overlay coul/long <cut_coul> eam/alloy`: the many-body oxide models that add
// an embedded-atom term to a long-range Coulomb sum.  As for the ionic styles (born_long_params.h) the parameters are the script lines
// themselves, read from any text file (in.strain.lammps included); the embedded-atom tables are the setfl file the script names
// (eam_setfl.h).  The block the kernels use is eam/ec_core.h.
#pragma once
#include <string>
#include <vector>

#include "../eam/ec_core.h"
#include "born_dsf_params.h"

namespace scema {

struct EamCoulParams {
  double cut_coul = 0.0, accuracy = 0.0;
  int pppm = 0;                          // 1: the script said `kspace_style pppm`
  int unit = 0;                          // 0: metal, 1: real (energy_unit, or what the script says where energy_unit is -1)
  double k = 0.0;                        // the Coulomb constant in kcal A/mol
  std::string setfl;                     // the setfl file, resolved
  std::vector<std::string> elements;     // one per atom type
};

// Words are blank-separated, `#` starts a comment.  The lines read:
//   pair_style hybrid/overlay coul/long <cut_coul> eam/alloy      (the two sub-styles in either order)
//   pair_coeff * * coul/long
//   pair_coeff * * eam/alloy <file> <El> ...                      (one element per atom type)
//   kspace_style ewald|pppm <accuracy>
//   units real|metal                                              (optional)
// and every other command but kspace_modify is ignored.  <file> with a `${locs}/` prefix, or a relative name, is taken relative to the
// script's own folder; an absolute path as given.  energy_unit 0, 1, -1 as for read_born_dsf_params.  has_style, when given, says
// whether a `pair_style hybrid/overlay` line was seen (also on failure).  The setfl file is not opened here.
// False with "<path> line <n>: <reason>" in err: no pair_style line (line 0) or two of them; a pair style that is not hybrid/overlay; a
// third sub-style or another sub-style, a sub-style twice; cut_coul missing, not a number or <= 0; either pair_coeff line missing (line
// 0) or given twice, one that does not start `* *`, one for another sub-style; surplus words on the coul/long line; no file or no
// element on the eam/alloy line, NULL as an element; no kspace_style line (line 0) or two, a solver that is neither ewald nor pppm, an
// accuracy outside (0, 1); a kspace_modify line; a units line that is neither real nor metal or that contradicts energy_unit.
bool read_eam_coul_script(const std::string &path, int energy_unit, EamCoulParams &P, std::string &err, bool *has_style = nullptr);

// The script, then the setfl file it names (read_eam_setfl: its refusals are passed on as they are), into the block of eam/ec_core.h:
// a BlTable with zero Born pairs, cut_coul, K, cutmax = max(setfl cutoff, cut_coul), accuracy and solver word; the EAM block at
// EC_EAM_OFF.  type_map is that of read_eam_setfl over the script's elements.
bool build_eam_coul_block(const std::string &path, int energy_unit, std::vector<double> &block, std::vector<int> &type_map, EamCoulParams &P, std::string &err,
                          bool *has_style = nullptr);

inline const BlTable &eam_coul_table(const std::vector<double> &block) { return *(const BlTable *)block.data(); }
inline const EamHead &eam_coul_head(const std::vector<double> &block) { return *(const EamHead *)(block.data() + EC_EAM_OFF); }

}  // namespace scema
