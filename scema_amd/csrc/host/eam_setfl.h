// eam_setfl.h -- reader of DYNAMO setfl files (what `pair_style eam/alloy` + `pair_coeff * * CuAg.eam.alloy Cu Ag` does): the spline
// tables of the elements named, in the one flat block the kernels use (eam/eam_core.h).
#pragma once
#include <string>
#include <vector>

#include "../eam/adp_core.h"
#include "../eam/eam_core.h"

namespace scema {

#define EAM_EV_TO_KCALMOL 23.060549

// elements[k] = element symbol of LAMMPS atom type k + 1, in any order, repeats allowed.  On success `block` holds an EamHead and the
// tables of the distinct elements (compact index = order of first appearance, at most EAM_MAXEL), as doubles (EamHead::ndoubles of them);
// type_map[k] is the compact index of LAMMPS type k + 1; masses, when given, the file's masses of the kept elements (read and checked,
// not applied: masses come from the replica).
// energy_unit 0: F and r phi are in eV and eV A (units metal, as the files LAMMPS ships) and are converted to kcal/mol with 23.060549;
// 1: as written.  The density has no unit.
// The layout: three comment lines; `Nelements name ...`; `Nrho drho Nr dr cutoff`; per element `Z mass a0 lattice`, Nrho values of F, Nr
// values of rho(r); then for every pair i >= j in file order Nr values of r phi_ij(r).  Numbers are free-format across lines.
// False with `path: message` in err: unreadable, short or truncated file, a non-numeric field, Nr or Nrho below 5 (the end formulae of
// the spline need five knots), dr, drho or cutoff not positive, a cutoff beyond (Nr - 1) dr, a mass not positive, an element that the
// file lacks, more than EAM_MAXEL distinct elements, counts that the file's length cannot hold (checked before anything is allocated).
bool read_eam_setfl(const std::string &path, const std::vector<std::string> &elements, int energy_unit, std::vector<double> &block, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *masses = nullptr);

inline const EamHead &eam_head(const std::vector<double> &block) { return *(const EamHead *)block.data(); }

// The same for the extended setfl files of `pair_style adp` (`pair_coeff * * CuAg.adp Cu Ag`): after the r phi tables come, for every
// pair i >= j in file order, Nr values of u_ij(r), then in the same order Nr values of w_ij(r), as written (not multiplied by r).  The
// block starts with an AdpHead (eam/adp_core.h): its EAM part is laid out exactly as read_eam_setfl lays it out, the u records and then
// the w records of the kept pairs follow the r phi records.  energy_unit 0 converts F and r phi with 23.060549 and u and w with its
// square root (mu^2 and lam^2 are energies); 1: everything as written.  The refusals are those of read_eam_setfl; a file that ends
// inside the u or the w tables (a plain eam/alloy file among them) is refused by its counts before anything is sized.
bool read_adp_setfl(const std::string &path, const std::vector<std::string> &elements, int energy_unit, std::vector<double> &block, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *masses = nullptr);

inline const AdpHead &adp_head(const std::vector<double> &block) { return *(const AdpHead *)block.data(); }

}  // namespace scema
