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

// ---- the forms tersoff/mod, tersoff/mod/c and tersoff/zbl (tersoff/ts_core.h).  Arguments, energy unit and `raw` as above, with
// TS_FORM_NFIELD numbers per triplet for both forms ----
#define TS_FORM_NFIELD 18
#define TS_MOD_NCOL 17   /* beta alpha h eta beta_ters lambda2 B R D lambda1 A n c1 c2 c3 c4 c5; a mod/c file has an 18th, c0 */

// `pair_style tersoff/mod` and `tersoff/mod/c`.  A file is recognised as mod/c by its FIRST entry: if the three element names are followed
// by 18 numeric words before the next word that is no number (or the end of the file), every entry has 18 numbers; otherwise every entry
// has 17 and c0 = 0 is filled in.  (A mod/c file holding one entry short by a number is therefore read as a mod file and ends in "short
// entry" or "where an element name is expected".)  c0 is an energy and is converted as A and B are.
// False with a message: as read_tersoff_params, and beta_ters other than 1, beta other than 1 or 3, a negative alpha, eta, lambda2, B, R,
// D, lambda1, A, n, c2, c3, c4 or c5, D > R, n = 0 or eta = 0 in an entry i j j, c3 = 0 with -1 <= h <= 1 (cos theta can reach h,
// where g would be 0/0; with h outside that range (h - cos)^2 > 0 and c3 = 0 is let through).
bool read_tersoff_mod_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsModTable &T, std::vector<int> &type_map,
                             std::string &err, std::vector<double> *raw = nullptr);

// `pair_style tersoff/zbl`: the fourteen numbers of a plain entry, then Z_i Z_j ZBLcut ZBLexpscale (the four of entry i j j are used).
// energy_unit 0: A, B in eV, K = 1/(4 pi 0.00552635) eV A, all converted with 23.060549; 1: A and B as written, K / 0.043365121 (what
// LAMMPS' `units real` gives).  False with a message: as read_tersoff_params, and Z_i <= 0 or Z_j <= 0, ZBLcut < 0, ZBLexpscale < 0.
bool read_tersoff_zbl_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsZblTable &T, std::vector<int> &type_map,
                             std::string &err, std::vector<double> *raw = nullptr);

}  // namespace scema
