// ionic_script.h -- what the readers of the ionic styles' script lines share (born_dsf_params.cpp: born/coul/dsf; born_long_params.cpp:
// born/coul/long, buck/coul/long): the lines of a script by their command, numbers and type words, the units against energy_unit, the
// pair_coeff lines into BdTable::pair, and the error buffer of the C faces.  A reader keeps what is its own: its style line and the form
// of its pair_coeff line.  A helper that refuses says why (and where, if that is not the line it was given); the reader puts path and
// line in front.  Internal to host/.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <sstream>
#include <string>
#include <vector>

#include "born_dsf_params.h"

namespace scema {
namespace ionic_script {

struct Line { int ln; std::vector<std::string> w; };

// The lines of the file whose command is heads[k] into lines[k]: words are blank-separated, `#` starts a comment.  False with err: an
// energy unit that is none of -1, 0, 1; a file that cannot be opened
inline bool read_lines(const std::string &path, int energy_unit, std::initializer_list<const char *> heads, std::vector<std::vector<Line>> &lines, std::string &err) {
  if (energy_unit < -1 || energy_unit > 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: A, C and D eV-based, 1: in kcal/mol)";
    return false;
  }
  std::ifstream in(path);
  if (!in) {
    err = path + ": cannot open";
    return false;
  }
  lines.assign(heads.size(), {});
  std::string text;
  for (int ln = 1; std::getline(in, text); ln++) {
    const size_t h = text.find('#');
    if (h != std::string::npos) text.resize(h);
    std::istringstream ss(text);
    Line L{ln, {}};
    for (std::string s; ss >> s;) L.w.push_back(s);
    if (L.w.empty()) continue;
    size_t k = 0;
    for (const char *head : heads) {
      if (L.w[0] == head) { lines[k].push_back(L); break; }
      k++;
    }
  }
  return true;
}

// a whole word as a finite number
inline bool number(const std::string &s, double &v) {
  if (s.empty()) return false;
  char *end = nullptr;
  v = std::strtod(s.c_str(), &end);
  return end && *end == 0 && std::isfinite(v);
}

// the words of a line from word `from` on as finite numbers into v[0 ..]
inline bool numbers(const Line &L, size_t from, double *v, std::string &why) {
  for (size_t k = from; k < L.w.size(); k++)
    if (!number(L.w[k], v[k - from])) { why = "`" + L.w[k] + "` is not a finite number"; return false; }
  return true;
}

// a type word: `*` (0), a number from 1 to BD_MAXEL, or a reason
inline std::string type_word(const std::string &s, int &ty) {
  if (s == "*") { ty = 0; return ""; }
  if (s.find('*') != std::string::npos) return "a type range `" + s + "` is not taken (a type number, or `*` alone)";
  if (s.empty() || s.size() > 9 || !std::all_of(s.begin(), s.end(), [](char c) { return c >= '0' && c <= '9'; })) return "`" + s + "` is not an atom type";
  ty = std::atoi(s.c_str());
  if (ty < 1) return "atom types count from 1";
  if (ty > BD_MAXEL) return "atom type " + s + " is above the " + std::to_string(BD_MAXEL) + " types this stage holds";
  return "";
}

// the `units real|metal` lines against energy_unit (-1: the script decides, metal if it is silent): unit 1 for real, 0 for metal
inline bool resolve_units(const std::vector<Line> &units, int energy_unit, int &unit, int &ln, std::string &why) {
  unit = energy_unit;
  for (const Line &L : units) {
    ln = L.ln;
    if (L.w.size() != 2 || (L.w[1] != "real" && L.w[1] != "metal")) { why = "units must be real or metal"; return false; }
    const int u = L.w[1] == "real" ? 1 : 0;
    if (energy_unit == -1) {
      if (unit != -1 && unit != u) { why = "a second units line that contradicts the first"; return false; }
      unit = u;
    } else if (u != energy_unit) {
      why = "units " + L.w[1] + " contradicts energy unit " + std::to_string(energy_unit) + " (0: metal, 1: real)";
      return false;
    }
  }
  if (unit == -1) unit = 0;
  return true;
}

// one pair_coeff line: the types (0: `*`) and A rho sigma C D cut_lj as written
struct Coeff { int ln, i, j; double v[BD_NFIELD]; };

// `pair_coeff I J <numbers>` of a line whose word count the reader has checked: the types into c, the numbers into v[0 ..]
inline bool coeff_words(const Line &L, Coeff &c, double *v, std::string &why) {
  c.ln = L.ln;
  why = type_word(L.w[1], c.i);
  if (why.empty()) why = type_word(L.w[2], c.j);
  if (!why.empty()) return false;
  if (c.i && c.j && c.i > c.j) { why = "pair_coeff I J needs I <= J"; return false; }
  return numbers(L, 3, v, why);
}

// a line's six values, complete, join the list; ntypes follows the largest type named
inline bool coeff_add(const Coeff &c, std::vector<Coeff> &cs, int &ntypes, std::string &why) {
  if (!(c.v[1] > 0.0)) { why = "rho must be positive"; return false; }
  if (!(c.v[5] > 0.0)) { why = "a cutoff must be positive"; return false; }
  ntypes = std::max(ntypes, std::max(c.i, c.j));
  cs.push_back(c);
  return true;
}

// The coefficient lines into the zeroed table B, the types named first, then `*` over them; a later line overrides an earlier one.  Sets
// pair, ntypes, cut_coul, cutmax and K of the unit; vals receives A rho sigma C D cut_lj of every ordered pair, [n][n][BD_NFIELD], energies
// in kcal/mol; type_map becomes the identity.  `style` names the pair style where a pair I <= J of the types present is never set
inline bool expand(const std::vector<Coeff> &cs, int ntypes, int unit, double cut_coul, const std::string &style, BdTable &B, std::vector<double> &vals,
                   std::vector<int> &type_map, std::string &why) {
  if (ntypes == 0) ntypes = BD_MAXEL;   // (every line says `*`, or there is none: the missing pairs are named below)
  const double conv = unit == 0 ? BD_EV_TO_KCALMOL : 1.0;
  bool set[BD_MAXEL][BD_MAXEL] = {};
  vals.assign((size_t)ntypes * ntypes * BD_NFIELD, 0.0);
  B.cutmax = cut_coul;
  for (const Coeff &c : cs)
    for (int i = (c.i ? c.i : 1); i <= (c.i ? c.i : ntypes); i++)
      for (int j = std::max(i, c.j ? c.j : 1); j <= (c.j ? c.j : ntypes); j++) {
        for (int ord = 0; ord < 2; ord++) {
          const int a = (ord ? j : i) - 1, b = (ord ? i : j) - 1;
          BdPairP &P = B.pair[a * BD_MAXEL + b];
          P.a = c.v[0] * conv; P.irho = 1.0 / c.v[1]; P.sigma = c.v[2]; P.c = c.v[3] * conv; P.d = c.v[4] * conv; P.cut_lj2 = c.v[5] * c.v[5];
          double *o = &vals[((size_t)a * ntypes + b) * BD_NFIELD];
          o[0] = P.a; o[1] = c.v[1]; o[2] = P.sigma; o[3] = P.c; o[4] = P.d; o[5] = c.v[5];
          set[a][b] = true;
        }
      }
  for (int i = 0; i < ntypes; i++)
    for (int j = i; j < ntypes; j++) {
      if (!set[i][j]) {
        why = "no pair_coeff line sets the pair " + std::to_string(i + 1) + " " + std::to_string(j + 1) + " (" + style + " has no mixing rule)";
        return false;
      }
      B.cutmax = std::max(B.cutmax, std::sqrt(B.pair[i * BD_MAXEL + j].cut_lj2));
    }
  B.ntypes = ntypes;
  B.cut_coul = cut_coul;
  B.k = unit == 0 ? BD_COULOMB_EV * BD_EV_TO_KCALMOL : BD_COULOMB_KCALMOL;
  type_map.resize(ntypes);
  for (int k = 0; k < ntypes; k++) type_map[k] = k;
  return true;
}

// a message into the error buffer of a C entry point
inline void say(char *errbuf, int32_t errcap, const std::string &m) {
  if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
}

}  // namespace ionic_script
}  // namespace scema
