// born_long_params.cpp -- reader of the script lines of `pair_style born/coul/long` and `buck/coul/long` (host/born_long_params.h) and
// its faces in the C ABI
#include "born_long_params.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "scema_md.h"

namespace scema {

namespace {

struct Line { int ln; std::vector<std::string> w; };

// a whole word as a finite number
bool number(const std::string &s, double &v) {
  if (s.empty()) return false;
  char *end = nullptr;
  v = std::strtod(s.c_str(), &end);
  return end && *end == 0 && std::isfinite(v);
}

// a type word: `*` (0), a number from 1 to BD_MAXEL, or a reason
std::string type_word(const std::string &s, int &ty) {
  if (s == "*") { ty = 0; return ""; }
  if (s.find('*') != std::string::npos) return "a type range `" + s + "` is not taken (a type number, or `*` alone)";
  if (s.empty() || s.size() > 9 || !std::all_of(s.begin(), s.end(), [](char c) { return c >= '0' && c <= '9'; })) return "`" + s + "` is not an atom type";
  ty = std::atoi(s.c_str());
  if (ty < 1) return "atom types count from 1";
  if (ty > BD_MAXEL) return "atom type " + s + " is above the " + std::to_string(BD_MAXEL) + " types this stage holds";
  return "";
}

bool long_style(const std::string &s) { return s == "born/coul/long" || s == "buck/coul/long"; }

}  // namespace

bool read_born_long_params(const std::string &path, int energy_unit, BlTable &T, std::vector<int> &type_map, std::string &err, std::vector<double> *raw,
                           bool *has_style) {
  if (has_style) *has_style = false;
  auto fail = [&](int ln, const std::string &why) {
    err = path + " line " + std::to_string(ln) + ": " + why;
    return false;
  };
  if (energy_unit < -1 || energy_unit > 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: A, C and D eV-based, 1: in kcal/mol)";
    return false;
  }
  std::ifstream in(path);
  if (!in) {
    err = path + ": cannot open";
    return false;
  }
  std::vector<Line> styles, coeffs, units, kstyles, kmods;
  std::string text;
  for (int ln = 1; std::getline(in, text); ln++) {
    const size_t h = text.find('#');
    if (h != std::string::npos) text.resize(h);
    std::istringstream ss(text);
    Line L{ln, {}};
    for (std::string s; ss >> s;) L.w.push_back(s);
    if (L.w.empty()) continue;
    if (L.w[0] == "pair_style") styles.push_back(L);
    else if (L.w[0] == "pair_coeff") coeffs.push_back(L);
    else if (L.w[0] == "units") units.push_back(L);
    else if (L.w[0] == "kspace_style") kstyles.push_back(L);
    else if (L.w[0] == "kspace_modify") kmods.push_back(L);
  }
  // the style
  for (const Line &L : styles)
    if (L.w.size() < 2 || !long_style(L.w[1]))
      return fail(L.ln, "pair_style " + (L.w.size() > 1 ? L.w[1] : std::string("(none)")) + " is neither born/coul/long nor buck/coul/long");
  if (styles.empty()) return fail(0, "no `pair_style born/coul/long <cut_lj> [<cut_coul>]` or `pair_style buck/coul/long ...` line");
  if (has_style) *has_style = true;
  if (styles.size() > 1) return fail(styles[1].ln, "a second pair_style line");
  const Line &S = styles[0];
  const bool buck = S.w[1] == "buck/coul/long";
  if (S.w.size() < 3 || S.w.size() > 4) return fail(S.ln, "expected `pair_style " + S.w[1] + " <cut_lj> [<cut_coul>]`");
  double cut_lj = 0.0, cut_coul = 0.0;
  for (size_t k = 2; k < S.w.size(); k++) {
    double v;
    if (!number(S.w[k], v)) return fail(S.ln, "`" + S.w[k] + "` is not a finite number");
  }
  number(S.w[2], cut_lj);
  cut_coul = cut_lj;
  if (S.w.size() == 4) number(S.w[3], cut_coul);
  if (!(cut_lj > 0.0) || !(cut_coul > 0.0)) return fail(S.ln, "a cutoff must be positive");
  // the solver
  if (!kmods.empty()) return fail(kmods[0].ln, "a kspace_modify line: none of its options is honoured");
  if (kstyles.empty()) return fail(0, "no `kspace_style ewald|pppm <accuracy>` line (" + S.w[1] + " needs a long-range solver)");
  if (kstyles.size() > 1) return fail(kstyles[1].ln, "a second kspace_style line");
  const Line &Ks = kstyles[0];
  if (Ks.w.size() < 2 || (Ks.w[1] != "ewald" && Ks.w[1] != "pppm"))
    return fail(Ks.ln, "kspace_style " + (Ks.w.size() > 1 ? Ks.w[1] : std::string("(none)")) + " is neither ewald nor pppm");
  if (Ks.w.size() != 3) return fail(Ks.ln, "expected `kspace_style " + Ks.w[1] + " <accuracy>`");
  double accuracy = 0.0;
  if (!number(Ks.w[2], accuracy)) return fail(Ks.ln, "`" + Ks.w[2] + "` is not a finite number");
  if (!(accuracy > 0.0) || !(accuracy < 1.0)) return fail(Ks.ln, "the accuracy must be above 0 and below 1");
  // the units
  int unit = energy_unit;
  for (const Line &L : units) {
    if (L.w.size() != 2 || (L.w[1] != "real" && L.w[1] != "metal")) return fail(L.ln, "units must be real or metal");
    const int u = L.w[1] == "real" ? 1 : 0;
    if (energy_unit == -1) {
      if (unit != -1 && unit != u) return fail(L.ln, "a second units line that contradicts the first");
      unit = u;
    } else if (u != energy_unit) {
      return fail(L.ln, "units " + L.w[1] + " contradicts energy unit " + std::to_string(energy_unit) + " (0: metal, 1: real)");
    }
  }
  if (unit == -1) unit = 0;
  const double conv = unit == 0 ? BD_EV_TO_KCALMOL : 1.0;
  // the coefficients: the types named first, then `*` over them
  struct Coeff { int ln, i, j; double v[BD_NFIELD]; };
  std::vector<Coeff> cs;
  int ntypes = 0;
  const size_t nw = buck ? 6 : 8;   // words of a pair_coeff line without its own cutoff
  for (const Line &L : coeffs) {
    if (L.w.size() < nw || L.w.size() > nw + 1)
      return fail(L.ln, buck ? "expected `pair_coeff I J A rho C [cut_lj]` (buck/coul/long)" : "expected `pair_coeff I J A rho sigma C D [cut_lj]` (born/coul/long)");
    Coeff c;
    c.ln = L.ln;
    std::string why = type_word(L.w[1], c.i);
    if (why.empty()) why = type_word(L.w[2], c.j);
    if (!why.empty()) return fail(L.ln, why);
    if (c.i && c.j && c.i > c.j) return fail(L.ln, "pair_coeff I J needs I <= J");
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, cut_lj};
    for (size_t k = 3; k < L.w.size(); k++)
      if (!number(L.w[k], v[k - 3])) return fail(L.ln, "`" + L.w[k] + "` is not a finite number");
    if (buck) {   // A rho C [cut]: sigma = 0, D = 0
      c.v[0] = v[0]; c.v[1] = v[1]; c.v[2] = 0.0; c.v[3] = v[2]; c.v[4] = 0.0; c.v[5] = L.w.size() == nw + 1 ? v[3] : cut_lj;
    } else {
      for (int k = 0; k < 6; k++) c.v[k] = v[k];
    }
    if (!(c.v[1] > 0.0)) return fail(L.ln, "rho must be positive");
    if (!(c.v[5] > 0.0)) return fail(L.ln, "a cutoff must be positive");
    ntypes = std::max(ntypes, std::max(c.i, c.j));
    cs.push_back(c);
  }
  if (ntypes == 0) ntypes = BD_MAXEL;   // (every line says `*`, or there is none: the missing pairs are named below)
  std::memset(&T, 0, sizeof T);
  BdTable &B = T.bd;
  bool set[BD_MAXEL][BD_MAXEL] = {};
  std::vector<double> vals((size_t)ntypes * ntypes * BD_NFIELD, 0.0);
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
      if (!set[i][j])
        return fail(S.ln, "no pair_coeff line sets the pair " + std::to_string(i + 1) + " " + std::to_string(j + 1) + " (" + S.w[1] + " has no mixing rule)");
      B.cutmax = std::max(B.cutmax, std::sqrt(B.pair[i * BD_MAXEL + j].cut_lj2));
    }
  B.ntypes = ntypes;
  B.cut_coul = cut_coul;
  B.k = unit == 0 ? BD_COULOMB_EV * BD_EV_TO_KCALMOL : BD_COULOMB_KCALMOL;
  T.accuracy = accuracy;
  T.pppm = Ks.w[1] == "pppm" ? 1 : 0;
  T.buck = buck ? 1 : 0;
  type_map.resize(ntypes);
  for (int k = 0; k < ntypes; k++) type_map[k] = k;
  if (raw) *raw = vals;
  return true;
}

}  // namespace scema

namespace {
void say(char *errbuf, int32_t errcap, const std::string &m) {
  if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
}
}  // namespace

extern "C" int scema_md_born_long_read_params(const char *path, int32_t energy_unit, int32_t *n_types, double *head, double *values, char *errbuf,
                                              int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1)) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BlTable T;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_born_long_params(path, energy_unit, T, map, err, &raw)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (n_types) *n_types = T.bd.ntypes;
  if (head) { head[0] = T.bd.cut_coul; head[1] = T.accuracy; head[2] = T.pppm; head[3] = T.bd.k; head[4] = T.bd.cutmax; head[5] = T.buck; }
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}

extern "C" int scema_md_born_long_eval(const char *path, int32_t energy_unit, double g_ewald, int32_t ti, int32_t tj, double qi, double qj, const double *r,
                                       int32_t n, double *out, char *errbuf, int32_t errcap) {
  say(errbuf, errcap, "");
  if (!path || (energy_unit != 0 && energy_unit != 1) || n < 0 || (n > 0 && (!r || !out)) || !(g_ewald >= 0.0)) { say(errbuf, errcap, "bad arguments"); return SCEMA_MD_ERR_ARG; }
  BlTable T;
  std::vector<int> map;
  std::string err;
  if (!scema::read_born_long_params(path, energy_unit, T, map, err)) { say(errbuf, errcap, err); return SCEMA_MD_ERR_IO; }
  if (ti < 0 || tj < 0 || ti >= T.bd.ntypes || tj >= T.bd.ntypes) { say(errbuf, errcap, "a type beyond the file's"); return SCEMA_MD_ERR_ARG; }
  for (int k = 0; k < n; k++) bl_pair(T, T.bd.pair[ti * BD_MAXEL + tj], g_ewald, qi, qj, r[k] * r[k], &out[4 * k], &out[4 * k + 1], &out[4 * k + 2], &out[4 * k + 3]);
  return SCEMA_MD_OK;
}
