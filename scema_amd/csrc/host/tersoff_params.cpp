// tersoff_params.cpp -- reader of LAMMPS Tersoff parameter files (host/tersoff_params.h) and its face in the C ABI
#include "tersoff_params.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "scema_md.h"

namespace scema {

namespace {
struct Tok { std::string s; int line; };
enum { F_M, F_GAMMA, F_LAM3, F_C, F_D, F_COS0, F_N, F_BETA, F_LAM2, F_B, F_R, F_BIGD, F_LAM1, F_A };
const int NW = 3 + TS_NFIELD;
}  // namespace

bool read_tersoff_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsTable &T, std::vector<int> &type_map,
                         std::string &err, std::vector<double> *raw) {
  auto bad = [&](const std::string &m) { err = path + ": " + m; return false; };
  if (energy_unit != 0 && energy_unit != 1) return bad("energy unit " + std::to_string(energy_unit) + " (0: A and B in eV, 1: in kcal/mol)");
  if (elements.empty()) return bad("no elements named");
  // the distinct elements in order of first appearance
  std::vector<std::string> el;
  type_map.assign(elements.size(), 0);
  for (size_t k = 0; k < elements.size(); k++) {
    if (elements[k].empty()) return bad("empty element name");
    size_t m = 0;
    while (m < el.size() && el[m] != elements[k]) m++;
    if (m == el.size()) el.push_back(elements[k]);
    type_map[k] = (int)m;
  }
  const int ne = (int)el.size();
  if (ne > TS_MAXEL) return bad("more than " + std::to_string(TS_MAXEL) + " distinct elements");
  std::ifstream in(path);
  if (!in) return bad("cannot open");
  // an entry is 17 words, on one line or several; `#` starts a comment
  std::vector<Tok> tok;
  std::string line;
  for (int ln = 1; std::getline(in, line); ln++) {
    const size_t h = line.find('#');
    if (h != std::string::npos) line.resize(h);
    std::istringstream ss(line);
    std::string w;
    while (ss >> w) tok.push_back({w, ln});
  }
  auto show = [](const std::string &w) { return w.size() > 32 ? w.substr(0, 32) + "..." : w; };
  auto index_of = [&](const std::string &s) {
    for (int m = 0; m < ne; m++) if (el[m] == s) return m;
    return -1;
  };
  std::vector<double> val((size_t)ne * ne * ne * TS_NFIELD, 0.0);
  std::vector<char> have((size_t)ne * ne * ne, 0);
  for (size_t t = 0; t < tok.size(); t += NW) {
    const std::string at = " (entry that starts on line " + std::to_string(tok[t].line) + ")";
    if (tok.size() - t < (size_t)NW) return bad("short entry: " + std::to_string(tok.size() - t) + " of " + std::to_string(NW) + " words" + at);
    double v[TS_NFIELD];
    for (int k = 0; k < TS_NFIELD; k++) {
      const std::string &s = tok[t + 3 + k].s;
      char *end = nullptr;
      v[k] = std::strtod(s.c_str(), &end);
      if (end == s.c_str() || *end != 0 || !std::isfinite(v[k])) return bad("'" + show(s) + "' on line " + std::to_string(tok[t + 3 + k].line) + " is not a number" + at);
    }
    for (int k = 0; k < 3; k++) {
      char *end = nullptr;
      (void)std::strtod(tok[t + k].s.c_str(), &end);
      if (end != tok[t + k].s.c_str() && *end == 0) return bad("'" + show(tok[t + k].s) + "' on line " + std::to_string(tok[t + k].line) + " where an element name is expected" + at);
    }
    const int i = index_of(tok[t].s), j = index_of(tok[t + 1].s), k = index_of(tok[t + 2].s);
    if (i < 0 || j < 0 || k < 0) continue;   // LAMMPS reads the entries it needs
    if (v[F_C] < 0.0 || v[F_D] < 0.0 || v[F_N] < 0.0 || v[F_BETA] < 0.0 || v[F_LAM2] < 0.0 || v[F_B] < 0.0 || v[F_R] < 0.0 || v[F_BIGD] < 0.0 ||
        v[F_LAM1] < 0.0 || v[F_A] < 0.0 || v[F_GAMMA] < 0.0)
      return bad("c, d, n, beta, lambda2, B, R, D, lambda1, A and gamma must not be negative" + at);
    if (v[F_BIGD] > v[F_R]) return bad("D must not exceed R" + at);
    if (v[F_M] != 1.0 && v[F_M] != 3.0) return bad("m must be 1 or 3" + at);
    if (j == k && !(v[F_N] > 0.0)) return bad("n of a pair entry (i j j) must be positive" + at);
    const size_t id = ((size_t)i * ne + j) * ne + k;
    if (have[id]) return bad("duplicate entry " + tok[t].s + " " + tok[t + 1].s + " " + tok[t + 2].s + at);
    have[id] = 1;
    if (energy_unit == 0) { v[F_A] *= TS_EV_TO_KCALMOL; v[F_B] *= TS_EV_TO_KCALMOL; }
    std::memcpy(&val[id * TS_NFIELD], v, sizeof v);
  }
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++)
      for (int k = 0; k < ne; k++)
        if (!have[((size_t)i * ne + j) * ne + k]) return bad("no entry for the triplet " + el[i] + " " + el[j] + " " + el[k]);
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * TS_NFIELD];   // the entry i j j
      TsPairP &P = T.pair[i * TS_MAXEL + j];
      P.biga = v[F_A]; P.bigb = v[F_B]; P.lam1 = v[F_LAM1]; P.lam2 = v[F_LAM2]; P.beta = v[F_BETA]; P.powern = v[F_N];
      P.bigr = v[F_R]; P.bigd = v[F_BIGD]; P.cut = v[F_R] + v[F_BIGD];
      P.c1 = std::pow(2.0 * P.powern * 1.0e-16, -1.0 / P.powern);
      P.c2 = std::pow(2.0 * P.powern * 1.0e-8, -1.0 / P.powern);
      P.c3 = 1.0 / P.c2;
      P.c4 = 1.0 / P.c1;
      T.cutin[i * TS_MAXEL + j] = std::max(T.cutin[i * TS_MAXEL + j], P.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * TS_NFIELD];
        TsTripP &Q = T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
        Q.gamma = u[F_GAMMA]; Q.lam3 = u[F_LAM3]; Q.c2 = u[F_C] * u[F_C]; Q.d2 = u[F_D] * u[F_D]; Q.cos0 = u[F_COS0];
        Q.bigr = u[F_R]; Q.bigd = u[F_BIGD]; Q.cut = u[F_R] + u[F_BIGD];
        Q.m3 = u[F_M] == 3.0 ? 1 : 0;
        T.cutin[i * TS_MAXEL + k] = std::max(T.cutin[i * TS_MAXEL + k], Q.cut);
        T.cutmax = std::max(T.cutmax, Q.cut);
      }
    }
  if (raw) *raw = val;
  return true;
}

}  // namespace scema

extern "C" int scema_md_tersoff_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                            int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto say = [&](const std::string &m) {
    if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
  };
  say("");
  if (!path || !elements || n_elements <= 0) { say("bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  TsTable T;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_tersoff_params(path, el, energy_unit, T, map, err, &raw)) { say(err); return SCEMA_MD_ERR_IO; }
  if (n_kept) *n_kept = T.nelem;
  if (type_map) for (int k = 0; k < n_elements; k++) type_map[k] = map[k];
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}
