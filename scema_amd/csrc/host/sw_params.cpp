// sw_params.cpp -- reader of LAMMPS Stillinger-Weber parameter files (host/sw_params.h) and its face in the C ABI
#include "sw_params.h"

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
}

bool read_sw_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, SwTable &T, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *raw) {
  auto bad = [&](const std::string &m) { err = path + ": " + m; return false; };
  if (energy_unit != 0 && energy_unit != 1) return bad("energy unit " + std::to_string(energy_unit) + " (0: epsilon in eV, 1: in kcal/mol)");
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
  if (ne > SW_MAXEL) return bad("more than " + std::to_string(SW_MAXEL) + " distinct elements");
  std::ifstream in(path);
  if (!in) return bad("cannot open");
  // an entry is 14 words, on one line or several; `#` starts a comment
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
  std::vector<double> val((size_t)ne * ne * ne * 11, 0.0);
  std::vector<char> have((size_t)ne * ne * ne, 0);
  for (size_t t = 0; t < tok.size(); t += 14) {
    const std::string at = " (entry that starts on line " + std::to_string(tok[t].line) + ")";
    if (tok.size() - t < 14) return bad("short entry: " + std::to_string(tok.size() - t) + " of 14 words" + at);
    double v[11];
    for (int k = 0; k < 11; k++) {
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
    // (an entry i j k with j != k gives lambda, epsilon and costheta0 only: the files LAMMPS ships write zeros for the rest)
    if (v[0] < 0.0 || v[1] < 0.0 || v[2] < 0.0 || v[3] < 0.0 || v[4] < 0.0 || v[6] < 0.0 || v[7] < 0.0 || v[8] < 0.0 || v[9] < 0.0 || v[10] < 0.0)
      return bad("epsilon, sigma, a, lambda, gamma, A, B, p, q and tol must not be negative" + at);
    if (j == k && (!(v[1] > 0.0) || !(v[2] > 0.0))) return bad("sigma and a of a pair entry (i j j) must be positive" + at);
    const size_t id = ((size_t)i * ne + j) * ne + k;
    if (have[id]) return bad("duplicate entry " + tok[t].s + " " + tok[t + 1].s + " " + tok[t + 2].s + at);
    have[id] = 1;
    if (energy_unit == 0) v[0] *= SW_EV_TO_KCALMOL;
    std::memcpy(&val[id * 11], v, sizeof v);
  }
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++)
      for (int k = 0; k < ne; k++)
        if (!have[((size_t)i * ne + j) * ne + k]) return bad("no entry for the triplet " + el[i] + " " + el[j] + " " + el[k]);
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      // epsilon sigma a lambda gamma costheta0 A B p q tol of the entry i j j
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * 11];
      SwPairP &P = T.pair[i * SW_MAXEL + j];
      P.aeps = v[6] * v[0]; P.bigb = v[7]; P.sigma = v[1]; P.powp = v[8]; P.powq = v[9];
      P.cut = v[2] * v[1]; P.gs = v[4] * v[1];
      P.fast = (v[8] == 4.0 && v[9] == 0.0) ? 1 : 0;
      T.cutmax = std::max(T.cutmax, P.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * 11];
        SwTripP &Q = T.trip[(i * SW_MAXEL + j) * SW_MAXEL + k];
        Q.leps = u[3] * u[0]; Q.cos0 = u[5];
      }
    }
  if (raw) *raw = val;
  return true;
}

}  // namespace scema

extern "C" int scema_md_sw_read_params(const char *sw_path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                       int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto say = [&](const std::string &m) {
    if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
  };
  say("");
  if (!sw_path || !elements || n_elements <= 0) { say("bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  SwTable T;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_sw_params(sw_path, el, energy_unit, T, map, err, &raw)) { say(err); return SCEMA_MD_ERR_IO; }
  if (n_kept) *n_kept = T.nelem;
  if (type_map) for (int k = 0; k < n_elements; k++) type_map[k] = map[k];
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}
