// triplet_file.h -- what the readers of LAMMPS many-body parameter files share (host/sw_params.cpp, host/tersoff_params.cpp): a file of
// entries `El1 El2 El3 <nfield numbers>`, an entry on one line or several, `#` starts a comment.  Header only: whatever compiles one of the
// readers alone (the host drivers under tests/) has all of it.  Its tokeniser and number check (file_tokens, word_number) also serve
// the setfl reader (host/eam_setfl.cpp), whose file is not made of such entries.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <string>
#include <vector>

#include "scema_md.h"

namespace scema {

// The words of a text file with the line each stands on: the first `skip_lines` lines are left out whole, `#` starts a comment where
// `hash_comments` says so.  What the readers of parameter files tokenise with (this file's, host/eam_setfl.cpp).
struct FileTok { std::string s; int line; };
inline void file_tokens(std::istream &in, int skip_lines, bool hash_comments, std::vector<FileTok> &tok) {
  std::string line;
  for (int ln = 1; std::getline(in, line); ln++) {
    if (ln <= skip_lines) continue;
    if (hash_comments) {
      const size_t h = line.find('#');
      if (h != std::string::npos) line.resize(h);
    }
    std::istringstream ss(line);
    std::string w;
    while (ss >> w) tok.push_back({w, ln});
  }
}
// the whole word as one finite number
inline bool word_number(const std::string &s, double &v) {
  char *end = nullptr;
  v = std::strtod(s.c_str(), &end);
  return end != s.c_str() && *end == 0 && std::isfinite(v);
}
inline std::string show_word(const std::string &w) { return w.size() > 32 ? w.substr(0, 32) + "..." : w; }

// An entry of three named elements i j k (compact indices), its numbers v[nfield] and " (entry that starts on line N)": checks the numbers,
// may rescale them in place, returns "" or what is wrong with them (`at` included).
typedef std::function<std::string(int i, int j, int k, double *v, const std::string &at)> TripletCheck;

// elements[k] = element symbol of LAMMPS atom type k + 1.  On success el holds the distinct elements in order of first appearance (at most
// maxel), type_map[k] the index in el of LAMMPS type k + 1 and val the numbers of every triplet of el, [ne][ne][ne][nfield], as `check`
// left them.  Entries that name another element are skipped (LAMMPS reads the entries it needs).  False with `path: message` in err:
// no or an empty element name, too many elements, unreadable file, short entry, non-numeric field, a number where a name belongs, what
// `check` says, duplicate entry, a triplet of el that the file lacks.
inline bool read_triplet_file(const std::string &path, const std::vector<std::string> &elements, int maxel, int nfield, const TripletCheck &check,
                              std::vector<std::string> &el, std::vector<int> &type_map, std::vector<double> &val, std::string &err) {
  auto bad = [&](const std::string &m) { err = path + ": " + m; return false; };
  if (elements.empty()) return bad("no elements named");
  // the distinct elements in order of first appearance
  el.clear();
  type_map.assign(elements.size(), 0);
  for (size_t k = 0; k < elements.size(); k++) {
    if (elements[k].empty()) return bad("empty element name");
    size_t m = 0;
    while (m < el.size() && el[m] != elements[k]) m++;
    if (m == el.size()) el.push_back(elements[k]);
    type_map[k] = (int)m;
  }
  const int ne = (int)el.size();
  if (ne > maxel) return bad("more than " + std::to_string(maxel) + " distinct elements");
  std::ifstream in(path);
  if (!in) return bad("cannot open");
  std::vector<FileTok> tok;
  file_tokens(in, 0, true, tok);
  auto show = show_word;
  auto index_of = [&](const std::string &s) {
    for (int m = 0; m < ne; m++) if (el[m] == s) return m;
    return -1;
  };
  const size_t nw = 3 + (size_t)nfield;
  val.assign((size_t)ne * ne * ne * nfield, 0.0);
  std::vector<char> have((size_t)ne * ne * ne, 0);
  std::vector<double> v(nfield);
  for (size_t t = 0; t < tok.size(); t += nw) {
    const std::string at = " (entry that starts on line " + std::to_string(tok[t].line) + ")";
    if (tok.size() - t < nw) return bad("short entry: " + std::to_string(tok.size() - t) + " of " + std::to_string(nw) + " words" + at);
    for (int k = 0; k < nfield; k++) {
      const std::string &s = tok[t + 3 + k].s;
      if (!word_number(s, v[k])) return bad("'" + show(s) + "' on line " + std::to_string(tok[t + 3 + k].line) + " is not a number" + at);
    }
    for (int k = 0; k < 3; k++) {
      char *end = nullptr;
      (void)std::strtod(tok[t + k].s.c_str(), &end);
      if (end != tok[t + k].s.c_str() && *end == 0) return bad("'" + show(tok[t + k].s) + "' on line " + std::to_string(tok[t + k].line) + " where an element name is expected" + at);
    }
    const int i = index_of(tok[t].s), j = index_of(tok[t + 1].s), k = index_of(tok[t + 2].s);
    if (i < 0 || j < 0 || k < 0) continue;   // LAMMPS reads the entries it needs
    const size_t id = ((size_t)i * ne + j) * ne + k;
    // (the entry's own numbers are judged before its place in the file, and `have` is looked at before the scaled numbers go anywhere)
    const std::string wrong = check(i, j, k, v.data(), at);
    if (!wrong.empty()) return bad(wrong);
    if (have[id]) return bad("duplicate entry " + tok[t].s + " " + tok[t + 1].s + " " + tok[t + 2].s + at);
    have[id] = 1;
    std::memcpy(&val[id * nfield], v.data(), (size_t)nfield * sizeof(double));
  }
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++)
      for (int k = 0; k < ne; k++)
        if (!have[((size_t)i * ne + j) * ne + k]) return bad("no entry for the triplet " + el[i] + " " + el[j] + " " + el[k]);
  return true;
}

// body of the readers' faces in the C ABI (scema_md_sw_read_params, scema_md_tersoff_read_params): `read` fills the number of elements
// kept, type_map and the raw values, or err
typedef std::function<bool(const std::vector<std::string> &elements, int &n_kept, std::vector<int> &type_map, std::vector<double> &raw, std::string &err)>
    TripletReader;
inline int read_params_capi(const TripletReader &read, const char *path, const char *const *elements, int32_t n_elements, int32_t *n_kept, int32_t *type_map,
                            double *values, char *errbuf, int32_t errcap) {
  auto say = [&](const std::string &m) {
    if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
  };
  say("");
  if (!path || !elements || n_elements <= 0) { say("bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  int ne = 0;
  std::vector<int> map;
  std::vector<double> raw;
  std::string err;
  if (!read(el, ne, map, raw, err)) { say(err); return SCEMA_MD_ERR_IO; }
  if (n_kept) *n_kept = ne;
  if (type_map) for (int k = 0; k < n_elements; k++) type_map[k] = map[k];
  if (values) std::memcpy(values, raw.data(), raw.size() * sizeof(double));
  return SCEMA_MD_OK;
}

}  // namespace scema
