// eam_setfl.cpp -- reader of DYNAMO setfl files, plain and with the u and w tables of `pair_style adp` (host/eam_setfl.h), and its faces
// in the C ABI
#include "eam_setfl.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

// the one parse: adp says that Nr values of u and of w per pair follow the r phi tables (AdpHead at the start of the block, else EamHead)
static bool read_setfl(const std::string &path, const std::vector<std::string> &elements, int energy_unit, bool adp, std::vector<double> &block,
                       std::vector<int> &type_map, std::string &err, std::vector<double> *masses) {
  auto bad = [&](const std::string &m) { err = path + ": " + m; return false; };
  if (energy_unit != 0 && energy_unit != 1) return bad("energy unit " + std::to_string(energy_unit) + " (0: F and r phi in eV, 1: in kcal/mol)");
  if (elements.empty()) return bad("no elements named");
  std::vector<std::string> el;   // the distinct elements in order of first appearance
  type_map.assign(elements.size(), 0);
  for (size_t k = 0; k < elements.size(); k++) {
    if (elements[k].empty()) return bad("empty element name");
    size_t m = 0;
    while (m < el.size() && el[m] != elements[k]) m++;
    if (m == el.size()) el.push_back(elements[k]);
    type_map[k] = (int)m;
  }
  const int ne = (int)el.size();
  if (ne > EAM_MAXEL) return bad("more than " + std::to_string(EAM_MAXEL) + " distinct elements");
  std::ifstream in(path);
  if (!in) return bad("cannot open");
  std::vector<FileTok> tok;
  file_tokens(in, 3, false, tok);   // (three comment lines)
  size_t t = 0;
  auto number = [&](const char *what, double &v) {
    if (t >= tok.size()) return bad(std::string("truncated file: it ends where ") + what + " is expected");
    if (!word_number(tok[t].s, v)) return bad("'" + show_word(tok[t].s) + "' on line " + std::to_string(tok[t].line) + " is not a number (" + what + ")");
    t++;
    return true;
  };
  auto count = [&](const char *what, double lo, int &n) {
    double v;
    if (!number(what, v)) return false;
    if (v != std::floor(v) || v < lo || v > 1.0e9) return bad(std::string(what) + " = " + show_word(tok[t - 1].s) + " on line " + std::to_string(tok[t - 1].line) + ": a whole number of at least " + std::to_string((int)lo) + " is expected");
    n = (int)v;
    return true;
  };
  int nfile = 0, nrho = 0, nr = 0;
  if (!count("the number of elements", 1.0, nfile)) return false;
  if (tok.size() - t < (size_t)nfile) return bad("truncated file: " + std::to_string(nfile) + " element names announced, " + std::to_string(tok.size() - t) + " words left");
  std::vector<std::string> names;
  for (int k = 0; k < nfile; k++) names.push_back(tok[t++].s);
  std::vector<int> src(ne, -1);   // compact element -> its place in the file
  for (int m = 0; m < ne; m++) {
    for (int k = 0; k < nfile; k++)
      if (names[k] == el[m]) { src[m] = k; break; }
    if (src[m] < 0) return bad("element " + show_word(el[m]) + " is not in the file");
  }
  double drho = 0.0, dr = 0.0, cutoff = 0.0;
  if (!count("Nrho", 5.0, nrho) || !number("drho", drho) || !count("Nr", 5.0, nr) || !number("dr", dr) || !number("cutoff", cutoff)) return false;
  if (!(drho > 0.0) || !(dr > 0.0) || !(cutoff > 0.0)) return bad("drho, dr and the cutoff must be positive");
  if (cutoff > (nr - 1) * dr) return bad("the cutoff " + std::to_string(cutoff) + " lies beyond the last knot (Nr - 1) dr = " + std::to_string((nr - 1) * dr));
  // what the counts announce against what the file holds, before anything is sized by them
  const double npairs = 0.5 * nfile * (nfile + 1.0);
  const double words_eam = (double)nfile * (4.0 + nrho + nr) + npairs * nr, words = words_eam + (adp ? 2.0 * npairs * nr : 0.0);
  if (adp && words_eam <= (double)(tok.size() - t) && words > (double)(tok.size() - t))
    return bad(std::string("truncated file: it ends inside the ") + (words_eam + npairs * nr > (double)(tok.size() - t) ? "u" : "w") + " tables of an ADP file (" +
               std::to_string(nfile * (nfile + 1) / 2) + " pairs of Nr " + std::to_string(nr) + " values of u, then as many of w, after r phi): its counts announce " +
               std::to_string((long long)words) + " numbers, it holds " + std::to_string(tok.size() - t));
  if (words > (double)(tok.size() - t))
    return bad("truncated file: its counts (" + std::to_string(nfile) + " elements, Nrho " + std::to_string(nrho) + ", Nr " + std::to_string(nr) + ") announce " +
               std::to_string((long long)words) + " numbers, it holds " + std::to_string(tok.size() - t));
  const double escale = energy_unit == 0 ? EAM_EV_TO_KCALMOL : 1.0;
  // the block: head, then per kept element F and rho, then per kept pair i >= j r phi; each function 8 n doubles
  // (ADP: then per kept pair u, then per kept pair w)
  const size_t ndoubles = EAM_HEAD_DOUBLES + (size_t)ne * 8 * ((size_t)nrho + nr) + (size_t)ne * (ne + 1) / 2 * 8 * nr * (adp ? 3 : 1);
  if (ndoubles > (size_t)0x7FFFFFFF) return bad("tables of more than 2^31 numbers: the block's offsets are 32-bit");
  block.assign(ndoubles, 0.0);
  AdpHead A;
  std::memset(&A, 0, sizeof A);
  EamHead &H = A.eam;
  H.nelem = ne; H.nrho = nrho; H.nr = nr;
  H.drho = drho; H.dr = dr; H.rdrho = 1.0 / drho; H.rdr = 1.0 / dr;
  H.cutoff = cutoff; H.cut2 = cutoff * cutoff; H.rhomax = (nrho - 1) * drho;
  H.ndoubles = (long long)ndoubles;
  size_t off = EAM_HEAD_DOUBLES;
  auto place = [&](int n) { const size_t o = off; off += 8 * (size_t)n; return (int)o; };
  std::vector<int> off_src(ne);
  for (int m = 0; m < ne; m++) { H.off_f[m] = place(nrho); off_src[m] = place(nr); }
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) H.off_rho[i * EAM_MAXEL + j] = off_src[j];
  for (int i = 0; i < ne; i++)
    for (int j = 0; j <= i; j++) H.off_z[i * EAM_MAXEL + j] = H.off_z[j * EAM_MAXEL + i] = place(nr);
  if (adp)
    for (int *o : {A.off_u, A.off_w})
      for (int i = 0; i < ne; i++)
        for (int j = 0; j <= i; j++) o[i * EAM_MAXEL + j] = o[j * EAM_MAXEL + i] = place(nr);
  std::vector<double> f((size_t)std::max(nrho, nr));
  auto table = [&](const char *what, int n, double delta, double scale, int where) {
    for (int k = 0; k < n; k++) {
      if (!number(what, f[k])) return false;
      f[k] *= scale;
    }
    if (where >= 0) eam_spline_build(f.data(), n, delta, &block[where], &block[where + 4 * (size_t)n]);
    return true;
  };
  if (masses) masses->assign(ne, 0.0);
  for (int k = 0; k < nfile; k++) {
    double z, mass, a0;
    if (!number("an atomic number", z) || !number("a mass", mass) || !number("a lattice constant", a0)) return false;
    if (t >= tok.size()) return bad("truncated file: it ends where a lattice name is expected");
    t++;   // (the lattice: a name)
    if (!(mass > 0.0)) return bad("the mass of " + show_word(names[k]) + " must be positive");
    int m = 0;
    while (m < ne && src[m] != k) m++;
    if (m < ne && masses) (*masses)[m] = mass;
    if (!table("F(rho)", nrho, drho, escale, m < ne ? H.off_f[m] : -1) || !table("rho(r)", nr, dr, 1.0, m < ne ? off_src[m] : -1)) return false;
  }
  for (int i = 0; i < nfile; i++)
    for (int j = 0; j <= i; j++) {
      int a = 0, b = 0;
      while (a < ne && src[a] != i) a++;
      while (b < ne && src[b] != j) b++;
      if (!table("r phi(r)", nr, dr, escale, a < ne && b < ne ? H.off_z[a * EAM_MAXEL + b] : -1)) return false;
    }
  if (adp) {
    // u and w as written, not multiplied by r; mu^2 and lam^2 are energies: the square root of the unit's factor
    const double ascale = std::sqrt(escale);
    for (int pass = 0; pass < 2; pass++)
      for (int i = 0; i < nfile; i++)
        for (int j = 0; j <= i; j++) {
          int a = 0, b = 0;
          while (a < ne && src[a] != i) a++;
          while (b < ne && src[b] != j) b++;
          const int *o = pass ? A.off_w : A.off_u;
          if (!table(pass ? "w(r)" : "u(r)", nr, dr, ascale, a < ne && b < ne ? o[a * EAM_MAXEL + b] : -1)) return false;
        }
  }
  std::memcpy(block.data(), &A, adp ? sizeof A : sizeof H);
  return true;
}

bool read_eam_setfl(const std::string &path, const std::vector<std::string> &elements, int energy_unit, std::vector<double> &block, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *masses) {
  return read_setfl(path, elements, energy_unit, false, block, type_map, err, masses);
}

bool read_adp_setfl(const std::string &path, const std::vector<std::string> &elements, int energy_unit, std::vector<double> &block, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *masses) {
  return read_setfl(path, elements, energy_unit, true, block, type_map, err, masses);
}

}  // namespace scema

static int read_setfl_c(bool adp, const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept, int32_t *type_map,
                        double *head, double *masses, double *tables, int64_t tables_cap, char *errbuf, int32_t errcap) {
  auto say = [&](const std::string &m) {
    if (errbuf && errcap > 0) { std::strncpy(errbuf, m.c_str(), (size_t)errcap - 1); errbuf[errcap - 1] = 0; }
  };
  say("");
  if (!path || !elements || n_elements <= 0) { say("bad arguments"); return SCEMA_MD_ERR_ARG; }
  std::vector<std::string> el;
  for (int k = 0; k < n_elements; k++) el.push_back(elements[k] ? elements[k] : "");
  std::vector<double> block, mass;
  std::vector<int> map;
  std::string err;
  if (!scema::read_setfl(path, el, energy_unit, adp, block, map, err, &mass)) { say(err); return SCEMA_MD_ERR_IO; }
  const EamHead &H = scema::eam_head(block);
  if (n_kept) *n_kept = H.nelem;
  if (type_map) for (int k = 0; k < n_elements; k++) type_map[k] = map[k];
  if (head) {
    const double v[8] = {(double)H.nrho, H.drho, (double)H.nr, H.dr, H.cutoff, H.rhomax, (double)(H.ndoubles - EAM_HEAD_DOUBLES), 0.0};
    for (int k = 0; k < 8; k++) head[k] = v[k];
  }
  if (masses) for (int k = 0; k < H.nelem; k++) masses[k] = mass[k];
  if (tables) {
    if (tables_cap < H.ndoubles - EAM_HEAD_DOUBLES) { say("the caller's room for the tables is too small"); return SCEMA_MD_ERR_ARG; }
    std::memcpy(tables, block.data() + EAM_HEAD_DOUBLES, (size_t)(H.ndoubles - EAM_HEAD_DOUBLES) * sizeof(double));
  }
  return SCEMA_MD_OK;
}

extern "C" int scema_md_eam_read_setfl(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                       int32_t *type_map, double *head, double *masses, double *tables, int64_t tables_cap, char *errbuf,
                                       int32_t errcap) {
  return read_setfl_c(false, path, elements, n_elements, energy_unit, n_kept, type_map, head, masses, tables, tables_cap, errbuf, errcap);
}

extern "C" int scema_md_adp_read_setfl(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                       int32_t *type_map, double *head, double *masses, double *tables, int64_t tables_cap, char *errbuf,
                                       int32_t errcap) {
  return read_setfl_c(true, path, elements, n_elements, energy_unit, n_kept, type_map, head, masses, tables, tables_cap, errbuf, errcap);
}
