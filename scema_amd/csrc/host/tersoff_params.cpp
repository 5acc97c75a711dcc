// tersoff_params.cpp -- readers of LAMMPS Tersoff parameter files, plain, mod(/c) and zbl (host/tersoff_params.h), and their faces in the C ABI
#include "tersoff_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

namespace {
enum { F_M, F_GAMMA, F_LAM3, F_C, F_D, F_COS0, F_N, F_BETA, F_LAM2, F_B, F_R, F_BIGD, F_LAM1, F_A, F_ZI, F_ZJ, F_ZCUT, F_ZSCALE };
enum { M_BETA, M_ALPHA, M_H, M_ETA, M_BETATERS, M_LAM2, M_B, M_R, M_BIGD, M_LAM1, M_A, M_N, M_C1, M_C2, M_C3, M_C4, M_C5, M_C0 };

// what the plain and the ZBL reader refuse in the fourteen numbers they share
std::string check_plain(int j, int k, const double *v, const std::string &at) {
  if (v[F_C] < 0.0 || v[F_D] < 0.0 || v[F_N] < 0.0 || v[F_BETA] < 0.0 || v[F_LAM2] < 0.0 || v[F_B] < 0.0 || v[F_R] < 0.0 || v[F_BIGD] < 0.0 ||
      v[F_LAM1] < 0.0 || v[F_A] < 0.0 || v[F_GAMMA] < 0.0)
    return "c, d, n, beta, lambda2, B, R, D, lambda1, A and gamma must not be negative" + at;
  if (v[F_BIGD] > v[F_R]) return "D must not exceed R" + at;
  if (v[F_M] != 1.0 && v[F_M] != 3.0) return "m must be 1 or 3" + at;
  if (j == k && !(v[F_N] > 0.0)) return "n of a pair entry (i j j) must be positive" + at;
  return "";
}

// the plain pair and triplet records of entry i j j (v) and i j k (u)
void fill_plain_pair(TsPairP &P, const double *v) {
  P.biga = v[F_A]; P.bigb = v[F_B]; P.lam1 = v[F_LAM1]; P.lam2 = v[F_LAM2]; P.beta = v[F_BETA]; P.powern = v[F_N];
  P.bigr = v[F_R]; P.bigd = v[F_BIGD]; P.cut = v[F_R] + v[F_BIGD];
  P.c1 = std::pow(2.0 * P.powern * 1.0e-16, -1.0 / P.powern);
  P.c2 = std::pow(2.0 * P.powern * 1.0e-8, -1.0 / P.powern);
  P.c3 = 1.0 / P.c2;
  P.c4 = 1.0 / P.c1;
}
void fill_plain_trip(TsTripP &Q, const double *u) {
  Q.gamma = u[F_GAMMA]; Q.lam3 = u[F_LAM3]; Q.c2 = u[F_C] * u[F_C]; Q.d2 = u[F_D] * u[F_D]; Q.cos0 = u[F_COS0];
  Q.bigr = u[F_R]; Q.bigd = u[F_BIGD]; Q.cut = u[F_R] + u[F_BIGD];
  Q.m3 = u[F_M] == 3.0 ? 1 : 0;
}

bool unit_ok(const std::string &path, int energy_unit, std::string &err) {
  if (energy_unit == 0 || energy_unit == 1) return true;
  err = path + ": energy unit " + std::to_string(energy_unit) + " (0: A and B in eV, 1: in kcal/mol)";
  return false;
}
}  // namespace

bool read_tersoff_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsTable &T, std::vector<int> &type_map,
                         std::string &err, std::vector<double> *raw) {
  if (!unit_ok(path, energy_unit, err)) return false;
  // an entry is 17 words: three elements and the TS_NFIELD numbers
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    const std::string wrong = check_plain(j, k, v, at);
    if (!wrong.empty()) return wrong;
    if (energy_unit == 0) { v[F_A] *= TS_EV_TO_KCALMOL; v[F_B] *= TS_EV_TO_KCALMOL; }
    return "";
  };
  if (!read_triplet_file(path, elements, TS_MAXEL, TS_NFIELD, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * TS_NFIELD];   // the entry i j j
      TsPairP &P = T.pair[i * TS_MAXEL + j];
      fill_plain_pair(P, v);
      T.cutin[i * TS_MAXEL + j] = std::max(T.cutin[i * TS_MAXEL + j], P.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * TS_NFIELD];
        TsTripP &Q = T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
        fill_plain_trip(Q, u);
        T.cutin[i * TS_MAXEL + k] = std::max(T.cutin[i * TS_MAXEL + k], Q.cut);
        T.cutmax = std::max(T.cutmax, Q.cut);
      }
    }
  if (raw) *raw = val;
  return true;
}

bool read_tersoff_mod_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsModTable &T, std::vector<int> &type_map,
                             std::string &err, std::vector<double> *raw) {
  if (!unit_ok(path, energy_unit, err)) return false;
  // mod or mod/c: the numeric words that follow the three names of the first entry
  int ncol = TS_MOD_NCOL;
  {
    std::ifstream in(path);
    std::vector<FileTok> tok;
    if (in) file_tokens(in, 0, true, tok);
    size_t k = 3;
    double x;
    while (k < tok.size() && k < 3 + (size_t)TS_FORM_NFIELD + 1 && word_number(tok[k].s, x)) k++;
    if (k == 3 + (size_t)TS_FORM_NFIELD) ncol = TS_FORM_NFIELD;
  }
  std::vector<std::string> el;
  std::vector<double> val;
  const double unit = energy_unit == 0 ? TS_EV_TO_KCALMOL : 1.0;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    if (v[M_BETATERS] != 1.0) return "beta_ters must be 1" + at;
    if (v[M_BETA] != 1.0 && v[M_BETA] != 3.0) return "beta must be 1 or 3" + at;
    if (v[M_ALPHA] < 0.0 || v[M_ETA] < 0.0 || v[M_LAM2] < 0.0 || v[M_B] < 0.0 || v[M_R] < 0.0 || v[M_BIGD] < 0.0 || v[M_LAM1] < 0.0 || v[M_A] < 0.0 ||
        v[M_N] < 0.0 || v[M_C2] < 0.0 || v[M_C3] < 0.0 || v[M_C4] < 0.0 || v[M_C5] < 0.0)
      return "alpha, eta, lambda2, B, R, D, lambda1, A, n, c2, c3, c4 and c5 must not be negative" + at;
    if (v[M_BIGD] > v[M_R]) return "D must not exceed R" + at;
    if (j == k && !(v[M_N] > 0.0)) return "n of a pair entry (i j j) must be positive" + at;
    if (j == k && !(v[M_ETA] > 0.0)) return "eta of a pair entry (i j j) must be positive" + at;
    if (v[M_C3] == 0.0 && v[M_H] >= -1.0 && v[M_H] <= 1.0) return "c3 must be positive where cos theta can reach h (-1 <= h <= 1)" + at;
    v[M_A] *= unit; v[M_B] *= unit;
    if (ncol == TS_FORM_NFIELD) v[M_C0] *= unit;
    return "";
  };
  if (!read_triplet_file(path, elements, TS_MAXEL, ncol, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  if (ncol != TS_FORM_NFIELD) {   // c0 = 0 behind the seventeen numbers of every entry
    std::vector<double> wide((size_t)ne * ne * ne * TS_FORM_NFIELD, 0.0);
    for (size_t t = 0; t < (size_t)ne * ne * ne; t++) std::memcpy(&wide[t * TS_FORM_NFIELD], &val[t * ncol], (size_t)ncol * sizeof(double));
    val.swap(wide);
  }
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * TS_FORM_NFIELD];   // the entry i j j
      TsModPairP &P = T.pair[i * TS_MAXEL + j];
      P.biga = v[M_A]; P.bigb = v[M_B]; P.lam1 = v[M_LAM1]; P.lam2 = v[M_LAM2]; P.beta = v[M_BETATERS]; P.eta = v[M_ETA]; P.powern = v[M_N];
      P.bigr = v[M_R]; P.bigd = v[M_BIGD]; P.cut = v[M_R] + v[M_BIGD]; P.c0 = v[M_C0];
      P.ca1 = std::pow(2.0 * P.powern * 1.0e-16, -1.0 / P.eta);
      P.ca4 = 1.0 / P.ca1;
      T.cutin[i * TS_MAXEL + j] = std::max(T.cutin[i * TS_MAXEL + j], P.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * TS_FORM_NFIELD];
        TsModTripP &Q = T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
        Q.lam3 = u[M_ALPHA]; Q.h = u[M_H]; Q.c1 = u[M_C1]; Q.c2 = u[M_C2]; Q.c3 = u[M_C3]; Q.c4 = u[M_C4]; Q.c5 = u[M_C5];
        Q.bigr = u[M_R]; Q.bigd = u[M_BIGD]; Q.cut = u[M_R] + u[M_BIGD];
        Q.m3 = u[M_BETA] == 3.0 ? 1 : 0;
        T.cutin[i * TS_MAXEL + k] = std::max(T.cutin[i * TS_MAXEL + k], Q.cut);
        T.cutmax = std::max(T.cutmax, Q.cut);
      }
    }
  if (raw) *raw = val;
  return true;
}

bool read_tersoff_zbl_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsZblTable &T, std::vector<int> &type_map,
                             std::string &err, std::vector<double> *raw) {
  if (!unit_ok(path, energy_unit, err)) return false;
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    const std::string wrong = check_plain(j, k, v, at);
    if (!wrong.empty()) return wrong;
    if (!(v[F_ZI] > 0.0) || !(v[F_ZJ] > 0.0)) return "Z_i and Z_j must be positive" + at;
    if (v[F_ZCUT] < 0.0 || v[F_ZSCALE] < 0.0) return "ZBLcut and ZBLexpscale must not be negative" + at;
    if (energy_unit == 0) { v[F_A] *= TS_EV_TO_KCALMOL; v[F_B] *= TS_EV_TO_KCALMOL; }
    return "";
  };
  if (!read_triplet_file(path, elements, TS_MAXEL, TS_FORM_NFIELD, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  const double bigk = energy_unit == 0 ? TS_ZBL_K_EV * TS_EV_TO_KCALMOL : TS_ZBL_K_EV / TS_ZBL_EV_REAL;
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * TS_FORM_NFIELD];   // the entry i j j
      TsZblPairP &P = T.pair[i * TS_MAXEL + j];
      fill_plain_pair(P.p, v);
      P.kzz = bigk * v[F_ZI] * v[F_ZJ];
      P.inva = (std::pow(v[F_ZI], 0.23) + std::pow(v[F_ZJ], 0.23)) / (0.8854 * 0.529);
      P.zcut = v[F_ZCUT]; P.zscale = v[F_ZSCALE];
      T.cutin[i * TS_MAXEL + j] = std::max(T.cutin[i * TS_MAXEL + j], P.p.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * TS_FORM_NFIELD];
        TsTripP &Q = T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
        fill_plain_trip(Q, u);
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
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    TsTable T;
    const bool ok = scema::read_tersoff_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}

extern "C" int scema_md_tersoff_mod_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                                int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    TsModTable T;
    const bool ok = scema::read_tersoff_mod_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}

extern "C" int scema_md_tersoff_zbl_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                                int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    TsZblTable T;
    const bool ok = scema::read_tersoff_zbl_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}
