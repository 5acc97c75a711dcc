// vashishta_params.cpp -- reader of LAMMPS Vashishta parameter files (host/vashishta_params.h) and its face in the C ABI
#include "vashishta_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

bool read_vashishta_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, VsTable &T, std::vector<int> &type_map,
                           std::string &err, std::vector<double> *raw) {
  if (energy_unit != 0 && energy_unit != 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: H, D, W and B in eV, 1: in kcal/mol)";
    return false;
  }
  // an entry is 17 words: three elements, H eta Zi Zj lambda1 D lambda4 W rc B gamma r0 C costheta0
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    // (an entry i j k with j != k gives B, C and costheta0 only)
    if (v[12] < 0.0) return "C must not be negative" + at;
    if (j == k) {
      if (!(v[8] > 0.0)) return "rc of a pair entry (i j j) must be positive" + at;
      if (v[0] != 0.0 && !(v[1] > 0.0)) return "eta of a pair entry (i j j) with H != 0 must be positive" + at;
      if (v[4] < 0.0 || v[6] < 0.0 || v[10] < 0.0 || v[11] < 0.0) return "lambda1, lambda4, gamma and r0 must not be negative" + at;
      if (v[11] > v[8]) return "r0 of a pair entry (i j j) must not exceed its rc" + at;
    }
    if (energy_unit == 0) { v[0] *= VS_EV_TO_KCALMOL; v[5] *= VS_EV_TO_KCALMOL; v[7] *= VS_EV_TO_KCALMOL; v[9] *= VS_EV_TO_KCALMOL; }
    return "";
  };
  if (!read_triplet_file(path, elements, VS_MAXEL, VS_NFIELD, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  auto entry = [&](int i, int j, int k) { return &val[(((size_t)i * ne + j) * ne + k) * VS_NFIELD]; };
  for (int i = 0; i < ne; i++)
    for (int j = i + 1; j < ne; j++) {
      const double *a = entry(i, j, j), *b = entry(j, i, i);
      if (a[8] != b[8] || a[11] != b[11]) {
        err = path + ": entries " + el[i] + " " + el[j] + " " + el[j] + " and " + el[j] + " " + el[i] + " " + el[i] + " differ in rc or r0 (a pair has one cutoff at both ends)";
        return false;
      }
    }
  const double kc = energy_unit == 0 ? VS_COULOMB_EV * VS_EV_TO_KCALMOL : VS_COULOMB_KCALMOL;
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = entry(i, j, j);
      VsPairP &P = T.pair[i * VS_MAXEL + j];
      P.h = v[0]; P.eta = v[1]; P.kzz = kc * v[2] * v[3];
      P.il1 = v[4] > 0.0 ? 1.0 / v[4] : 0.0; P.il4 = v[6] > 0.0 ? 1.0 / v[6] : 0.0;
      P.d = v[5]; P.w = v[7]; P.rc = v[8]; P.gamma = v[10]; P.r0 = v[11];
      P.ieta = (v[1] >= 1.0 && v[1] <= 32.0 && v[1] == std::floor(v[1])) ? (int)v[1] : 0;
      vs_u(P, P.rc, &P.urc, &P.durc);
      T.cutmax = std::max(T.cutmax, std::max(P.rc, P.r0));
      for (int k = 0; k < ne; k++) {
        const double *u = entry(i, j, k);
        VsTripP &Q = T.trip[(i * VS_MAXEL + j) * VS_MAXEL + k];
        Q.b = u[9]; Q.c = u[12]; Q.cos0 = u[13];
      }
    }
  if (raw) *raw = val;
  return true;
}

}  // namespace scema

extern "C" int scema_md_vashishta_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                              int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    VsTable T;
    const bool ok = scema::read_vashishta_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}
