// tersoff_params.cpp -- reader of LAMMPS Tersoff parameter files (host/tersoff_params.h) and its face in the C ABI
#include "tersoff_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

namespace {
enum { F_M, F_GAMMA, F_LAM3, F_C, F_D, F_COS0, F_N, F_BETA, F_LAM2, F_B, F_R, F_BIGD, F_LAM1, F_A };
}  // namespace

bool read_tersoff_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, TsTable &T, std::vector<int> &type_map,
                         std::string &err, std::vector<double> *raw) {
  if (energy_unit != 0 && energy_unit != 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: A and B in eV, 1: in kcal/mol)";
    return false;
  }
  // an entry is 17 words: three elements and the TS_NFIELD numbers
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    if (v[F_C] < 0.0 || v[F_D] < 0.0 || v[F_N] < 0.0 || v[F_BETA] < 0.0 || v[F_LAM2] < 0.0 || v[F_B] < 0.0 || v[F_R] < 0.0 || v[F_BIGD] < 0.0 ||
        v[F_LAM1] < 0.0 || v[F_A] < 0.0 || v[F_GAMMA] < 0.0)
      return "c, d, n, beta, lambda2, B, R, D, lambda1, A and gamma must not be negative" + at;
    if (v[F_BIGD] > v[F_R]) return "D must not exceed R" + at;
    if (v[F_M] != 1.0 && v[F_M] != 3.0) return "m must be 1 or 3" + at;
    if (j == k && !(v[F_N] > 0.0)) return "n of a pair entry (i j j) must be positive" + at;
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
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    TsTable T;
    const bool ok = scema::read_tersoff_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}
