// sw_params.cpp -- reader of LAMMPS Stillinger-Weber parameter files (host/sw_params.h) and its face in the C ABI
#include "sw_params.h"

#include <algorithm>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

bool read_sw_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, SwTable &T, std::vector<int> &type_map,
                    std::string &err, std::vector<double> *raw) {
  if (energy_unit != 0 && energy_unit != 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: epsilon in eV, 1: in kcal/mol)";
    return false;
  }
  // an entry is 14 words: three elements, epsilon sigma a lambda gamma costheta0 A B p q tol
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    // (an entry i j k with j != k gives lambda, epsilon and costheta0 only: the files LAMMPS ships write zeros for the rest)
    if (v[0] < 0.0 || v[1] < 0.0 || v[2] < 0.0 || v[3] < 0.0 || v[4] < 0.0 || v[6] < 0.0 || v[7] < 0.0 || v[8] < 0.0 || v[9] < 0.0 || v[10] < 0.0)
      return "epsilon, sigma, a, lambda, gamma, A, B, p, q and tol must not be negative" + at;
    if (j == k && (!(v[1] > 0.0) || !(v[2] > 0.0))) return "sigma and a of a pair entry (i j j) must be positive" + at;
    if (energy_unit == 0) v[0] *= SW_EV_TO_KCALMOL;
    return "";
  };
  if (!read_triplet_file(path, elements, SW_MAXEL, SW_NFIELD, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      // epsilon sigma a lambda gamma costheta0 A B p q tol of the entry i j j
      const double *v = &val[(((size_t)i * ne + j) * ne + j) * SW_NFIELD];
      SwPairP &P = T.pair[i * SW_MAXEL + j];
      P.aeps = v[6] * v[0]; P.bigb = v[7]; P.sigma = v[1]; P.powp = v[8]; P.powq = v[9];
      P.cut = v[2] * v[1]; P.gs = v[4] * v[1];
      P.fast = (v[8] == 4.0 && v[9] == 0.0) ? 1 : 0;
      T.cutmax = std::max(T.cutmax, P.cut);
      for (int k = 0; k < ne; k++) {
        const double *u = &val[(((size_t)i * ne + j) * ne + k) * SW_NFIELD];
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
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    SwTable T;
    const bool ok = scema::read_sw_params(sw_path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, sw_path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}
