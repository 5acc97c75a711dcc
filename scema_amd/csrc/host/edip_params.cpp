// edip_params.cpp -- reader of LAMMPS EDIP parameter files (host/edip_params.h) and its face in the C ABI
#include "edip_params.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "scema_md.h"
#include "triplet_file.h"

namespace scema {

// places of the numbers in an entry
enum { ED_A, ED_B, ED_CUTA, ED_CUTC, ED_ALPHA, ED_BETA, ED_ETA, ED_GAMMA, ED_LAMBDA, ED_MU, ED_RHO, ED_SIGMA, ED_Q0, ED_U1, ED_U2, ED_U3, ED_U4 };
static const int ED_TRIP[8] = {ED_LAMBDA, ED_ETA, ED_Q0, ED_MU, ED_U1, ED_U2, ED_U3, ED_U4};

bool read_edip_params(const std::string &path, const std::vector<std::string> &elements, int energy_unit, EdipTable &T, std::vector<int> &type_map,
                      std::string &err, std::vector<double> *raw) {
  if (energy_unit != 0 && energy_unit != 1) {
    err = path + ": energy unit " + std::to_string(energy_unit) + " (0: A and lambda in eV, 1: in kcal/mol)";
    return false;
  }
  std::vector<std::string> el;
  std::vector<double> val;
  auto check = [&](int, int j, int k, double *v, const std::string &at) -> std::string {
    // (an entry i j k with j != k gives the eight numbers of h only)
    if (j == k) {
      if (!(v[ED_CUTA] > 0.0)) return "cutoffA of a pair entry (i j j) must be positive" + at;
      if (v[ED_CUTC] < 0.0) return "cutoffC of a pair entry (i j j) must not be negative" + at;
      if (!(v[ED_CUTC] < v[ED_CUTA])) return "cutoffC of a pair entry (i j j) must lie below its cutoffA" + at;
      if (v[ED_ALPHA] < 0.0) return "alpha of a pair entry (i j j) must not be negative" + at;
      if (v[ED_SIGMA] < 0.0) return "sigma of a pair entry (i j j) must not be negative" + at;
      if (v[ED_GAMMA] < 0.0) return "gamma of a pair entry (i j j) must not be negative" + at;
      if (v[ED_RHO] < 0.0) return "rho of a pair entry (i j j) must not be negative" + at;
      if (v[ED_A] != 0.0 && !(v[ED_B] > 0.0)) return "B of a pair entry (i j j) with A != 0 must be positive" + at;
    }
    if (energy_unit == 0) { v[ED_A] *= EDIP_EV_TO_KCALMOL; v[ED_LAMBDA] *= EDIP_EV_TO_KCALMOL; }
    return "";
  };
  if (!read_triplet_file(path, elements, EDIP_MAXEL, EDIP_NFIELD, check, el, type_map, val, err)) return false;
  const int ne = (int)el.size();
  auto entry = [&](int i, int j, int k) { return &val[(((size_t)i * ne + j) * ne + k) * EDIP_NFIELD]; };
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++)
      for (int k = j + 1; k < ne; k++) {
        const double *a = entry(i, j, k), *b = entry(i, k, j);
        for (int q : ED_TRIP)
          if (a[q] != b[q]) {
            err = path + ": entries " + el[i] + " " + el[j] + " " + el[k] + " and " + el[i] + " " + el[k] + " " + el[j] +
                  " differ in eta, lambda, mu, Q0 or u1..u4 (the sum over the pairs of arms must not depend on their order)";
            return false;
          }
      }
  for (int i = 0; i < ne; i++)
    for (int j = i + 1; j < ne; j++)
      if (entry(i, j, j)[ED_CUTA] != entry(j, i, i)[ED_CUTA]) {
        err = path + ": entries " + el[i] + " " + el[j] + " " + el[j] + " and " + el[j] + " " + el[i] + " " + el[i] + " differ in cutoffA (a pair has one cutoff at both ends)";
        return false;
      }
  std::memset(&T, 0, sizeof T);
  T.nelem = ne;
  for (int i = 0; i < ne; i++)
    for (int j = 0; j < ne; j++) {
      const double *v = entry(i, j, j);
      EdipPairP &P = T.pair[i * EDIP_MAXEL + j];
      P.A = v[ED_A]; P.B = v[ED_B]; P.rho = v[ED_RHO]; P.beta = v[ED_BETA]; P.sigma = v[ED_SIGMA];
      P.a = v[ED_CUTA]; P.c = v[ED_CUTC]; P.alpha = v[ED_ALPHA]; P.gamma = v[ED_GAMMA];
      P.iw = 1.0 / (P.a - P.c);
      T.cutmax = std::max(T.cutmax, P.a);
      for (int k = 0; k < ne; k++) {
        const double *u = entry(i, j, k);
        EdipTripP &Q = T.trip[(i * EDIP_MAXEL + j) * EDIP_MAXEL + k];
        Q.lambda = u[ED_LAMBDA]; Q.eta = u[ED_ETA]; Q.q0 = u[ED_Q0]; Q.mu = u[ED_MU];
        Q.u1 = u[ED_U1]; Q.u2 = u[ED_U2]; Q.u3 = u[ED_U3]; Q.u4 = u[ED_U4];
      }
    }
  if (raw) *raw = val;
  return true;
}

}  // namespace scema

extern "C" int scema_md_edip_read_params(const char *path, const char *const *elements, int32_t n_elements, int32_t energy_unit, int32_t *n_kept,
                                         int32_t *type_map, double *values, char *errbuf, int32_t errcap) {
  auto read = [&](const std::vector<std::string> &el, int &ne, std::vector<int> &map, std::vector<double> &raw, std::string &err) {
    EdipTable T;
    const bool ok = scema::read_edip_params(path, el, energy_unit, T, map, err, &raw);
    if (ok) ne = T.nelem;
    return ok;
  };
  return scema::read_params_capi(read, path, elements, n_elements, n_kept, type_map, values, errbuf, errcap);
}
