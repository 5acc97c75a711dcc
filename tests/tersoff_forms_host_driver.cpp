// tersoff_forms_host_driver.cpp -- TEST HARNESS, not part of the product: runs the functions of scema_amd/csrc/tersoff/ts_core.h for the
// forms tersoff/mod(/c) and tersoff/zbl (the arithmetic k_ts_force<TsModTable, .> and k_ts_force<TsZblTable, .> execute) as plain loops
// on the host, with the tables of the product's readers (host/tersoff_params.cpp), so that tests/test_tersoff_forms_host.py can hold
// energies, forces and virial against tests/tersoff_forms_numpy.py and against central differences without a GPU.  The loops are those of
// tests/tersoff_host_driver.cpp, over the form's table type.  Built by the test with g++; nothing in scema_amd/ links it.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/tersoff_params.h"
#include "../scema_amd/csrc/tersoff/ts_core.h"

namespace {
// deliberately wrong builds, for the test that shows what the suite catches:
//   1 (mod) the plain fC for the pair's own cutoff function       2 (mod) eta and 1/(2n) exchanged in b
//   3 (zbl) F left off fA, in the bond-order energy and the zeta prefactor alike
//   4 (zbl) F left off the zeta prefactor only: the energy is right, the forces are not
//   5 (mod) c0 multiplied by b (moved from the part without b to the part with it)
struct Driver {
  int form;   // 0 mod, 1 zbl
  TsModTable M;
  TsZblTable Z;
  std::vector<int> type_map;
  int wrong;
};
struct Nb { int j, tj, code; double d[3], r, fc, dfc, pref; };

void pair_fc(const Driver &D, const TsModPairP &P, double r, double *fc, double *dfc) {
  if (D.wrong == 1) ts_fc(P.bigr, P.bigd, r, fc, dfc);
  else ts_pair_fc(P, r, fc, dfc);
}
void pair_fc(const Driver &, const TsZblPairP &P, double r, double *fc, double *dfc) { ts_pair_fc(P, r, fc, dfc); }

void pair_term(const Driver &D, const TsModPairP &P, double r, double fc, double dfc, double b, double *erep, double *eatt, double *fprep, double *fpatt, double *fa) {
  ts_pair(P, r, fc, dfc, b, erep, eatt, fprep, fpatt, fa);
  if (D.wrong == 5) {
    *erep -= 0.5 * fc * P.c0; *eatt += 0.5 * fc * b * P.c0;
    *fprep += 0.5 * dfc * P.c0 / r; *fpatt -= 0.5 * b * dfc * P.c0 / r;
  }
}
void pair_term(const Driver &D, const TsZblPairP &P, double r, double fc, double dfc, double b, double *erep, double *eatt, double *fprep, double *fpatt, double *fa) {
  ts_pair(P, r, fc, dfc, b, erep, eatt, fprep, fpatt, fa);
  const double fat = -P.p.bigb * std::exp(-P.p.lam2 * r);
  if (D.wrong == 3) { *eatt = 0.5 * fc * b * fat; *fpatt = -0.5 * b * (dfc - fc * P.p.lam2) * fat / r; }
  if (D.wrong == 3 || D.wrong == 4) *fa = fat;
}
double beta_of(const TsModPairP &P) { return P.beta; }
double beta_of(const TsZblPairP &P) { return P.p.beta; }

template <class Table>
int compute(const Driver &D, const Table &T, int n, const int *types, const double *x, const double *box, double *f, double *e, double *w, int *counts, double *zetas, double *fcsum) {
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  for (int k = 0; k < 3 * n; k++) f[k] = 0.0;
  e[0] = e[1] = 0.0;
  *fcsum = 0.0;
  for (int k = 0; k < 6; k++) w[k] = 0.0;
  counts[0] = counts[1] = counts[2] = 0;
  if (zetas) for (int k = 0; k < 32 * n; k++) zetas[k] = -1.0;
  std::vector<Nb> nb;
  for (int i = 0; i < n; i++) {
    if (types[i] < 0 || types[i] >= (int)D.type_map.size()) return 1;
    const int ti = D.type_map[types[i]];
    nb.clear();
    for (int j = 0; j < n; j++) {
      if (types[j] < 0 || types[j] >= (int)D.type_map.size()) return 1;
      const int tj = D.type_map[types[j]];
      const auto &P = T.pair[ti * TS_MAXEL + tj];
      double d[3] = {x[3 * j] - x[3 * i], x[3 * j + 1] - x[3 * i + 1], x[3 * j + 2] - x[3 * i + 2]};
      double s2 = d[2] / hz, s1 = (d[1] - yz * s2) / hy, s0 = (d[0] - xy * s1 - xz * s2) / hx;
      s0 -= std::rint(s0); s1 -= std::rint(s1); s2 -= std::rint(s2);
      d[0] = hx * s0 + xy * s1 + xz * s2; d[1] = hy * s1 + yz * s2; d[2] = hz * s2;
      for (int sz = -1; sz <= 1; sz++)
        for (int sy = -1; sy <= 1; sy++)
          for (int sx = -1; sx <= 1; sx++) {
            if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
            Nb q;
            q.d[0] = d[0] + sx * hx + sy * xy + sz * xz; q.d[1] = d[1] + sy * hy + sz * yz; q.d[2] = d[2] + sz * hz;
            q.r = std::sqrt(q.d[0] * q.d[0] + q.d[1] * q.d[1] + q.d[2] * q.d[2]);
            if (!(q.r < T.cutin[ti * TS_MAXEL + tj])) continue;
            q.j = j; q.tj = tj; q.code = (sx + 1) + 3 * (sy + 1) + 9 * (sz + 1);
            q.fc = q.dfc = q.pref = 0.0;
            if (q.r < ts_pair_cut(P)) pair_fc(D, P, q.r, &q.fc, &q.dfc);
            nb.push_back(q);
          }
    }
    counts[2] = std::max(counts[2], (int)nb.size());
    int nz = 0;
    for (size_t a = 0; a < nb.size(); a++) {   // pass 1
      Nb &A = nb[a];
      const auto &P = T.pair[ti * TS_MAXEL + A.tj];
      if (!(A.r < ts_pair_cut(P))) continue;
      double zeta = 0.0;
      for (size_t b = 0; b < nb.size(); b++) {
        if (b == a) continue;
        const auto &Q = T.trip[(ti * TS_MAXEL + A.tj) * TS_MAXEL + nb[b].tj];
        if (!(nb[b].r < Q.cut)) continue;
        zeta += ts_zeta_term(Q, A.d, A.r, nb[b].d, nb[b].r);
      }
      if (zetas && nz < 32) zetas[32 * i + nz++] = beta_of(P) * zeta;
      double bo, db, erep, eatt, fprep, fpatt, fa;
      ts_bond_order(P, zeta, &bo, &db);
      pair_term(D, P, A.r, A.fc, A.dfc, bo, &erep, &eatt, &fprep, &fpatt, &fa);
      A.pref = 0.5 * A.fc * fa * db;
      const double fp = fprep + fpatt;
      const double g[3] = {fp * A.d[0], fp * A.d[1], fp * A.d[2]};
      for (int k = 0; k < 3; k++) { f[3 * A.j + k] += g[k]; f[3 * i + k] -= g[k]; }
      e[0] += erep; e[1] += eatt;
      *fcsum += A.fc;
      counts[0]++;
      w[0] += A.d[0] * g[0]; w[1] += A.d[1] * g[1]; w[2] += A.d[2] * g[2]; w[3] += A.d[0] * g[1]; w[4] += A.d[0] * g[2]; w[5] += A.d[1] * g[2];
    }
    for (size_t a = 0; a < nb.size(); a++)   // pass 2
      for (size_t b = 0; b < nb.size(); b++) {
        if (b == a) continue;
        const Nb &A = nb[a], &B = nb[b];
        const auto &Q = T.trip[(ti * TS_MAXEL + A.tj) * TS_MAXEL + B.tj];
        if (!(A.r < ts_pair_cut(T.pair[ti * TS_MAXEL + A.tj])) || !(B.r < Q.cut)) continue;
        counts[1]++;
        if (A.pref == 0.0) continue;
        double fj[3], fk[3];
        ts_zeta_force(Q, A.pref, A.d, A.r, B.d, B.r, fj, fk);
        for (int c = 0; c < 3; c++) { f[3 * A.j + c] += fj[c]; f[3 * B.j + c] += fk[c]; f[3 * i + c] -= fj[c] + fk[c]; }
        w[0] += A.d[0] * fj[0] + B.d[0] * fk[0]; w[1] += A.d[1] * fj[1] + B.d[1] * fk[1]; w[2] += A.d[2] * fj[2] + B.d[2] * fk[2];
        w[3] += A.d[0] * fj[1] + B.d[0] * fk[1]; w[4] += A.d[0] * fj[2] + B.d[0] * fk[2]; w[5] += A.d[1] * fj[2] + B.d[1] * fk[2];
      }
  }
  return 0;
}
}  // namespace

extern "C" {

void *tfh_create(int form, const char *path, const char *const *elements, int nel, int energy_unit, int wrong) {
  Driver *d = new Driver();
  std::vector<std::string> el(elements, elements + nel);
  std::string err;
  d->form = form;
  d->wrong = wrong;
  const bool ok = form == 0 ? scema::read_tersoff_mod_params(path, el, energy_unit, d->M, d->type_map, err)
                            : scema::read_tersoff_zbl_params(path, el, energy_unit, d->Z, d->type_map, err);
  if (!ok) {
    std::fprintf(stderr, "tfh_create: %s\n", err.c_str());
    delete d;
    return nullptr;
  }
  if (form == 0 && wrong == 2)
    for (TsModPairP &P : d->M.pair)
      if (P.powern > 0.0 && P.eta > 0.0) {
        const double eta = P.eta, n = P.powern;
        P.eta = 1.0 / (2.0 * n); P.powern = 1.0 / (2.0 * eta);
      }
  return d;
}
void tfh_destroy(void *h) { delete (Driver *)h; }
double tfh_cutmax(void *h) { return ((Driver *)h)->form == 0 ? ((Driver *)h)->M.cutmax : ((Driver *)h)->Z.cutmax; }
// b, db/dzeta of the pair (i, j) as the kernels evaluate them, and the switch points (mod: ca1, ca4)
void tfh_bond_order(void *h, int i, int j, double zeta, double *out) {
  const Driver &D = *(Driver *)h;
  out[2] = out[3] = 0.0;
  if (D.form == 0) {
    const TsModPairP &P = D.M.pair[i * TS_MAXEL + j];
    ts_bond_order(P, zeta, &out[0], &out[1]);
    out[2] = P.ca1; out[3] = P.ca4;
  } else {
    ts_bond_order(D.Z.pair[i * TS_MAXEL + j], zeta, &out[0], &out[1]);
  }
}
void tfh_g(void *h, int i, int j, int k, double c, double *out) {
  const Driver &D = *(Driver *)h;
  if (D.form == 0) ts_g(D.M.trip[(i * TS_MAXEL + j) * TS_MAXEL + k], c, &out[0], &out[1]);
  else ts_g(D.Z.trip[(i * TS_MAXEL + j) * TS_MAXEL + k], c, &out[0], &out[1]);
}
// fC and fC' of the pair (i, j) at r < R + D
void tfh_fc(void *h, int i, int j, double r, double *out) {
  const Driver &D = *(Driver *)h;
  if (D.form == 0) ts_pair_fc(D.M.pair[i * TS_MAXEL + j], r, &out[0], &out[1]);
  else ts_pair_fc(D.Z.pair[i * TS_MAXEL + j], r, &out[0], &out[1]);
}
// F, F', V_ZBL, V_ZBL' of the pair (i, j) (zbl)
void tfh_zbl(void *h, int i, int j, double r, double *out) {
  const TsZblPairP &P = ((Driver *)h)->Z.pair[i * TS_MAXEL + j];
  ts_zbl_fermi(P, r, &out[0], &out[1]);
  ts_zbl_v(P, r, &out[2], &out[3]);
}

// as tsh_compute (tests/tersoff_host_driver.cpp); fcsum: the sum of fC(r_ij) over the ordered pairs evaluated
int tfh_compute(void *h, int n, const int *types, const double *x, const double *box, double *f, double *e, double *w, int *counts, double *zetas, double *fcsum) {
  const Driver &D = *(Driver *)h;
  return D.form == 0 ? compute(D, D.M, n, types, x, box, f, e, w, counts, zetas, fcsum) : compute(D, D.Z, n, types, x, box, f, e, w, counts, zetas, fcsum);
}

}  // extern "C"
