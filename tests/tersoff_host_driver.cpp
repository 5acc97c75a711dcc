// tersoff_host_driver.cpp -- TEST HARNESS, not part of the product: runs the functions of scema_amd/csrc/tersoff/ts_core.h (the arithmetic
// the HIP kernels of md_tersoff.hip execute) as plain loops on the host, with the tables of the product's reader
// (host/tersoff_params.cpp), so that tests/test_tersoff_host.py can hold energies, forces and virial against tests/tersoff_numpy.py and
// against central differences without a GPU.  The loop structure follows k_ts_force: per central atom the neighbours inside the cutoff
// under which they are used, pass 1 over the neighbours j (zeta, b, the pair term, pref), pass 2 over the ordered (j, k).
// Built by the test with g++; nothing in scema_amd/ links it.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/tersoff_params.h"
#include "../scema_amd/csrc/tersoff/ts_core.h"

namespace {
struct Driver {
  TsTable T;
  std::vector<int> type_map;
  int wrong;   // deliberately wrong builds, for the tests that show what the suite catches: 1 the pair term owned by the lower index
               // (and doubled), 2 the R, D of fC(r_ik) taken from the pair entry i k k, 3 the same taken from the pair entry i j j (the
               // pair's own parameter set used where pair_tersoff.cpp uses that of i j k), 4 the neighbour list cut at the pair's own
               // R + D instead of cutin, so that no entry serves as a third atom only
};
struct Nb { int j, tj, code; double d[3], r, fc, dfc, pref; };
}  // namespace

extern "C" {

void *tsh_create(const char *path, const char *const *elements, int nel, int energy_unit, int wrong) {
  Driver *d = new Driver();
  std::vector<std::string> el(elements, elements + nel);
  std::string err;
  if (!scema::read_tersoff_params(path, el, energy_unit, d->T, d->type_map, err)) {
    std::fprintf(stderr, "tsh_create: %s\n", err.c_str());
    delete d;
    return nullptr;
  }
  d->wrong = wrong;
  if (wrong == 2 || wrong == 3)
    for (int i = 0; i < TS_MAXEL; i++)
      for (int j = 0; j < TS_MAXEL; j++)
        for (int k = 0; k < TS_MAXEL; k++) {
          TsTripP &Q = d->T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
          const TsPairP &P = d->T.pair[i * TS_MAXEL + (wrong == 2 ? k : j)];
          Q.bigr = P.bigr; Q.bigd = P.bigd; Q.cut = P.cut;
        }
  return d;
}
void tsh_destroy(void *h) { delete (Driver *)h; }
double tsh_cutmax(void *h) { return ((Driver *)h)->T.cutmax; }
// b and db/dzeta of the pair (i, j) as the kernels evaluate them (with the end forms), and the four switch points
void tsh_bond_order(void *h, int i, int j, double zeta, double *out) {
  const TsPairP &P = ((Driver *)h)->T.pair[i * TS_MAXEL + j];
  ts_bond_order(P, zeta, &out[0], &out[1]);
  out[2] = P.c1; out[3] = P.c2; out[4] = P.c3; out[5] = P.c4;
}
// the table slots as the kernels read them: out[0..8) of pair [i][j]: A B lambda1 lambda2 beta n R D; out[8..16) of triplet [i][j][k]: gamma
// lambda3 c^2 d^2 costheta0 R D m
void tsh_slot(void *h, int i, int j, int k, double *out) {
  const TsPairP &P = ((Driver *)h)->T.pair[i * TS_MAXEL + j];
  const TsTripP &Q = ((Driver *)h)->T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k];
  const double v[16] = {P.biga, P.bigb, P.lam1, P.lam2, P.beta, P.powern, P.bigr, P.bigd, Q.gamma, Q.lam3, Q.c2, Q.d2, Q.cos0, Q.bigr, Q.bigd, Q.m3 ? 3.0 : 1.0};
  for (int m = 0; m < 16; m++) out[m] = v[m];
}
void tsh_g(void *h, int i, int j, int k, double c, double *out) { ts_g(((Driver *)h)->T.trip[(i * TS_MAXEL + j) * TS_MAXEL + k], c, &out[0], &out[1]); }

// types: LAMMPS type - 1 per atom; box: xlo ylo zlo xhi yhi zhi xy xz yz; out: f [n][3], e [2] (repulsive, bond-order part), w [6]
// (xx yy zz xy xz yz), counts [3] (ordered pairs, ordered (j, k), most neighbours kept); zetas, when given: [n][32] beta zeta of every
// pair evaluated, in list order, -1 beyond
int tsh_compute(void *h, int n, const int *types, const double *x, const double *box, double *f, double *e, double *w, int *counts, double *zetas) {
  const Driver &D = *(Driver *)h;
  const TsTable &T = D.T;
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  for (int k = 0; k < 3 * n; k++) f[k] = 0.0;
  e[0] = e[1] = 0.0;
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
      const TsPairP &P = T.pair[ti * TS_MAXEL + tj];
      double d[3] = {x[3 * j] - x[3 * i], x[3 * j + 1] - x[3 * i + 1], x[3 * j + 2] - x[3 * i + 2]};
      // minimum image in fractional coordinates
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
            if (!(q.r < (D.wrong == 4 ? P.cut : T.cutin[ti * TS_MAXEL + tj]))) continue;   // at or beyond every cutoff it could be used under
            q.j = j; q.tj = tj; q.code = (sx + 1) + 3 * (sy + 1) + 9 * (sz + 1);
            q.fc = q.dfc = q.pref = 0.0;
            if (q.r < P.cut) ts_fc(P.bigr, P.bigd, q.r, &q.fc, &q.dfc);
            nb.push_back(q);
          }
    }
    counts[2] = std::max(counts[2], (int)nb.size());
    // pass 1
    int nz = 0;
    for (size_t a = 0; a < nb.size(); a++) {
      Nb &A = nb[a];
      const TsPairP &P = T.pair[ti * TS_MAXEL + A.tj];
      if (!(A.r < P.cut)) continue;
      if (D.wrong == 1 && !(A.j > i || (A.j == i && A.code > 13))) continue;
      double zeta = 0.0;
      for (size_t b = 0; b < nb.size(); b++) {
        if (b == a) continue;
        const TsTripP &Q = T.trip[(ti * TS_MAXEL + A.tj) * TS_MAXEL + nb[b].tj];
        if (!(nb[b].r < Q.cut)) continue;
        zeta += ts_zeta_term(Q, A.d, A.r, nb[b].d, nb[b].r);
      }
      if (zetas && nz < 32) zetas[32 * i + nz++] = P.beta * zeta;
      double bo, db, erep, eatt, fprep, fpatt, fa;
      ts_bond_order(P, zeta, &bo, &db);
      ts_pair(P, A.r, A.fc, A.dfc, bo, &erep, &eatt, &fprep, &fpatt, &fa);
      const double twice = D.wrong == 1 ? 2.0 : 1.0;
      A.pref = twice * 0.5 * A.fc * fa * db;
      const double fp = twice * (fprep + fpatt);
      const double g[3] = {fp * A.d[0], fp * A.d[1], fp * A.d[2]};
      for (int k = 0; k < 3; k++) { f[3 * A.j + k] += g[k]; f[3 * i + k] -= g[k]; }
      e[0] += twice * erep; e[1] += twice * eatt;
      counts[0]++;
      w[0] += A.d[0] * g[0]; w[1] += A.d[1] * g[1]; w[2] += A.d[2] * g[2]; w[3] += A.d[0] * g[1]; w[4] += A.d[0] * g[2]; w[5] += A.d[1] * g[2];
    }
    // pass 2
    for (size_t a = 0; a < nb.size(); a++)
      for (size_t b = 0; b < nb.size(); b++) {
        if (b == a) continue;
        const Nb &A = nb[a], &B = nb[b];
        const TsTripP &Q = T.trip[(ti * TS_MAXEL + A.tj) * TS_MAXEL + B.tj];
        if (!(A.r < T.pair[ti * TS_MAXEL + A.tj].cut) || !(B.r < Q.cut)) continue;
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

}  // extern "C"
