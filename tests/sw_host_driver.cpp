// sw_host_driver.cpp -- TEST HARNESS, not part of the product: runs the functions of scema_amd/csrc/sw/sw_core.h (the arithmetic the HIP
// kernels of md_sw.hip execute) as plain loops on the host, with the tables of the product's reader (host/sw_params.cpp), so that
// tests/test_sw_host.py can hold energies, forces and virial against tests/sw_numpy.py and against central differences without a GPU.
// The loop structure follows k_sw_force: per central atom the neighbours inside their cutoff, the pairs the atom owns, the triplets a < b.
// Built by the test with g++; nothing in scema_amd/ links it.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/sw_params.h"
#include "../scema_amd/csrc/sw/sw_core.h"

namespace {
struct Driver {
  SwTable T;
  std::vector<int> type_map;
};
struct Nb { int ent, tj; double d[3], r, ex, da; };
}  // namespace

extern "C" {

// general != 0: the pow path for every pair, whatever p and q are
void *swh_create(const char *path, const char *const *elements, int nel, int energy_unit, int general) {
  Driver *d = new Driver();
  std::vector<std::string> el(elements, elements + nel);
  std::string err;
  if (!scema::read_sw_params(path, el, energy_unit, d->T, d->type_map, err)) {
    std::fprintf(stderr, "swh_create: %s\n", err.c_str());
    delete d;
    return nullptr;
  }
  if (general)
    for (SwPairP &P : d->T.pair) P.fast = 0;
  return d;
}
void swh_destroy(void *h) { delete (Driver *)h; }
double swh_cutmax(void *h) { return ((Driver *)h)->T.cutmax; }
int swh_fast_pairs(void *h) {
  int n = 0;
  for (const SwPairP &P : ((Driver *)h)->T.pair) n += P.fast;
  return n;
}

// types: LAMMPS type - 1 per atom; box: xlo ylo zlo xhi yhi zhi xy xz yz; out: f [n][3], e [2], w [6] (xx yy zz xy xz yz), counts [3]
// (pairs, triplets, most neighbours inside the cutoff)
int swh_compute(void *h, int n, const int *types, const double *x, const double *box, double *f, double *e, double *w, int *counts) {
  const Driver &D = *(Driver *)h;
  const SwTable &T = D.T;
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  for (int k = 0; k < 3 * n; k++) f[k] = 0.0;
  e[0] = e[1] = 0.0;
  for (int k = 0; k < 6; k++) w[k] = 0.0;
  counts[0] = counts[1] = counts[2] = 0;
  std::vector<Nb> nb;
  for (int i = 0; i < n; i++) {
    if (types[i] < 0 || types[i] >= (int)D.type_map.size()) return 1;
    const int ti = D.type_map[types[i]];
    nb.clear();
    for (int j = 0; j < n; j++) {
      if (types[j] < 0 || types[j] >= (int)D.type_map.size()) return 1;
      const int tj = D.type_map[types[j]];
      const SwPairP &P = T.pair[ti * SW_MAXEL + tj];
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
            if (!(q.r < P.cut)) continue;   // at or beyond the cutoff: exactly zero, never an exponential
            q.ent = j | (((sx + 2) + 5 * (sy + 2) + 25 * (sz + 2)) << 24);
            q.tj = tj;
            sw_arm(P, q.r, &q.ex, &q.da);
            nb.push_back(q);
          }
    }
    counts[2] = std::max(counts[2], (int)nb.size());
    for (const Nb &q : nb) {
      if (!sw_owns(i, q.ent)) continue;
      double ep, fp;
      sw_two(T.pair[ti * SW_MAXEL + q.tj], q.r, &ep, &fp);
      const int j = q.ent & SW_JMASK;
      const double g[3] = {fp * q.d[0], fp * q.d[1], fp * q.d[2]};
      for (int k = 0; k < 3; k++) { f[3 * j + k] += g[k]; f[3 * i + k] -= g[k]; }
      e[0] += ep;
      counts[0]++;
      w[0] += q.d[0] * g[0]; w[1] += q.d[1] * g[1]; w[2] += q.d[2] * g[2]; w[3] += q.d[0] * g[1]; w[4] += q.d[0] * g[2]; w[5] += q.d[1] * g[2];
    }
    for (size_t a = 0; a < nb.size(); a++)
      for (size_t b = a + 1; b < nb.size(); b++) {
        const Nb &A = nb[a], &B = nb[b];
        double et, fj[3], fk[3];
        sw_three(T.trip[(ti * SW_MAXEL + A.tj) * SW_MAXEL + B.tj], A.d, A.r, A.ex, A.da, B.d, B.r, B.ex, B.da, &et, fj, fk);
        const int j = A.ent & SW_JMASK, k = B.ent & SW_JMASK;
        for (int c = 0; c < 3; c++) { f[3 * j + c] += fj[c]; f[3 * k + c] += fk[c]; f[3 * i + c] -= fj[c] + fk[c]; }
        e[1] += et;
        counts[1]++;
        w[0] += A.d[0] * fj[0] + B.d[0] * fk[0]; w[1] += A.d[1] * fj[1] + B.d[1] * fk[1]; w[2] += A.d[2] * fj[2] + B.d[2] * fk[2];
        w[3] += A.d[0] * fj[1] + B.d[0] * fk[1]; w[4] += A.d[0] * fj[2] + B.d[0] * fk[2]; w[5] += A.d[1] * fj[2] + B.d[1] * fk[2];
      }
  }
  return 0;
}

}  // extern "C"
