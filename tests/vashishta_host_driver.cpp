// vashishta_host_driver.cpp -- TEST HARNESS, not part of the product: a stand-alone program that runs the functions of
// scema_amd/csrc/vashishta/vs_core.h (the arithmetic the HIP kernel of md_vashishta.hip executes) as plain loops on the host, with the
// tables of the product's reader (host/vashishta_params.cpp), so that tests/test_vashishta_host.py can hold energies, forces and virial
// against tests/vashishta_numpy.py without a GPU.  The loop structure follows k_vs_force: per central atom one walk over its
// neighbours, the pair term in place for every one inside rc (this end's half), the ones inside r0 into a list, then the triplets (a < b)
// of the list.  Built by the test with g++; nothing in scema_amd/ links it.
//
//   vashishta_host_driver <file> <energy unit> <element> ... < input        input: n, the box (9 numbers), n lines `type x y z`
//   output: `e2 e3 npairs ntriplets maxin`, the virial (6), then n lines of forces, all %.17g
//
// Deliberately wrong builds, for the test that shows what the suite catches (switches of this file, not of the product):
//   -DVSH_WRONG=1  the shift terms U(rc), (r - rc) U'(rc) left out          2  r0, gamma of an arm from entry i j k, not i j j / i k k
//              3  Zi Zj without its sign                                     4  the pair energy counted at both ends in full
//              5  1 + C dc^2 missing from the derivative of the three-body term (one power of it)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/vashishta_params.h"
#include "../scema_amd/csrc/vashishta/vs_core.h"

#ifndef VSH_WRONG
#define VSH_WRONG 0
#endif

namespace {
struct Nb { int j, tj; double d[3], r, ex, da; };

#if VSH_WRONG == 5
// vs_three with the angular derivative 2 dc / (1 + C dc^2) in place of 2 dc / (1 + C dc^2)^2
void three(const VsTripP &T, const double *d1, double r1, double ex1, double da1, const double *d2, double r2, double ex2, double da2, double *e, double *fj,
           double *fk) {
  const double ir1 = 1.0 / r1, ir2 = 1.0 / r2;
  const double c = (d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2]) * ir1 * ir2, dc = c - T.cos0, den = 1.0 / (1.0 + T.c * dc * dc);
  const double pre = T.b * ex1 * ex2, erad = pre * dc * dc * den, eang = 2.0 * pre * dc * den;
  *e = erad;
  const double a12 = eang * ir1 * ir2, g1 = erad * da1 * ir1 - eang * c * ir1 * ir1, g2 = erad * da2 * ir2 - eang * c * ir2 * ir2;
  for (int k = 0; k < 3; k++) { fj[k] = -(g1 * d1[k] + a12 * d2[k]); fk[k] = -(g2 * d2[k] + a12 * d1[k]); }
}
#else
#define three vs_three
#endif
}  // namespace

int main(int argc, char **argv) {
  if (argc < 4) { std::fprintf(stderr, "usage: %s <file> <energy unit> <element> ... < input\n", argv[0]); return 2; }
  std::vector<std::string> el(argv + 3, argv + argc);
  VsTable T;
  std::vector<int> type_map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_vashishta_params(argv[1], el, std::atoi(argv[2]), T, type_map, err, &raw)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  const int ne = T.nelem;
  (void)ne;
#if VSH_WRONG == 1
  for (VsPairP &P : T.pair) P.urc = P.durc = 0.0;
#elif VSH_WRONG == 3
  for (VsPairP &P : T.pair) { P.kzz = std::fabs(P.kzz); if (P.rc > 0.0) vs_u(P, P.rc, &P.urc, &P.durc); }
#endif
  int n = 0;
  double box[9];
  if (std::scanf("%d", &n) != 1 || n <= 0) return 2;
  for (double &b : box) if (std::scanf("%lf", &b) != 1) return 2;
  std::vector<int> ty(n);
  std::vector<double> x(3 * (size_t)n), f(3 * (size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    int t;
    if (std::scanf("%d %lf %lf %lf", &t, &x[3 * i], &x[3 * i + 1], &x[3 * i + 2]) != 4 || t < 0 || t >= (int)type_map.size()) return 2;
    ty[i] = type_map[t];
  }
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  // images as deep as the largest cutoff reaches (an orthogonal estimate made safe by one more image in a tilted box)
  const int tilt = (xy != 0.0 || xz != 0.0 || yz != 0.0) ? 1 : 0;
  const int mx = (int)std::floor(T.cutmax / hx + 0.5) + tilt, my = (int)std::floor(T.cutmax / hy + 0.5) + tilt, mz = (int)std::floor(T.cutmax / hz + 0.5) + tilt;
  double e2 = 0.0, e3 = 0.0, w[6] = {0, 0, 0, 0, 0, 0};
  long npairs = 0, ntrip = 0;
  int maxin = 0;
  std::vector<Nb> nb;
  for (int i = 0; i < n; i++) {
    const int ti = ty[i];
    nb.clear();
    for (int j = 0; j < n; j++) {
      const int tj = ty[j];
      const VsPairP &P = T.pair[ti * VS_MAXEL + tj];
      double d[3] = {x[3 * j] - x[3 * i], x[3 * j + 1] - x[3 * i + 1], x[3 * j + 2] - x[3 * i + 2]};
      double s2 = d[2] / hz, s1 = (d[1] - yz * s2) / hy, s0 = (d[0] - xy * s1 - xz * s2) / hx;
      s0 -= std::rint(s0); s1 -= std::rint(s1); s2 -= std::rint(s2);
      d[0] = hx * s0 + xy * s1 + xz * s2; d[1] = hy * s1 + yz * s2; d[2] = hz * s2;
      for (int sz = -mz; sz <= mz; sz++)
        for (int sy = -my; sy <= my; sy++)
          for (int sx = -mx; sx <= mx; sx++) {
            if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
            Nb q;
            q.d[0] = d[0] + sx * hx + sy * xy + sz * xz; q.d[1] = d[1] + sy * hy + sz * yz; q.d[2] = d[2] + sz * hz;
            q.r = std::sqrt(q.d[0] * q.d[0] + q.d[1] * q.d[1] + q.d[2] * q.d[2]);
            if (!(q.r > 0.0)) continue;
            if (q.r < P.rc) {   // the pair term, this end's half
              double e, fp;
              vs_two(P, q.r, &e, &fp);
              for (int k = 0; k < 3; k++) f[3 * i + k] -= fp * q.d[k];
#if VSH_WRONG == 4
              e2 += e;
#else
              e2 += 0.5 * e;
#endif
              npairs++;
              const double hf = 0.5 * fp;
              w[0] += hf * q.d[0] * q.d[0]; w[1] += hf * q.d[1] * q.d[1]; w[2] += hf * q.d[2] * q.d[2];
              w[3] += hf * q.d[0] * q.d[1]; w[4] += hf * q.d[0] * q.d[2]; w[5] += hf * q.d[1] * q.d[2];
            }
            if (q.r < P.r0) {
              q.j = j; q.tj = tj;
              vs_arm(P, q.r, &q.ex, &q.da);
              nb.push_back(q);
            }
          }
    }
    maxin = std::max(maxin, (int)nb.size());
    for (size_t b = 1; b < nb.size(); b++)
      for (size_t a = 0; a < b; a++) {
        Nb A = nb[a], B = nb[b];
        ntrip++;
        const VsTripP &Q = T.trip[(ti * VS_MAXEL + A.tj) * VS_MAXEL + B.tj];
#if VSH_WRONG == 2
        {   // both arms with gamma, r0 of the triplet's own entry i j k
          const double *u = &raw[(((size_t)ti * ne + A.tj) * ne + B.tj) * VS_NFIELD];
          VsPairP W = T.pair[ti * VS_MAXEL + A.tj];
          W.gamma = u[10]; W.r0 = u[11];
          if (!(A.r < W.r0) || !(B.r < W.r0)) continue;
          vs_arm(W, A.r, &A.ex, &A.da);
          vs_arm(W, B.r, &B.ex, &B.da);
        }
#endif
        if (Q.b == 0.0) continue;
        double e, fj[3], fk[3];
        three(Q, A.d, A.r, A.ex, A.da, B.d, B.r, B.ex, B.da, &e, fj, fk);
        for (int c = 0; c < 3; c++) { f[3 * A.j + c] += fj[c]; f[3 * B.j + c] += fk[c]; f[3 * i + c] -= fj[c] + fk[c]; }
        e3 += e;
        w[0] += A.d[0] * fj[0] + B.d[0] * fk[0]; w[1] += A.d[1] * fj[1] + B.d[1] * fk[1]; w[2] += A.d[2] * fj[2] + B.d[2] * fk[2];
        w[3] += A.d[0] * fj[1] + B.d[0] * fk[1]; w[4] += A.d[0] * fj[2] + B.d[0] * fk[2]; w[5] += A.d[1] * fj[2] + B.d[1] * fk[2];
      }
  }
  std::printf("%.17g %.17g %ld %ld %d\n", e2, e3, npairs, ntrip, maxin);
  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", w[0], w[1], w[2], w[3], w[4], w[5]);
  for (int i = 0; i < n; i++) std::printf("%.17g %.17g %.17g\n", f[3 * i], f[3 * i + 1], f[3 * i + 2]);
  return 0;
}
