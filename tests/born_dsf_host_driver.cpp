// born_dsf_host_driver.cpp -- TEST HARNESS, not part of the product: a stand-alone program that runs the functions of
// scema_amd/csrc/ionic/bd_core.h (the arithmetic the HIP kernel of md_born_dsf.hip executes) as plain loops on the host, with the table of
// the product's reader (host/born_dsf_params.cpp), so that tests/test_born_dsf_host.py can hold energies, forces and virial against
// tests/born_dsf_numpy.py without a GPU.  The loop structure follows k_bd_force (ionic_force, md_ionic_force.h, with the terms of md_born_dsf.hip): per central atom one walk over its neighbours inside
// cutmax, this end's half of the pair's energies and virial, then the atom's self energy.  Built by the test with g++; nothing in
// scema_amd/ links it.
//
//   born_dsf_host_driver <file> <energy unit> < input        input: n, the box (9 numbers), n lines `type q x y z`
//   output: `e_born e_coul npairs ncoul`, the virial (6), then n lines of forces, all %.17g
//   born_dsf_host_driver <file> <energy unit> --read         the reader alone, then bd_pair of every pair of types at a few distances:
//   prints `ok <types> <cutmax> <checksum>`, or the reader's message on stderr and exit status 1 (the corrupt-file tests)
//
// Deliberately wrong builds, for the test that shows what the suite catches (switches of this file, not of the product):
//   -DBDH_WRONG=1  the sign of f_s swapped          2  the self term missing          3  q_i^2 in place of q_i q_j
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/born_dsf_params.h"
#include "../scema_amd/csrc/ionic/bd_core.h"

#ifndef BDH_WRONG
#define BDH_WRONG 0
#endif

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <file> <energy unit> [--read] < input\n", argv[0]); return 2; }
  BdTable T;
  std::vector<int> type_map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_born_dsf_params(argv[1], std::atoi(argv[2]), T, type_map, err, &raw)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  if (argc > 3 && std::strcmp(argv[3], "--read") == 0) {
    double sum = 0.0;
    for (int a = 0; a < T.ntypes; a++)
      for (int b = 0; b < T.ntypes; b++)
        for (double r : {0.5, 2.0, 0.999 * T.cutmax, T.cutmax}) {
          double eb, ec, fb, fc;
          bd_pair(T, T.pair[a * BD_MAXEL + b], 1.0, -1.0, r * r, &eb, &ec, &fb, &fc);
          sum += eb + ec + fb + fc;
        }
    std::printf("ok %d %.17g %.17g\n", T.ntypes, T.cutmax, sum + bd_self(T, 1.0));
    return 0;
  }
#if BDH_WRONG == 1
  T.f_s = -T.f_s;
#endif
  int n = 0;
  double box[9];
  if (std::scanf("%d", &n) != 1 || n <= 0) return 2;
  for (double &b : box) if (std::scanf("%lf", &b) != 1) return 2;
  std::vector<int> ty(n);
  std::vector<double> q(n), x(3 * (size_t)n), f(3 * (size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    int t;
    if (std::scanf("%d %lf %lf %lf %lf", &t, &q[i], &x[3 * i], &x[3 * i + 1], &x[3 * i + 2]) != 5 || t < 0 || t >= (int)type_map.size()) return 2;
    ty[i] = type_map[t];
  }
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  // images as deep as the largest cutoff reaches (an orthogonal estimate made safe by one more image in a tilted box)
  const int tilt = (xy != 0.0 || xz != 0.0 || yz != 0.0) ? 1 : 0;
  const int mx = (int)std::floor(T.cutmax / hx + 0.5) + tilt, my = (int)std::floor(T.cutmax / hy + 0.5) + tilt, mz = (int)std::floor(T.cutmax / hz + 0.5) + tilt;
  double e_born = 0.0, e_coul = 0.0, wb[6] = {0, 0, 0, 0, 0, 0}, wc[6] = {0, 0, 0, 0, 0, 0};
  long npairs = 0, ncoul = 0;
  for (int i = 0; i < n; i++) {
    for (int j = 0; j < n; j++) {
      const BdPairP &P = T.pair[ty[i] * BD_MAXEL + ty[j]];
      double d[3] = {x[3 * j] - x[3 * i], x[3 * j + 1] - x[3 * i + 1], x[3 * j + 2] - x[3 * i + 2]};
      double s2 = d[2] / hz, s1 = (d[1] - yz * s2) / hy, s0 = (d[0] - xy * s1 - xz * s2) / hx;
      s0 -= std::rint(s0); s1 -= std::rint(s1); s2 -= std::rint(s2);
      d[0] = hx * s0 + xy * s1 + xz * s2; d[1] = hy * s1 + yz * s2; d[2] = hz * s2;
      for (int sz = -mz; sz <= mz; sz++)
        for (int sy = -my; sy <= my; sy++)
          for (int sx = -mx; sx <= mx; sx++) {
            if (j == i && sx == 0 && sy == 0 && sz == 0) continue;
            const double e[3] = {d[0] + sx * hx + sy * xy + sz * xz, d[1] + sy * hy + sz * yz, d[2] + sz * hz};
            const double r2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2];
            if (!(r2 > 0.0) || !(r2 < T.cutmax * T.cutmax)) continue;
            double eb, ec, fb, fc;
#if BDH_WRONG == 3
            bd_pair(T, P, q[i], q[i], r2, &eb, &ec, &fb, &fc);
#else
            bd_pair(T, P, q[i], q[j], r2, &eb, &ec, &fb, &fc);
#endif
            const double fp = fb + fc;
            for (int k = 0; k < 3; k++) f[3 * i + k] -= fp * e[k];
            e_born += 0.5 * eb; e_coul += 0.5 * ec;
            npairs++;
            if (std::sqrt(r2) < T.cut_coul) ncoul++;
            const double hb = 0.5 * fb, hc = 0.5 * fc;
            wb[0] += hb * e[0] * e[0]; wb[1] += hb * e[1] * e[1]; wb[2] += hb * e[2] * e[2]; wb[3] += hb * e[0] * e[1]; wb[4] += hb * e[0] * e[2]; wb[5] += hb * e[1] * e[2];
            wc[0] += hc * e[0] * e[0]; wc[1] += hc * e[1] * e[1]; wc[2] += hc * e[2] * e[2]; wc[3] += hc * e[0] * e[1]; wc[4] += hc * e[0] * e[2]; wc[5] += hc * e[1] * e[2];
          }
    }
#if BDH_WRONG != 2
    e_coul += bd_self(T, q[i]);
#endif
  }
  std::printf("%.17g %.17g %ld %ld\n", e_born, e_coul, npairs, ncoul);
  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", wb[0] + wc[0], wb[1] + wc[1], wb[2] + wc[2], wb[3] + wc[3], wb[4] + wc[4], wb[5] + wc[5]);
  for (int i = 0; i < n; i++) std::printf("%.17g %.17g %.17g\n", f[3 * i], f[3 * i + 1], f[3 * i + 2]);
  return 0;
}
