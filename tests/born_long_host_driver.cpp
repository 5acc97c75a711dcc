// born_long_host_driver.cpp -- TEST HARNESS, not part of the product: a stand-alone program that runs the functions of
// scema_amd/csrc/ionic/bl_core.h (the arithmetic the HIP kernels of md_born_long.hip execute) as plain loops on the host, with the table of
// the product's reader (host/born_long_params.cpp), so that tests/test_born_long_host.py can hold energies, forces and virial against
// tests/born_long_numpy.py without a GPU.  The loop structure follows the kernels: per central atom one walk over its neighbours inside
// cutmax (k_bl_force: ionic_force, md_ionic_force.h, with the terms of md_born_long.hip); per k-vector S(k) over the atoms in atom order, c_k, the reciprocal energy and virial, then the self and background
// terms (k_bl_sfac); per atom the reciprocal force over the k list (k_bl_recip).  g_ewald and the triples come with the input (the test
// takes them from scema_md_born_long_kvectors or from its own rule).  Built by the test with g++; nothing in scema_amd/ links it.
//
//   born_long_host_driver <file> <energy unit> < input       input: n, the box (9 numbers), g, nk, nk lines `n1 n2 n3`, n lines `type q x y z`
//   output: `e_born e_coul npairs ncoul`, the virial (6), then n lines of forces, all %.17g
//   born_long_host_driver <file> <energy unit> --read        the reader alone, then bl_pair of every pair of types at a few distances:
//   prints `ok <types> <cutmax> <checksum>`, or the reader's message on stderr and exit status 1 (the corrupt-file tests)
//
// Deliberately wrong builds, for the test that shows what the suite catches (switches of this file, not of the product):
//   -DBLH_WRONG=1  the -g/sqrt(pi) term missing     2  the half-space factor 1 for 2     3  the sign of the reciprocal force
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/born_long_params.h"
#include "../scema_amd/csrc/ionic/bl_core.h"

#ifndef BLH_WRONG
#define BLH_WRONG 0
#endif

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <file> <energy unit> [--read] < input\n", argv[0]); return 2; }
  BlTable T;
  std::vector<int> type_map;
  std::vector<double> raw;
  std::string err;
  if (!scema::read_born_long_params(argv[1], std::atoi(argv[2]), T, type_map, err, &raw)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  const BdTable &B = T.bd;
  if (argc > 3 && std::strcmp(argv[3], "--read") == 0) {
    double sum = 0.0;
    for (int a = 0; a < B.ntypes; a++)
      for (int b = 0; b < B.ntypes; b++)
        for (double r : {0.5, 2.0, 0.999 * B.cutmax, B.cutmax}) {
          double eb, ec, fb, fc;
          bl_pair(T, B.pair[a * BD_MAXEL + b], 0.3, 1.0, -1.0, r * r, &eb, &ec, &fb, &fc);
          sum += eb + ec + fb + fc;
        }
    std::printf("ok %d %.17g %.17g\n", B.ntypes, B.cutmax, sum + T.accuracy);
    return 0;
  }
  int n = 0, nk = 0;
  double box[9], g = 0.0;
  if (std::scanf("%d", &n) != 1 || n <= 0) return 2;
  for (double &b : box) if (std::scanf("%lf", &b) != 1) return 2;
  if (std::scanf("%lf %d", &g, &nk) != 2 || !(g > 0.0) || nk < 0 || nk > (1 << 20)) return 2;
  std::vector<int> kn(3 * (size_t)nk);
  for (int &v : kn) if (std::scanf("%d", &v) != 1) return 2;
  std::vector<int> ty(n);
  std::vector<double> q(n), x(3 * (size_t)n), f(3 * (size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    int t;
    if (std::scanf("%d %lf %lf %lf %lf", &t, &q[i], &x[3 * i], &x[3 * i + 1], &x[3 * i + 2]) != 5 || t < 0 || t >= (int)type_map.size()) return 2;
    ty[i] = type_map[t];
  }
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  const double h[6] = {hx, hy, hz, yz, xz, xy}, vol = hx * hy * hz;
  // ---- real space (k_bl_force): images as deep as the largest cutoff reaches, one more in a tilted box
  const int tilt = (xy != 0.0 || xz != 0.0 || yz != 0.0) ? 1 : 0;
  const int mx = (int)std::floor(B.cutmax / hx + 0.5) + tilt, my = (int)std::floor(B.cutmax / hy + 0.5) + tilt, mz = (int)std::floor(B.cutmax / hz + 0.5) + tilt;
  double e_born = 0.0, e_coul = 0.0, wb[6] = {0, 0, 0, 0, 0, 0}, wc[6] = {0, 0, 0, 0, 0, 0};
  long npairs = 0, ncoul = 0;
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      const BdPairP &P = B.pair[ty[i] * BD_MAXEL + ty[j]];
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
            if (!(r2 > 0.0) || !(r2 < B.cutmax * B.cutmax)) continue;
            double eb, ec, fb, fc;
            bl_pair(T, P, g, q[i], q[j], r2, &eb, &ec, &fb, &fc);
            const double fp = fb + fc;
            for (int k = 0; k < 3; k++) f[3 * i + k] -= fp * e[k];
            e_born += 0.5 * eb; e_coul += 0.5 * ec;
            npairs++;
            if (std::sqrt(r2) < B.cut_coul) ncoul++;
            const double hb = 0.5 * fb, hc = 0.5 * fc;
            wb[0] += hb * e[0] * e[0]; wb[1] += hb * e[1] * e[1]; wb[2] += hb * e[2] * e[2]; wb[3] += hb * e[0] * e[1]; wb[4] += hb * e[0] * e[2]; wb[5] += hb * e[1] * e[2];
            wc[0] += hc * e[0] * e[0]; wc[1] += hc * e[1] * e[1]; wc[2] += hc * e[2] * e[2]; wc[3] += hc * e[0] * e[1]; wc[4] += hc * e[0] * e[2]; wc[5] += hc * e[1] * e[2];
          }
    }
  // ---- structure factors, reciprocal energy and virial (k_bl_sfac), reciprocal forces (k_bl_recip)
  std::vector<double> u(3 * (size_t)n);
  for (int i = 0; i < n; i++) bl_frac(h, &x[3 * i], &u[3 * i]);
  double qsqsum = 0.0, qsum = 0.0;
  for (int i = 0; i < n; i++) { qsqsum += q[i] * q[i]; qsum += q[i]; }
  for (int k = 0; k < nk; k++) {
    const int n1 = kn[3 * k], n2 = kn[3 * k + 1], n3 = kn[3 * k + 2];
    double sre = 0.0, sim = 0.0;
    std::vector<double> cs(n), sn(n);
    for (int i = 0; i < n; i++) {
      const double ph = BL_TWO_PI * (n1 * u[3 * i] + n2 * u[3 * i + 1] + n3 * u[3 * i + 2]);
      cs[i] = std::cos(ph); sn[i] = std::sin(ph);
      sre += q[i] * cs[i]; sim += q[i] * sn[i];
    }
    double kv[3];
    bl_kvec(h, n1, n2, n3, kv);
    const double k2 = kv[0] * kv[0] + kv[1] * kv[1] + kv[2] * kv[2];
    double ck = bl_coef(B.k, g, vol, k2);
#if BLH_WRONG == 2
    ck *= 0.5;
#endif
    const double ek = ck * (sre * sre + sim * sim), vf = -2.0 * (1.0 / k2 + 0.25 / (g * g)) * ek;
    e_coul += ek;
    wc[0] += ek + vf * kv[0] * kv[0]; wc[1] += ek + vf * kv[1] * kv[1]; wc[2] += ek + vf * kv[2] * kv[2];
    wc[3] += vf * kv[0] * kv[1]; wc[4] += vf * kv[0] * kv[2]; wc[5] += vf * kv[1] * kv[2];
    for (int i = 0; i < n; i++) {
      double t = -2.0 * q[i] * ck * (sim * cs[i] - sre * sn[i]);
#if BLH_WRONG == 3
      t = -t;
#endif
      for (int c = 0; c < 3; c++) f[3 * i + c] += t * kv[c];
    }
  }
  double ebg;
  double es = bl_self(B.k, g, vol, qsqsum, qsum, &ebg);
#if BLH_WRONG == 1
  es = ebg;
#endif
  e_coul += es;
  wc[0] += ebg; wc[1] += ebg; wc[2] += ebg;
  std::printf("%.17g %.17g %ld %ld\n", e_born, e_coul, npairs, ncoul);
  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", wb[0] + wc[0], wb[1] + wc[1], wb[2] + wc[2], wb[3] + wc[3], wb[4] + wc[4], wb[5] + wc[5]);
  for (int i = 0; i < n; i++) std::printf("%.17g %.17g %.17g\n", f[3 * i], f[3 * i + 1], f[3 * i + 2]);
  return 0;
}
