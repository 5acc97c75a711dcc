// born_long_mesh_host_driver.cpp -- TEST HARNESS, not part of the product: a stand-alone program that runs the functions of
// scema_amd/csrc/pppm/pppm_core.h and ionic/blm_core.h (the arithmetic the HIP kernels of md_born_long_mesh.hip execute, and -- the core --
// those of md_pppm.hip) as plain loops on the host, with a plain
// DFT in place of hipFFT and the table of the product's reader, so that tests/test_born_long_mesh_host.py can hold energies, forces and
// virial against tests/born_long_mesh_numpy.py without a GPU.  The loop structure follows the kernels: real space as
// born_long_host_driver.cpp; per atom 125 fixed-point adds to the charge grid (k_blm_assign), fixed point -> complex (k_blm_convert), the
// forward transform, the influence function (k_blm_gf), per mode energy, virial and field spectra and the self and background terms
// (k_blm_poisson), three backward transforms, per atom the gather over its 125 points (k_blm_interp).  g_ewald and the mesh come with the
// input.  Built by the test with g++; nothing in scema_amd/ links it.
//
//   born_long_mesh_host_driver <file> <energy unit> < input   input: n, the box (9 numbers), g, nx ny nz, n lines `type q x y z`
//   output: `e_born e_coul npairs ncoul`, the virial (6), then n lines of forces, all %.17g
//
// Deliberately wrong builds, for the test that shows what the suite catches (switches of this file, not of the product):
//   -DBLMH_WRONG=1  the -g/sqrt(pi) term missing     2  K of the other unit on the mesh (eV for kcal/mol)     3  the sign of the field
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../scema_amd/csrc/host/born_long_params.h"
#include "../scema_amd/csrc/ionic/blm_core.h"

#ifndef BLMH_WRONG
#define BLMH_WRONG 0
#endif

typedef std::complex<double> cplx;

// a plain DFT along dimension d of a grid n[0] x n[1] x n[2] (x fastest), sign -1 forward, +1 backward, unnormalised
static void dft_dim(std::vector<cplx> &a, const int *n, int d, int sign) {
  const int len = n[d], stride = d == 0 ? 1 : (d == 1 ? n[0] : n[0] * n[1]);
  std::vector<cplx> tw(len), line(len);
  for (int j = 0; j < len; j++) tw[j] = std::polar(1.0, sign * BL_TWO_PI * j / len);
  const int ng = n[0] * n[1] * n[2];
  for (int base = 0; base < ng; base++) {
    if ((base / stride) % len != 0) continue;   // (the first point of every line)
    for (int m = 0; m < len; m++) {
      cplx s = 0.0;
      for (int j = 0; j < len; j++) s += a[base + (size_t)j * stride] * tw[(int)(((long long)j * m) % len)];
      line[m] = s;
    }
    for (int m = 0; m < len; m++) a[base + (size_t)m * stride] = line[m];
  }
}
static void dft3(std::vector<cplx> &a, const int *n, int sign) { for (int d = 0; d < 3; d++) dft_dim(a, n, d, sign); }

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <file> <energy unit> < input\n", argv[0]); return 2; }
  BlTable T;
  std::vector<int> type_map;
  std::string err;
  if (!scema::read_born_long_params(argv[1], std::atoi(argv[2]), T, type_map, err, nullptr)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  const BdTable &B = T.bd;
  int n = 0, mesh[3];
  double box[9], g = 0.0;
  if (std::scanf("%d", &n) != 1 || n <= 0) return 2;
  for (double &b : box) if (std::scanf("%lf", &b) != 1) return 2;
  if (std::scanf("%lf %d %d %d", &g, &mesh[0], &mesh[1], &mesh[2]) != 4 || !(g > 0.0)) return 2;
  for (int d = 0; d < 3; d++) if (mesh[d] < 2 || mesh[d] > 512) return 2;
  const int ng = mesh[0] * mesh[1] * mesh[2];
  if (ng > (1 << 20)) return 2;
  std::vector<int> ty(n);
  std::vector<double> q(n), x(3 * (size_t)n), f(3 * (size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    int t;
    if (std::scanf("%d %lf %lf %lf %lf", &t, &q[i], &x[3 * i], &x[3 * i + 1], &x[3 * i + 2]) != 5 || t < 0 || t >= (int)type_map.size()) return 2;
    ty[i] = type_map[t];
  }
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  const double h[6] = {hx, hy, hz, yz, xz, xy}, lo[3] = {box[0], box[1], box[2]}, vol = hx * hy * hz;
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
  // ---- the mesh
  double kc = B.k;
#if BLMH_WRONG == 2
  kc = 14.399645;
#endif
  double qsqsum = 0.0, qsum = 0.0, qabs = 0.0;
  for (int i = 0; i < n; i++) { qsqsum += q[i] * q[i]; qsum += q[i]; qabs += std::fabs(q[i]); }
  const int shift = blm_fixed_shift(qabs, ng, vol);
  const double delvolinv = (double)ng / vol;
  // k_blm_assign: fixed-point adds, atoms in reverse order (the sum does not depend on it)
  std::vector<long long> igrid(ng, 0);
  std::vector<int> gidx((size_t)n * 125);
  std::vector<double> gw((size_t)n * 125);
  for (int i = n - 1; i >= 0; i--) {
    double t[3], wx[5], wy[5], wz[5];
    blm_frac(h, lo, &x[3 * i], t);
    const int ix = pppm_weights(t[0] * mesh[0], wx), iy = pppm_weights(t[1] * mesh[1], wy), iz = pppm_weights(t[2] * mesh[2], wz);
    for (int p = 0; p < 125; p++) {
      const int c = p / 25, b = (p / 5) % 5, k = p % 5;
      const int idx = (pppm_wrap1(iz + c - 2, mesh[2]) * mesh[1] + pppm_wrap1(iy + b - 2, mesh[1])) * mesh[0] + pppm_wrap1(ix + k - 2, mesh[0]);
      const double w = wz[c] * wy[b] * wx[k];
      gidx[(size_t)i * 125 + p] = idx; gw[(size_t)i * 125 + p] = w;
      igrid[idx] += blm_to_fixed(q[i] * delvolinv * w, shift);
    }
  }
  // k_blm_convert and the forward transform
  std::vector<cplx> rho(ng);
  for (int k = 0; k < ng; k++) rho[k] = cplx(blm_from_fixed(igrid[k], shift), 0.0);
  dft3(rho, mesh, -1);
  // k_blm_gf, k_blm_poisson
  std::vector<cplx> field[3] = {std::vector<cplx>(ng), std::vector<cplx>(ng), std::vector<cplx>(ng)};
  double er = 0.0, hinv[6];
  bl_hinv(h, hinv);
  for (int idx = 0; idx < ng; idx++) {
    const int m1 = idx % mesh[0], m2 = (idx / mesh[0]) % mesh[1], m3 = idx / (mesh[0] * mesh[1]);
    const double gf = pppm_gf(hinv, g, mesh[0], mesh[1], mesh[2], m1, m2, m3), scaleinv = 1.0 / (double)ng;
    double kv[3], pr, pi;
    pppm_kvec(hinv, pppm_signed(m1, mesh[0]), pppm_signed(m2, mesh[1]), pppm_signed(m3, mesh[2]), kv[0], kv[1], kv[2]);
    pppm_mode_term(vol, kc, g, kv[0], kv[1], kv[2], rho[idx].real() * scaleinv, rho[idx].imag() * scaleinv, gf, wc, er, pr, pi);
    for (int c = 0; c < 3; c++) field[c][idx] = cplx(kv[c] * pi, -kv[c] * pr);
  }
  e_coul += er;
  double ebg;
  double es = bl_self(kc, g, vol, qsqsum, qsum, &ebg);
#if BLMH_WRONG == 1
  es = ebg;
#endif
  e_coul += es;
  wc[0] += ebg; wc[1] += ebg; wc[2] += ebg;
  // the backward transforms and k_blm_interp
  for (int c = 0; c < 3; c++) dft3(field[c], mesh, +1);
  for (int i = 0; i < n; i++) {
    double fs[3] = {0.0, 0.0, 0.0};
    for (int p = 0; p < 125; p++)
      for (int c = 0; c < 3; c++) fs[c] = fma(gw[(size_t)i * 125 + p], field[c][gidx[(size_t)i * 125 + p]].real(), fs[c]);
    double kq = kc * q[i];
#if BLMH_WRONG == 3
    kq = -kq;
#endif
    for (int c = 0; c < 3; c++) f[3 * i + c] += kq * fs[c];
  }
  std::printf("%.17g %.17g %ld %ld\n", e_born, e_coul, npairs, ncoul);
  std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", wb[0] + wc[0], wb[1] + wc[1], wb[2] + wc[2], wb[3] + wc[3], wb[4] + wc[4], wb[5] + wc[5]);
  for (int i = 0; i < n; i++) std::printf("%.17g %.17g %.17g\n", f[3 * i], f[3 * i + 1], f[3 * i + 2]);
  return 0;
}
