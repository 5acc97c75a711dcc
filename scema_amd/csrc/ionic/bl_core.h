// bl_core.h -- the arithmetic of the Ewald ionic stage (`pair_style born/coul/long`, `buck/coul/long` with `kspace_style ewald`): the
// Born-Mayer-Huggins term of bd_core.h (Buckingham is sigma = 0, D = 0) and the Coulomb sum split by Ewald's method.  Compiled by hipcc
// for the kernels of md_born_long.hip and by plain g++ for the host (host/born_long_params.cpp fills the table,
// tests/born_long_host_driver.cpp pins the derivatives on the CPU).
//
//   E_born  = A exp((sigma - r)/rho) - C/r^6 + D/r^8                        r < cut_lj[ti][tj], not shifted
//   E_real  = K q_i q_j erfc(g r)/r                                         r < cut_coul, not shifted
//   E_recip = (2 pi K/V) sum_{k != 0} exp(-k^2/4g^2)/k^2 |S(k)|^2,          S(k) = sum_i q_i exp(i k.r_i)
//             = sum over the half space of c_k |S(k)|^2,                    c_k = (4 pi K/V) exp(-k^2/4g^2)/k^2
//   E_self  = -K g/sqrt(pi) sum q_i^2  -  K pi (sum q_i)^2 / (2 g^2 V)      (the second term: the neutralising background)
//
// Forces are the exact gradients: the reciprocal force on atom i is -2 q_i sum_half c_k k Im(S(k) exp(-i k.r_i)).  The virial is the
// strain derivative of the whole energy at fixed g and fixed integer triples: the pair virial, c_k |S|^2 [delta_ab - 2 (1/k^2 + 1/4g^2)
// k_a k_b] per k-vector of the half space, and E_background on the diagonal; the -g/sqrt(pi) term has none.
// g (g_ewald) belongs to the replica and the run, not to the material: it follows from the run's start box, the replica's charges and the
// accuracy (scema_eng::ewald_setup), so every function here takes it beside the table.
#pragma once
#include "bd_core.h"

#define BL_MAXK 4096   /* k-vectors of the half space one replica may hold */
#define BL_MAXKD 20    /* largest |n_d| of a triple (the phase tables of the kernels hold m = 0 .. BL_MAXKD per dimension) */
#define BL_TWO_PI 6.283185307179586476925

typedef struct {
  BdTable bd;              // types, pair constants, cut_coul, K, cutmax of the Born/DSF table; alpha, e_s and f_s are 0 and unused
  double accuracy;         // of the kspace_style line
  int pppm, buck;          // 1: the script said `kspace_style pppm` (honoured as the Ewald sum at that accuracy); 1: buck/coul/long
} BlTable;

// The real-space Coulomb term of a pair at distance r > 0 (kc: K of the table): energy and force factor, exactly 0 at and beyond cut_coul
BD_HD void bl_coul(double kc, double cut_coul, double g, double qi, double qj, double r, double *e_coul, double *fc) {
  *e_coul = *fc = 0.0;
  const double qq = kc * qi * qj;
  if (r < cut_coul && qq != 0.0) {
    const double ir = 1.0 / r, gr = g * r;
    const double erfcc = erfc(gr), erfcd = exp(-gr * gr);
    *e_coul = qq * erfcc * ir;
    *fc = qq * (erfcc * ir + BD_TWO_OVER_SQRTPI * g * erfcd) * ir * ir;
  }
}

// A pair of atoms with charges qi, qj at squared distance r2 > 0: the whole energies of the pair and the force factors fb, fc with
// (force on i) = -(fb + fc) d, d = x_j - x_i, as bd_pair.  Beyond a term's cutoff its two outputs are exactly 0.
BD_HD void bl_pair(const BlTable &T, const BdPairP &P, double g, double qi, double qj, double r2, double *e_born, double *e_coul, double *fb, double *fc) {
  double unused_e, unused_f;
  bd_pair(T.bd, P, 0.0, 0.0, r2, e_born, &unused_e, fb, &unused_f);   // (charges 0: the Born term alone)
  bl_coul(T.bd.k, T.bd.cut_coul, g, qi, qj, sqrt(r2), e_coul, fc);
}

// the self energy of a replica: the point term and the neutralising background (its only strain-dependent part, returned apart)
BD_HD double bl_self(double k, double g, double vol, double qsqsum, double qsum, double *e_background) {
  *e_background = -k * 3.14159265358979323846 * qsum * qsum / (2.0 * g * g * vol);
  return -k * g * BD_ONE_OVER_SQRTPI * qsqsum + *e_background;
}

// the six inverse entries of the box h = lx, ly, lz, yz, xz, xy in the layout of BoxD::hinv (1/lx, 1/ly, 1/lz, the yz-, xz- and xy-term), with
// the expressions of box_derive (md_device.h)
BD_HD void bl_hinv(const double *h, double *i) {
  i[0] = 1.0 / h[0]; i[1] = 1.0 / h[1]; i[2] = 1.0 / h[2];
  i[3] = -h[3] / (h[1] * h[2]); i[4] = (h[3] * h[5] - h[1] * h[4]) / (h[0] * h[1] * h[2]); i[5] = -h[5] / (h[0] * h[1]);
}
// Cartesian k of an integer triple in that box (k = 2 pi n . h^-1), the layout of scema_eng::ewald_setup
BD_HD void bl_kvec(const double *h, int n1, int n2, int n3, double *k) {
  double i[6];
  bl_hinv(h, i);
  k[0] = BL_TWO_PI * (i[0] * n1);
  k[1] = BL_TWO_PI * (i[5] * n1 + i[1] * n2);
  k[2] = BL_TWO_PI * (i[4] * n1 + i[3] * n2 + i[2] * n3);
}

// c_k of a k-vector: (4 pi K/V) exp(-k^2/4g^2)/k^2 (the half-space factor 2 is inside)
BD_HD double bl_coef(double kc, double g, double vol, double k2) { return 4.0 * 3.14159265358979323846 * kc / vol * exp(-k2 / (4.0 * g * g)) / k2; }

// fractional coordinates of a point in that box, without the origin (a common origin is a common phase of S(k) and of every atom)
BD_HD void bl_frac(const double *h, const double *x, double *s) {
  s[2] = x[2] / h[2];
  s[1] = (x[1] - h[3] * s[2]) / h[1];
  s[0] = (x[0] - h[5] * s[1] - h[4] * s[2]) / h[0];
}
