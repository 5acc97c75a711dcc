// eam_coul_host_driver.cpp -- TEST HARNESS, not part of the product: a stand-alone program that runs the reader and the block builder of
// the EAM + long-range Coulomb stage (scema_amd/csrc/host/eam_coul_params.cpp on host/eam_setfl.cpp) on one script and holds the block
// against what the kernels of md_eam_coul.hip and the reciprocal kernels of md_born_long.hip assume of it: a BlTable at the start whose
// Born pairs are all zero and whose cut_coul, K, cutmax, accuracy and solver word are set, the EAM block at EC_EAM_OFF, 32-byte aligned,
// every offset of its head inside the block.  Built by the test with g++ (tests/test_eam_coul_corrupt_files.py); nothing in scema_amd/
// links it.
//
//   eam_coul_host_driver <script> <energy unit>
//   prints `ok <types> <cut_coul> <cutmax> <setfl cutoff> <EC_EAM_OFF> <checksum>` (exit status 0), the reader's message on stderr (1),
//   or `layout: <what>` on stderr (3) where the block is not what the kernels assume
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../scema_amd/csrc/eam/ec_core.h"
#include "../scema_amd/csrc/host/eam_coul_params.h"

static int layout(const char *what) {
  std::fprintf(stderr, "layout: %s\n", what);
  return 3;
}

int main(int argc, char **argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: %s <script> <energy unit>\n", argv[0]); return 2; }
  std::vector<double> block;
  std::vector<int> type_map;
  scema::EamCoulParams P;
  std::string err;
  if (!scema::build_eam_coul_block(argv[1], std::atoi(argv[2]), block, type_map, P, err)) { std::fprintf(stderr, "%s\n", err.c_str()); return 1; }
  // the prefix: what k_bl_sfac, k_bl_recip and the mesh kernels read as ((const BlTable *)tab)->bd.k, and what k_ec_force reads
  if (EC_EAM_OFF % 4 != 0 || (size_t)EC_EAM_OFF * sizeof(double) < sizeof(BlTable)) return layout("EC_EAM_OFF");
  if (block.size() <= (size_t)EC_EAM_OFF + EAM_HEAD_DOUBLES) return layout("the block is shorter than its two heads");
  BlTable T;
  std::memcpy(&T, block.data(), sizeof T);
  for (int k = 0; k < BD_MAXEL * BD_MAXEL; k++) {
    const BdPairP &B = T.bd.pair[k];
    if (B.a != 0.0 || B.irho != 0.0 || B.sigma != 0.0 || B.c != 0.0 || B.d != 0.0 || B.cut_lj2 != 0.0) return layout("a Born pair is not zero");
  }
  if (!(T.bd.cut_coul > 0.0) || T.bd.cut_coul != P.cut_coul || !(T.bd.k > 0.0) || T.bd.k != P.k) return layout("cut_coul or K");
  if (!(T.accuracy > 0.0 && T.accuracy < 1.0) || T.accuracy != P.accuracy || T.pppm != P.pppm || (T.pppm != 0 && T.pppm != 1)) return layout("accuracy or solver word");
  if (T.bd.alpha != 0.0 || T.bd.e_s != 0.0 || T.bd.f_s != 0.0 || T.buck != 0) return layout("a field of the other ionic styles is set");
  // the EAM block: the head and every offset the kernels add to tab + EC_EAM_OFF
  EamHead H;
  std::memcpy(&H, block.data() + EC_EAM_OFF, sizeof H);
  if ((size_t)H.ndoubles + EC_EAM_OFF != block.size()) return layout("the EAM block's own size");
  if (T.bd.cutmax != std::fmax(H.cutoff, T.bd.cut_coul) || H.cut2 != H.cutoff * H.cutoff) return layout("cutmax");
  if (H.nelem < 1 || H.nelem > EAM_MAXEL || T.bd.ntypes != H.nelem || H.nr < 5 || H.nrho < 5) return layout("counts");
  for (int v : type_map)
    if (v < 0 || v >= H.nelem) return layout("type map");
  double sum = 0.0;
  auto records = [&](int off, int n) {   // value and derivative records of n knots, 32-byte aligned inside the block
    if (off < EAM_HEAD_DOUBLES || off % 4 != 0 || (long long)off + 8LL * n > H.ndoubles) return false;
    for (int k = 0; k < 8 * n; k++) {
      const double v = block[(size_t)EC_EAM_OFF + off + k];
      if (!std::isfinite(v)) return false;
      sum += v;
    }
    return true;
  };
  for (int i = 0; i < H.nelem; i++) {
    if (!records(H.off_f[i], H.nrho)) return layout("off_f");
    for (int j = 0; j < H.nelem; j++)
      if (!records(H.off_rho[i * EAM_MAXEL + j], H.nr) || !records(H.off_z[i * EAM_MAXEL + j], H.nr)) return layout("off_rho or off_z");
  }
  // the two terms of k_ec_force at and beyond their cutoffs, by the code it runs
  double ec, fc;
  bl_coul(T.bd.k, T.bd.cut_coul, 0.3, 1.0, -1.0, T.bd.cut_coul, &ec, &fc);
  if (ec != 0.0 || fc != 0.0) return layout("the Coulomb term at cut_coul");
  bl_coul(T.bd.k, T.bd.cut_coul, 0.3, 1.0, -1.0, 0.999 * T.bd.cut_coul, &ec, &fc);
  if (!(ec < 0.0) || !std::isfinite(fc)) return layout("the Coulomb term inside cut_coul");
  std::printf("ok %d %.17g %.17g %.17g %d %.17g\n", H.nelem, T.bd.cut_coul, T.bd.cutmax, H.cutoff, EC_EAM_OFF, sum + ec + fc);
  return 0;
}
