// eam_host_driver.cpp -- TEST HARNESS, not part of the product: runs the functions of scema_amd/csrc/eam/eam_core.h (the arithmetic the
// HIP kernels of md_eam.hip execute) as plain loops on the host, with the tables of the product's reader (host/eam_setfl.cpp), so that
// tests/test_eam_host.py can hold energies, forces and virial against tests/eam_numpy.py and against central differences without a GPU.
// The loop structure follows the two kernels: a density pass over every atom's neighbours, then a force pass.
// Built by the test with g++; nothing in scema_amd/ links it.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../scema_amd/csrc/eam/eam_core.h"
#include "../scema_amd/csrc/host/eam_setfl.h"

namespace {
struct Driver {
  std::vector<double> block;
  std::vector<int> type_map;
  int wrong;   // deliberately wrong builds, for the tests that show what the suite catches: 1 F'_i and F'_j swapped in the pair term,
               // 2 the density taken from the central atom's element, 3 the extrapolation above rhomax left out
};
struct Nb { int j, tj; double d[3], r; };
}  // namespace

extern "C" {

void *eamh_create(const char *path, const char *const *elements, int nel, int energy_unit, int wrong) {
  Driver *d = new Driver();
  std::vector<std::string> el(elements, elements + nel);
  std::string err;
  if (!scema::read_eam_setfl(path, el, energy_unit, d->block, d->type_map, err)) {
    std::fprintf(stderr, "eamh_create: %s\n", err.c_str());
    delete d;
    return nullptr;
  }
  d->wrong = wrong;
  return d;
}
void eamh_destroy(void *h) { delete (Driver *)h; }
double eamh_cutoff(void *h) { return scema::eam_head(((Driver *)h)->block).cutoff; }

// types: LAMMPS type - 1 per atom; box: xlo ylo zlo xhi yhi zhi xy xz yz; out: f [n][3], e [2] (pair, embedding), w [6] (xx yy zz xy xz
// yz), counts [3] (ordered pairs inside the cutoff, atoms above rhomax, most neighbours of one atom), rho [n]
int eamh_compute(void *h, int n, const int *types, const double *x, const double *box, double *f, double *e, double *w, int *counts, double *rho) {
  const Driver &D = *(Driver *)h;
  const EamHead &H = scema::eam_head(D.block);
  const double *blk = D.block.data();
  const double hx = box[3] - box[0], hy = box[4] - box[1], hz = box[5] - box[2], xy = box[6], xz = box[7], yz = box[8];
  // perpendicular widths -> how many images the cutoff reaches (the fold leaves |s| <= 0.5)
  const double c23[3] = {hy * hz, -xy * hz, xy * yz - hy * xz}, c31[3] = {0.0, hz * hx, -yz * hx};   // a2 x a3, a3 x a1 (a1 x a2 is along z)
  const double vol = hx * hy * hz;
  const double wd[3] = {vol / std::sqrt(c23[0] * c23[0] + c23[1] * c23[1] + c23[2] * c23[2]), vol / std::sqrt(c31[1] * c31[1] + c31[2] * c31[2]), hz};
  int m[3];
  for (int d = 0; d < 3; d++) m[d] = (int)std::floor(H.cutoff / wd[d] + 0.5) + 1;
  for (int k = 0; k < 3 * n; k++) f[k] = 0.0;
  e[0] = e[1] = 0.0;
  for (int k = 0; k < 6; k++) w[k] = 0.0;
  counts[0] = counts[1] = counts[2] = 0;
  std::vector<std::vector<Nb>> nb(n);
  std::vector<double> fp(n);
  for (int i = 0; i < n; i++) {
    if (types[i] < 0 || types[i] >= (int)D.type_map.size()) return 1;
    for (int j = 0; j < n; j++) {
      if (types[j] < 0 || types[j] >= (int)D.type_map.size()) return 1;
      double d[3] = {x[3 * j] - x[3 * i], x[3 * j + 1] - x[3 * i + 1], x[3 * j + 2] - x[3 * i + 2]};
      double s2 = d[2] / hz, s1 = (d[1] - yz * s2) / hy, s0 = (d[0] - xy * s1 - xz * s2) / hx;
      s0 -= std::rint(s0); s1 -= std::rint(s1); s2 -= std::rint(s2);
      d[0] = hx * s0 + xy * s1 + xz * s2; d[1] = hy * s1 + yz * s2; d[2] = hz * s2;
      for (int sz = -m[2]; sz <= m[2]; sz++)
        for (int sy = -m[1]; sy <= m[1]; sy++)
          for (int sx = -m[0]; sx <= m[0]; sx++) {
            Nb q;
            q.d[0] = d[0] + sx * hx + sy * xy + sz * xz; q.d[1] = d[1] + sy * hy + sz * yz; q.d[2] = d[2] + sz * hz;
            const double r2 = q.d[0] * q.d[0] + q.d[1] * q.d[1] + q.d[2] * q.d[2];
            if (!(r2 < H.cut2 && r2 > 0.0)) continue;
            q.r = std::sqrt(r2); q.j = j; q.tj = D.type_map[types[j]];
            nb[i].push_back(q);
          }
    }
    counts[0] += (int)nb[i].size();
    counts[2] = std::max(counts[2], (int)nb[i].size());
    // density pass
    const int ti = D.type_map[types[i]];
    double r = 0.0;
    for (const Nb &q : nb[i]) {
      int k;
      double p;
      eam_locate(q.r, H.rdr, H.nr, &k, &p);
      r += eam_value(blk + H.off_rho[ti * EAM_MAXEL + (D.wrong == 2 ? ti : q.tj)], k, p);
    }
    rho[i] = r;
    const double *fv = blk + H.off_f[ti];
    double ee;
    eam_embed(fv, fv + 4 * (size_t)H.nrho, H.nrho, H.rdrho, H.rhomax, r, &ee, &fp[i]);
    if (D.wrong == 3 && r > H.rhomax) ee -= fp[i] * (r - H.rhomax);
    e[1] += ee;
    if (r > H.rhomax) counts[1]++;
  }
  // force pass
  const size_t der = 4 * (size_t)H.nr;
  for (int i = 0; i < n; i++) {
    const int ti = D.type_map[types[i]];
    for (const Nb &q : nb[i]) {
      int k;
      double p;
      eam_locate(q.r, H.rdr, H.nr, &k, &p);
      const double *zt = blk + H.off_z[ti * EAM_MAXEL + q.tj];
      const double z = eam_value(zt, k, p), dz = eam_deriv(zt + der, k, p);
      const double drho_j = eam_deriv(blk + H.off_rho[ti * EAM_MAXEL + (D.wrong == 2 ? ti : q.tj)] + der, k, p);
      const double drho_i = eam_deriv(blk + H.off_rho[q.tj * EAM_MAXEL + (D.wrong == 2 ? q.tj : ti)] + der, k, p);
      double phi, fa, fb;
      if (D.wrong == 1) eam_pair(q.r, z, dz, fp[q.j], drho_j, fp[i], drho_i, &phi, &fa, &fb);
      else eam_pair(q.r, z, dz, fp[i], drho_j, fp[q.j], drho_i, &phi, &fa, &fb);
      const double fpair = fa + fb;
      for (int c = 0; c < 3; c++) f[3 * i + c] -= q.d[c] * fpair;
      e[0] += 0.5 * phi;
      const double hf = 0.5 * fpair;
      w[0] += hf * q.d[0] * q.d[0]; w[1] += hf * q.d[1] * q.d[1]; w[2] += hf * q.d[2] * q.d[2];
      w[3] += hf * q.d[0] * q.d[1]; w[4] += hf * q.d[0] * q.d[2]; w[5] += hf * q.d[1] * q.d[2];
    }
  }
  return 0;
}

}  // extern "C"
