// md_skin_bands.h -- how far into the skin part of a neighbour row k_pair has to walk, for device and host code alike (the CPU test of the
// rule compiles this header with g++).
//
// A row is [A | B | band 0 | ... | band K-1]: the skin entries (build-time distance beyond the cutoff + margin) sorted into K bands by the
// build-time distance r0 of the NEAREST of the cluster's four atoms, band b holding r0 >= cutmax + w[b] (w ascending, w[0] = the margin of
// segment B).  A pair of band b is inside the cutoff only once
//     |D_i| + |D_j| + corner motion  >  r0 - cutmax  >=  w[b]
// with D the displacements of its two atoms since the build and the corner term what the images of a deforming box add (the d1 + d2 of
// pre_scalars).  The i side is bounded by the row's own cluster (the largest of its four slots), the j side by the replica's fastest atom.
// Every rounding is towards "open": displacements and the corner term are rounded up, the thresholds w down.
#pragma once

#ifndef MD_SKIN_BANDS
#define MD_SKIN_BANDS 2     /* K: bands of the skin part of a row (2, 4 and 8 compile; 4 did not beat 2 on the headline, 8 was not run: DESIGN.md 5.3) */
#endif
#define MD_BAND_CNT (MD_SKIN_BANDS < 4 ? 4 : (MD_SKIN_BANDS < 8 ? 8 : 16))   /* 16-bit cumulative counts per cluster: K + 1, padded to a power of two */
#define MD_DLEVELS 64       /* the replica's bound is kept as level flags: level l raised <=> some atom has moved more than (l - 1) quanta */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MD_HD __host__ __device__ __forceinline__
#else
#define MD_HD inline
#endif

// a non-negative double as a float that is not below it
MD_HD float skin_up(double v) { return (float)v * 1.000001f; }
// a non-negative double as a float that is not above it
MD_HD float skin_down(double v) { return (float)v * 0.999999f; }

// the level of a displacement d (already an upper bound): the smallest l >= 1 with d <= l * quantum, capped at the last level.  (The cap
// loses nothing: the quantum is skin / MD_DLEVELS and the last band opens below (1 - 0.9 / K) skin, so the last level opens every band.)
MD_HD int skin_level(float d_up, float inv_quantum) {
  const int l = (int)(d_up * 1.00001f * inv_quantum) + 1;
  return l < MD_DLEVELS - 1 ? l : MD_DLEVELS - 1;
}
// ... and the bound a level stands for
MD_HD float skin_level_bound(int level, float quantum) { return (float)level * quantum * 1.000001f; }

// How many bands of a row are open: d_i the bound of the row's cluster, d_g the replica's, corner the box term (all rounded up already),
// w[K] the band thresholds (rounded down already).  The sum of three non-negative floats carries two roundings: 1.000001 covers them.
MD_HD int skin_bands_open(float d_i, float d_g, float corner, const float *w) {
  const float s = ((d_i + d_g) + corner) * 1.000001f;
  int n = 0;
#pragma unroll
  for (int b = 0; b < MD_SKIN_BANDS; b++) n += (s >= w[b]) ? 1 : 0;   // (w ascending: the open bands are the first n)
  return n;
}
