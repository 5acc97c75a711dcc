// md_bonded_groups.h -- the grouped stream of the bonded tiles (md_bonded.hip, engine/engine_topo.cpp): dihedrals gathered per central
// bond, special pairs attached to the bond or angle term that already holds their two atoms.  Plain C++ (no HIP): the grouping is a pure
// function of the term lists, so a host program can include this header alone (tests/bonded_groups_host_driver.cpp).
//
// Why: the nine torsions around one C-C bond of a chain read the same eight positions and add to the same eight force vectors -- 108 LDS
// reads and 108 FP64 LDS atomics where 24 + 24 do; every 1-2 special pair is the atom pair of a bond term and every 1-3 pair the outer
// pair of an angle term, whose thread already holds both positions and issues the atomics for both atoms.
//
// Streams of a tile (both live in the one bt_terms buffer; the tile descriptor says where):
//   per-term stream  desc[2] first chunk, desc[3] chunks: every term on its own (the parity hook, and grouping switched off);
//   grouped stream   desc[BTG_DESC_TERM0] first chunk, desc[BTG_DESC_NTERM] chunks: bonds and angles with the level of their attached
//                    special pair in the BT_D_LVL bits (0 = none), the dihedrals no group holds, impropers, the special pairs without host;
//                    desc[BTG_DESC_GRP0] first 64-word unit, desc[BTG_DESC_NGRP] chunks of the groups: a chunk is 64 first words
//                    followed by 64 second words.
// A group: central atoms (2, 3), up to three "k" atoms bonded on the side of atom 2 and three "m" atoms on the side of atom 3, and a
// type field for each of the nine (k, m) pairs (0 = no such dihedral, else type + 1).
//   word 0: ten bits each for the local indices of atom 2, atom 3, k0, k1, k2, m0; two bits nk; two bits nm
//   word 1: ten bits each for m1, m2; nine four-bit type fields from bit 20, field 3 * k + m; BTG_NOCOUNT; BTG_VALID
#pragma once
#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#define BTG_DESC_TERM0 4
#define BTG_DESC_NTERM 5
#define BTG_DESC_GRP0 6
#define BTG_DESC_NGRP 7
#define BTG_SIDE 3                  /* end atoms per side of a group */
#define BTG_TYPE_BITS 4
#define BTG_TYPE_SHIFT 20
#define BTG_MAXTYPE 15              /* dihedral types 0..14 fit the field; a dihedral of a higher type stays a term of its own */
#define BTG_NOCOUNT (1ull << 56)    /* evaluated for this tile's owner forces only; the virial is counted by the tile that owns the lower-ranked central atom */
#define BTG_VALID (1ull << 57)

namespace bonded_groups {

struct Group {
  int c2 = -1, c3 = -1;             // central atoms
  int nk = 0, nm = 0;
  int k[BTG_SIDE] = {-1, -1, -1}, m[BTG_SIDE] = {-1, -1, -1};
  int type[BTG_SIDE * BTG_SIDE] = {-1, -1, -1, -1, -1, -1, -1, -1, -1};   // [3 * k + m], -1 = absent
};

struct DihedralGroups {
  std::vector<Group> groups;
  std::vector<int> left;            // indices of the listed dihedrals that stay terms of their own
};

// Dihedrals (atoms[4 * i ..], type[i]) by unordered central bond.  A bond whose dihedrals name more than BTG_SIDE distinct end atoms on
// a side, list one (k, m) twice or carry a type the field does not hold keeps ALL its dihedrals as terms, so that the expansion of the
// groups plus the left-over terms is the input multiset.
inline DihedralGroups group_dihedrals(int n, const int *atoms, const int *type) {
  DihedralGroups out;
  std::map<std::pair<int, int>, std::vector<int>> by_bond;
  std::vector<std::pair<int, int>> order;   // central bonds in order of first appearance: the result does not depend on the map's order
  for (int i = 0; i < n; i++) {
    const int a2 = atoms[4 * i + 1], a3 = atoms[4 * i + 2];
    const std::pair<int, int> key(std::min(a2, a3), std::max(a2, a3));
    std::vector<int> &v = by_bond[key];
    if (v.empty()) order.push_back(key);
    v.push_back(i);
  }
  for (const std::pair<int, int> &key : order) {
    const std::vector<int> &members = by_bond[key];
    Group g;
    g.c2 = key.first; g.c3 = key.second;
    bool ok = g.c2 != g.c3;
    for (size_t q = 0; q < members.size() && ok; q++) {
      const int i = members[q];
      // a dihedral listed as l-k-j-i joins with its ends swapped
      const bool rev = atoms[4 * i + 1] != g.c2;
      const int ak = rev ? atoms[4 * i + 3] : atoms[4 * i], am = rev ? atoms[4 * i] : atoms[4 * i + 3];
      if (type[i] < 0 || type[i] >= BTG_MAXTYPE) { ok = false; break; }
      int ik = 0, im = 0;
      while (ik < g.nk && g.k[ik] != ak) ik++;
      while (im < g.nm && g.m[im] != am) im++;
      if (ik == BTG_SIDE || im == BTG_SIDE) { ok = false; break; }
      if (ik == g.nk) g.k[g.nk++] = ak;
      if (im == g.nm) g.m[g.nm++] = am;
      if (g.type[BTG_SIDE * ik + im] >= 0) { ok = false; break; }
      g.type[BTG_SIDE * ik + im] = type[i];
    }
    if (ok) out.groups.push_back(g);
    else out.left.insert(out.left.end(), members.begin(), members.end());
  }
  std::sort(out.left.begin(), out.left.end());
  return out;
}

struct SpecialHosts {
  std::vector<int> bond_pair, angle_pair;   // per bond / per angle: index of the attached special pair, -1 = none
  std::vector<int> pair_host_kind;          // per special pair: 0 = none (stays a term of its own), 1 = a bond, 2 = an angle
  std::vector<int> pair_host;               // ... and the index of that bond / angle
};

// Special pairs (pair[2 * i ..]) onto the terms that hold both their atoms: a bond with these two atoms, else the lowest-indexed angle
// whose outer atoms they are.  A pair is attached at most once and a term hosts at most one pair.
inline SpecialHosts attach_specials(int npair, const int *pair, int nbond, const int *bond, int nangle, const int *angle) {
  SpecialHosts out;
  out.bond_pair.assign(nbond, -1);
  out.angle_pair.assign(nangle, -1);
  out.pair_host_kind.assign(npair, 0);
  out.pair_host.assign(npair, -1);
  std::map<std::pair<int, int>, int> pair_of;
  for (int i = 0; i < npair; i++) pair_of.insert({{std::min(pair[2 * i], pair[2 * i + 1]), std::max(pair[2 * i], pair[2 * i + 1])}, i});
  auto attach = [&](int a, int b, int kind, int idx, std::vector<int> &slot) {
    const auto it = pair_of.find({std::min(a, b), std::max(a, b)});
    if (it == pair_of.end() || out.pair_host_kind[it->second]) return;
    out.pair_host_kind[it->second] = kind;
    out.pair_host[it->second] = idx;
    slot[idx] = it->second;
  };
  for (int b = 0; b < nbond; b++) attach(bond[2 * b], bond[2 * b + 1], 1, b, out.bond_pair);
  for (int a = 0; a < nangle; a++) attach(angle[3 * a], angle[3 * a + 2], 2, a, out.angle_pair);
  return out;
}

// The tiles (owners = consecutive ranks) that evaluate a set of atoms -- every tile that owns one of them -- and the one that counts it:
// the owner of `count_atom`.
inline void tiles_of(const int *atoms, int n, const int *rank, int owners, std::vector<int> &tiles) {
  tiles.clear();
  for (int q = 0; q < n; q++) {
    const int tl = rank[atoms[q]] / owners;
    if (std::find(tiles.begin(), tiles.end(), tl) == tiles.end()) tiles.push_back(tl);
  }
}
inline int group_atoms(const Group &g, int *atoms) {
  int n = 0;
  atoms[n++] = g.c2; atoms[n++] = g.c3;
  for (int q = 0; q < g.nk; q++) atoms[n++] = g.k[q];
  for (int q = 0; q < g.nm; q++) atoms[n++] = g.m[q];
  return n;
}
inline int group_count_tile(const Group &g, const int *rank, int owners) { return std::min(rank[g.c2], rank[g.c3]) / owners; }

// the two words of a group; local[] maps an atom to its local index in the tile
template <class Local>
inline void pack_group(const Group &g, const Local &local, bool counted, unsigned long long w[2]) {
  const int l[8] = {local(g.c2), local(g.c3), g.nk > 0 ? local(g.k[0]) : 0, g.nk > 1 ? local(g.k[1]) : 0, g.nk > 2 ? local(g.k[2]) : 0,
                    g.nm > 0 ? local(g.m[0]) : 0, g.nm > 1 ? local(g.m[1]) : 0, g.nm > 2 ? local(g.m[2]) : 0};
  w[0] = 0ull;
  for (int q = 0; q < 6; q++) w[0] |= (unsigned long long)l[q] << (10 * q);
  w[0] |= (unsigned long long)g.nk << 60 | (unsigned long long)g.nm << 62;
  w[1] = (unsigned long long)l[6] | (unsigned long long)l[7] << 10 | BTG_VALID | (counted ? 0ull : BTG_NOCOUNT);
  for (int q = 0; q < BTG_SIDE * BTG_SIDE; q++)
    if (g.type[q] >= 0) w[1] |= (unsigned long long)(g.type[q] + 1) << (BTG_TYPE_SHIFT + BTG_TYPE_BITS * q);
}

}  // namespace bonded_groups
