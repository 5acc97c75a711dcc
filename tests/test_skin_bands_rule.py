"""The skin-band rule (scema_amd/csrc/md_skin_bands.h), compiled for the host by tests/skin_bands_host_driver.cpp: whenever a pair that was
listed at a build-time distance r0 in the skin has moved inside the cutoff, the band that holds it is open.  No GPU needed.

The chain under test is the one the kernels run: k_initial_integrate turns an atom's displacement into an FP32 upper bound (as the test
does with sqrtf and the kernel's factor) and raises the replica's level flag of it, k_pair turns the highest level back into a bound and
adds the bound of the row's own cluster and the corner term; the engine's layout rounds the band thresholds down.  The truth is float64
arithmetic on the same numbers, worst case geometry (both atoms and the image shift move straight towards each other).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rule():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libskin_bands_host.so")
    srcs = [os.path.join(ROOT, "tests", "skin_bands_host_driver.cpp")]
    deps = srcs + [os.path.join(ROOT, "scema_amd", "csrc", "md_skin_bands.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so] + srcs)
    L = C.CDLL(so)
    L.sbh_up.restype = C.c_float; L.sbh_up.argtypes = [C.c_double]
    L.sbh_down.restype = C.c_float; L.sbh_down.argtypes = [C.c_double]
    L.sbh_level.restype = C.c_int; L.sbh_level.argtypes = [C.c_float, C.c_float]
    L.sbh_level_bound.restype = C.c_float; L.sbh_level_bound.argtypes = [C.c_int, C.c_float]
    L.sbh_open.restype = C.c_int; L.sbh_open.argtypes = [C.c_float, C.c_float, C.c_float, C.POINTER(C.c_float)]
    return L


class Bands:
    """what lay_out_sim computes for a replica: thresholds w[b] = m + b (skin - m) / K beyond the larger cutoff, quantum skin / levels"""

    def __init__(self, L, cut, skin, pskin=None):
        self.L, self.cut, self.skin = L, cut, skin
        self.K = L.sbh_bands()
        m = 0.1 * (skin if pskin is None else pskin)
        self.w = np.array([m + b * (skin - m) / self.K for b in range(self.K)])
        self.edge = cut + self.w                                  # band b holds r0 >= edge[b] (k_neigh_build compares squares of these)
        self.wf = (C.c_float * self.K)(*[L.sbh_down(float(v)) for v in self.w])
        self.quantum = np.float32(skin / L.sbh_levels())
        self.inv_quantum = np.float32(L.sbh_levels() / skin)

    def band_of(self, r0):
        """the FARTHEST band the build may put an entry of exact distance r0 into (it may always choose a nearer one), -1: segment B"""
        return int(np.searchsorted(self.edge ** 2, r0 * r0, side="right")) - 1

    def dup(self, d):
        """k_initial_integrate: sqrtf((float)dsq) * 1.00001f"""
        return float(np.float32(np.sqrt(np.float32(d * d))) * np.float32(1.00001))

    def open_bands(self, d_i, d_all, corner):
        """d_i: the displacements of the row's four atoms; d_all: those of every atom of the replica since the build"""
        L = self.L
        lev = max(L.sbh_level(self.dup(d), float(self.inv_quantum)) for d in d_all)
        d_g = L.sbh_level_bound(lev, float(self.quantum))
        return L.sbh_open(max(self.dup(d) for d in d_i), d_g, L.sbh_up(corner), self.wf)


def _check(B, r0, di, dj, corner, others=()):
    b = B.band_of(r0)
    if b < 0:
        return 0                                                  # segment B: always walked
    r_now = r0 - di - dj - corner                                 # the nearest the pair can be now
    nopen = B.open_bands([di, 0.3 * di, 0.0, 0.0], [di, dj, *others], corner)
    if r_now < B.cut:
        assert nopen > b, (r0, di, dj, corner, b, nopen)
        return 1
    return 0


@pytest.mark.parametrize("cut,skin,pskin", [(12.0, 2.0, None), (5.0, 1.0, None), (4.5, 0.3, None), (12.0, 2.5, 2.0), (9.0, 1e-3, None)])
def test_a_pair_inside_the_cutoff_is_in_an_open_band(rule, cut, skin, pskin):
    B = Bands(rule, cut, skin, pskin)
    rng = np.random.default_rng(11)
    inside = 0
    for _ in range(20000):
        r0 = cut + skin * rng.random()
        di, dj = skin * 0.6 * rng.random(2) ** 2
        corner = 0.0 if rng.random() < 0.5 else 0.4 * skin * rng.random() ** 3
        inside += _check(B, r0, di, dj, corner, others=(0.5 * dj,))
    assert inside > 2000                                          # the draw does exercise the rule
    # nothing moved: nothing open, whatever the thresholds' rounding
    assert rule.sbh_open(0.0, 0.0, 0.0, B.wf) == 0


@pytest.mark.parametrize("cut,skin", [(12.0, 2.0), (5.0, 1.0), (4.5, 0.3)])
def test_band_edges_and_thresholds_hit_to_the_last_bit(rule, cut, skin):
    """r0 on a band edge and one ulp to either side; a total motion that equals the band's threshold and one ulp to either side (where
    the pair is at the cutoff exactly, or a last bit inside it)."""
    B = Bands(rule, cut, skin)
    rng = np.random.default_rng(5)
    inside = 0
    for b in range(B.K):
        for r0 in (B.edge[b], np.nextafter(B.edge[b], 0.0), np.nextafter(B.edge[b], 100.0)):
            gap = r0 - cut
            for tot in (gap, np.nextafter(gap, 0.0), np.nextafter(gap, 100.0), gap * (1 + 1e-7), gap * (1 + 1e-6)):
                for _ in range(40):
                    f = rng.random(3)
                    f /= f.sum()
                    split = f * tot if rng.random() < 0.7 else np.array([tot * f[0], tot * (1 - f[0]), 0.0])
                    inside += _check(B, r0, split[0], split[1], split[2])
    assert inside > 100


def test_levels_bound_the_displacement_they_stand_for(rule):
    """an atom's level, turned back into a bound, is never below the displacement; the last level stands for "every band open" """
    rng = np.random.default_rng(2)
    for skin in (2.0, 1.0, 0.3, 2.75):
        B = Bands(rule, 12.0, skin)
        for d in np.concatenate([skin * rng.random(5000), skin * np.arange(0, 80) / 64.0, [0.0, 5 * skin]]):
            lev = rule.sbh_level(B.dup(d), float(B.inv_quantum))
            assert 1 <= lev < rule.sbh_levels()
            bound = rule.sbh_level_bound(lev, float(B.quantum))
            if lev < rule.sbh_levels() - 1:
                assert bound >= d, (skin, d, lev, bound)
            else:
                assert rule.sbh_open(0.0, bound, 0.0, B.wf) == B.K
