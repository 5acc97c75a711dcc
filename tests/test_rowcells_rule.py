"""The grid rule of the cell-binned row build (scema_amd/csrc/md_rowcells.h), compiled for the host by tests/rowcells_host_driver.cpp,
against a restatement in Python: the grid of a replica, its eligibility, the clamp of an atom's cell, and completeness -- every pair the
N^2 build accepts (restated in numpy with the rint sequence of k_row_build) lies in cells that are periodic neighbours.  No GPU needed.
"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF, FORCE, AUTO = 0, 1, 2


@pytest.fixture(scope="module")
def rule():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "librowcells_host.so")
    srcs = [os.path.join(ROOT, "tests", "rowcells_host_driver.cpp")]
    deps = srcs + [os.path.join(ROOT, "scema_amd", "csrc", "md_rowcells.h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-std=c++17", "-o", so] + srcs)
    L = C.CDLL(so)
    L.rch_grid.argtypes = [C.c_void_p, C.c_double, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.rch_of.argtypes = [C.c_double, C.c_int]
    L.rch_cells.argtypes = [C.c_int] + [C.c_void_p] * 6
    return L


def grid_c(L, w, rlist, mimg=(0, 0, 0), cap=64, n=1000, npad=None, mode=FORCE):
    w = np.ascontiguousarray(w, np.float64)
    mi = np.ascontiguousarray(mimg, np.int32)
    nc = np.full(3, -7, np.int32)
    ok = L.rch_grid(w.ctypes.data, rlist, mi.ctypes.data, cap, n, (n + 63) // 64 * 64 if npad is None else npad, mode, nc.ctypes.data)
    return ok, [int(v) for v in nc]


def grid_py(L, w, rlist, mimg=(0, 0, 0), cap=64, n=1000, npad=None, mode=FORCE):
    """the rule as the issue states it"""
    npad = (n + 63) // 64 * 64 if npad is None else npad
    if mode == OFF or any(mimg) or cap > L.rch_maxcap() or (mode == AUTO and n < L.rch_min_atoms()):
        return 0, [0, 0, 0]
    nc = [int(math.floor(w[d] / rlist)) for d in range(3)]
    if min(nc) < 3:
        return 0, [0, 0, 0]
    most = L.rch_cells_per_pad() * npad
    while nc[0] * nc[1] * nc[2] > most:
        d = max(range(3), key=lambda k: (nc[k], -k))   # the dimension with the most cells, the first of equals
        if nc[d] <= 3:
            return 0, [0, 0, 0]
        nc[d] -= 1
    return 1, nc


def test_grid_just_below_and_above_three_and_four_list_radii(rule):
    rl = 6.5
    for k in (3, 4):
        for d in range(3):
            for eps, hit in ((-1e-9, 0), (+1e-9, 1)):
                w = [5.5 * rl] * 3
                w[d] = k * rl * (1.0 + eps)
                ok, nc = grid_c(rule, w, rl)
                assert (ok, nc) == grid_py(rule, w, rl)
                want = k if hit else k - 1
                if want < 3:
                    assert ok == 0 and nc == [0, 0, 0]
                else:
                    assert ok == 1 and nc[d] == want and all(nc[e] == 5 for e in range(3) if e != d)
    assert grid_c(rule, [3 * rl] * 3, rl) == (1, [3, 3, 3])       # exactly three radii wide: three cells


def test_grid_eligibility(rule):
    rl, w = 4.0, [20.0, 24.5, 28.1]
    assert grid_c(rule, w, rl) == (1, [5, 6, 7])
    for mimg in ((1, 0, 0), (0, 1, 0), (0, 0, 2), (1, 1, 1)):
        assert grid_c(rule, w, rl, mimg=mimg) == (0, [0, 0, 0])                    # not minimum image
    assert grid_c(rule, w, rl, mode=OFF) == (0, [0, 0, 0])
    assert grid_c(rule, w, rl, cap=rule.rch_maxcap()) [0] == 1
    assert grid_c(rule, w, rl, cap=rule.rch_maxcap() + 8) == (0, [0, 0, 0])       # a row the build kernel cannot stage
    nmin = rule.rch_min_atoms()
    assert grid_c(rule, w, rl, n=nmin - 1, mode=AUTO) == (0, [0, 0, 0])           # below the threshold
    assert grid_c(rule, w, rl, n=nmin, mode=AUTO) == (1, [5, 6, 7])
    assert grid_c(rule, w, rl, n=nmin - 1, mode=FORCE)[0] == 1
    assert grid_c(rule, [20.0, 11.9, 28.1], rl) == (0, [0, 0, 0])                  # two wide dimensions, one narrow
    assert grid_c(rule, [float("nan"), 20.0, 20.0], rl) == (0, [0, 0, 0])
    assert grid_c(rule, w, 0.0) == (0, [0, 0, 0])


def test_cell_cap_and_coarsening(rule):
    per = rule.rch_cells_per_pad()
    # a gas of 300 atoms (npad 320) in a box 40 radii wide: 64 000 cells asked for, at most per * 320 given, no dimension below 3
    ok, nc = grid_c(rule, [40.0, 40.0, 40.0], 1.0, n=300)
    assert ok == 1 and nc[0] * nc[1] * nc[2] <= per * 320 and min(nc) >= 3 and max(nc) - min(nc) <= 1
    assert (ok, nc) == grid_py(rule, [40.0, 40.0, 40.0], 1.0, n=300)
    assert (nc[0] + 1) * nc[1] * nc[2] > per * 320               # (the dimension that gave up a cell last could not have kept it)
    rng = np.random.default_rng(11)
    for _ in range(300):
        w = rng.uniform(2.5, 60.0, 3)
        n = int(rng.integers(1, 4000))
        got, want = grid_c(rule, w, 1.0, n=n), grid_py(rule, w, 1.0, n=n)
        assert got == want
        if got[0]:
            assert all(3 <= got[1][d] <= math.floor(w[d]) for d in range(3))
            assert got[1][0] * got[1][1] * got[1][2] <= per * ((n + 63) // 64 * 64)
    assert grid_c(rule, [3.5, 3.5, 3.5], 1.0, n=1) == (1, [3, 3, 3])               # 27 cells fit the smallest replica


def test_cell_of_a_fraction_is_clamped(rule):
    for nc in (3, 4, 5, 7, 64):
        assert rule.rch_of(0.0, nc) == 0
        assert rule.rch_of(-0.0, nc) == 0
        assert rule.rch_of(-1e-17, nc) == 0
        assert rule.rch_of(1.0 - 2.0 ** -53, nc) == nc - 1
        assert rule.rch_of(1.0, nc) == nc - 1                     # a fraction that has rounded to 1.0
        assert rule.rch_of(float(np.nextafter(1.0, 2.0)), nc) == nc - 1
        assert rule.rch_of(float("nan"), nc) == 0
        for c in range(nc):
            assert rule.rch_of((c + 0.5) / nc, nc) == c
    # a wrapped coordinate whose fraction rounds to 1.0: x one ulp below hi = 5 in a box from -5, where x - lo rounds to the box length
    h = np.array([10.0, 10.0, 10.0, 0.0, 0.0, 0.0]); lo = np.array([-5.0, -5.0, -5.0])
    below = float(np.nextafter(5.0, 0.0))
    assert below < 5.0 and (below - lo[0]) / h[0] == 1.0
    x = np.array([[below] * 3, [-5.0] * 3])
    nc = np.array([3, 4, 5], np.int32)
    cell = np.zeros(2, np.int32); c3 = np.zeros((2, 3), np.int32)
    rule.rch_cells(2, x.ctypes.data, h.ctypes.data, lo.ctypes.data, nc.ctypes.data, cell.ctypes.data, c3.ctypes.data)
    assert c3.tolist() == [[2, 3, 4], [0, 0, 0]] and cell.tolist() == [2 + 3 * (3 + 4 * 4), 0]


def n2_accepts(x, h, rlist):
    """the minimum-image branch of k_row_build: d = x_j - x_i, rint reductions in z, y, x order, !(r2 > rl2)"""
    d = x[None, :, :] - x[:, None, :]
    dx, dy, dz = d[..., 0].copy(), d[..., 1].copy(), d[..., 2].copy()
    ih0, ih1, ih2 = 1.0 / h[0], 1.0 / h[1], 1.0 / h[2]
    n2 = np.rint(dz * ih2); dz -= n2 * h[2]; dy -= n2 * h[3]; dx -= n2 * h[4]
    n1 = np.rint(dy * ih1); dy -= n1 * h[1]; dx -= n1 * h[5]
    n0 = np.rint(dx * ih0); dx -= n0 * h[0]
    r2 = dx * dx + dy * dy + dz * dz
    ok = ~(r2 > rlist * rlist)
    np.fill_diagonal(ok, False)
    return ok


def perp_widths(h):
    hinv = [1.0 / h[0], 1.0 / h[1], 1.0 / h[2], -h[3] / (h[1] * h[2]), (h[3] * h[5] - h[1] * h[4]) / (h[0] * h[1] * h[2]), -h[5] / (h[0] * h[1])]
    return [1.0 / math.sqrt(hinv[0] ** 2 + hinv[5] ** 2 + hinv[4] ** 2), 1.0 / math.sqrt(hinv[1] ** 2 + hinv[3] ** 2), 1.0 / abs(hinv[2])]


def test_every_accepted_pair_lies_in_neighbouring_cells(rule):
    """200 seeded random boxes, tilts up to +-0.45 of the lengths, 3 to 6 cells per dimension, 300 random atoms each"""
    rng = np.random.default_rng(20261)
    rl, nbox, natoms = 3.0, 200, 300
    skipped = pairs = 0
    seen = set()
    for _ in range(nbox):
        L3 = rng.uniform(3.9, 7.0, 3) * rl
        h = np.array([L3[0], L3[1], L3[2], rng.uniform(-0.45, 0.45) * L3[1], rng.uniform(-0.45, 0.45) * L3[0], rng.uniform(-0.45, 0.45) * L3[0]])
        lo = rng.uniform(-20.0, 20.0, 3)
        w = perp_widths(h)
        ok_py, nc_py = grid_py(rule, w, rl, n=natoms)
        ok, nc = grid_c(rule, w, rl, n=natoms)
        assert (ok, nc) == (ok_py, nc_py)
        if not ok:
            skipped += 1
            continue
        assert all(3 <= c <= 6 for c in nc)
        seen.update(nc)
        fr = rng.uniform(0.0, 1.0, (natoms, 3))
        x = np.empty((natoms, 3))
        x[:, 0] = lo[0] + fr[:, 0] * h[0] + fr[:, 1] * h[5] + fr[:, 2] * h[4]
        x[:, 1] = lo[1] + fr[:, 1] * h[1] + fr[:, 2] * h[3]
        x[:, 2] = lo[2] + fr[:, 2] * h[2]
        nca = np.array(nc, np.int32)
        cell = np.zeros(natoms, np.int32); c3 = np.zeros((natoms, 3), np.int32)
        rule.rch_cells(natoms, x.ctypes.data, h.ctypes.data, lo.ctypes.data, nca.ctypes.data, cell.ctypes.data, c3.ctypes.data)
        assert (c3 >= 0).all() and (c3 < nca).all()
        assert (cell == c3[:, 0] + nc[0] * (c3[:, 1] + nc[1] * c3[:, 2])).all()
        acc = n2_accepts(x, h, rl)
        ii, jj = np.nonzero(acc)
        pairs += ii.size
        for d in range(3):
            step = (c3[jj, d] - c3[ii, d]) % nc[d]
            assert np.isin(step, (0, 1, nc[d] - 1)).all(), (h, nc, d)
    assert skipped * 10 <= nbox, skipped          # (the restatement alone decides this: grid_py)
    assert seen == {3, 4, 5, 6} and pairs > 100 * nbox
