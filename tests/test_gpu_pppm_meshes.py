"""The PPPM chain of md_pppm.hip (k_pppm_spread, k_pppm_gf, k_pppm_solve / hipFFT + k_pppm_poisson, k_pppm_force) against the CPU oracle
on the meshes of tests/test_oracle_pppm_meshes.py: odd-only meshes, meshes with fewer than 5 and fewer than 4 points in a dimension,
anisotropic ones with the long axis in x, y and z, meshes just under the in-LDS solve's limit, the hipFFT path behind them -- and on
those meshes the branches that depend on where atoms sit, how many there are and in which order, and launches whose replicas have
different meshes.  Every test asserts the mesh of its system (product's rule and oracle's) before it compares anything.  Tolerances: the
project's own, 1e-10 of the largest component for static results (1e-9 for the 18x27x27 mesh), 1e-7 for evaluated stresses, 1e-9 between
two launch shapes of the engine; the oracle's own reordering noise is 2e-15 (test_oracle_pppm_meshes.py)."""
import functools
import json
import os
import subprocess
import sys
from copy import deepcopy

import numpy as np
import pytest

from test_oracle_pppm_meshes import (BY_NAME, KW, LDS_ROWS, PP_SOLVE_MAX, ROWS, STATIC_ROWS, ionic, oracle_compute, permuted_atoms, product_setup,
                                     rel, relabel_sym6, row_fixture, shifted_by_lattice_vectors, _cell, to_lamda, from_lamda, min_distance, on_faces)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLACEMENT_MESHES = ("4x5x8", "5x5x8", "12x10x24")    # tilted without padded row; padded row, odd nx; just under PP_SOLVE_MAX


def engine(acc, **kw):
    from scema_amd import capi
    return capi.Engine(capi.default_params(kspace_accuracy=acc, **dict(KW, **kw)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(system, forces, energies, virials, g_ewald) of a table row by the oracle, computed once per session and never changed"""
    row = BY_NAME[name]
    d = row_fixture(row, eps=1e-9)
    f, e, w, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid, (name, o.pppm_grid)
    for a in (f, e, w):
        a.setflags(write=False)
    return d, f, e, w, o.g_ewald


def assert_mesh(d, acc, grid):
    """the mesh the product's rule gives this system; returns its g_ewald"""
    g, got = product_setup(d, acc)
    assert got == tuple(grid), (got, grid)
    return g


def assert_static(got, exp, tol, label=""):
    """forces, e[1], e[6], w[6] of debug_compute against the oracle's, each within tol of its largest component"""
    (f, e, w), (fo, eo, wo) = got, exp
    figures = dict(f=rel(f, fo), e6=abs(e[6] - eo[6]) / abs(eo[6]), w6=rel(w[6], wo[6]), e1=abs(e[1] - eo[1]) / max(1e-300, abs(eo[1])))
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert np.isfinite(f).all()
    for k, v in figures.items():
        assert v < tol, (label, k, v, figures)


def static_run(eng, name, d, acc, grid, tol, g_oracle=None, exp=None, label=None):
    if exp is None:
        fo, eo, wo, o = oracle_compute(d, acc)
        assert o.pppm_grid == tuple(grid), (o.pppm_grid, grid)
        exp, g_oracle = (fo, eo, wo), o.g_ewald
    assert abs(assert_mesh(d, acc, grid) - g_oracle) < 1e-12
    eng.register_replica(name, 1, d)
    f, e, w, info = eng.debug_compute(name, 1, use_shake=False)
    assert info["nk"] == 0 and abs(info["g_ewald"] - g_oracle) < 1e-12
    assert_static((f, e, w), exp, tol, label or name)
    return f, e, w


# ---- 1. static parity per mesh --------------------------------------------------------------------------------------------------
_STATIC = [(r.name, False) for r in STATIC_ROWS] + [(r.name, True) for r in STATIC_ROWS if np.prod(r.grid) <= PP_SOLVE_MAX]


@pytest.mark.parametrize("name,library", _STATIC, ids=[n + ("-hipfft" if lib else "") for n, lib in _STATIC])
def test_static_parity_on_every_mesh(name, library, monkeypatch):
    """one replica per mesh of the table through the kernel shapes its row names; meshes of the in-LDS solve also through hipFFT"""
    row = BY_NAME[name]
    if library:
        monkeypatch.setenv("SCEMA_MD_PPPM_FFT", "1")
    d, fo, eo, wo, g = reference(name)
    eng = engine(row.acc)
    static_run(eng, "m", d, row.acc, row.grid, row.tol, g, (fo, eo, wo), label=name + (" hipFFT" if library else ""))
    eng.close()


# ---- 2. the other in-LDS shapes on every small mesh -------------------------------------------------------------------------------
_CHILD_ROWS = ("import json, os, sys, numpy as np\n"
               "sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))\n"
               "from scema_amd import capi\n"
               "from test_oracle_pppm_meshes import KW, LDS_ROWS, row_fixture\n"
               "out = {}\n"
               "for row in LDS_ROWS:\n"
               "    e = capi.Engine(capi.default_params(kspace_accuracy=row.acc, **KW))\n"
               "    e.register_replica('m', 1, row_fixture(row, eps=1e-9))\n"
               "    f, en, w, info = e.debug_compute('m', 1, use_shake=False)\n"
               "    out[row.name] = dict(f=np.asarray(f).ravel().tolist(), e=np.asarray(en).tolist(), w=np.asarray(w).ravel().tolist(), nk=info['nk'], g=info['g_ewald'])\n"
               "    e.close()\n"
               "print(json.dumps(out))\n")


def _child(code, env, timeout=300):
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-2500:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("switch", ["SCEMA_MD_PPPM_SOLVE_WIDE", "SCEMA_MD_PPPM_SOLVE_TWO", "SCEMA_MD_PPPM_PADX"])
def test_the_other_in_lds_shapes_on_every_small_mesh(switch):
    """The switches are read once per process: one child per setting evaluates every mesh of the in-LDS solve.  SOLVE_WIDE=0: 512 threads with
    rho(k) in memory (a single replica never takes it by default); SOLVE_TWO=0: one workgroup per replica instead of two with a ticket;
    PADX=0: the LDS copy of the spreading kernel without pad columns on the meshes that have them by default."""
    # (an engine per accuracy: the engine of a row is closed before the next opens)
    got = _child(_CHILD_ROWS, {switch: "0"})
    assert set(got) == {r.name for r in LDS_ROWS}
    for row in LDS_ROWS:
        d, fo, eo, wo, g = reference(row.name)
        assert_mesh(d, row.acc, row.grid)
        r = got[row.name]
        assert r["nk"] == 0 and abs(r["g"] - g) < 1e-12
        assert_static((np.array(r["f"]).reshape(-1, 3), np.array(r["e"]), np.array(r["w"]).reshape(-1, 6)), (fo, eo, wo), row.tol, f"{switch}=0 {row.name}")


# ---- 3. placement and count edges -------------------------------------------------------------------------------------------------
def on_planes(d, grid, half):
    """every atom moved to the nearest grid plane in each lamda coordinate (half: half-way between two planes, the tie of floor(u + 1/2))"""
    u = to_lamda(d) * np.array(grid, float)
    u = np.floor(u) + 0.5 if half else np.round(u)
    return from_lamda(d, u / np.array(grid, float))


def some_uncharged(d, every=4):
    """every fourth atom uncharged, further ones of the surplus sign until the system is neutral, the rest scaled so that sum q^2 -- and
    with it the mesh -- stays what it was; no LJ, so that an uncharged atom feels nothing at all"""
    out = deepcopy(d)
    q = np.asarray(d["charge"], float).copy()
    q2 = (q ** 2).sum()
    q[::every] = 0.0
    while abs(q.sum()) > 1e-12:
        surplus = np.nonzero(np.sign(q) == np.sign(q.sum()))[0]
        q[surplus[-1]] = 0.0
    q *= np.sqrt(q2 / (q ** 2).sum())
    out["charge"] = q
    out["eps"] = np.zeros((1, 1))
    return out


def merged_pairs(d, grid, seed=2):
    """atoms 2m and 2m + 1 share their nearest grid point and carry opposite charges (the spreading kernel adds both with one atomic per
    point, and the sums cancel in part); the pairs sit at the nearest grid points of every other lattice site"""
    rng = np.random.default_rng(seed)
    n = d["natoms"] - d["natoms"] % 2
    g = np.array(grid, float)
    centre = np.round(to_lamda(d)[0:n:2] * g)
    delta = rng.uniform(0.15, 0.3, centre.shape) * rng.choice([-1.0, 1.0], centre.shape)
    lam = np.empty((n, 3))
    lam[0::2] = (centre + delta) / g
    lam[1::2] = (centre - delta) / g
    out = from_lamda(d, np.vstack([lam, to_lamda(d)[n:]]))
    q = np.abs(np.asarray(d["charge"], float)).max()
    out["charge"] = np.concatenate([np.tile([q, -q], n // 2), np.zeros(d["natoms"] - n)])
    assert abs((out["charge"] ** 2).sum() - (np.asarray(d["charge"]) ** 2).sum()) < 1e-12
    u = to_lamda(out)[:n] * g
    assert np.array_equal(np.floor(u[0::2] + 0.5), np.floor(u[1::2] + 0.5))
    return out


def placement_case(name, case):
    row = BY_NAME[name]
    d = row_fixture(row, eps=1e-9)
    if case == "on_planes":
        out = on_planes(d, row.grid, half=False)
        u = to_lamda(out) * np.array(row.grid, float)
        assert np.abs(u - np.round(u)).max() < 1e-12
    elif case == "half_way":
        out = on_planes(d, row.grid, half=True)
        u = to_lamda(out) * np.array(row.grid, float)
        assert np.abs(u - np.floor(u) - 0.5).max() < 1e-12
    elif case == "faces":
        out = on_faces(d, row.cells)
    elif case == "lattice_shifts":
        out = shifted_by_lattice_vectors(d, seed=9, choices=(-1, 1, 2))
        lam = to_lamda(out)
        assert lam.min() < -0.5 and lam.max() > 2.0
    elif case == "some_uncharged":
        out = some_uncharged(d)
    elif case == "merged_pairs":
        out = merged_pairs(d, row.grid)
    elif case == "merged_pairs_scrambled":
        out, _ = permuted_atoms(merged_pairs(d, row.grid), seed=4)
    else:
        raise KeyError(case)
    assert min_distance(out) > 0.3, min_distance(out)
    return row, out


CASES = ("on_planes", "half_way", "faces", "lattice_shifts", "some_uncharged", "merged_pairs", "merged_pairs_scrambled")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("name", PLACEMENT_MESHES)
def test_atom_placement_edges(name, case):
    """Positions of a table system overwritten (charges neutral, sum q^2 and hence the mesh unchanged): atoms exactly on grid planes in all
    three lamda coordinates and exactly half-way between them; on the low faces of the box and at lo - 1e-17 L, hi - 1e-17 L, where the lamda
    coordinate rounds to 1.0 and the nearest plane is i == n; a third of the atoms 1 or 2 lattice vectors outside the box; every fourth atom
    uncharged (the single replica's chain runs on the side stream and STORES its forces: an uncharged atom must come out with exactly 0, here
    with the LJ part off too); consecutive atoms of opposite charge around one grid point -- the merged two-atoms-per-lane add -- and the same
    atoms in scrambled order through the unmerged one."""
    row, d = placement_case(name, case)
    eng = engine(row.acc)
    f, e, w = static_run(eng, "p", d, row.acc, row.grid, 1e-10, label=f"{name} {case}")
    if case == "faces":
        # and against itself 1e-9 of a box length inside the box, whatever the oracle says (the cell binning of the neighbour list gave an
        # atom at lamda = -1e-17 the cell of one periodic image and the position of another; the bound is that of the oracle's own
        # continuity test in test_oracle_pppm_meshes.py)
        inside = from_lamda(d, np.clip(to_lamda(d), 1e-9, 1.0 - 1e-9))
        eng.register_replica("inside", 1, inside)
        fi, ei, wi, _ = eng.debug_compute("inside", 1, use_shake=False)
        print(f"{name} faces against 1e-9 inside: f {rel(f, fi):.2e}  e1 {abs(e[1] - ei[1]) / abs(ei[1]):.2e}")
        assert rel(f, fi) < 1e-6 and abs(e[1] - ei[1]) < 1e-6 * abs(ei[1]) and abs(e[6] - ei[6]) < 1e-6 * abs(ei[6])
    if case == "some_uncharged":
        zero = np.asarray(d["charge"]) == 0.0
        assert zero.sum() >= d["natoms"] // 4 and np.all(f[zero] == 0.0), np.abs(f[zero]).max()
    eng.close()


# atom counts: alternating charges in file order on the sites of a 5 x 5 x 6 lattice, cut after n atoms (odd n: the last atom uncharged; a
# lone atom keeps its charge, with the neutralising background of both implementations).  The spreading kernel gives lane l the atoms
# l rows .. (l + 1) rows - 1 with rows = ceil(n / 64), two per turn: rows 1 (no B atom at all), 2 and 3 (a turn with an A atom only), last
# lanes empty or half filled.  The charges and accuracies are chosen so that every count has the same mesh.
COUNT_BOXES = {"8x8x8": dict(tilt=(0, 0, 0), q=0.1, acc=1e-2, grid=(8, 8, 8)),
               "6x6x8-tilted": dict(tilt=(1.1, -0.8, 0.9), q=0.05, acc=0.03, grid=(6, 6, 8))}
COUNTS = (1, 2, 63, 65, 127, 129)


def cut_to(d, n, q):
    out = deepcopy(d)
    out["natoms"] = n
    for k in ("type", "x", "v"):
        out[k] = np.asarray(d[k])[:n].copy()
    out["charge"] = q * (1.0 - 2.0 * (np.arange(n) % 2))
    if n % 2 and n > 1:
        out["charge"][-1] = 0.0
    return out


@pytest.mark.parametrize("box", list(COUNT_BOXES))
def test_atom_counts_around_the_lane_layout_of_the_spreading_kernel(box):
    c = COUNT_BOXES[box]
    full = ionic((5, 5, 6), 3.0, c["q"], c["tilt"], seed=3, eps=1e-9)
    eng = engine(c["acc"])
    pair_scale = None
    for n in sorted(COUNTS, reverse=True):
        d = cut_to(full, n, c["q"])
        fo, eo, wo, o = oracle_compute(d, c["acc"])
        assert o.pppm_grid == c["grid"], (n, o.pppm_grid)
        if n == 2:
            pair_scale = np.abs(fo).max()
        if n > 1:
            static_run(eng, f"n{n}", d, c["acc"], c["grid"], 1e-10, o.g_ewald, (fo, eo, wo), label=f"{box} n={n}")
            continue
        # A lone charge feels its own images only: by symmetry the sum cancels to rounding in oracle and kernel alike (1e-16 of a
        # term), so there is no largest component to measure against; the yardstick for its force is the force on the same charge in
        # the two-atom system of the same box.  (No real-space energy either: e[1] is not compared.)
        assert abs(assert_mesh(d, c["acc"], c["grid"]) - o.g_ewald) < 1e-12
        eng.register_replica("n1", 1, d)
        f, e, w, info = eng.debug_compute("n1", 1, use_shake=False)
        print(f"{box} n=1: |f| {np.abs(f).max():.2e} (oracle {np.abs(fo).max():.2e}, pair scale {pair_scale:.2e})  e6 {abs(e[6] - eo[6]) / abs(eo[6]):.2e}  w6 {rel(w[6], wo[6]):.2e}")
        assert info["nk"] == 0 and abs(info["g_ewald"] - o.g_ewald) < 1e-12
        assert np.abs(f - fo).max() < 1e-10 * pair_scale
        assert abs(e[6] - eo[6]) < 1e-10 * abs(eo[6]) and rel(w[6], wo[6]) < 1e-10
    eng.close()


def test_two_atom_ranges_meet_the_padded_fold():
    """600 atoms on a 12 x 15 x 15 mesh, alone in their launch: two workgroups per replica in k_pppm_spread and k_pppm_force (split = 2), each
    folds its padded LDS copy and adds it to the charge grid with atomics"""
    row = BY_NAME["batch600"]
    d, fo, eo, wo, g = reference("batch600")
    assert d["natoms"] == 600 and d["natoms"] // 256 == 2 and row.spread == "padded"
    eng = engine(row.acc)
    static_run(eng, "m", d, row.acc, row.grid, 1e-10, g, (fo, eo, wo), label="batch600 static")
    eng.close()


# ---- 4. axis relabelling ----------------------------------------------------------------------------------------------------------
def test_the_kernels_treat_the_axes_alike():
    """x is the fast, padded, stride-1 axis of every PPPM kernel: one set of atoms with its long axis along x, y and z (10x4x4, 4x10x4,
    4x4x10; test_oracle_pppm_meshes.py pins the property for the oracle) -- forces and virial permute, energies agree"""
    first = BY_NAME["10x4x4"]
    res = {}
    for name in ("10x4x4", "4x10x4", "4x4x10"):
        row = BY_NAME[name]
        d = reference(name)[0]
        assert_mesh(d, row.acc, row.grid)
        eng = engine(row.acc)
        eng.register_replica("m", 1, d)
        res[name] = eng.debug_compute("m", 1, use_shake=False)[:3]
        eng.close()
    f0, e0, w0 = res[first.name]
    for name in ("4x10x4", "4x4x10"):
        perm = list(BY_NAME[name].relabel)
        f, e, w = res[name]
        figures = (rel(f, f0[:, perm]), rel(w[6], relabel_sym6(w0[6], perm)), rel(w[1], relabel_sym6(w0[1], perm)),
                   abs(e[1] - e0[1]) / abs(e0[1]), abs(e[6] - e0[6]) / abs(e0[6]))
        print(name, " ".join(f"{v:.2e}" for v in figures))
        assert max(figures) < 1e-10, (name, figures)


# ---- 5. mixed meshes inside one in-LDS launch -------------------------------------------------------------------------------------
BATCH_ACC, BATCH_T = 0.03, 50.0
BATCH_MATS = ("batch4", "batch5", "batch600")


def batch_strain(d, q, sign=1.0):
    L = d["box"][3:6] - d["box"][:3]
    return sign * np.array([-3e-4 * L[0], -2e-4 * L[1], -1e-3 * L[2], 2e-5 * L[2], -1e-5 * L[2], 1e-5 * L[1]]) * (1.0 + 0.03 * q)


@functools.lru_cache(maxsize=None)
def batch_material(name):
    row = BY_NAME[name]
    d = row_fixture(row, eps=0.1)
    assert_mesh(d, BATCH_ACC, row.grid)
    return d


@functools.lru_cache(maxsize=None)
def batch_reference(name, q, updates):
    """stresses of request q on material `name` by the oracle: one evaluation per update, the second continuing the first with the strain reversed"""
    from oracle import pyoracle as po
    d = batch_material(name)
    o = po.Oracle(d, po.default_params(kspace_accuracy=BATCH_ACC, kspace_pppm=1, neigh_delay=0, **KW))
    out = []
    for u in range(updates):
        s, _ = o.eval(batch_strain(d, q, 1.0 if u == 0 else -1.0), 2.0, BATCH_T, 1e-4, 10)
        out.append(s)
        # (the mesh follows the box from run to run: the straining run of the first update has the mesh the table names, the strained boxes of
        # the later runs may get another one, by the same rule in oracle and product -- 4 x 4 x 3 and 5 x 5 x 4 for the two small materials)
        assert 0 < np.prod(o.pppm_grid) <= PP_SOLVE_MAX and (o.pppm_grid[0] >= 5) == (BY_NAME[name].grid[0] >= 5), (name, q, u, o.pppm_grid)
    return np.array(out)


def run_batch(mats_of_request, updates=1):
    from scema_amd import capi
    eng = engine(BATCH_ACC, neigh_delay=0)
    for m, name in enumerate(BATCH_MATS):
        eng.register_replica(name, 1, batch_material(name))
    out = []
    for u in range(updates):
        sims = [capi.make_sim(q, name, 1, batch_strain(batch_material(name), q, 1.0 if u == 0 else -1.0), nss=10, temperature=BATCH_T,
                              most_recent=capi.QP_NONE if u == 0 else None, material=BATCH_MATS.index(name)) for q, name in enumerate(mats_of_request)]
        out.append(np.array([list(o.stress) for o in eng.strain_batch(sims)]))
    eng.close()
    return np.array(out)


def assert_batch(got, mats_of_request, label):
    worst = 0.0
    for u in range(got.shape[0]):
        for q, name in enumerate(mats_of_request):
            exp = batch_reference(name, q, got.shape[0])[u]
            err = np.abs(got[u, q] - exp).max() / np.abs(exp).max()
            worst = max(worst, err)
            assert err < 1e-7, (label, u, q, name, err)
    print(f"{label}: largest deviation from the oracle {worst:.2e}")


def test_three_meshes_in_one_whole_launch():
    """six requests, materials interleaved: the launch runs whole with the wide solve, two workgroups per replica; one mesh has nx = 4, so no
    replica spreads on padded rows, and the 64-point mesh lies in buffers 2 700 points apart"""
    mats = ("batch4", "batch600", "batch5", "batch4", "batch5", "batch600")
    assert_batch(run_batch(mats), mats, "4^3 + 5^3 + 12x15x15, six requests")


def test_two_padded_meshes_in_one_whole_launch():
    """the same without the 4 x 4 x 4 material: padded-row spreading with two padded sizes (10 x 5 x 5 and 17 x 15 x 15) in one launch"""
    mats = ("batch600", "batch5", "batch5", "batch600")
    assert_batch(run_batch(mats), mats, "5^3 + 12x15x15, four requests")


_CHILD_BATCH = ("import json, os, sys\n"
                "sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))\n"
                "import test_gpu_pppm_meshes as t\n"
                "print(json.dumps({'s': t.run_batch(t.MATS_36, updates=2).tolist()}))\n")
MATS_36 = tuple(BATCH_MATS[(q + q // 9) % 3] for q in range(36))      # every part of nine holds all three meshes, in another order each


def test_three_meshes_in_part_batches_over_two_updates():
    """36 requests over the three materials and a second update that continues their states with the strains reversed: four part batches
    of nine with the 512-thread solve, mixed meshes in every part -- against the oracle, and against the same batch run whole
    (SCEMA_MD_SPLIT=0, read once per process: a child)"""
    for p in range(4):
        assert set(MATS_36[9 * p:9 * p + 9]) == set(BATCH_MATS)
    got = run_batch(MATS_36, updates=2)
    assert got.shape == (2, 36, 6) and np.isfinite(got).all()
    assert_batch(got, MATS_36, "36 requests in parts, two updates")
    whole = np.array(_child(_CHILD_BATCH, {"SCEMA_MD_SPLIT": "0"})["s"])
    dev = max(np.abs(got[u, q] - whole[u, q]).max() / np.abs(whole[u, q]).max() for u in range(2) for q in range(36))
    print(f"parts against whole: {dev:.2e}")
    assert dev < 1e-9, dev
