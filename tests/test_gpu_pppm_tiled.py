"""The tiled PPPM kernels of md_pppm.hip (k_pppm_keys, k_pppm_spread_tiled, k_pppm_force_tiled) against the CPU oracle and against the
kernels they replace: on the meshes beyond the LDS that tests/test_pppm_tiled_host.py defines (and the 18x27x27 row of the mesh table),
and -- with a forced LDS budget (scema_md_pppm_tiling) -- on the small meshes of tests/test_oracle_pppm_meshes.py cut into several
tiles, with atoms on the planes where tiles meet, uncharged atoms, tiles without atoms, fewer atoms than a wave, and launches whose
replicas have different meshes and tile counts.  Every test asserts the mesh of its system before it compares anything, and through
scema_md_pppm_paths that the kernel shape it means to test ran, with the tile counts the rule gives.

Tolerances: the project's own -- 1e-10 of the largest component for static results (1e-9 for the 18x27x27 row, as the mesh table
has it), 1e-7 for evaluated stresses, 1e-9 between two launch shapes of the engine -- and 1e-12 between the tiled kernels and
the ones they replace on one engine: only the order of summation differs (the oracle's own reordering noise is 2e-15,
test_oracle_pppm_meshes.py), three orders above that noise and two below the static tolerance."""
import functools
from copy import deepcopy

import numpy as np
import pytest

from test_oracle_pppm_meshes import BY_NAME, oracle_compute, product_setup, rel, row_fixture, from_lamda, to_lamda, min_distance
from test_gpu_pppm_meshes import (BATCH_ACC, BATCH_MATS, BATCH_T, assert_mesh, assert_static, batch_material, batch_reference, batch_strain, cut_to,
                                  engine, on_planes, reference, some_uncharged)
from test_pppm_tiled_host import BIG, BIG_BY_NAME, DEFAULT_LDS, big_fixture

pytestmark = pytest.mark.gpu
WHOLE, TILED, NO_LDS = 0, 1, 2


def tile_shape(grid, lds, which):
    from scema_amd import capi
    return capi.pppm_tile_shape(grid, lds, which)


def whole_paths(grid, lds):
    """which kernels take the whole mesh at this budget (restated from mdk_pppm_spread_path / mdk_pppm_force_path)"""
    nx, ny, nz = grid
    padded = nx >= 5 and (nx + 5) * ny * nz * 8 <= min(36 * 1024, lds)
    return ((nx + 5 if padded else nx) * ny * nz * 8 <= lds), (3 * nx * ny * nz * 8 <= lds)


def expected_paths(grid, lds, mode=1):
    """what scema_md_pppm_paths must report for a launch of replicas with this one mesh"""
    out = dict(lds_bytes=lds, mode=mode)
    for which, (key, whole) in enumerate(zip(("spread", "force"), whole_paths(grid, lds))):
        by, bz, ty, tz = tile_shape(grid, lds, which)
        path = WHOLE if whole else (TILED if mode == 1 and ty > 0 else NO_LDS)
        out[key] = path
        out[key + "_tiles"] = (ty, tz) if path == TILED else (1, 1)
    return out


@functools.lru_cache(maxsize=None)
def big_reference(name):
    """(system, forces, energies, virials, g_ewald) of a large fixture by the oracle, computed once per session and never changed"""
    b = BIG_BY_NAME[name]
    d = big_fixture(b)
    f, e, w, o = oracle_compute(d, b.acc)
    assert o.pppm_grid == b.grid, (name, o.pppm_grid)
    for a in (f, e, w):
        a.setflags(write=False)
    return d, f, e, w, o.g_ewald


def figures(got, exp):
    (f, e, w), (fo, eo, wo) = got, exp
    return dict(f=rel(f, fo), e6=abs(e[6] - eo[6]) / abs(eo[6]), w6=rel(w[6], wo[6]), e1=abs(e[1] - eo[1]) / max(1e-300, abs(eo[1])))


def assert_same(got, exp, tol, label):
    fig = figures(got, exp)
    print(f"{label}: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert np.isfinite(got[0]).all()
    for k, v in fig.items():
        assert v < tol, (label, k, v, fig)


def compute(eng, name, grid, mode, lds, qp=None, want=None):
    """a static evaluation under (mode, budget); asserts the reported paths (want: kernels that must be the tiled ones, e.g. "sf")"""
    from scema_amd import capi
    eng.pppm_tiling(mode, lds)
    f, e, w, info = eng.debug_compute(name, 1, qp=capi.QP_NONE if qp is None else qp, use_shake=False)
    assert info["nk"] == 0
    paths = eng.pppm_paths()
    exp = expected_paths(grid, lds if lds else DEFAULT_LDS, mode)
    assert paths == exp, (paths, exp)
    if want is not None:
        assert (paths["spread"] == TILED) == ("s" in want) and (paths["force"] == TILED) == ("f" in want), (want, paths)
        for key, n in (("spread", "s"), ("force", "f")):
            if n in want:
                assert paths[key + "_tiles"][0] * paths[key + "_tiles"][1] >= 2, paths
    return (f, e, w), paths


# ---- 1. and 2. the large meshes at the default budget: against the oracle, and the tiled kernels against the ones they replace -------
# name -> (tolerance against the oracle, kernels that are tiled, kernels of mode 0).  The project's 1e-10 holds on the three new fixtures
# (measured, mode 0 and tiled alike, largest figure per row: 24x32x36 f 6.5e-13, 27x30x36 f 2.4e-13, 36x45x54 f 2.9e-13 -- none needs the
# wider bound the hipFFT meshes were allowed); 18x27x27 keeps the 1e-9 its row has in the mesh table (measured 2.5e-13).
LARGE = {
    "18x27x27": (1e-9, "f", (WHOLE, NO_LDS)),
    "24x32x36": (1e-10, "sf", (NO_LDS, NO_LDS)),
    "27x30x36": (1e-10, "sf", (NO_LDS, NO_LDS)),
    "36x45x54": (1e-10, "sf", (NO_LDS, NO_LDS)),
}


def large_case(name):
    if name in BIG_BY_NAME:
        b = BIG_BY_NAME[name]
        return (b.grid, b.acc) + big_reference(name)
    row = BY_NAME[name]
    return (row.grid, row.acc) + reference(name)


@pytest.mark.parametrize("name", list(LARGE))
def test_large_meshes_tiled_against_the_oracle_and_against_the_kernels_without_lds(name):
    """At the default budget: 18x27x27 keeps its charge grid whole and tiles the interpolation (four z-slabs); the three large fixtures tile
    both, 36x45x54 with y tiles in the interpolation (five staged planes are 194 KB).  Mode 0 on the same engine runs the global-atomic
    charge assignment and the unstaged interpolation, which had no test of their own."""
    tol, want, mode0 = LARGE[name]
    grid, acc, d, fo, eo, wo, g = large_case(name)
    assert abs(assert_mesh(d, acc, grid) - g) < 1e-12
    if name == "36x45x54":
        assert tile_shape(grid, 0, 1)[2] >= 2 and tile_shape(grid, 0, 0)[2] == 1
    eng = engine(acc)
    eng.register_replica("m", 1, d)
    tiled, paths = compute(eng, "m", grid, 1, 0, want=want)
    plain, paths0 = compute(eng, "m", grid, 0, 0, want="")
    assert (paths0["spread"], paths0["force"]) == mode0, paths0
    again, _ = compute(eng, "m", grid, 1, 0, want=want)      # (and back: the charge grid holds what the transforms of mode 0 left)
    eng.close()
    print(name, paths)
    fig0 = figures(plain, (fo, eo, wo))
    print(f"{name} mode 0 against the oracle: " + "  ".join(f"{k} {v:.2e}" for k, v in fig0.items()))
    assert_same(tiled, plain, 1e-12, f"{name} tiled against mode 0")
    assert_same(again, plain, 1e-12, f"{name} tiled after mode 0 against mode 0")
    assert_static(plain, (fo, eo, wo), tol, f"{name} mode 0")
    assert_static(tiled, (fo, eo, wo), tol, f"{name} tiled")


# ---- 3. forced tiles on small meshes --------------------------------------------------------------------------------------------------
# row -> ((LDS budget in bytes, kernels that are tiled at it), ...): at least two tiles along every tiled axis and a ragged last tile in
# one of the two kernels.  The interpolation stages a halo of four rows per tiled axis, so no budget tiles both kernels of a mesh of a
# few rows: most rows run once per kernel (the other one whole, or without LDS where even its smallest brick is beyond the budget).
FORCED = {
    "3x3x3": ((48, "s"), (144, "s")),                       # y and z tiles of 2 + 1 rows; z-slabs.  (Three field planes never tile: 5 staged > 3.)
    "4x4x10": ((384, "s"), (2688, "f")),                    # z-slabs 3 3 3 1 in either kernel; x and y wrap
    "4x10x4": ((96, "s"), (3360, "f")),                     # y tiles 3 3 3 1, one plane thick: the interpolation stages 5 planes of a mesh of 4
    "4x5x8": ((480, "s"), (64, "s"), (3360, "f")),          # tilted: slabs 3 3 2; y tiles 2 2 1
    "9x8x6": ((216, "s"), (7560, "f")),                     # tilted: y tiles 3 3 2
    "5x5x15": ((400, "s"), (3600, "f")),                    # slabs of two planes, the last of one
    "12x10x24": ((4800, "s"), (10080, "sf"), (25920, "f")), # slabs 5 5 5 5 4; y tiles 3 3 3 1 under slabs of the charge grid; slabs
    "batch600": ((25920, "f"), (15552, "sf"), (384, "s")),  # z-slabs only; y and z tiles 5 5 5 x 2 .. 1 under two slabs 8 7; y tiles 4 4 4 3
}
BOTH = 15552      # batch600 (12 x 15 x 15): charge grid as two z-slabs (8, 7), field grids as 3 x 8 tiles of 5 x 2 rows (the last plane alone)


def ragged(grid, lds, which):
    by, bz, ty, tz = tile_shape(grid, lds, which)
    return (ty > 1 and grid[1] % by != 0) or (tz > 1 and grid[2] % bz != 0)


@pytest.mark.parametrize("name", list(FORCED))
def test_forced_tiles_on_small_meshes(name):
    row = BY_NAME[name]
    d, fo, eo, wo, g = reference(name)
    assert abs(assert_mesh(d, row.acc, row.grid) - g) < 1e-12
    assert any(ragged(row.grid, lds, which) for lds, want in FORCED[name] for which, k in enumerate("sf") if k in want), name
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    whole, paths = compute(eng, "m", row.grid, 1, 0, want="")
    assert (paths["spread"], paths["force"]) == (WHOLE, WHOLE)
    assert_static(whole, (fo, eo, wo), row.tol, f"{name} whole")
    for lds, want in FORCED[name]:
        got, paths = compute(eng, "m", row.grid, 1, lds, want=want)
        label = f"{name} at {lds} B, spread {paths['spread']} {paths['spread_tiles']}, force {paths['force']} {paths['force_tiles']}"
        assert_same(got, whole, 1e-12, label + " against the whole mesh")
        assert_static(got, (fo, eo, wo), row.tol, label)
    eng.close()


def test_batch600_tiles_y_only_under_the_smaller_budget():
    grid = BY_NAME["batch600"].grid
    assert tile_shape(grid, 25920, 1) == (15, 2, 1, 8)                                       # z-slabs only
    assert tile_shape(grid, BOTH, 1) == (5, 2, 3, 8) and tile_shape(grid, BOTH, 0) == (15, 8, 1, 2)
    assert tile_shape(grid, 384, 0) == (4, 1, 4, 15)


def test_tiling_refuses_what_it_cannot_run():
    from scema_amd import capi
    eng = engine(0.03)
    for mode, lds in ((2, -1), (-2, -1), (1, 8), (1, 161 * 1024), (1, -2)):
        with pytest.raises(capi.EngineError):
            eng.pppm_tiling(mode, lds)
    eng.pppm_tiling(0, 4096)
    eng.pppm_tiling(-1, -1)
    eng.close()


# ---- 4. placement on batch600 with forced tiles ---------------------------------------------------------------------------------------
def batch600():
    row = BY_NAME["batch600"]
    return row, row_fixture(row, eps=1e-9)


def static_case(d, row, lds, want, label, tol=1e-10):
    fo, eo, wo, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid and abs(assert_mesh(d, row.acc, row.grid) - o.g_ewald) < 1e-12
    eng = engine(row.acc)
    eng.register_replica("p", 1, d)
    got, paths = compute(eng, "p", row.grid, 1, lds, want=want)
    eng.close()
    assert_static(got, (fo, eo, wo), tol, label)
    return got


def test_atoms_on_the_planes_where_tiles_meet():
    """every atom exactly on a grid plane in all three lamda coordinates: the planes y = 5, 10 and every second z plane are tile borders of the
    interpolation, z = 8 of the charge assignment, and the atoms on plane 0 / n sit on the periodic seam"""
    row, d = batch600()
    out = on_planes(d, row.grid, half=False)
    # (the lattice has no site nearest to plane 0: every third atom of plane 1 in y, and of the others in z, moves onto the seam)
    u = np.round(to_lamda(out) * np.array(row.grid, float))
    to_y = np.nonzero(u[:, 1] == 1)[0][::3]
    u[to_y, 1] = 0.0
    to_z = np.setdiff1d(np.nonzero(u[:, 2] == 1)[0], to_y)[::3]
    u[to_z, 2] = 0.0
    assert len(to_y) >= 10 and len(to_z) >= 10
    out = from_lamda(out, u / np.array(row.grid, float))
    u = to_lamda(out) * np.array(row.grid, float)
    assert np.abs(u - np.round(u)).max() < 1e-12 and min_distance(out) > 0.3
    iy, iz = np.round(u[:, 1]).astype(int) % 15, np.round(u[:, 2]).astype(int) % 15
    assert {0, 5, 10} <= set(iy) and {0, 8} <= set(iz)
    static_case(out, row, BOTH, "sf", "batch600 on planes")


def test_uncharged_atoms_get_exact_zeros_from_their_home_tile():
    """every fourth atom uncharged, no LJ: the single replica's chain runs on the side stream and STORES its forces (add = 0)"""
    row, d = batch600()
    out = some_uncharged(d)
    f, e, w = static_case(out, row, BOTH, "sf", "batch600 some uncharged")
    zero = np.asarray(out["charge"]) == 0.0
    assert zero.sum() >= out["natoms"] // 4 and np.all(f[zero] == 0.0), np.abs(f[zero]).max()


def test_uncharged_atoms_keep_their_forces_where_the_chain_adds():
    """nine requests run as three part batches whose PPPM chains ADD to the assembled forces (add = 1): uncharged atoms, here with LJ, must
    keep theirs.  Against the same requests under mode 0, the project's 1e-9 between two launch shapes."""
    from scema_amd import capi
    row = BY_NAME["batch600"]
    d = some_uncharged(row_fixture(row, eps=0.1))
    d["eps"] = np.array([[0.1]])
    assert_mesh(d, BATCH_ACC, row.grid)
    got = {}
    for mode in (1, 0):
        eng = engine(BATCH_ACC, neigh_delay=0)
        eng.register_replica("u", 1, d)
        eng.pppm_tiling(mode, BOTH)
        sims = [capi.make_sim(q, "u", 1, batch_strain(d, q), nss=10, temperature=BATCH_T, most_recent=capi.QP_NONE) for q in range(9)]
        got[mode] = np.array([list(o.stress) for o in eng.strain_batch(sims)])
        paths = eng.pppm_paths()
        assert (paths["spread"], paths["force"]) == ((TILED, TILED) if mode else (NO_LDS, NO_LDS)), paths
        assert eng.concurrency()["split"] == 1
        eng.close()
    dev = max(np.abs(got[1][q] - got[0][q]).max() / np.abs(got[0][q]).max() for q in range(9))
    print(f"uncharged atoms, chain adds: tiled against mode 0 {dev:.2e}")
    assert np.isfinite(got[1]).all() and dev < 1e-9, dev


@pytest.mark.parametrize("lds,want", [(2880, "s"), (BOTH, "sf")])
def test_a_tile_without_atoms_leaves_zeros(lds, want):
    """All charged atoms in z < L/2 (the others uncharged): at 2 880 B the charge grid goes as slabs of two planes and the slab of planes
    10, 11 is touched by no stencil; the interpolation tiles beyond plane 9 have no home atom.  Evaluated twice on one engine, first with
    every atom moved by L/2 in z: the second result must match a fresh engine's, because the slabs that are empty now were full before."""
    row, d = batch600()
    lam = to_lamda(d)
    q = np.asarray(d["charge"], float).copy()
    q2 = (q ** 2).sum()
    q[lam[:, 2] >= 0.5] = 0.0
    assert abs(q.sum()) < 1e-12 and (q != 0).sum() == 300
    d = deepcopy(d)
    d["charge"] = q * np.sqrt(q2 / (q ** 2).sum())
    if lds == 2880:
        by, bz, ty, tz = tile_shape(row.grid, lds, 0)
        assert (by, bz, ty, tz) == (15, 2, 1, 8)
        near = np.floor(lam[q != 0, 2] * 15 + 0.5).astype(int)
        touched = {(k + o) % 15 for k in near for o in range(-2, 3)}
        assert not {10, 11} & touched
    fo, eo, wo, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid and abs(assert_mesh(d, row.acc, row.grid) - o.g_ewald) < 1e-12
    moved = d["x"].copy()
    moved[:, 2] += 0.5 * (d["box"][5] - d["box"][2])
    eng = engine(row.acc)
    eng.register_replica("p", 1, d)
    eng.set_state(5, "p", 1, d["box"], moved, d["v"])
    first, _ = compute(eng, "p", row.grid, 1, lds, qp=5, want=want)
    eng.set_state(5, "p", 1, d["box"], d["x"], d["v"])
    second, _ = compute(eng, "p", row.grid, 1, lds, qp=5, want=want)
    eng.close()
    fresh_eng = engine(row.acc)
    fresh_eng.register_replica("p", 1, d)
    fresh_eng.set_state(5, "p", 1, d["box"], d["x"], d["v"])
    fresh, _ = compute(fresh_eng, "p", row.grid, 1, lds, qp=5, want=want)
    fresh_eng.close()
    assert_same(second, fresh, 1e-12, f"empty tiles at {lds} B: second evaluation against a fresh engine")
    assert_static(second, (fo, eo, wo), 1e-10, f"empty tiles at {lds} B")


@pytest.mark.parametrize("lds,want", [(BOTH, "sf"), (384, "s")])
def test_fewer_atoms_than_a_wave(lds, want):
    """the first 40 atoms of batch600 with charges +-2.2, which keep the 12 x 15 x 15 mesh: most lanes of the one wave that has atoms have none,
    most tiles have no atom at all"""
    row, d = batch600()
    static_case(cut_to(d, 40, 2.2), row, lds, want, f"batch600 cut to 40 atoms at {lds} B")


# ---- 5. mixed meshes and tile counts in one launch ------------------------------------------------------------------------------------
MIXED = ("batch4", "batch5", "batch600", "batch4", "batch5", "batch600")      # (the first six of MATS_36 in test_gpu_pppm_meshes.py: one oracle run serves both)


def run_mixed(mode, lds, updates=2):
    from scema_amd import capi
    eng = engine(BATCH_ACC, neigh_delay=0)
    eng.pppm_tiling(mode, lds)
    for name in BATCH_MATS:
        eng.register_replica(name, 1, batch_material(name))
    out, paths = [], []
    for u in range(updates):
        sims = [capi.make_sim(q, name, 1, batch_strain(batch_material(name), q, 1.0 if u == 0 else -1.0), nss=10, temperature=BATCH_T,
                              most_recent=capi.QP_NONE if u == 0 else None, material=BATCH_MATS.index(name)) for q, name in enumerate(MIXED)]
        out.append(np.array([list(o.stress) for o in eng.strain_batch(sims)]))
        paths.append(eng.pppm_paths())
    eng.close()
    return np.array(out), paths


@pytest.mark.parametrize("lds", [600, 11520])
def test_three_meshes_and_tile_counts_in_one_launch(lds):
    """Six requests over the 4^3, 5^3 and 12 x 15 x 15 materials in one launch, two updates.  At 600 B the charge assignment holds a mesh of one
    tile (512 B), one of two z-slabs and one of 3 x 15 y tiles, and the interpolation runs unstaged (the 4^3 mesh neither fits nor tiles);
    at 11 520 B the two small meshes are one tile each beside two slabs of the charge grid and 4 x 15 tiles of the field grids of the large
    one (behind the in-LDS solve: real field arrays).  Stresses against the oracle at 1e-7 and against mode 0 at 1e-9."""
    g4, g5, g600 = (BY_NAME[n].grid for n in BATCH_MATS)
    if lds == 600:
        assert tile_shape(g4, lds, 0)[2:] == (1, 1) and tile_shape(g5, lds, 0)[2:] == (1, 2) and tile_shape(g600, lds, 0)[2:] == (3, 15)
        assert tile_shape(g4, lds, 1) == (0, 0, 0, 0)
        want = dict(spread=TILED, force=NO_LDS, spread_tiles=(3, 15), force_tiles=(1, 1))
    else:
        assert tile_shape(g4, lds, 1)[2:] == (1, 1) and tile_shape(g5, lds, 1)[2:] == (1, 1) and tile_shape(g600, lds, 1)[2:] == (4, 15)
        assert tile_shape(g600, lds, 0)[2:] == (1, 2)
        want = dict(spread=TILED, force=TILED, spread_tiles=(1, 2), force_tiles=(4, 15))
    got, paths = run_mixed(1, lds)
    plain, paths0 = run_mixed(0, lds)
    assert got.shape == (2, 6, 6) and np.isfinite(got).all()
    first = paths[0]
    assert {k: first[k] for k in want} == want and first["lds_bytes"] == lds and first["mode"] == 1, first
    assert (paths0[0]["spread"], paths0[0]["force"]) == (NO_LDS, NO_LDS), paths0
    worst = 0.0
    for u in range(2):
        for q, name in enumerate(MIXED):
            exp = batch_reference(name, q, 2)[u]
            err = np.abs(got[u, q] - exp).max() / np.abs(exp).max()
            worst = max(worst, err)
            assert err < 1e-7, (lds, u, q, name, err)
    dev = max(np.abs(got[u, q] - plain[u, q]).max() / np.abs(plain[u, q]).max() for u in range(2) for q in range(6))
    print(f"mixed meshes at {lds} B: largest deviation from the oracle {worst:.2e}, from mode 0 {dev:.2e}")
    assert dev < 1e-9, dev
