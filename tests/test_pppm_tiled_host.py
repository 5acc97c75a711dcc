"""The tile rule of the tiled PPPM kernels (md_pppm_tile.h through scema_md_pppm_tile_shape, a pure host function) and the three large
ionic fixtures whose meshes lie beyond the LDS: what can be pinned without a GPU.  tests/test_gpu_pppm_tiled.py runs the kernels on them.

The rule: bricks of by x bz mesh rows in (y, z) over whole x rows; the charge assignment keeps nx by bz doubles, the interpolation stages
three field grids over the brick and a halo of two rows on each tiled side, 3 nx (by + 4)(bz + 4) doubles; a mesh that fits whole is one
tile; z-slabs while one plane (assignment) or five planes (interpolation) fit, y tiles only beyond that; zeros where even one row (with its
halo 5 x 5 rows) does not fit: 8 nx and 600 nx bytes."""
from collections import namedtuple

import numpy as np
import pytest

from oracle import pyoracle as po
from test_oracle_pppm_meshes import ROWS, ionic, oracle_params, product_setup

Big = namedtuple("Big", "name cells a q tilt acc grid natoms")
BIG = [
    Big("24x32x36", (6, 8, 10), 3.0, 0.4, (0.8, -0.5, 0.6), 1e-4, (24, 32, 36), 480),   # tilted, three different dimensions; beyond both limits
    Big("27x30x36", (7, 8, 10), 3.0, 0.4, (0.0, 0.0, 0.0), 1e-4, (27, 30, 36), 560),    # odd nx
    Big("36x45x54", (6, 8, 10), 3.0, 1.0, (0.8, -0.5, 0.6), 1e-4, (36, 45, 54), 480),   # five field planes are 194 KB: y tiles at the default budget
]
BIG_BY_NAME = {b.name: b for b in BIG}
BUDGETS = (512, 2 * 1024, 8 * 1024, 36 * 1024, 144 * 1024)
DEFAULT_LDS = 144 * 1024


def big_fixture(b, eps=1e-9):
    return ionic(b.cells, b.a, b.q, b.tilt, eps=eps)


def tile_shape(grid, lds, which):
    from scema_amd import capi
    return capi.pppm_tile_shape(grid, lds, which)


def staged_bytes(grid, by, bz, which):
    nx, ny, nz = grid
    if which == 0:
        return 8 * nx * by * bz
    return 24 * nx * (by + (4 if by < ny else 0)) * (bz + (4 if bz < nz else 0))


def sampled_meshes():
    rng = np.random.default_rng(20)
    return [tuple(int(n) for n in rng.integers(2, 151, 3)) for _ in range(200)]


def all_meshes():
    return sorted({b.grid for b in BIG} | {r.grid for r in ROWS} | set(sampled_meshes()))


def check_rule(grid, lds, which):
    nx, ny, nz = grid
    by, bz, ty, tz = tile_shape(grid, lds, which)
    whole = (8 if which == 0 else 24) * nx * ny * nz
    # the smallest brick: one row; three grids over one row and its halo, 5 x 5 rows -- or, with fewer than five rows in y, a slab of five planes
    least = 8 * nx if which == 0 else min(600 * nx, 120 * nx * ny)
    if (by, bz, ty, tz) == (0, 0, 0, 0):
        assert whole > lds and least > lds, (grid, lds, which)      # a reported "does not fit" is true
        return None
    assert least <= lds or whole <= lds, (grid, lds, which)
    assert 1 <= by <= ny and 1 <= bz <= nz and ty >= 1 and tz >= 1
    if whole <= lds:
        assert (by, bz, ty, tz) == (ny, nz, 1, 1), (grid, lds, which)   # a mesh that fits whole is one tile
    # the bricks cover every (y, z) row exactly once: per axis the tiles are [k b, min((k + 1) b, n)), none empty
    for n, b, t in ((ny, by, ty), (nz, bz, tz)):
        cover = np.zeros(n, int)
        for k in range(t):
            lo, hi = k * b, min((k + 1) * b, n)
            assert lo < hi, (grid, lds, which, n, b, t)
            cover[lo:hi] += 1
        assert (cover == 1).all(), (grid, lds, which, n, b, t)
    assert staged_bytes(grid, by, bz, which) <= lds, (grid, lds, which, by, bz)
    # z-slabs are preferred: y is tiled only when one plane (assignment) / five planes (interpolation) exceed the budget
    slab = staged_bytes(grid, ny, 1, which) if nz > 1 else whole
    if by < ny:
        assert slab > lds, (grid, lds, which, by)
    elif whole > lds:
        assert slab <= lds
    return by, bz, ty, tz


@pytest.mark.parametrize("which", [0, 1], ids=["spread", "force"])
def test_tile_rule_covers_every_mesh_within_every_budget(which):
    tiled = 0
    for grid in all_meshes():
        for lds in BUDGETS:
            got = check_rule(grid, lds, which)
            tiled += got is not None and got[2] * got[3] > 1
    assert tiled > 200      # (of about 1 100 combinations: the rule was walked on tiled meshes, not only on whole and unfit ones)


def test_tile_rule_at_the_default_budget_is_what_the_tests_on_the_gpu_expect():
    # (0 stands for the device default, 144 KB)
    for grid in [b.grid for b in BIG] + [(18, 27, 27)]:
        for which in (0, 1):
            assert tile_shape(grid, 0, which) == tile_shape(grid, DEFAULT_LDS, which)
    assert tile_shape((18, 27, 27), 0, 0) == (27, 27, 1, 1)           # 13 122 points: the charge grid fits whole
    # a field plane is 3 * 18 * 27 * 8 B = 11 664 B: 12 staged planes fit, 8 of them owned, so 27 planes make four z-slabs (evened out: 7)
    assert tile_shape((18, 27, 27), 0, 1) == (27, 7, 1, 4)
    assert tile_shape((24, 32, 36), 0, 0)[2:] == (1, 2) and tile_shape((24, 32, 36), 0, 1)[2] == 1
    assert tile_shape((27, 30, 36), 0, 0)[2:] == (1, 2) and tile_shape((27, 30, 36), 0, 1)[2] == 1
    # 36 x 45 x 54: five field planes are 3 * 36 * 45 * 5 * 8 B = 194 KB, the interpolation must tile y; the charge grid goes as z-slabs
    assert 3 * 36 * 45 * 5 * 8 > DEFAULT_LDS
    assert tile_shape((36, 45, 54), 0, 1)[2] >= 2 and tile_shape((36, 45, 54), 0, 0)[2] == 1 and tile_shape((36, 45, 54), 0, 0)[3] >= 2


def test_a_budget_below_the_smallest_brick_is_reported():
    from scema_amd import capi
    assert tile_shape((100, 40, 40), 512, 0) == (0, 0, 0, 0)          # one x row of 100 points is 800 bytes
    assert tile_shape((64, 40, 40), 512, 0)[0] == 1                   # 512 bytes: exactly one row
    assert tile_shape((10, 40, 40), 5999, 1) == (0, 0, 0, 0)          # 3 * 10 * 25 * 8 = 6 000 bytes
    assert tile_shape((10, 40, 40), 6000, 1)[:2] == (1, 1)
    # interpolation at the default budget: nx beyond 245 (600 nx bytes > 144 KB) keeps the unstaged kernel
    assert tile_shape((245, 60, 60), 0, 1) != (0, 0, 0, 0) and tile_shape((246, 60, 60), 0, 1) == (0, 0, 0, 0)
    for bad in (((0, 4, 4), 0, 0), ((4, 4, 4), -1, 0), ((4, 4, 4), 0, 2)):
        with pytest.raises(capi.EngineError):
            tile_shape(*bad)


@pytest.mark.parametrize("b", BIG, ids=[b.name for b in BIG])
def test_the_large_fixtures_get_their_named_meshes_from_oracle_and_product(b):
    d = big_fixture(b)
    assert d["natoms"] == b.natoms and abs(d["charge"].sum()) < 1e-12
    o = po.Oracle(d, oracle_params(b.acc))
    o.setup(False)
    assert o.pppm_grid == b.grid, (b.name, o.pppm_grid)
    g, grid = product_setup(d, b.acc)
    assert grid == b.grid, (b.name, grid)
    assert abs(g - o.g_ewald) < 1e-12, (g, o.g_ewald)
    nx, ny, nz = b.grid
    assert nx * ny * nz > 18432      # beyond the whole-mesh charge assignment (and with it the staged interpolation)
