"""PPPM mesh shapes: the table of ionic lattices whose meshes the GPU tests of tests/test_gpu_pppm_meshes.py walk, its fixture builder,
and what can be pinned without a GPU -- the grid rule of oracle and product per row, and three properties of the oracle's mesh sum that
make it a sound reference for those tests: invariance under lattice-vector shifts of atoms (atoms outside the box), under a relabelling
of the axes, and under the order of the atoms (its own summation noise, the yardstick of the GPU tolerances), and continuity where an
atom sits on a face of the box.

Reordering noise of the oracle, measured by test_oracle_reordering_noise_is_the_yardstick over every row of ROWS (largest relative
deviation of forces, e[6] and w[6] between a seeded atom permutation and the file order): the maximum is 2.2e-15, the w[6] of row
"3x3x3"; forces 1.3e-15 at most (row "batch600"), e[6] unchanged to the last bit on every row.  No row comes near 1e-11, so every GPU
tolerance is the project's own (1e-10, 1e-9 for the 18x27x27 mesh, 1e-7 for evaluated stresses)."""
from collections import namedtuple
from copy import deepcopy

import numpy as np
import pytest

from oracle import pyoracle as po

KW = dict(cut_lj=3.5, cut_coul=3.5, skin=0.5)
PP_SOLVE_MAX = 2900          # md_pppm.hip: grid points up to which the solve stays in LDS
PADX_MAX = 36 * 1024 // 8    # mdk_pppm_spread: padded points ((nx + 5) ny nz) up to which the padded-row spreading is taken
LDS_MAX = 144 * 1024 // 8    # mdk_pppm_lds_limit in doubles: charge grid of the spreading kernel, three field grids of the force kernel

# One row per mesh.  cells, a, q, accuracy and tilt are the input; grid is what the grid rule must give (asserted before anything is
# compared); relabel: the fixture is the first permutation row with its axes relabelled (new axis j = old axis relabel[j]).
# solve / spread / force name the kernel shapes a single replica of the row reaches with the default switches:
#   solve   "lds": k_pppm_solve (grid <= PP_SOLVE_MAX)            "fft": hipFFT + k_pppm_poisson
#   spread  "padded": LDS copy with nx + 5 points per x row         "plain": LDS copy without pad columns (nx < 5, or too large to pad)
#           "global": global atomics (no row: needs more than 18 432 points)
#   force   "staged": field grids in LDS                            "unstaged": through the caches (more than 6 144 points)
# tol: forces, e[1], e[6], w[6] against the oracle, of the largest component.  (No row's reordering noise exceeds 1e-11, see the
# module docstring: none is widened.)
Row = namedtuple("Row", "name cells a q acc tilt grid relabel solve spread force tol batch note")
_R = lambda name, cells, a, q, acc, tilt, grid, solve, spread, force, note="", relabel=None, tol=1e-10, batch=False: \
    Row(name, cells, a, q, acc, tilt, grid, relabel, solve, spread, force, tol, batch, note)
ROWS = [
    _R("3x3x3", (3, 3, 3), 2.7, 0.02, 0.3, (0, 0, 0), (3, 3, 3), "lds", "plain", "staged", "every dimension wraps twice"),
    _R("3x3x5", (3, 3, 6), 2.7, 0.02, 0.3, (0, 0, 0), (3, 3, 5), "lds", "plain", "staged", "no Nyquist plane at all"),
    _R("4x4x8", (3, 3, 8), 3.0, 0.02, 0.1, (0, 0, 0), (4, 4, 8), "lds", "plain", "staged", "nx = 4: no padded row"),
    _R("10x4x4", (12, 3, 3), 3.0, 0.02, 0.1, (0, 0, 0), (10, 4, 4), "lds", "padded", "staged", "long axis x"),
    _R("4x10x4", (3, 12, 3), 3.0, 0.02, 0.1, (0, 0, 0), (4, 10, 4), "lds", "plain", "staged", "long axis y", relabel=(1, 0, 2)),
    _R("4x4x10", (3, 3, 12), 3.0, 0.02, 0.1, (0, 0, 0), (4, 4, 10), "lds", "plain", "staged", "long axis z", relabel=(2, 1, 0)),
    _R("8x4x4", (8, 3, 3), 3.0, 0.02, 0.1, (0, 0, 0), (8, 4, 4), "lds", "padded", "staged"),
    _R("4x5x8", (3, 4, 6), 3.0, 0.02, 0.03, (1.1, -0.8, 0.9), (4, 5, 8), "lds", "plain", "staged", "tilted, no padded row"),
    _R("5x4x8", (4, 3, 9), 3.0, 0.02, 0.03, (0.9, 0.7, -1.0), (5, 4, 8), "lds", "padded", "staged", "tilted"),
    _R("5x5x8", (3, 3, 4), 3.0, 0.02, 1e-3, (0, 0, 0), (5, 5, 8), "lds", "padded", "staged", "nx = 5: smallest padded row"),
    _R("5x5x15", (3, 3, 12), 3.0, 0.02, 1e-2, (0, 0, 0), (5, 5, 15), "lds", "padded", "staged", "odd long axis"),
    _R("9x8x6", (5, 4, 3), 3.0, 0.02, 1e-4, (1.2, -0.6, 0.8), (9, 8, 6), "lds", "padded", "staged", "tilted"),
    _R("8x15x8", (3, 12, 3), 3.0, 0.05, 1e-4, (0, 0, 0), (8, 15, 8), "lds", "padded", "staged"),
    _R("8x8x8", (3, 4, 6), 3.0, 0.2, 1e-3, (1.1, -0.8, 0.9), (8, 8, 8), "lds", "padded", "staged", "tilted"),
    _R("10x10x27", (3, 3, 12), 3.0, 0.6, 1e-3, (0.8, -0.5, 0.6), (10, 10, 27), "lds", "padded", "staged", "2 700 points, tilted"),
    _R("12x10x24", (4, 3, 9), 3.0, 0.6, 1e-3, (0, 0, 0), (12, 10, 24), "lds", "padded", "staged", "2 880 points: just under PP_SOLVE_MAX"),
    _R("18x15x12", (5, 4, 3), 3.0, 1.0, 1e-3, (0, 0, 0), (18, 15, 12), "fft", "padded", "staged", "3 240 points: hipFFT between LDS kernels"),
    _R("15x16x15", (3, 3, 3), 3.0, 0.2, 1e-5, (0.8, 0.5, -0.6), (15, 16, 15), "fft", "plain", "staged", "tilted; too large to pad"),
    _R("18x27x27", (6, 10, 10), 3.0, 0.2, 1e-4, (0, 0, 0), (18, 27, 27), "fft", "plain", "unstaged", "600 atoms: two atom ranges per replica",
       tol=1e-9),
    # the three materials of the mixed-mesh batches: one engine-wide accuracy, three meshes
    _R("batch4", (3, 3, 3), 3.0, 0.6, 0.03, (0, 0, 0), (4, 4, 4), "lds", "plain", "staged", batch=True),
    _R("batch5", (3, 3, 3), 3.0, 1.0, 0.03, (0, 0, 0), (5, 5, 5), "lds", "padded", "staged", batch=True),
    _R("batch600", (6, 10, 10), 3.0, 1.0, 0.03, (0, 0, 0), (12, 15, 15), "lds", "padded", "staged", "600 atoms, 2 700 points: two atom ranges", batch=True),
]
BY_NAME = {r.name: r for r in ROWS}
STATIC_ROWS = [r for r in ROWS if not r.batch]
LDS_ROWS = [r for r in STATIC_ROWS if r.solve == "lds"]


def ionic(cells, a, q, tilt=(0.0, 0.0, 0.0), seed=1, jitter=0.15, eps=1e-9, temperature=50.0):
    """Rock-salt charges +-q on a simple cubic lattice of spacing a with uniform jitter, one type of mass 20, no bonded terms, special
    weights 1; the lattice is sheared with the box.  A system with an odd number of atoms leaves its last atom uncharged (neutral)."""
    rng = np.random.default_rng(seed)
    ijk = np.array([(i, j, k) for i in range(cells[0]) for j in range(cells[1]) for k in range(cells[2])], float)
    n = len(ijk)
    x = (ijk + 0.5) * a + rng.uniform(-jitter, jitter, (n, 3))
    charge = q * (1.0 - 2.0 * (ijk.sum(1) % 2))
    if n % 2:
        charge[-1] = 0.0
    L = np.array(cells, float) * a
    xy, xz, yz = (float(t) for t in tilt)
    x = x + np.outer(x[:, 1] / L[1], [xy, 0.0, 0.0]) + np.outer(x[:, 2] / L[2], [xz, yz, 0.0])
    m = 20.0
    v = rng.normal(0, 1, (n, 3)) * np.sqrt(0.0019872067 * temperature / (m * 48.88821291 ** 2))
    v -= v.mean(0)
    z = lambda *s: np.zeros(s, np.int32)
    return dict(natoms=n, ntypes=1, type=z(n), charge=charge, mass=np.array([m]), eps=np.array([[eps]]), sigma=np.array([[2.5]]),
                bonds=z(0, 2), bond_type=z(0), bond_coeff=np.zeros((0, 2)), angles=z(0, 3), angle_type=z(0), angle_coeff=np.zeros((0, 2)),
                dihedrals=z(0, 4), dihedral_type=z(0), dihedral_coeff=np.zeros((0, 4)), impropers=z(0, 4), improper_type=z(0),
                improper_coeff=np.zeros((0, 2)), special_lj=np.ones(3), special_coul=np.ones(3),
                box=np.array([0.0, 0.0, 0.0, L[0], L[1], L[2], xy, xz, yz]), x=x, v=v)


def relabelled(d, perm):
    """the same atoms in a frame whose axis j is the old axis perm[j] (orthogonal boxes only)"""
    assert not np.any(d["box"][6:9])
    perm = list(perm)
    out = deepcopy(d)
    out["x"] = d["x"][:, perm].copy()
    out["v"] = d["v"][:, perm].copy()
    out["box"] = np.concatenate([d["box"][:3][perm], d["box"][3:6][perm], np.zeros(3)])
    return out


def relabel_sym6(w, perm):
    """a symmetric tensor (xx, yy, zz, xy, xz, yz) in the frame of `relabelled`"""
    m = np.array([[w[0], w[3], w[4]], [w[3], w[1], w[5]], [w[4], w[5], w[2]]])
    m = m[np.ix_(list(perm), list(perm))]
    return np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 1], m[0, 2], m[1, 2]])


def row_fixture(row, eps=None, seed=1):
    """the system of a table row (static rows: LJ of 1e-9 kcal/mol, so that the force scale is the Coulomb force's; batch rows integrate: 0.1)"""
    if eps is None:
        eps = 0.1 if row.batch else 1e-9
    if row.relabel is not None:
        first = next(r for r in ROWS if r.relabel is None and sorted(r.cells) == sorted(row.cells) and (r.a, r.q, r.acc) == (row.a, row.q, row.acc)
                     and tuple(np.array(r.cells)[list(row.relabel)]) == tuple(row.cells))
        return relabelled(row_fixture(first, eps, seed), row.relabel)
    return ionic(row.cells, row.a, row.q, row.tilt, seed=seed, eps=eps)


def oracle_params(acc):
    return po.default_params(kspace_accuracy=acc, kspace_pppm=1, **KW)


def oracle_compute(d, acc):
    """(forces, energies, virials, oracle) of a static evaluation without SHAKE"""
    o = po.Oracle(d, oracle_params(acc))
    o.setup(False)
    f, e, w = o.compute()
    return f, e, w, o


def product_setup(d, acc):
    """(g_ewald, grid) of the product's own rule for this system (a host function: no GPU)"""
    from scema_amd import capi
    qsq = float((np.asarray(d["charge"]) ** 2).sum())
    _, g, grid = capi.kspace_setup(capi.default_params(kspace_accuracy=acc, **KW), np.asarray(d["box"], float), qsq, d["natoms"])
    return g, grid


def shapes_of(grid, natoms):
    """what mdk_pppm_spread / the launch policy / mdk_pppm_force choose for a single replica with this mesh (restated from md_pppm.hip)"""
    nx, ny, nz = grid
    ng = nx * ny * nz
    spread = "padded" if nx >= 5 and (nx + 5) * ny * nz <= PADX_MAX else ("plain" if ng <= LDS_MAX else "global")
    return ("lds" if ng <= PP_SOLVE_MAX else "fft"), spread, ("staged" if 3 * ng <= LDS_MAX else "unstaged")


def shifted_by_lattice_vectors(d, seed, choices=(-1, 1), every=3):
    """every `every`-th atom moved by whole lattice vectors (per atom and vector one of `choices`)"""
    rng = np.random.default_rng(seed)
    b = np.asarray(d["box"], float)
    lat = np.array([[b[3] - b[0], 0, 0], [b[6], b[4] - b[1], 0], [b[7], b[8], b[5] - b[2]]])
    out = deepcopy(d)
    idx = np.arange(0, d["natoms"], every)
    out["x"] = d["x"].copy()
    out["x"][idx] += rng.choice(choices, (len(idx), 3)).astype(float) @ lat
    return out


def permuted_atoms(d, seed):
    """(system with its atoms in a seeded random order, p) with new atom i = old atom p[i]"""
    p = np.random.default_rng(seed).permutation(d["natoms"])
    out = deepcopy(d)
    for k in ("type", "charge", "x", "v"):
        out[k] = np.asarray(d[k])[p].copy()
    return out, p


def rel(a, b):
    a = np.asarray(a, float); b = np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


# ---- lamda coordinates and placements on the faces of the box (shared with the GPU tests) ----
def _cell(d):
    b = np.asarray(d["box"], float)
    return b[:3], np.array([[b[3] - b[0], 0, 0], [b[6], b[4] - b[1], 0], [b[7], b[8], b[5] - b[2]]])   # rows: the lattice vectors


def to_lamda(d):
    lo, lat = _cell(d)
    return (np.asarray(d["x"]) - lo) @ np.linalg.inv(lat)


def from_lamda(d, lam):
    lo, lat = _cell(d)
    out = deepcopy(d)
    out["x"] = lo + np.asarray(lam) @ lat
    return out


def min_distance(d):
    lam = to_lamda(d)
    _, lat = _cell(d)
    dl = lam[:, None, :] - lam[None, :, :]
    dl -= np.round(dl)
    r = np.sqrt(((dl @ lat) ** 2).sum(-1))
    return r[np.triu_indices(len(lam), 1)].min()


def on_faces(d, cells):
    """per coordinate c one atom at lamda_c = 0 exactly, one at -1e-17 and one at 1 - 1e-17 (in a box with lo = 0: lo - 1e-17 L and
    hi - 1e-17 L; the kernel's lamda - floor(lamda) rounds to 1.0 and the nearest plane is i == n), and one atom in the corner"""
    lam = to_lamda(d)
    site = lambda i, j, k: (i * cells[1] + j) * cells[2] + k
    moved = []
    for c in range(3):
        for (p, q), value in (((0, 1), 0.0), ((1, 2), -1e-17), ((2, 0), 1.0 - 1e-17)):
            ijk = [0, 0, 0]
            ijk[c] = cells[c] - 1 if value > 0.5 else 0          # taken from the layer next to the face it moves to
            ijk[(c + 1) % 3], ijk[(c + 2) % 3] = p, q
            a = site(*ijk)
            assert a not in moved
            lam[a, c] = value
            moved.append(a)
    corner = site(1, 1, 1)
    assert corner not in moved
    lam[corner] = 0.0
    out = from_lamda(d, lam)
    lo, lat = _cell(d)
    if not np.any(d["box"][6:9]):   # orthogonal, lo = 0: the positions are the literal ones
        L = np.diag(lat)
        for c in range(3):
            a0, a1, a2 = moved[3 * c:3 * c + 3]
            out["x"][a0, c] = lo[c]
            out["x"][a1, c] = lo[c] - 1e-17 * L[c]
            out["x"][a2, c] = (lo[c] + L[c]) - 1e-17 * L[c]
        out["x"][corner] = lo
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_row_gets_its_named_grid_from_oracle_and_product(row):
    d = row_fixture(row)
    assert abs(d["charge"].sum()) < 1e-12 and d["natoms"] == int(np.prod(row.cells))
    o = po.Oracle(d, oracle_params(row.acc))
    o.setup(False)
    assert o.pppm_grid == row.grid, (row.name, o.pppm_grid)
    g, grid = product_setup(d, row.acc)
    assert grid == row.grid, (row.name, grid)
    assert abs(g - o.g_ewald) < 1e-12, (g, o.g_ewald)
    # the kernel shapes the table names are those the launch code's own thresholds give for this mesh
    assert shapes_of(row.grid, d["natoms"]) == (row.solve, row.spread, row.force), shapes_of(row.grid, d["natoms"])


def test_the_table_covers_the_shapes_it_is_there_for():
    grids = [r.grid for r in STATIC_ROWS]
    assert any(all(n % 2 for n in g) for g in grids)                                  # odd only: no Nyquist plane
    assert any(g[0] < 5 for g in grids) and any(g[0] == 5 for g in grids)             # without and with the smallest padded row
    assert any(min(g) < 4 for g in grids)                                             # more than one wrap per stencil
    assert {int(np.argmax(g)) for g in grids if max(g) >= 2 * sorted(g)[1]} == {0, 1, 2}   # a long axis in x, in y and in z
    assert any(PP_SOLVE_MAX - 100 < np.prod(g) <= PP_SOLVE_MAX for g in grids)
    assert {r.solve for r in STATIC_ROWS} == {"lds", "fft"} and {r.spread for r in STATIC_ROWS} == {"padded", "plain"}
    assert {r.force for r in STATIC_ROWS} == {"staged", "unstaged"}


@pytest.mark.parametrize("name", ["4x5x8", "3x3x5"])
def test_oracle_does_not_see_lattice_vector_shifts(name):
    """atoms moved out of the box by whole lattice vectors: same forces, reciprocal energy and virial (one tilted row, one with a
    3-point dimension) -- the reference of the GPU tests that place atoms outside the box"""
    row = BY_NAME[name]
    d = row_fixture(row)
    f0, e0, w0, o0 = oracle_compute(d, row.acc)
    d1 = shifted_by_lattice_vectors(d, seed=5)
    assert np.abs(d1["x"] - d["x"]).max() > 7.0
    f1, e1, w1, o1 = oracle_compute(d1, row.acc)
    assert o1.pppm_grid == o0.pppm_grid == row.grid
    assert rel(f1, f0) < 1e-12 and abs(e1[6] - e0[6]) < 1e-12 * abs(e0[6]) and rel(w1[6], w0[6]) < 1e-12


def test_oracle_treats_the_axes_alike():
    """the three permutation rows are one set of atoms in three frames: forces and virial permute, energies agree"""
    first = BY_NAME["10x4x4"]
    d0 = row_fixture(first)
    f0, e0, w0, o0 = oracle_compute(d0, first.acc)
    assert o0.pppm_grid == first.grid
    for name in ("4x10x4", "4x4x10"):
        row = BY_NAME[name]
        d = row_fixture(row)
        assert np.array_equal(d["x"], d0["x"][:, list(row.relabel)]) and np.array_equal(d["charge"], d0["charge"])
        f, e, w, o = oracle_compute(d, row.acc)
        assert o.pppm_grid == row.grid
        assert rel(f, f0[:, list(row.relabel)]) < 1e-12
        assert rel(w[6], relabel_sym6(w0[6], row.relabel)) < 1e-12 and rel(w[1], relabel_sym6(w0[1], row.relabel)) < 1e-12
        assert abs(e[1] - e0[1]) < 1e-12 * abs(e0[1]) and abs(e[6] - e0[6]) < 1e-12 * abs(e0[6])


def reordering_noise(row):
    d = row_fixture(row)
    f0, e0, w0, _ = oracle_compute(d, row.acc)
    dp, p = permuted_atoms(d, seed=11)
    fp, ep, wp, _ = oracle_compute(dp, row.acc)
    back = np.empty_like(fp)
    back[p] = fp
    return rel(back, f0), abs(ep[6] - e0[6]) / abs(e0[6]), rel(wp[6], w0[6])


def test_oracle_reordering_noise_is_the_yardstick():
    """the reference's own summation-order noise per row, far below the 1e-10 the GPU tests ask for (the figures of the module docstring)"""
    noise = {r.name: reordering_noise(r) for r in ROWS}
    for k, label in enumerate(("forces", "e[6]", "w[6]")):
        worst = max(noise, key=lambda n: noise[n][k])
        print(f"oracle reordering noise, {label}: max {noise[worst][k]:.2e} on row {worst}")
    for name, v in noise.items():
        assert max(v) < 1e-11, (name, v)


@pytest.mark.parametrize("name", ["4x5x8", "5x5x8"])
def test_oracle_is_continuous_at_the_faces_of_the_box(name):
    """An atom at lamda = -1e-17 (lo - 1e-17 L) wraps to lamda - floor(lamda) = 1.0 in floating point.  The neighbour list then places it at
    lamda 0; its image count must say the same, or its pairs are listed for one image and evaluated for another, a box length away (the
    guard took floor(lamda) as it stood until the GPU tests of the faces found oracle and product wrong in different ways in a tilted
    box, and wrong alike in an orthogonal one).  Against the same atoms 1e-9 of a box length inside the box: a displacement of 1e-8 A
    changes forces of 0.1 kcal/mol/A with gradients of 1 per A by 1e-8 -- asked for: 1e-6 of the largest force; the defect was 0.7."""
    row = BY_NAME[name]
    d = on_faces(row_fixture(row), row.cells)
    lam = to_lamda(d)
    assert (lam < 0.0).any() and (lam == 0.0).any() and (lam == 1.0).any()
    inside = from_lamda(d, np.clip(lam, 1e-9, 1.0 - 1e-9))
    f, e, w, o = oracle_compute(d, row.acc)
    fi, ei, wi, oi = oracle_compute(inside, row.acc)
    assert o.npairs == oi.npairs and o.pppm_grid == row.grid
    assert rel(f, fi) < 1e-6 and abs(e[1] - ei[1]) < 1e-6 * abs(ei[1]) and abs(e[6] - ei[6]) < 1e-6 * abs(ei[6])
