"""The binned charge assignment of md_pppm.hip (k_pppm_bins + k_pppm_spread_binned: the charged atoms of a replica grouped by nearest
grid point, a lane adds the sum of up to BIN_M atoms with one set of 125 LDS atomics) against the unbinned kernel on the same engine and
against the CPU oracle, on the meshes and fixtures of tests/test_oracle_pppm_meshes.py and tests/test_gpu_pppm_meshes.py.  Every case asserts
through scema_md_pppm_binned_launches that the path it means to test ran, or did not run.  Tolerances, the project's own: 1e-12 of the
largest component between binned and unbinned on one engine (only the order of summation differs: the bound of test_gpu_pppm_tiled.py for
the same situation), 1e-10 against the oracle for static forces, energies and virials, 1e-7 for evaluated stresses against the oracle, 1e-9
between two launch shapes of the engine (stresses of a batch, stored states after MD steps).  The item rule of k_pppm_bins is restated in
numpy below and checked without a GPU, so that the occupancy assertions of the fixtures have something to stand on."""
import functools

import numpy as np
import pytest

from test_gpu_pppm_meshes import (BATCH_ACC, BATCH_MATS, BATCH_T, COUNT_BOXES, assert_batch, assert_mesh, assert_static, batch_material, batch_strain, cut_to,
                                  engine, on_planes, reference, some_uncharged)
from test_oracle_pppm_meshes import BY_NAME, ionic, oracle_compute, rel, row_fixture, from_lamda, to_lamda, min_distance

gpu = pytest.mark.gpu
BIN_M = 4         # md_pppm.hip PP_BIN_M: atoms per item at most
BIN_ROUNDS = 4    # md_pppm.hip PP_BIN_ROUNDS


# ---- the item rule, restated ---------------------------------------------------------------------------------------------------------
def bins_of(d, grid):
    """bin of every atom as k_pppm_bins takes it: nearest grid point floor(u + 1/2), x unwrapped 0 .. nx, y and z mod n; -1: uncharged"""
    nx, ny, nz = grid
    lam = to_lamda(d)
    u = (lam - np.floor(lam)) * np.array(grid, float)
    i = np.floor(u + 0.5).astype(int)
    b = ((i[:, 2] % nz) * ny + i[:, 1] % ny) * (nx + 1) + np.clip(i[:, 0], 0, nx)
    return np.where(np.asarray(d["charge"]) != 0.0, b, -1)


def occupancy(d, grid):
    """charged atoms per bin"""
    b = bins_of(d, grid)
    return np.bincount(b[b >= 0], minlength=(grid[0] + 1) * grid[1] * grid[2])


def item_rule(bins, nbins, M, rounds=BIN_ROUNDS):
    """(perm, items) from the bin of every atom (-1: not listed).  perm: the listed atoms grouped by bin; items: (bin, first, count) in the
    order of the kernel -- round r holds part r of every bin that has one, in bin order; parts from rounds - 1 on share the last round."""
    bins = np.asarray(bins)
    listed = np.nonzero(bins >= 0)[0]
    perm = listed[np.argsort(bins[listed], kind="stable")]
    counts = np.bincount(bins[listed], minlength=nbins)
    start = np.concatenate([[0], np.cumsum(counts)[:-1]])
    per_round = [[] for _ in range(rounds)]
    for b in np.nonzero(counts)[0]:
        for p in range(-(-counts[b] // M)):
            per_round[min(p, rounds - 1)].append((int(b), int(start[b] + p * M), int(min(M, counts[b] - p * M))))
    return perm, [it for r in per_round for it in r]


@pytest.mark.parametrize("M", [2, 4, 8])
def test_item_rule_on_bin_counts(M):
    """item count sum ceil(n_b / M), item sizes 1 .. M that add up to the bin, perm a permutation of the charged atoms grouped by bin; inside
    a round before the last the bins are distinct and ascending (neighbouring lanes: neighbouring points); and with the occupancy of the
    PE crystal and of its jittered form (4 .. 8 and 1 .. 14 atoms per point, every point taken) no group of 64 consecutive items holds
    two items of one bin"""
    rng = np.random.default_rng(11)
    nb_pe = 13 * 12 * 12
    cases = [(np.repeat(np.arange(nb_pe), rng.integers(4, 9, nb_pe)), nb_pe, True), (np.repeat(np.arange(nb_pe), rng.integers(1, 15, nb_pe)), nb_pe, M >= 4)]
    for nbins, natoms, zero_every in [(6 * 5 * 5, 1728, 0), (9 * 8 * 8, 150, 3), (6 * 5 * 8, 40, 2), (6 * 5 * 5, 5, 0)]:
        bins = rng.integers(0, nbins, natoms)
        if zero_every:
            bins[::zero_every] = -1
        cases.append((bins, nbins, False))
    for bins, nbins, apart in cases:
        bins = rng.permutation(bins)
        perm, items = item_rule(bins, nbins, M)
        counts = np.bincount(bins[bins >= 0], minlength=nbins)
        parts = -(-counts // M)
        assert len(items) == int(parts.sum())
        assert sorted(perm.tolist()) == np.nonzero(bins >= 0)[0].tolist()
        assert np.all(np.diff(bins[perm]) >= 0)
        covered = np.zeros(len(perm), int)
        for b, first, n in items:
            assert 1 <= n <= M and np.all(bins[perm[first:first + n]] == b)
            covered[first:first + n] += 1
        assert np.all(covered == 1)
        at = 0
        for r in range(BIN_ROUNDS - 1):
            n_r = int(np.count_nonzero(parts > r))
            assert [b for b, _, _ in items[at:at + n_r]] == np.nonzero(parts > r)[0].tolist()
            at += n_r
        if apart:
            assert parts.max() <= BIN_ROUNDS
            for g in range(0, len(items) - 63):
                group = [b for b, _, _ in items[g:g + 64]]
                assert len(set(group)) == 64, (M, g)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------------
def on_and_off(eng, name, d, eligible=True, label=None):
    """static evaluation of a registered system with the binned kernels off and on (wherever eligible): both results, the launch counter
    checked, the two within 1e-12 of the largest component"""
    eng.register_replica(name, 1, d)
    eng.pppm_binning(0)
    n0 = eng.pppm_binned_launches()
    off = eng.debug_compute(name, 1, use_shake=False)[:3]
    assert eng.pppm_binned_launches() == n0
    eng.pppm_binning(1)
    on = eng.debug_compute(name, 1, use_shake=False)[:3]
    taken = eng.pppm_binned_launches() - n0
    assert (taken > 0) == eligible, (label or name, taken)
    figures = dict(f=rel(on[0], off[0]), e6=abs(on[1][6] - off[1][6]) / abs(off[1][6]), w6=rel(on[2][6], off[2][6]))
    print(f"{label or name}: binned against unbinned " + "  ".join(f"{k} {v:.2e}" for k, v in figures.items()))
    assert max(figures.values()) < 1e-12, (label or name, figures)
    return on, off


@gpu
@pytest.mark.parametrize("name", ["8x8x8", "9x8x6", "5x5x8", "4x4x8"])
def test_small_meshes_of_the_table(name):
    """a cubic mesh, one with three different dimensions, the smallest with nx >= 5 -- and nx = 4, which has no padded rows: the binned
    kernels are not taken and the results are what they were"""
    row = BY_NAME[name]
    d, fo, eo, wo, g = reference(name)
    assert abs(assert_mesh(d, row.acc, row.grid) - g) < 1e-12
    eng = engine(row.acc)
    on, off = on_and_off(eng, "m", d, eligible=row.grid[0] >= 5, label=name)
    assert_static(on, (fo, eo, wo), 1e-10, name + " binned")
    assert_static(off, (fo, eo, wo), 1e-10, name + " unbinned")
    eng.close()


@gpu
def test_a_small_launch_keeps_the_unbinned_kernel_by_default():
    """mode 2, the default: a launch of one replica is far below the policy's launch size (k_pppm_bins is one more launch on a chain of
    dependent launches, which a small batch waits for), so nothing is binned until it is asked for"""
    row = BY_NAME["8x8x8"]
    d, fo, eo, wo, g = reference("8x8x8")
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    got = eng.debug_compute("m", 1, use_shake=False)[:3]
    assert eng.pppm_binned_launches() == 0
    assert_static(got, (fo, eo, wo), 1e-10, "8x8x8 default mode")
    eng.pppm_binning(1)
    eng.debug_compute("m", 1, use_shake=False)
    assert eng.pppm_binned_launches() == 1
    eng.pppm_binning(2)
    eng.debug_compute("m", 1, use_shake=False)
    assert eng.pppm_binned_launches() == 1
    eng.close()


def near_the_wrap(d, grid, dims):
    """the atoms of the last mesh cell of the dimensions `dims` moved to u in [n - 0.45, n - 0.05): their nearest grid point is n, not 0"""
    g = np.array(grid, float)
    lam = to_lamda(d)
    u = (lam - np.floor(lam)) * g
    for k in dims:
        top = u[:, k] >= g[k] - 1.0
        assert top.sum() >= 3, (k, top.sum())
        u[top, k] = g[k] - 0.45 + 0.4 * (u[top, k] - (g[k] - 1.0))
    out = from_lamda(d, u / g)
    un = to_lamda(out) * g
    for k in dims:
        assert np.count_nonzero(np.floor(un[:, k] + 0.5) == grid[k]) >= 3
    assert min_distance(out) > 0.3
    return out


@gpu
@pytest.mark.parametrize("case", ["half_way", "wrap_x", "wrap_yz"])
@pytest.mark.parametrize("name", ["5x5x8", "9x8x6"])
def test_half_planes_and_the_wrap(name, case):
    """atoms half-way between two grid planes in every dimension (the tie of floor(u + 1/2)); atoms whose nearest point is nx -- a column of
    its own in the padded rows, a bin of its own --, and atoms whose nearest point is ny or nz, which share the bin of 0"""
    row = BY_NAME[name]
    d = row_fixture(row, eps=1e-9)
    if case == "half_way":
        d = on_planes(d, row.grid, half=True)
        u = to_lamda(d) * np.array(row.grid, float)
        assert np.abs(u - np.floor(u) - 0.5).max() < 1e-12 and min_distance(d) > 0.3
    else:
        d = near_the_wrap(d, row.grid, (0,) if case == "wrap_x" else (1, 2))
    if case == "wrap_x":
        occ = occupancy(d, row.grid).reshape(row.grid[2], row.grid[1], row.grid[0] + 1)
        assert occ[:, :, row.grid[0]].sum() >= 3
    fo, eo, wo, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid
    eng = engine(row.acc)
    on, _ = on_and_off(eng, "m", d, label=f"{name} {case}")
    assert_static(on, (fo, eo, wo), 1e-10, f"{name} {case} binned")
    eng.close()


@gpu
def test_some_uncharged_atoms():
    """every fourth atom uncharged (not listed in any bin): their forces come out as exactly 0, the rest as the oracle's"""
    row = BY_NAME["9x8x6"]
    d = some_uncharged(row_fixture(row, eps=1e-9))
    zero = np.asarray(d["charge"]) == 0.0
    assert zero.sum() >= d["natoms"] // 4 and np.count_nonzero(bins_of(d, row.grid) < 0) == zero.sum()
    fo, eo, wo, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid
    eng = engine(row.acc)
    on, _ = on_and_off(eng, "m", d, label="9x8x6 some uncharged")
    assert_static(on, (fo, eo, wo), 1e-10, "9x8x6 some uncharged binned")
    assert np.all(on[0][zero] == 0.0)
    eng.close()


@gpu
@pytest.mark.parametrize("n", [2, 63, 65])
def test_fewer_charged_atoms_than_a_wave_and_empty_grid_points(n):
    """the first n atoms of a 5 x 5 x 6 lattice on an 8 x 8 x 8 mesh: 2 and 62 charged atoms (fewer items than the lanes of one wave), and 64
    of them in a slab that leaves most grid points -- whole planes of bins -- empty"""
    c = COUNT_BOXES["8x8x8"]
    d = cut_to(ionic((5, 5, 6), 3.0, c["q"], c["tilt"], seed=3, eps=1e-9), n, c["q"])
    occ = occupancy(d, c["grid"])
    assert occ.sum() == n - n % 2 and occ.sum() <= 64 and np.count_nonzero(occ == 0) > occ.size // 2
    fo, eo, wo, o = oracle_compute(d, c["acc"])
    assert o.pppm_grid == c["grid"]
    eng = engine(c["acc"])
    on, _ = on_and_off(eng, "m", d, label=f"8x8x8 n={n}")
    assert_static(on, (fo, eo, wo), 1e-10, f"8x8x8 n={n} binned")
    eng.close()


FULL = dict(cells=(12, 12, 12), a=1.2, q=0.02, acc=0.1, grid=(5, 5, 5))


@gpu
def test_a_full_bin_makes_three_items_and_more():
    """1 728 atoms on a 5 x 5 x 5 mesh: 14 per grid point in the mean, the fullest bin well beyond 2 BIN_M, so that bins are cut into three
    items and more, and into more parts than there are rounds (the last round then holds several items of one bin)"""
    d = ionic(FULL["cells"], FULL["a"], FULL["q"], seed=5, eps=1e-9)
    grid = FULL["grid"]
    assert_mesh(d, FULL["acc"], grid)
    occ = occupancy(d, grid)
    assert occ.max() > 2 * 8 >= 2 * BIN_M and occ.max() > BIN_M * BIN_ROUNDS and occ.sum() == d["natoms"]
    perm, items = item_rule(bins_of(d, grid), occ.size, BIN_M)
    assert max(np.bincount([b for b, _, _ in items])) >= 3
    fo, eo, wo, o = oracle_compute(d, FULL["acc"])
    assert o.pppm_grid == grid
    eng = engine(FULL["acc"])
    on, _ = on_and_off(eng, "m", d, label="full bins")
    assert_static(on, (fo, eo, wo), 1e-10, "full bins binned")
    eng.close()


# ---- launches of several replicas ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uncharged_material():
    """the 5 x 5 x 5 material of the batches with every charge 0: it has no mesh at all, and its replicas leave the PPPM kernels at once"""
    d = dict(batch_material("batch5"))
    d["charge"] = np.zeros(d["natoms"])
    return d


def run_batch_mode(mats, mode, updates=1):
    """the run_batch of test_gpu_pppm_meshes.py with the binning mode set: (stresses [update, request, 6], binned launches)"""
    from scema_amd import capi
    eng = engine(BATCH_ACC, neigh_delay=0)
    names = sorted(set(mats))
    for name in names:
        eng.register_replica(name, 1, uncharged_material() if name == "neutral" else batch_material(name))
    eng.pppm_binning(mode)
    out = []
    for u in range(updates):
        sims = [capi.make_sim(q, name, 1, batch_strain(batch_material("batch5" if name == "neutral" else name), q, 1.0 if u == 0 else -1.0), nss=10,
                              temperature=BATCH_T, most_recent=capi.QP_NONE if u == 0 else None, material=names.index(name)) for q, name in enumerate(mats)]
        out.append(np.array([list(o.stress) for o in eng.strain_batch(sims)]))
    n = eng.pppm_binned_launches()
    eng.close()
    return np.array(out), n


def between_modes(mats, label, eligible=True, updates=1):
    off, n_off = run_batch_mode(mats, 0, updates)
    on, n_on = run_batch_mode(mats, 1, updates)
    assert n_off == 0 and (n_on > 0) == eligible, (label, n_off, n_on)
    dev = max(np.abs(on[u, q] - off[u, q]).max() / np.abs(off[u, q]).max() for u in range(updates) for q in range(len(mats)))
    print(f"{label}: binned against unbinned {dev:.2e} ({n_on} binned launches)")
    assert np.isfinite(on).all() and dev < 1e-9, (label, dev)
    return on


@gpu
def test_two_padded_meshes_in_one_launch():
    """5 x 5 x 5 and 12 x 15 x 15 in one whole launch, both eligible: bins of two sizes in LDS of one size"""
    mats = ("batch600", "batch5", "batch5", "batch600")
    on = between_modes(mats, "5^3 + 12x15x15")
    assert_batch(on, mats, "5^3 + 12x15x15 binned")


@gpu
def test_a_launch_with_a_mesh_that_is_not_eligible_keeps_the_unbinned_kernel():
    """one replica with nx = 4 among eligible ones: no replica of the launch spreads on padded rows, so none is binned"""
    mats = ("batch4", "batch600", "batch5", "batch4", "batch5", "batch600")
    on = between_modes(mats, "4^3 + 5^3 + 12x15x15", eligible=False)
    assert_batch(on, mats, "4^3 + 5^3 + 12x15x15, binning asked for")


@gpu
def test_a_replica_without_any_charge_beside_charged_ones():
    """a replica whose atoms are all uncharged has no mesh: k_pppm_bins and the spreading kernel skip it, its neighbours in the launch are binned"""
    mats = ("neutral", "batch5", "batch600", "neutral")
    on = between_modes(mats, "charged + uncharged replicas")
    alone = between_modes(("neutral",), "an uncharged replica alone", eligible=False)   # (request 0 in both: the same strain)
    assert np.abs(on[0, 0] - alone[0, 0]).max() < 1e-9 * np.abs(alone[0, 0]).max()


@gpu
def test_twelve_replicas_in_part_batches_over_two_updates():
    """twelve requests over the two padded meshes run as four part batches of three on streams of their own, each with its own k_pppm_bins,
    and a second update continues their states"""
    mats = tuple(("batch5", "batch600")[(q + q // 3) % 2] for q in range(12))
    between_modes(mats, "twelve requests in parts, two updates", updates=2)


@gpu
def test_stored_states_after_ten_steps():
    """ten MD steps of one small replica with the binned kernels on and off: the bins follow the positions of every step (nothing is kept from
    the step before), and the stored states agree to 1e-9"""
    d = batch_material("batch5")
    states = {}
    for mode in (0, 1):
        eng = engine(BATCH_ACC, neigh_delay=0)
        eng.register_replica("m", 1, d)
        eng.pppm_binning(mode)
        eng.set_state(3, "m", 1, d["box"], d["x"], d["v"])
        eng.debug_run("m", 1, 10, 2.0, BATCH_T, qp=3, nvt=True, use_shake=False)
        n = eng.pppm_binned_launches()
        assert (n >= 10) if mode else (n == 0), (mode, n)
        states[mode] = eng.get_state(3, "m", 1)
        eng.close()
    (b0, x0, v0), (b1, x1, v1) = states[0], states[1]
    moved = np.abs(x0 - d["x"]).max()
    print(f"ten steps: x {np.abs(x1 - x0).max():.2e} (moved {moved:.2e})  v {rel(v1, v0):.2e}")
    assert moved > 1e-3 and np.array_equal(b0, b1)
    assert np.abs(x1 - x0).max() < 1e-9 * max(1.0, np.abs(x0).max()) and rel(v1, v0) < 1e-9
