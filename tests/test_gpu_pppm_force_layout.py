"""The LDS layout of the staged interpolation kernel (k_pppm_force<true, *> of md_pppm.hip with the strides of md_pppm_fstride.h) against
the dense layout on the same engine (scema_md_pppm_force_layout 1 / 0) and against the CPU oracle, on the meshes and fixtures of
tests/test_oracle_pppm_meshes.py and tests/test_gpu_pppm_meshes.py.

Tolerances, the project's own: 1e-12 of the largest component between the two layouts on one engine (the figure of test_gpu_pppm_tiled.py
between two forms of one kernel; the interpolation runs the same arithmetic in both, what differs from run to run is the order of the
spreading kernel's atomics), the row's own tolerance against the oracle (1e-10), 1e-7 for evaluated stresses against the oracle and 1e-9
between two runs of a batch over MD steps (test_gpu_pppm_meshes.py, test_gpu_pppm_binned.py).

Meshes, the smallest at which the stride logic can go wrong: 4x4x8 (nx ny = 16: every second plane on the same banks), 8x4x4 and 8x8x8
(nx ny a multiple of 32), 3x3x3 (every index wraps twice), 5x5x15 (odd), 12x10x24 (the largest in-LDS solve), 15x16x15 (staged from the
complex hipFFT grids), batch600 (two atom ranges per replica).  The rule keeps the dense strides where a dimension has five points or
fewer; PADDED names the rows on which it must not, so that the comparison is one of two layouts."""
import numpy as np
import pytest

from test_gpu_pppm_meshes import (BATCH_ACC, BATCH_MATS, BATCH_T, assert_batch, assert_mesh, assert_static, batch_material, batch_strain, engine,
                                  reference, some_uncharged)
from test_oracle_pppm_meshes import BY_NAME, oracle_compute, rel, row_fixture

pytestmark = pytest.mark.gpu
STAGED = 0
MESHES = ("4x4x8", "8x4x4", "8x8x8", "3x3x3", "5x5x15", "12x10x24", "15x16x15", "batch600")
PADDED = ("8x8x8", "12x10x24", "15x16x15", "batch600")


def strides(grid, budget=0):
    from scema_amd import capi
    return capi.pppm_force_strides(grid, budget)


def dense_of(grid):
    return grid[0], grid[0] * grid[1], 24 * grid[0] * grid[1] * grid[2]


def both_layouts(eng, name, label):
    """a static evaluation of a registered system under the rule and under the dense layout: (rule, dense), the two within 1e-12 of the
    largest component, both through the staged kernel"""
    out = {}
    for mode in (1, 0):
        eng.pppm_force_layout(mode)
        f, e, w, info = eng.debug_compute(name, 1, use_shake=False)
        assert info["nk"] == 0 and eng.pppm_paths()["force"] == STAGED, eng.pppm_paths()
        out[mode] = (f, e, w)
    (f1, e1, w1), (f0, e0, w0) = out[1], out[0]
    fig = dict(f=rel(f1, f0), e6=abs(e1[6] - e0[6]) / abs(e0[6]), w6=rel(w1[6], w0[6]), e1=abs(e1[1] - e0[1]) / max(1e-300, abs(e0[1])))
    print(f"{label}: rule against dense " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert np.isfinite(f1).all() and max(fig.values()) < 1e-12, (label, fig)
    return out[1], out[0]


@pytest.mark.parametrize("name", MESHES)
def test_rule_against_dense_and_oracle(name):
    row = BY_NAME[name]
    d, fo, eo, wo, g = reference(name)
    assert abs(assert_mesh(d, row.acc, row.grid) - g) < 1e-12
    rs, ps, nbytes = strides(row.grid)
    assert ((rs, ps) != dense_of(row.grid)[:2]) == (name in PADDED), (name, rs, ps)
    if name == "batch600":
        assert d["natoms"] // 256 == 2      # two atom ranges: two workgroups stage the padded copy
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    rule, dense = both_layouts(eng, "m", f"{name} ({rs}, {ps})")
    assert_static(rule, (fo, eo, wo), row.tol, f"{name} rule")
    assert_static(dense, (fo, eo, wo), row.tol, f"{name} dense")
    eng.close()


def test_default_is_the_rule_and_refuses_other_modes():
    from scema_amd import capi
    row = BY_NAME["8x8x8"]
    d, fo, eo, wo, g = reference("8x8x8")
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    got = eng.debug_compute("m", 1, use_shake=False)[:3]
    assert_static(got, (fo, eo, wo), row.tol, "8x8x8 default layout")
    for mode in (2, -2):
        with pytest.raises(capi.EngineError):
            eng.pppm_force_layout(mode)
    eng.pppm_force_layout(0)
    eng.pppm_force_layout(-1)
    eng.close()


def test_a_budget_between_the_dense_and_the_padded_copy_keeps_the_dense_layout():
    """8 x 8 x 8: 12 288 bytes dense, 12 864 at the rule's plane stride of 67.  Under a forced budget of 12 400 bytes the rule answers with the
    dense strides, the launch takes the same kernels as under mode 0 and gives the same numbers"""
    row = BY_NAME["8x8x8"]
    budget = 12400
    assert strides(row.grid)[2] > budget >= dense_of(row.grid)[2] and strides(row.grid, budget) == dense_of(row.grid)
    d, fo, eo, wo, g = reference("8x8x8")
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    eng.pppm_tiling(-1, budget)
    paths = {}
    out = {}
    for mode in (1, 0):
        eng.pppm_force_layout(mode)
        out[mode] = eng.debug_compute("m", 1, use_shake=False)[:3]
        paths[mode] = eng.pppm_paths()
    assert paths[1] == paths[0] and paths[1]["force"] == STAGED and paths[1]["lds_bytes"] == budget, paths
    fig = dict(f=rel(out[1][0], out[0][0]), e6=abs(out[1][1][6] - out[0][1][6]) / abs(out[0][1][6]), w6=rel(out[1][2][6], out[0][2][6]))
    print("8x8x8 at 12 400 B: " + "  ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    assert max(fig.values()) < 1e-12, fig
    assert_static(out[1], (fo, eo, wo), row.tol, "8x8x8 at 12 400 B")
    eng.close()


def test_uncharged_atoms_get_exact_zeros():
    """every fourth atom uncharged, no LJ, on the padded 12 x 15 x 15 mesh: the single replica's chain STORES its forces, an uncharged atom
    comes out with exactly 0 in both layouts"""
    row = BY_NAME["batch600"]
    d = some_uncharged(row_fixture(row, eps=1e-9))
    fo, eo, wo, o = oracle_compute(d, row.acc)
    assert o.pppm_grid == row.grid and strides(row.grid)[:2] != dense_of(row.grid)[:2]
    eng = engine(row.acc)
    eng.register_replica("m", 1, d)
    rule, dense = both_layouts(eng, "m", "batch600 some uncharged")
    assert_static(rule, (fo, eo, wo), 1e-10, "batch600 some uncharged, rule")
    zero = np.asarray(d["charge"]) == 0.0
    assert zero.sum() >= d["natoms"] // 4 and np.all(rule[0][zero] == 0.0) and np.all(dense[0][zero] == 0.0)
    eng.close()


def run_requests(register, sims_of, mode, updates=1):
    eng = engine(BATCH_ACC, neigh_delay=0)
    register(eng)
    eng.pppm_force_layout(mode)
    out = []
    for u in range(updates):
        out.append(np.array([list(o.stress) for o in eng.strain_batch(sims_of(u))]))
    info = dict(paths=eng.pppm_paths(), split=eng.concurrency()["split"])
    eng.close()
    return np.array(out), info


def test_uncharged_atoms_keep_their_forces_where_the_chain_adds():
    """nine requests run as three part batches whose PPPM chains ADD to the assembled forces (add = 1): uncharged atoms, here with LJ, keep
    theirs.  The rule against the dense layout, the project's 1e-9 between two runs of a batch over MD steps."""
    from scema_amd import capi
    row = BY_NAME["batch600"]
    d = some_uncharged(row_fixture(row, eps=0.1))
    d["eps"] = np.array([[0.1]])
    assert_mesh(d, BATCH_ACC, row.grid)
    got = {}
    for mode in (1, 0):
        got[mode], info = run_requests(lambda eng: eng.register_replica("u", 1, d),
                                       lambda u: [capi.make_sim(q, "u", 1, batch_strain(d, q), nss=10, temperature=BATCH_T, most_recent=capi.QP_NONE)
                                                  for q in range(9)], mode)
        assert info["paths"]["force"] == STAGED and info["split"] == 1, info
    dev = max(np.abs(got[1][0, q] - got[0][0, q]).max() / np.abs(got[0][0, q]).max() for q in range(9))
    print(f"uncharged atoms, chain adds: rule against dense {dev:.2e}")
    assert np.isfinite(got[1]).all() and dev < 1e-9, dev


def test_three_meshes_in_one_whole_launch():
    """4 x 4 x 4, 5 x 5 x 5 (dense by the rule) and 12 x 15 x 15 (plane stride 183) interleaved in one launch: the LDS of the launch is the
    largest PADDED copy, 65 880 bytes, not the largest mesh's 64 800 -- against the oracle and against the dense layout"""
    from scema_amd import capi
    mats = ("batch4", "batch600", "batch5", "batch4", "batch5", "batch600")
    sizes = {name: strides(BY_NAME[name].grid)[2] for name in BATCH_MATS}
    assert max(sizes.values()) == sizes["batch600"] == 65880 > dense_of(BY_NAME["batch600"].grid)[2]
    assert all(strides(BY_NAME[n].grid) == dense_of(BY_NAME[n].grid) for n in ("batch4", "batch5"))

    def register(eng):
        for name in BATCH_MATS:
            eng.register_replica(name, 1, batch_material(name))

    def sims_of(u):
        return [capi.make_sim(q, name, 1, batch_strain(batch_material(name), q), nss=10, temperature=BATCH_T, most_recent=capi.QP_NONE,
                              material=BATCH_MATS.index(name)) for q, name in enumerate(mats)]

    got = {}
    for mode in (1, 0):
        got[mode], info = run_requests(register, sims_of, mode)
        assert info["paths"]["force"] == STAGED, info
    assert_batch(got[1], mats, "4^3 + 5^3 + 12x15x15, rule")
    dev = max(np.abs(got[1][0, q] - got[0][0, q]).max() / np.abs(got[0][0, q]).max() for q in range(len(mats)))
    print(f"three meshes in one launch: rule against dense {dev:.2e}")
    assert dev < 1e-9, dev
