"""The LDS layout of the staged interpolation kernel (csrc/md_pppm_fstride.h, scema_md_pppm_force_strides) without a GPU: the properties
of the stride rule over the staged meshes of test_oracle_pppm_meshes.ROWS plus 12x12x12 and 16x16x24, and what the bank model of
tools/pppm_bank_model.py says about its choices -- on PE-10k with 0.15 A of Gaussian jitter at most 2.6 LDS cycles per wave read
(conflict-free 2.0, the dense layout 6.0; (12, 146) gives 2.46 and (13, 158) 2.43 there, so the cap can be met), and on every staged
row's own fixture never more than the dense layout of that mesh."""
import os
import sys

import numpy as np
import pytest

from test_oracle_pppm_meshes import ROWS, row_fixture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pppm_bank_model as bm  # noqa: E402

LDS_LIMIT = 144 * 1024
STAGED = [r for r in ROWS if r.force == "staged"]
MESHES = sorted({r.grid for r in STAGED} | {(12, 12, 12), (16, 16, 24)})


def strides(grid, budget=0):
    from scema_amd import capi
    return capi.pppm_force_strides(grid, budget)


def dense_of(grid):
    nx, ny, nz = grid
    return nx, nx * ny, 24 * nx * ny * nz


@pytest.mark.parametrize("grid", MESHES, ids=["x".join(map(str, g)) for g in MESHES])
def test_rule_properties(grid):
    nx, ny, nz = grid
    dense = dense_of(grid)
    # the device budget, budgets just around the dense size, and one that leaves room for any pad
    for budget in (0, dense[2], dense[2] + 8, dense[2] + 24 * nz, dense[2] + 24 * nz - 1, 160 * 1024):
        limit = budget if budget > 0 else LDS_LIMIT
        rs, ps, nbytes = strides(grid, budget)
        assert rs >= nx and ps >= rs * ny, (grid, budget, rs, ps)
        assert nbytes == 24 * ps * nz
        if dense[2] <= limit:
            assert nbytes <= limit, (grid, budget, nbytes)
        if (rs, ps) != dense[:2]:
            assert nbytes > dense[2] and nbytes <= limit
        # one more point per plane is the least a padded layout costs: a budget below that keeps the dense strides exactly
        if limit < dense[2] + 24 * nz:
            assert (rs, ps, nbytes) == dense, (grid, budget, rs, ps)


def test_the_dense_size_at_the_device_limit_comes_back_dense():
    assert dense_of((16, 16, 24))[2] == LDS_LIMIT
    assert strides((16, 16, 24)) == dense_of((16, 16, 24))


def test_the_headline_mesh_is_padded_and_keeps_its_workgroups():
    rs, ps, nbytes = strides((12, 12, 12))
    assert (rs, ps) != dense_of((12, 12, 12))[:2]
    assert 160 * 1024 // nbytes == 160 * 1024 // dense_of((12, 12, 12))[2] == 3
    # a mesh whose dense copy leaves no room for a pad beside the workgroups it has resident keeps the dense strides: two copies of
    # 9 x 27 x 14 fill 163 296 of the CU's 163 840 bytes, one more point per plane would leave room for one copy only
    assert 2 * 24 * 9 * 27 * 14 <= 160 * 1024 < 2 * 24 * (9 * 27 + 1) * 14
    assert strides((9, 27, 14), 160 * 1024) == dense_of((9, 27, 14))


def test_model_reproduces_the_pe10k_figures():
    d = bm.pe10k_jitter(0.15, 1234)
    lam = bm.lamda(d)
    assert abs(bm.cycles_per_wave_read((12, 12, 12), (12, 144), lam) - 6.00) < 0.01
    assert abs(bm.cycles_per_wave_read((12, 12, 12), (12, 146), lam) - 2.46) < 0.01
    assert abs(bm.cycles_per_wave_read((12, 12, 12), (12, 160), lam) - 10.0) < 0.01


def test_model_on_pe10k_with_the_rules_choice():
    d = bm.pe10k_jitter(0.15, 1234)
    rs, ps, _ = strides((12, 12, 12))
    got = bm.cycles_per_wave_read((12, 12, 12), (rs, ps), bm.lamda(d), np.asarray(d["charge"]) != 0.0)
    print(f"PE-10k, 0.15 A jitter: ({rs}, {ps}) models at {got:.2f} cycles per wave read")
    assert got <= 2.6, (rs, ps, got)


@pytest.mark.parametrize("row", STAGED, ids=[r.name for r in STAGED])
def test_model_never_above_dense_on_the_rows_own_fixture(row):
    d = row_fixture(row)
    lam, charged = bm.lamda(d), np.asarray(d["charge"]) != 0.0
    rs, ps, _ = strides(row.grid)
    dense = bm.cycles_per_wave_read(row.grid, dense_of(row.grid)[:2], lam, charged)
    got = bm.cycles_per_wave_read(row.grid, (rs, ps), lam, charged)
    print(f"{row.name}: dense {dense:.2f}, ({rs}, {ps}) {got:.2f}")
    assert got <= dense, (row.name, rs, ps, got, dense)
