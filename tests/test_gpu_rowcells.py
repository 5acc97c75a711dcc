"""The cell-binned row build of the row potentials (md_rowcells.hip, md_rowcells.h, engine_rowpot.cpp) on the GPU: its rows
against those of the N^2 build (k_row_build) entry for entry, and everything computed from them.  SCEMA_MD_ROW_CELLS is read when an engine
is created: 1 takes the cell path wherever the geometry allows it, 0 never, unset from the size threshold.

"Rows identical" (rows_identical): debug_rows of the two engines gives equal counts and equal rows[i][:cnt[i]] as integers, the entries of
a row ascend in their atom index, and the path flag is 1 and 0.  Where rows are identical the embedded-atom and the angular-dependent
stage, which have no atomic on a force, must return the same forces to the bit (their energies and virial, atomic sums: same_bits); the stages that sum
forces with atomics are held to the standing static budget (1e-10 of the largest force component, 1e-9 of energy and virial:
tests/test_gpu_sw.py).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import eam_numpy as en
import rowkit as rk
import sw_numpy as swn
import tersoff_numpy as tsn
import vashishta_numpy as vn
from scema_amd import capi
from test_gpu_eam import CUAG as CUAG_EAM, EAM
from test_gpu_sw import SW

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# kind -> potential file, elements, masses
KINDS = {"sw": ("Si.sw", ("Si",), (28.0855,)), "eam": ("CuAg.eam.alloy", ("Cu",), (en.CU_MASS,)), "tersoff": ("SiC.tersoff", ("Si",), (28.0855,)),
         "tersoff_mod": ("Si.tersoff.mod", ("Si",), (28.0855,)), "tersoff_zbl": ("SiC.tersoff.zbl", ("Si", "C"), (28.0855, 12.011)),
         "vashishta": ("SiC.vashishta", ("Si", "C"), (28.0855, 12.011)), "adp": ("CuAg.adp", ("Cu", "Ag"), (en.CU_MASS, en.AG_MASS))}


def set_cells(mp, cells):
    if cells is None:
        mp.delenv("SCEMA_MD_ROW_CELLS", raising=False)
    else:
        mp.setenv("SCEMA_MD_ROW_CELLS", str(cells))


def engine(mp, cells, kind="eam", systems=(), matid="m"):
    """an engine created under the switch, the potential attached, systems = [(replica, x, box, t, v)] registered"""
    set_cells(mp, cells)
    e = capi.Engine(capi.default_params())
    path, el, masses = KINDS[kind]
    getattr(e, kind + "_configure")(matid, os.path.join(G, path), el)
    for rep, x, box, t, v in systems:
        e.register_replica(matid, rep, capi.bare_system(t, x, box, v=v, masses=masses))
    return e


def static(mp, kind, case, cells):
    """the static evaluation of a case under the switch, with the rows it was computed from and the profile"""
    x, box, t = case
    e = engine(mp, cells, kind, [(1, x, box, t, None)])
    try:
        out = getattr(e, kind + "_compute")("m", 1)
        out["rows"] = e.debug_rows(0)
        out["prof"] = e.profile()
        return out
    finally:
        e.close()


def rows_identical(on, off):
    a, b = on["rows"], off["rows"]
    assert (a["cells"], b["cells"]) == (1, 0), (a["cells"], b["cells"], a["ncell"])
    assert min(a["ncell"]) >= 3 and b["ncell"] == [0, 0, 0]
    assert a["n"] == b["n"] and a["cap"] == b["cap"]
    assert np.array_equal(a["cnt"], b["cnt"]), np.nonzero(a["cnt"] != b["cnt"])[0][:8]
    live = np.arange(a["cap"])[None, :] < a["cnt"][:, None]
    assert np.array_equal(a["rows"][live], b["rows"][live])
    key = a["rows"] & 0xFFFFFF
    assert (np.diff(key, axis=1)[live[:, 1:]] > 0).all()
    assert a["cnt"].max() <= a["cap"] and a["cnt"].sum() > 0
    assert on["prof"]["row_cell_builds"] == on["prof"]["neigh_builds"] >= 1 and off["prof"]["row_cell_builds"] == 0


def energies(d):
    return [k for k, v in d.items() if isinstance(v, float)]


def same_bits(a, b):
    """Forces bit for bit; energies and virial at the standing budget (1e-9).  The one departure from "forces, energies and virial bit for
    bit": the energies and the virial of the embedded-atom and the angular-dependent stage are sums over workgroups by atomic adds in the
    order of arrival (block_atomic_add_n into RowView::eacc and the engine's virial), so they do not repeat their bits from one evaluation
    to the next on EITHER path.  Measured on the MI355X, 12 evaluations per path of the 306-atom case of
    test_atoms_on_the_box_origin_on_cell_faces_and_below_hi and of 864 copper atoms: rows and forces identical in all 48 evaluations; 12
    distinct (energies, virial) tuples of 12 on the N^2 path in both cases, 10 and 12 of 12 on the cell path; largest relative
    difference of e_embed 4.1e-16.  An assertion of equal bits on those sums fails now and then with nothing wrong (an earlier version
    of this file asserted them whenever two N^2 evaluations happened to agree, and failed that way)."""
    assert np.array_equal(a["f"], b["f"]) and np.abs(a["f"]).max() > 0.0 and a["npairs"] == b["npairs"]
    es, ws = max(abs(b[k]) for k in energies(b)), np.abs(b["w"]).max()
    assert max(abs(a[k] - b[k]) for k in energies(b)) <= 1e-9 * es and np.abs(a["w"] - b["w"]).max() <= 1e-9 * ws


def within_budget(a, b, what):
    fs, ws = np.abs(b["f"]).max(), np.abs(b["w"]).max()
    es = max(abs(b[k]) for k in energies(b))
    df, dw = np.abs(a["f"] - b["f"]).max(), np.abs(a["w"] - b["w"]).max()
    de = max(abs(a[k] - b[k]) for k in energies(b))
    print(f"{what}: cells on against off: force {df / fs:.2e}, energy {de / es:.2e}, virial {dw / ws:.2e}")
    assert fs > 0.0 and df <= 1e-10 * fs and de <= 1e-9 * es and dw <= 1e-9 * ws and a["npairs"] == b["npairs"]


def on_and_off(mp, kind, case, what, bits):
    on, off = static(mp, kind, case, 1), static(mp, kind, case, 0)
    rows_identical(on, off)
    if bits:
        same_bits(on, off)
    else:
        within_budget(on, off, what)
    return on, off


def jitter(x, seed, amp=0.1):
    return x + np.random.default_rng(seed).uniform(-amp, amp, x.shape)


def cu(nx, ny, nz, seed=3):
    x, box = en.fcc(nx, ny, nz, en.A_CU)
    return jitter(x, seed), box, en.zeros(len(x))


def si(n, seed=5, a=None):
    x, box = swn.diamond(n, n, n, swn.si_lattice_constant() if a is None else a)
    return jitter(x, seed), box, np.zeros(len(x), int)


# ---- 1. the smallest eligible shapes ----

def test_si216_sw_three_cells_per_dimension(monkeypatch):
    """216 silicon atoms, list radius 4.77 A in a 16.3 A box: 3 x 3 x 3 cells, the stencil is the whole box"""
    case = si(3)
    on, off = on_and_off(monkeypatch, "sw", case, "sw 216", bits=False)
    assert on["rows"]["n"] == 216 and on["rows"]["ncell"] == [3, 3, 3]
    ref = swn.SW(swn.read_sw(os.path.join(G, "Si.sw"), ["Si"])[0]).compute(*case)
    rk.check_static(on, ref, SW, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, what="sw static")      # (the static budget of tests/test_gpu_sw.py)


@pytest.fixture(scope="module")
def cu864():
    case = cu(6, 6, 6)
    return case, en.EAM(en.read_setfl(CUAG_EAM, ["Cu"])[0]).compute(*case)


def test_cu864_eam(monkeypatch, cu864):
    case, ref = cu864
    on, _ = on_and_off(monkeypatch, "eam", case, "eam 864", bits=True)
    assert on["rows"]["n"] == 864 and on["rows"]["ncell"] == [3, 3, 3]
    rk.check_static(on, ref, EAM, tol_f=1e-10, tol_e=1e-10, tol_w=1e-10, what="eam 864 atoms through cells")      # (that of tests/test_gpu_eam.py)


def test_cu1920_a_grid_of_3_4_5_cells(monkeypatch):
    """6 x 8 x 10 cells: a transposed cell index would show"""
    on, _ = on_and_off(monkeypatch, "eam", cu(6, 8, 10), "eam 1920", bits=True)
    assert on["rows"]["n"] == 1920 and on["rows"]["ncell"] == [3, 4, 5]


# ---- 2. every stage once, at its smallest shape that gives 3 cells ----

def sic(n, seed):
    x, box, t = vn.case_jitter(n, seed)
    return x, box, t


def alloy864():
    x, box, _ = cu(6, 6, 6, seed=8)
    s = 3.85 / en.A_CU
    return x * s, box * s, np.random.default_rng(9).integers(0, 2, len(x))


# (case, bit for bit, cells per dimension: 2 x 2 x 2 cells of silicon are 10.9 A wide, under three list radii of every form, and 3 x 3 x 3 cells,
# 16.3 A, are four radii of 4.0 A of plain Tersoff; the others are the smallest replica with three cells)
STAGES = {"tersoff": (lambda: si(3, 6, tsn.A_SI), False, 4), "tersoff_mod": (lambda: si(3, 7, tsn.A_SI), False, 3), "tersoff_zbl": (lambda: sic(3, 8), False, 3),
          "vashishta": (lambda: sic(6, 9), False, 3), "adp": (alloy864, True, 3)}


@pytest.mark.parametrize("kind", sorted(STAGES))
def test_every_stage_once(monkeypatch, kind):
    make, bits, ncell = STAGES[kind]
    case = make()
    on, _ = on_and_off(monkeypatch, kind, case, kind, bits)
    assert on["rows"]["ncell"] == [ncell] * 3
    if kind in ("tersoff_zbl", "vashishta", "adp"):
        assert len(set(case[2])) == 2


# ---- 3. geometry ----

@pytest.mark.parametrize("sign", [+1, -1])
def test_tilted_copper(monkeypatch, sign):
    """xy = +-0.4 lx on 6 x 6 x 6 cells: the width across x is lx / sqrt(1.16) = 20.1 A, three list radii and a little"""
    x, box, t = cu(6, 6, 6, seed=12)
    lx, ly = box[3] - box[0], box[4] - box[1]
    box = box.copy()
    box[6] = sign * 0.4 * lx
    x = x.copy()
    x[:, 0] += box[6] * x[:, 1] / ly
    on, _ = on_and_off(monkeypatch, "eam", (x, box, t), f"eam tilted {sign:+d}", bits=True)
    assert on["rows"]["ncell"] == [3, 3, 3]
    assert lx / math.sqrt(1.16) < 4 * 6.5 and (lx - en.A_CU) / math.sqrt(1.16) < 3 * 6.5      # one cell fewer along x would not do


def gas300(box_len=40.0, seed=2):
    box = np.array([0.0, 0.0, 0.0, box_len, box_len, box_len, 0.0, 0.0, 0.0])
    return en.gas(300, box, 2.0, seed), box, en.zeros(300)


def test_gas_in_a_wide_box(monkeypatch):
    """300 atoms in 216 cells: empty cells, cells of one atom, ragged rows that outgrow the first capacity"""
    on, _ = on_and_off(monkeypatch, "eam", gas300(), "eam gas", bits=True)
    assert on["rows"]["ncell"] == [6, 6, 6] and on["rows"]["cnt"].min() < 3 < on["rows"]["cnt"].max()


def test_cluster_in_one_corner(monkeypatch):
    """108 atoms across the corner of a 40 A box: every other cell is empty, the stencil wraps in all three dimensions"""
    x, _, t = cu(3, 3, 3, seed=14)
    box = np.array([0.0, 0.0, 0.0, 40.0, 40.0, 40.0, 0.0, 0.0, 0.0])
    on, _ = on_and_off(monkeypatch, "eam", (x - 4.0, box, t), "eam corner cluster", bits=True)
    assert on["rows"]["ncell"] == [6, 6, 6]


def test_atoms_on_the_box_origin_on_cell_faces_and_below_hi(monkeypatch):
    """a 39 A box is six list radii wide to the bit: cell faces at multiples of 6.5 A"""
    x, box, t = gas300(39.0, seed=4)
    assert 39.0 / 6.5 == 6.0
    below = float(np.nextafter(39.0, 0.0))
    put = np.array([[0.0, 0.0, 0.0], [below, 13.0, 13.0], [13.0, below, below], [6.5, 6.5, 6.5], [13.0, 19.5, 26.0], [32.5, 3.0, 6.5], [19.5, 19.5, below]])
    d = x[:, None, :] - put[None, :, :]
    d -= 39.0 * np.rint(d / 39.0)
    x = np.vstack([put, x[(np.einsum("ijk,ijk->ij", d, d) > 4.0).all(axis=1)]])
    # Cells exactly one list radius wide: a pair exactly at the list radius could lie two cells apart, where the N^2 build keeps it
    # (!(r2 > rl2)) and the stencil does not reach it.  This case holds no such pair: none within 1e-9 of the list radius.
    dd = x[:, None, :] - x[None, :, :]
    dd -= 39.0 * np.rint(dd / 39.0)
    r = np.sqrt(np.einsum("ijk,ijk->ij", dd, dd))
    assert np.abs(r - 6.5).min() > 1e-9 * 6.5
    on, _ = on_and_off(monkeypatch, "eam", (x, box, en.zeros(len(x))), "eam faces", bits=True)
    assert on["rows"]["ncell"] == [6, 6, 6] and on["rows"]["cnt"][:7].sum() > 0


@pytest.mark.parametrize("n", [861, 865])
def test_atom_counts_off_the_tile(monkeypatch, n):
    """three vacancies; one interstitial at an octahedral site: n is no multiple of 64 or 16"""
    x, box, t = cu(6, 6, 6, seed=15)
    if n == 861:
        x = np.delete(x, [5, 400, 863], axis=0)
    else:
        x = np.vstack([x, np.array([[2.5 * en.A_CU, 3.0 * en.A_CU, 3.0 * en.A_CU]])])
    on, _ = on_and_off(monkeypatch, "eam", (x, box, en.zeros(len(x))), f"eam {n}", bits=True)
    assert on["rows"]["n"] == n


# ---- 4. fallbacks: the N^2 build where the geometry does not allow cells, or the size does not warrant them ----

FALLBACKS = {"cu500_under_three_radii": lambda: cu(5, 5, 5), "two_wide_one_narrow": lambda: cu(6, 6, 4), "two_images_deep": en.case_cell4}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_ineligible_geometry_takes_the_n2_build(monkeypatch, name):
    case = FALLBACKS[name]()
    on, off = static(monkeypatch, "eam", case, 1), static(monkeypatch, "eam", case, 0)
    for r in (on, off):
        assert r["rows"]["cells"] == 0 and r["rows"]["ncell"] == [0, 0, 0] and r["prof"]["row_cell_builds"] == 0
    assert np.array_equal(on["rows"]["cnt"], off["rows"]["cnt"]) and np.array_equal(on["rows"]["rows"], off["rows"]["rows"])
    same_bits(on, off)


def test_unset_switch_below_the_threshold(monkeypatch):
    """216 silicon atoms are eligible (test_si216_sw_three_cells_per_dimension) and fewer than the threshold"""
    r = static(monkeypatch, "sw", si(3), None)
    assert r["rows"]["cells"] == 0 and r["prof"]["row_cell_builds"] == 0


# ---- 5. overflow ----

def test_row_overflow_on_the_cell_path_regrows_and_retries(monkeypatch, cu864):
    case, _ = cu864
    normal = static(monkeypatch, "eam", case, 1)
    monkeypatch.setenv("SCEMA_MD_NEIGH_GROW0", "0.05")
    got = static(monkeypatch, "eam", case, 1)
    monkeypatch.delenv("SCEMA_MD_NEIGH_GROW0")
    assert got["rows"]["cells"] == 1 and got["prof"]["row_cell_builds"] >= 2             # the failed attempt and the retry
    assert got["rows"]["cap"] == got["rowcap"] < normal["rowcap"] and got["maxrow"] <= got["rowcap"]   # grown to what the rows asked for
    assert np.array_equal(got["rows"]["cnt"], normal["rows"]["cnt"])
    live = np.arange(got["rows"]["cap"])[None, :] < got["rows"]["cnt"][:, None]
    live_n = np.arange(normal["rows"]["cap"])[None, :] < normal["rows"]["cnt"][:, None]
    assert np.array_equal(got["rows"]["rows"][live], normal["rows"]["rows"][live_n])
    same_bits(got, normal)


# ---- 6. dynamics ----

def velocities(n, temp, seed, mass=en.CU_MASS):
    v = np.random.default_rng(seed).normal(size=(n, 3)) * math.sqrt(en.BOLTZ * temp / mass / en.MVV2E)
    return v - v.mean(axis=0)


def nve(mp, case, v, cells, nsteps=60):
    x, box, t = case
    e = engine(mp, cells, "eam", [(1, x, box, t, v)])
    try:
        e.set_state(0, "m", 1, box, x, v)
        e.debug_run("m", 1, nsteps, 1.0, 300.0, qp=0, nvt=False, use_shake=False)
        _, xg, vg = e.get_state(0, "m", 1)
        return xg, vg, e.profile(), e.debug_rows(0, rows=False)
    finally:
        e.close()


def test_nve_with_rebuilds_in_mid_run(monkeypatch, cu864):
    """864 copper atoms started at 3 000 K: the fastest cross half the skin within the run, so the rows are rebuilt through cells"""
    case, _ = cu864
    v = velocities(864, 3000.0, 21)
    x0, v0, p0, r0 = nve(monkeypatch, case, v, 0)
    x1, v1, p1, r1 = nve(monkeypatch, case, v, 0)
    xc, vc, pc, rc = nve(monkeypatch, case, v, 1)
    assert (r0["cells"], rc["cells"]) == (0, 1)
    assert pc["row_cell_builds"] >= 2 and pc["row_cell_builds"] == pc["neigh_builds"] == p0["neigh_builds"] and p0["row_cell_builds"] == 0
    dx, dv = np.abs(xc - x0).max(), np.abs(vc - v0).max()
    print(f"eam nve 60 steps, {pc['neigh_builds']} builds: cells on against off {dx:.2e} A, {dv:.2e} A/fs")
    if np.array_equal(x0, x1) and np.array_equal(v0, v1):      # the N^2 path repeats itself to the bit: so must the cell path
        assert np.array_equal(xc, x0) and np.array_equal(vc, v0)
    else:
        assert dx <= 1e-12 and dv <= 1e-14


def sheared_update(mp, cells):
    """10 x 6 x 6 cells (1 440 atoms) written with xy = 4 a = 0.4 lx, sheared by 0.11 lx: crosses lx / 2 and flips once.  Not the 864-atom
    replica of the other dynamics tests: sheared to xy = lx / 2 its width across x is 21.69 / sqrt(1.25) = 19.4 A, under three list radii
    (19.5 A), and BoxRange::w takes the narrowest box of the run, so that replica would run on the N^2 build and test nothing here; ten
    cells along x keep four cells at the flip."""
    x, box = en.fcc(10, 6, 6, en.A_CU)
    box[6] = 4.0 * en.A_CU
    x = jitter(x, 23, 0.05)
    lx, ly, lz = box[3:6] - box[:3]
    e = engine(mp, cells, "eam", [(1, x, box, en.zeros(len(x)), velocities(len(x), 300.0, 24))])
    try:
        sim = capi.make_sim(0, "m", 1, np.array([0.0, 0.0, 0.0, 0.11 * lx * lz / ly, 0.0, 0.0]), nss=10, dt=1.0, temperature=300.0, strain_rate=3.4e-3,
                            most_recent=capi.QP_NONE)
        return np.array(e.strain_batch([sim])[0].stress[:]), e.profile(), e.debug_rows(0, rows=False)
    finally:
        e.close()


def test_sheared_update_that_flips_its_box(monkeypatch):
    s1, p1, r1 = sheared_update(monkeypatch, 1)
    s0, p0, r0 = sheared_update(monkeypatch, 0)
    assert (r1["cells"], r0["cells"]) == (1, 0) and min(r1["ncell"]) >= 3
    assert p1["box_flips"] == p0["box_flips"] == 1 and p1["neigh_builds"] == p0["neigh_builds"] and p1["row_cell_builds"] == p1["neigh_builds"]
    err = np.abs(s1 - s0).max() / np.abs(s0).max()
    print(f"eam sheared update of 1 440 atoms: cells on against off {err:.2e}, builds {p1['neigh_builds']}")
    assert err <= 1e-9


def test_kept_rows_on_both_paths(monkeypatch, cu864):
    """a small strain at 10 K: the straining run builds once and the sampling run behind it keeps the list, on either path"""
    (x, box, t), _ = cu864
    L = box[3:6] - box[:3]
    res = []
    for cells in (1, 0):
        e = engine(monkeypatch, cells, "eam", [(1, x, box, t, velocities(864, 10.0, 25))])
        try:
            sim = capi.make_sim(0, "m", 1, np.array([1e-3 * L[0], 0.0, 0.0, 0.0, 0.0, 0.0]), nss=10, dt=1.0, temperature=10.0, strain_rate=1e-4, most_recent=capi.QP_NONE)
            res.append((np.array(e.strain_batch([sim])[0].stress[:]), e.profile(), e.debug_rows(0, rows=False)["cells"]))
        finally:
            e.close()
    (s1, p1, c1), (s0, p0, c0) = res
    assert (c1, c0) == (1, 0) and p1["neigh_builds"] == p0["neigh_builds"] == 1 and p1["row_cell_builds"] == 1 and p1["md_steps"] == p0["md_steps"] > 10
    assert np.abs(s1 - s0).max() <= 1e-9 * np.abs(s0).max()


# ---- 7. a launch that mixes the two paths ----

@pytest.fixture(scope="module")
def mixed():
    """nine simulations over replicas of 108 atoms (two images deep: the N^2 build), 864 and 1 920 atoms (cells), and each one's stress alone"""
    mp = pytest.MonkeyPatch()
    reps = {1: cu(3, 3, 3, seed=31), 2: cu(6, 6, 6, seed=32), 3: cu(6, 8, 10, seed=33)}
    vel = {r: velocities(len(c[0]), 300.0, 40 + r) for r, c in reps.items()}
    rng = np.random.default_rng(34)

    def fresh(cells=1):
        return engine(mp, cells, "eam", [(r, c[0], c[1], c[2], vel[r]) for r, c in reps.items()])

    sims = []
    for q in range(9):
        r = 1 + q % 3
        L = reps[r][1][3:6] - reps[r][1][:3]
        ezz = rng.uniform(5e-4, 2.5e-3)
        sims.append(capi.make_sim(q, "m", r, np.array([-0.3 * ezz * L[0], -0.3 * ezz * L[1], ezz * L[2], 0.2 * ezz * L[2], 0.0, 0.0]), nss=10, dt=1.0,
                                  temperature=300.0, strain_rate=1e-4, most_recent=capi.QP_NONE))
    alone = []
    try:
        for s in sims:
            e = fresh()
            alone.append(np.array(e.strain_batch([s])[0].stress[:]))
            e.close()
        yield fresh, sims, np.array(alone)
    finally:
        mp.undo()


@pytest.mark.parametrize("split", [0, 1])
def test_mixed_batch_equals_each_alone(mixed, split):
    fresh, sims, alone = mixed
    e = fresh()
    try:
        e.batch_split(split)
        out = np.array([list(o.stress) for o in e.strain_batch(sims)])
        paths = sorted((e.debug_rows(p, rows=False)["n"], e.debug_rows(p, rows=False)["cells"]) for p in range(9))
        p = e.profile()
    finally:
        e.close()
    assert paths == [(108, 0)] * 3 + [(864, 1)] * 3 + [(1920, 1)] * 3
    assert 0 < p["row_cell_builds"] < p["neigh_builds"]
    err = np.abs(out - alone).max(axis=1) / np.abs(alone).max(axis=1)
    print(f"eam mixed batch of 9 (split {split}): max rel err {err.max():.2e}, builds {p['neigh_builds']}, through cells {p['row_cell_builds']}")
    assert err.max() <= 1e-9


def test_a_batch_of_small_replicas_builds_nothing_through_cells(monkeypatch):
    x, box, t = en.case_jitter(2)
    e = engine(monkeypatch, None, "eam", [(1, x, box, t, velocities(len(x), 300.0, 51))])
    try:
        L = box[3:6] - box[:3]
        sims = [capi.make_sim(q, "m", 1, np.array([0.0, 0.0, 1e-3 * (1 + q) * L[2], 0.0, 0.0, 0.0]), nss=10, dt=1.0, temperature=300.0, strain_rate=1e-4,
                              most_recent=capi.QP_NONE) for q in range(9)]
        e.strain_batch(sims)
        p = e.profile()
        assert p["neigh_builds"] >= 9 and p["row_cell_builds"] == 0 and e.debug_rows(0, rows=False)["cells"] == 0
    finally:
        e.close()


# ---- 8. the interface ----

def test_debug_rows_refusals(monkeypatch, cu864):
    (x, box, t), _ = cu864
    e = engine(monkeypatch, 1, "eam", [(1, x, box, t, None)])
    try:
        with pytest.raises(capi.EngineError, match="no run or static evaluation of a row potential"):
            e.debug_rows(0)
        e.eam_compute("m", 1)
        r = e.debug_rows(0)
        with pytest.raises(capi.EngineError, match=r"position 1 of a run of 1 replicas"):
            e.debug_rows(1)
        cnt = np.zeros(r["n"], np.int32); tab = np.zeros(r["n"] * r["cap"], np.int32); info = np.zeros(6, np.int32)
        f = capi.lib().scema_md_debug_rows
        rc = f(e.h, 0, cnt.ctypes.data, tab.ctypes.data, C.c_int64(r["n"] * r["cap"] - 1), info.ctypes.data)
        assert rc != 0
        with pytest.raises(capi.EngineError, match=rf"rows_cap {r['n'] * r['cap'] - 1} < n \* capacity = 864 \* {r['cap']}"):
            e._chk(rc)
        assert not cnt.any() and not tab.any()
    finally:
        e.close()
