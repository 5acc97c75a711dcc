"""Skin bands of the pair rows (scema_amd/csrc/md_skin_bands.h): k_pair walks the skin part of a row only as far as the
displacement bound of the row's own cluster, the replica's bound and the motion of the box corners allow a pair inside the cutoff.
SCEMA_MD_SKIN_BANDS=0 walks every listed entry on every step: the reference behaviour every test here compares with.  The switch is read
once per process, hence child processes.  Tolerances are those of test_fp32_list_builds_list_a_superset_and_change_no_force and
test_kept_neighbour_rows_equal_rebuilt_ones ("same lists, FP64 atomics noise"): trajectories 1e-8 A absolute, forces 1e-11 relative,
stresses 1e-9 relative.  A pair that a closed band hid while it was inside the cutoff is a missing force of the size of a pair force at
the cutoff, five orders of magnitude above these."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = ("import json, os, numpy as np\n"
        "from scema_amd import capi\n"
        "from scema_amd.systems import build_pe\n"
        "d = build_pe(2, 3, 5, jitter=0.05, seed=7); d['box'][6:9] = [0.7, -0.4, 0.5]\n"
        "kw = dict(cut_lj=5.0, cut_coul=4.0, skin=1.0, kspace_accuracy=1e-5)\n"
        "RATES = [2e-5, -1e-5, 1e-5, 3e-6, -2e-6, 1e-6]\n")


def _child(code, env):
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **env))
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-2500:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _pair(code, env=None):
    """the same child with the bands on (default) and off"""
    env = dict(env or {})
    return _child(code, env), _child(code, dict(env, SCEMA_MD_SKIN_BANDS="0"))


def _same_state(a, b):
    xa, xb, va, vb = (np.array(t) for t in (a["x"], b["x"], a["v"], b["v"]))
    print("max |dx| %.3e A, max |dv| %.3e of %.3e" % (np.abs(xa - xb).max(), np.abs(va - vb).max(), np.abs(vb).max()))
    assert np.abs(xa - xb).max() < 1e-8
    assert np.abs(va - vb).max() < 1e-8 * np.abs(vb).max() + 1e-12


# 60 steps of NVT + SHAKE + fix deform on the tilted 480-atom replica, at a time step of 0.5 fs: the jittered crystal is hot, and at 2 fs
# its atoms cover half the 1 A skin within the five steps of neigh_modify delay (a build every 5 steps, none 10 apart).  Also, for every n <= 60, the builds of an n-step run from the same
# state (the build history of the 60-step run: every run starts with one build) and what the pair launch behind the last step would walk.
MAIN = HEAD + (
    "e = capi.Engine(capi.default_params(**kw))\n"
    "e.register_replica('pe', 1, d)\n"
    "f, en, w, info = e.debug_compute('pe', 1, use_shake=True)\n"
    "fresh = e.debug_skin_bands()\n"
    "hist, stats = [], []\n"
    "for n in range(1, 61):\n"
    "    e.set_state(5, 'pe', 1, d['box'], d['x'], d['v'])\n"
    "    e.profile(reset=True)\n"
    "    e.debug_run('pe', 1, n, 0.5, 300.0, qp=5, nvt=True, use_shake=True, rates=RATES)\n"
    "    hist.append(int(e.profile()['neigh_builds']))\n"
    "    stats.append(e.debug_skin_bands())\n"
    "box, x, v = e.get_state(5, 'pe', 1)\n"
    "print(json.dumps({'f': np.asarray(f).ravel().tolist(), 'fresh': fresh, 'hist': hist, 'stats': stats,\n"
    "                  'x': np.asarray(x).ravel().tolist(), 'v': np.asarray(v).ravel().tolist()}))\n")


def test_banded_trajectory_equals_the_whole_row_one_and_the_bands_do_open_and_close():
    """Default against SCEMA_MD_SKIN_BANDS=0: the same forces at a fresh build, the same x and v after 60 steps, the same builds.  Not
    vacuous: a fresh build walks exactly A | B (no skin entry) with the bands and every listed entry without; at the end of the run some
    rows have a band open and not all rows have all of them open; and mode 0 alone shows at least two rebuilds with at least 10 steps
    between two builds."""
    on, off = _pair(MAIN)
    fa, fb = np.array(on["f"]), np.array(off["f"])
    assert np.abs(fa - fb).max() < 1e-11 * np.abs(fb).max()
    _same_state(on, off)
    assert on["hist"] == off["hist"], (on["hist"], off["hist"])
    # the build history of mode 0: builds(n) - 1 rebuilds within n steps; a rebuild happens at step n where the count goes up
    hist = off["hist"]
    at = [0] + [n + 1 for n in range(60) if hist[n] > (hist[n - 1] if n else 1)]
    print("mode 0: builds at steps", at)
    assert len(at) - 1 >= 2 and max(b - a for a, b in zip(at, at[1:])) >= 10, at
    k = on["fresh"]["K"]
    assert sum(on["fresh"]["listed"]) > 0 and on["fresh"]["walked"] == [0] * k and on["fresh"]["rows_open"] == 0
    assert off["fresh"]["walked"] == off["fresh"]["listed"] == on["fresh"]["listed"]
    end = on["stats"][-1]
    print("after 60 steps: walked / listed per band", list(zip(end["walked"], end["listed"])), "rows", end["rows"], "with a band open",
          end["rows_open"], "with all open", end["rows_all_open"])
    assert 0 < end["rows_open"] and end["rows_all_open"] < end["rows"]
    assert 0 < sum(end["walked"]) < sum(end["listed"])
    assert off["stats"][-1]["walked"] == off["stats"][-1]["listed"]
    # over the life of a list the walk grows band by band: nearer bands are never walked less than farther ones, row by row
    for s in on["stats"]:
        assert s["rows_all_open"] <= s["rows_open"] <= s["rows"]


# Batches: the integrator writes the slot records itself in launches of up to 32 replicas and leaves them to k_pack beyond (the size of the
# batch decides, engine_run.cpp plan_launch); two materials of different size and box in one launch.  Two updates each, so that the
# second one starts on kept rows.
BATCH = HEAD + (
    "big = build_pe(3, 4, 6, jitter=0.04, seed=21)\n"
    "L = d['box'][3:6] - d['box'][:3]\n"
    "st = np.array([-3e-4 * L[0], -3e-4 * L[1], 1e-3 * L[2], 2e-5 * L[2], 0, 0])\n"
    "out = {}\n"
    "for name, n in (('two', 2), ('many', 33), ('mixed', 3)):\n"
    "    e = capi.Engine(capi.default_params(**kw))\n"
    "    e.register_replica('pe', 1, d)\n"
    "    e.register_replica('big', 1, big)\n"
    "    mat = lambda q: 'big' if name == 'mixed' and q == 1 else 'pe'\n"
    "    s = []\n"
    "    a = e.strain_batch([capi.make_sim(q, mat(q), 1, st * (1 + 0.03 * q), nss=30, most_recent=capi.QP_NONE, material=int(mat(q) == 'big')) for q in range(n)])\n"
    "    s += [list(o.stress) for o in a]\n"
    "    a = e.strain_batch([capi.make_sim(q, mat(q), 1, -st * (1 + 0.01 * q), nss=30, material=int(mat(q) == 'big')) for q in range(n)])\n"
    "    s += [list(o.stress) for o in a]\n"
    "    p = e.profile()\n"
    "    xs = [np.asarray(e.get_state(q, mat(q), 1)[1]).ravel().tolist() for q in (0, n - 1)]\n"
    "    out[name] = dict(s=s, x=xs, builds=int(p['neigh_builds']), steps=int(p['md_steps']))\n"
    "    e.close()\n"
    "print(json.dumps(out))\n")


@pytest.mark.parametrize("env", [{}, {"SCEMA_MD_SMALL_BATCH_MAX": "0"}], ids=["default_grid", "largest_cells"])
def test_both_record_paths_and_mixed_materials(env):
    """2 replicas (k_initial_integrate writes records and bounds), 33 replicas (k_pack writes the records) and a launch of two
    materials, on the cell grid a small batch takes and on the one a large batch takes: banded against mode 0."""
    on, off = _pair(BATCH, env)
    for name in ("two", "many", "mixed"):
        a, b = np.array(on[name]["s"]), np.array(off[name]["s"])
        print(name, "max rel stress difference %.3e" % (np.abs(a - b).max() / np.abs(b).max()), "builds", on[name]["builds"], off[name]["builds"])
        assert np.abs(a - b).max() < 1e-9 * np.abs(b).max(), name
        assert on[name]["steps"] == off[name]["steps"] and on[name]["builds"] == off[name]["builds"], name
        for xa, xb in zip(on[name]["x"], off[name]["x"]):
            assert np.abs(np.array(xa) - np.array(xb)).max() < 1e-8, name


# the set-up of test_triclinic_box_flip_matches_the_oracle, sheared at 1e-2 per fs: the box corners move 0.1 A per step
FLIP = HEAD + (
    "kw = dict(cut_lj=4.5, cut_coul=4.0, skin=0.9, kspace_accuracy=1e-5)\n"
    "d = build_pe(2, 3, 5, jitter=0.05, seed=7)\n"
    "def hmat(b):\n"
    "    return np.array([[b[3] - b[0], b[6], b[7]], [0.0, b[4] - b[1], b[8]], [0.0, 0.0, b[5] - b[2]]])\n"
    "box = np.array(d['box'], float)\n"
    "lx, ly, lz = box[3] - box[0], box[4] - box[1], box[5] - box[2]\n"
    "box[6], box[7], box[8] = 0.485 * lx, -0.47 * lx, 0.0\n"
    "lam = np.linalg.solve(hmat(d['box']), (d['x'] - d['box'][:3]).T)\n"
    "d['x'] = (hmat(box) @ lam).T + box[:3]\n"
    "d['box'] = box\n"
    "rates = np.array([1e-5, -1e-5, 2e-5, 1e-2, -0.003 * lx / lz, 1e-5])\n"
    "e = capi.Engine(capi.default_params(**kw))\n"
    "e.register_replica('pe', 1, d)\n"
    "e.set_state(3, 'pe', 1, d['box'], d['x'], d['v'])\n"
    "e.debug_run('pe', 1, 24, 1.0, 300.0, qp=3, nvt=True, use_shake=True, rates=rates)\n"
    "bx, x, v = e.get_state(3, 'pe', 1)\n"
    "p = e.profile()\n"
    "print(json.dumps({'x': np.asarray(x).ravel().tolist(), 'v': np.asarray(v).ravel().tolist(), 'box': list(bx), 'flips': int(p['box_flips']),\n"
    "                  'builds': int(p['neigh_builds'])}))\n")


def test_corner_term_of_a_fast_sheared_box_across_a_flip():
    on, off = _pair(FLIP)
    assert on["flips"] == off["flips"] >= 1 and on["builds"] == off["builds"]
    assert np.abs(np.array(on["box"]) - np.array(off["box"])).max() < 1e-11
    _same_state(on, off)


# the three-update sequence of test_kept_neighbour_rows_equal_rebuilt_ones, the replaced state included
KEPT = HEAD + (
    "e = capi.Engine(capi.default_params(**kw))\n"
    "e.register_replica('pe', 1, d)\n"
    "L = d['box'][3:6] - d['box'][:3]\n"
    "st = np.array([-3e-4 * L[0], -3e-4 * L[1], 1e-3 * L[2], 2e-5 * L[2], 0, 0])\n"
    "out = []\n"
    "a = e.strain_batch([capi.make_sim(q, 'pe', 1, st * (1 + 0.2 * q), nss=20, most_recent=capi.QP_NONE) for q in (0, 1)])\n"
    "out += [list(o.stress) for o in a]\n"
    "a = e.strain_batch([capi.make_sim(q, 'pe', 1, -st, nss=20) for q in (0, 1)])\n"
    "out += [list(o.stress) for o in a]\n"
    "box, x, v = e.get_state(1, 'pe', 1)\n"
    "rng = np.random.default_rng(3)\n"
    "e.set_state(0, 'pe', 1, box, x + rng.normal(0, 0.02, x.shape), v)\n"
    "a = e.strain_batch([capi.make_sim(q, 'pe', 1, st, nss=20) for q in (0, 1)])\n"
    "out += [list(o.stress) for o in a]\n"
    "p = e.profile()\n"
    "print(json.dumps({'s': out, 'builds': int(p['neigh_builds']), 'steps': int(p['md_steps'])}))\n")


def test_kept_rows_walk_whole_rows_in_the_set_up_evaluation():
    """Rows kept from the run or the update before: the set-up evaluation of such a run has no bounds for the positions it starts from and
    walks whole rows.  Same stresses, same md_steps, same builds as mode 0; and the kept rows are in fact kept."""
    on, off = _pair(KEPT)
    a, b = np.array(on["s"]), np.array(off["s"])
    print("max rel stress difference %.3e" % (np.abs(a - b).max() / np.abs(b).max()), "builds", on["builds"], off["builds"])
    assert np.abs(a - b).max() < 1e-9 * np.abs(b).max()
    assert on["steps"] == off["steps"] and on["builds"] == off["builds"]
    nokeep = _child(KEPT, {"SCEMA_MD_KEEP_LIST": "0"})
    assert on["builds"] <= nokeep["builds"] - 6


# Shapes: a 3-atom system with a lone uncharged atom (an empty row; every cell holds fewer than 4 atoms: pad slots in every cluster) in
# memory that held a crystal's rows; the 480-atom replica (cell populations that are no multiples of 4) with a skin of 0.3 A, whose
# bands are narrower than a step's motion; a coulomb cutoff beyond the LJ one (segment B is empty, the other branch of k_pair).
EDGES = HEAD + (
    "z = lambda *s: np.zeros(s, np.int32)\n"
    "lone = dict(natoms=3, ntypes=1, type=z(3), charge=np.array([0.3, -0.3, 0.0]), mass=np.array([12.0]), eps=np.array([[0.1]]), sigma=np.array([[3.4]]),\n"
    "            bonds=z(0, 2), bond_type=z(0), bond_coeff=np.zeros((0, 2)), angles=z(0, 3), angle_type=z(0), angle_coeff=np.zeros((0, 2)),\n"
    "            dihedrals=z(0, 4), dihedral_type=z(0), dihedral_coeff=np.zeros((0, 4)), impropers=z(0, 4), improper_type=z(0),\n"
    "            improper_coeff=np.zeros((0, 2)), special_lj=np.ones(3), special_coul=np.ones(3),\n"
    "            box=np.array([0, 0, 0, 60, 60, 60, 0, 0, 0.0]), x=np.array([[30.0, 30, 30], [34.2, 30, 30], [5.0, 5.0, 5.0]]),\n"
    "            v=np.array([[2e-3, 1e-3, 0], [-2e-3, -1e-3, 0], [0, 0, 0.0]]))\n"
    "out = {}\n"
    "e = capi.Engine(capi.default_params(shake_mass=0.0, kspace_style=0))\n"
    "e.register_replica('dense', 1, build_pe(4, 6, 12))\n"
    "e.debug_compute('dense', 1)\n"
    "e.register_replica('lone', 1, lone)\n"
    "e.set_state(1, 'lone', 1, lone['box'], lone['x'], lone['v'])\n"
    "e.debug_run('lone', 1, 200, 2.0, 300.0, qp=1, nvt=False, use_shake=False)\n"
    "b, x, v = e.get_state(1, 'lone', 1)\n"
    "out['lone'] = dict(x=np.asarray(x).ravel().tolist(), v=np.asarray(v).ravel().tolist(), builds=int(e.profile()['neigh_builds']))\n"
    "e.close()\n"
    "for name, k in (('skin03', dict(kw, skin=0.3)), ('coul_beyond_lj', dict(kw, cut_lj=4.0, cut_coul=5.0))):\n"
    "    e = capi.Engine(capi.default_params(**k))\n"
    "    e.register_replica('pe', 1, d)\n"
    "    e.set_state(5, 'pe', 1, d['box'], d['x'], d['v'])\n"
    "    e.debug_run('pe', 1, 40, 2.0, 300.0, qp=5, nvt=True, use_shake=True, rates=RATES)\n"
    "    b, x, v = e.get_state(5, 'pe', 1)\n"
    "    out[name] = dict(x=np.asarray(x).ravel().tolist(), v=np.asarray(v).ravel().tolist(), builds=int(e.profile()['neigh_builds']),\n"
    "                     stats=e.debug_skin_bands())\n"
    "    e.close()\n"
    "print(json.dumps(out))\n")


def test_shape_edges():
    on, off = _pair(EDGES)
    for name in ("lone", "skin03", "coul_beyond_lj"):
        print(name, "builds", on[name]["builds"], off[name]["builds"])
        assert on[name]["builds"] == off[name]["builds"], name
        _same_state(on[name], off[name])
    assert np.abs(np.array(on["lone"]["x"][6:]) - 5.0).max() < 1e-9      # the lone, uncharged atom stays where it is
    assert on["skin03"]["builds"] >= 3                                   # a 0.3 A skin does not last 40 steps
    assert sum(on["coul_beyond_lj"]["stats"]["listed"]) > 0
