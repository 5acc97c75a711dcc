"""Whole strained evaluations with md_force_field "reax" on the GPU against the oracle's expected stresses (SURVEY.md 8(f) row
f-4, BASELINE config 5): scema_md_strain_batch -> md_reax.hip, compared through the C ABI with
tests/golden/oracle_eval_reax.json (generator tests/golden/make_golden_reax.py: oracle/reax_md.py = the dynamics of
oracle/md_oracle.c around reverse-mode forces of the oracle's own energy and fix qeq/reax).

Tolerance: the north star's 1e-4 relative (of the largest stress component), stated in TOL; the measured error is printed.
What separates the two sides is the conjugate-gradient tolerance of `fix qeq/reax` (1e-6, as the reference's script asks): the
engine's batched two-system sweeps and the oracle's plain CG stop at different iterates, so charges agree to ~1e-6, stresses to
~1e-6..1e-5 over a 30-step evaluation.  PARITY UNPINNED against LAMMPS itself, like the oracle."""
import json
import os
import shutil

import numpy as np
import pytest

from scema_amd import capi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FFIELD = os.path.join(HERE, "golden", "ffield.reax.2")
TOL = 1e-4
MASS = dict(H=1.008, C=12.011, N=14.007, O=15.999)


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(HERE, "golden", "oracle_eval_reax.json")))


@pytest.fixture()
def scripts(tmp_path):
    d = tmp_path / "lammps_scripts_reax"
    d.mkdir()
    shutil.copy(FFIELD, d / "ffield.reax.2")      # what the reference's script names: pair_coeff * * ${locs}/ffield.reax.2 H C N O
    return str(d)


def _thermal_velocities(sym, seed):
    m = np.array([MASS[s] for s in sym])
    v = np.random.default_rng(seed).standard_normal((len(sym), 3)) * np.sqrt(0.0019872067 * 300.0 / (m[:, None] * 48.88821291 ** 2))
    return v - (m[:, None] * v).sum(0) / m.sum()


def _pe1620(gold):
    from scema_amd.systems import build_pe
    d = build_pe(3, 5, 9)
    sym = ["C" if d["mass"][k] > 5 else "H" for k in d["type"]]
    x, box, v = np.array(d["x"], float), np.array(d["box"], float), _thermal_velocities(sym, 3)
    c = gold["pe1620"]
    # the fixture is rebuilt from seeded generators: refuse to compare if a library drifted
    assert abs(np.abs(x).sum() - c["x_checksum"]) < 1e-9 * c["x_checksum"] and abs(np.abs(v).sum() - c["v_checksum"]) < 1e-9 * c["v_checksum"]
    return sym, x, box, v


def _mixture(gold):
    c = gold["mixture"]
    return c["sym"], np.array(c["x"]), np.array(c["box"]), np.array(c["v"])


def _sim(qp, strain, gold, scripts, recent):
    p = gold["params"]
    return capi.make_sim(qp, "g0", 1, np.array(strain), nss=p["nss"], dt=p["dt"], temperature=p["temperature"], strain_rate=p["strain_rate"],
                         most_recent=recent, force_field="reax", scripts_folder=scripts)


@pytest.mark.parametrize("case", ["mixture", "pe1620"])
def test_reax_evaluations_match_the_oracle(gold, scripts, case):
    """every chain of the golden file as ONE batch (one quadrature point per chain), then the continued second evaluations"""
    sym, x, box, v = _mixture(gold) if case == "mixture" else _pe1620(gold)
    e = capi.Engine()
    e.register_replica("g0", 1, capi.reax_system(sym, x, box, v=v))
    chains = gold[case]["chains"]
    worst = 0.0
    for step in range(2):
        sims = [_sim(k, ch["evals"][step]["strain_len"], gold, scripts, capi.QP_NONE if step == 0 else k) for k, ch in enumerate(chains)]
        out = e.strain_batch(sims)
        for k, ch in enumerate(chains):
            exp = np.array(ch["evals"][step]["stress"])
            got = np.array(list(out[k].stress))
            err = np.abs(got - exp).max() / np.abs(exp).max()
            worst = max(worst, err)
            print(f"reax {case} chain {ch['name']} evaluation {step + 1}: nts {ch['evals'][step]['nts']}, max rel err vs oracle {err:.2e}")
            assert out[k].stress_updated and err < TOL, (case, ch["name"], step, err)
    st = e.reax_stats()
    assert st["qeq_tol"] == 1e-6
    print(f"reax {case}: worst relative stress error {worst:.2e} (tolerance {TOL:g}); {st['qeq_iters'] / st['qeq_solves']:.1f} CG iterations per solve "
          f"(oracle: {np.mean([c['qeq_iterations_per_solve'] for c in chains]):.1f})")
    e.close()


def test_the_replica_set_at_its_batch_size(gold, scripts):
    """BASELINE config 5 at the size bench.py --force-field reax runs it: 72 replicas of 1 620 atoms in one update.  Members 0..2
    carry the golden strains and are pinned on the oracle's stresses; the strains of the others come from the bench's draw and
    have to pass what the domain guarantees: every box ends where fix deform should leave it, equal requests give equal stresses
    wherever they sit in the batch, the update is reproducible, and a second update continues from the stored states."""
    from scema_amd.systems import synthetic_strains
    sym, x, box, v = _pe1620(gold)
    lens = box[3:6] - box[:3]
    chains = gold["pe1620"]["chains"]
    strains = [np.array(ch["evals"][0]["strain_len"]) for ch in chains]
    draw = synthetic_strains(72, lens, seed=2026)
    strains += [draw[k] for k in range(len(chains), 70)]
    strains += [strains[0], strains[5]]                 # duplicates at the far end of the batch
    assert len(strains) == 72
    res = []
    for rep in range(2):
        e = capi.Engine()
        e.register_replica("g0", 1, capi.reax_system(sym, x, box, v=v))
        out = e.strain_batch([_sim(k, s, gold, scripts, capi.QP_NONE) for k, s in enumerate(strains)])
        s1 = np.array([list(o.stress) for o in out])
        assert all(o.stress_updated for o in out) and np.isfinite(s1).all()
        res.append(s1)
        if rep == 0:
            for k, ch in enumerate(chains):
                exp = np.array(ch["evals"][0]["stress"])
                err = np.abs(s1[k] - exp).max() / np.abs(exp).max()
                print(f"reax 72-replica batch, member {k} ({ch['name']}): max rel err vs oracle {err:.2e}")
                assert err < TOL, (k, err)
            for k in (3, 17, 40, 69):
                b, _, _ = e.get_state(k, "g0", 1)
                eps = strains[k] / lens[[0, 1, 2, 2, 1, 0]]
                assert np.allclose((b[3:6] - b[:3]) / lens - 1.0, eps[:3], atol=2e-6)
            # the continued second evaluations of the golden chains, inside a full-size second update
            out2 = e.strain_batch([_sim(k, 0.5 * s, gold, scripts, k) for k, s in enumerate(strains)])
            for k, ch in enumerate(chains):
                exp = np.array(ch["evals"][1]["stress"])
                got = np.array(list(out2[k].stress))
                err = np.abs(got - exp).max() / np.abs(exp).max()
                print(f"reax 72-replica batch, member {k} continued: max rel err vs oracle {err:.2e}")
                assert err < TOL, (k, err)
        e.close()
    scale = np.abs(res[0]).max()
    assert np.abs(res[0][70] - res[0][0]).max() < 1e-6 * scale and np.abs(res[0][71] - res[0][5]).max() < 1e-6 * scale
    assert np.abs(res[0] - res[1]).max() < 1e-6 * scale


def test_stresses_do_not_depend_on_how_the_batch_is_issued(gold, scripts):
    """a batch runs as part batches on several streams, each with the bond-order chain of its force stage on a side stream (the parts take
    every P-th rank of the run-length order); issued as ONE sequence of launches on one stream the same requests give the same stresses
    (to the order of FP64 atomic sums), whatever the run lengths -- the draw below has evaluations of 10 to 30 straining steps."""
    from scema_amd.systems import synthetic_strains
    sym, x, box, v = _mixture(gold)
    lens = box[3:6] - box[:3]
    draw = synthetic_strains(19, lens, seed=7)   # (a batch runs as P parts from 6 P replicas on)
    strains = [draw[k] * (0.4 + 0.2 * (k % 5)) for k in range(19)]
    res = []
    for parts, overlap in ((2, 1), (1, 0), (3, 1)):
        e = capi.Engine()
        e.reax_configure(FFIELD)
        e.reax_concurrency(parts, overlap)
        e.register_replica("g0", 1, capi.reax_system(sym, x, box, v=v))
        sims = [_sim(k, st, gold, scripts, capi.QP_NONE) for k, st in enumerate(strains)]
        out = e.strain_batch(sims)
        assert all(o.stress_updated for o in out)
        res.append(np.array([list(o.stress) for o in out]))
        e.close()
    scale = np.abs(res[0]).max()
    assert np.isfinite(res[0]).all() and scale > 0
    assert np.abs(res[0] - res[1]).max() < 1e-6 * scale
    assert np.abs(res[2] - res[1]).max() < 1e-6 * scale


def test_kept_reax_neighbour_rows_equal_rebuilt_ones(tmp_path):
    """ReaxFF rows (full and near rows, reference positions, the preconditioner) survive from the straining run to the sampling run and from one update to
    the next on the same slot where the device finds every atom within the list's displacement bound (as the OPLS rows do); SCEMA_MD_KEEP_LIST=0 rebuilds at
    every run start.  A sequence in which one state is REPLACED between two updates and another continues: same stresses either way, fewer builds."""
    import json, subprocess, sys
    root = os.path.dirname(HERE)
    d = tmp_path / "lammps_scripts_reax"
    d.mkdir()
    shutil.copy(FFIELD, d / "ffield.reax.2")
    code = ("import json, sys, numpy as np\n"
            "from scema_amd import capi\n"
            "from scema_amd.systems import build_pe\n"
            "d = build_pe(3, 5, 9, jitter=0.05, seed=7)\n"
            "sym = ['C' if d['mass'][t] > 5 else 'H' for t in d['type']]\n"
            "m = np.array([12.011 if c == 'C' else 1.008 for c in sym])\n"
            "v = np.random.default_rng(3).standard_normal((len(sym), 3)) * np.sqrt(0.0019872067 * 300.0 / (m[:, None] * 48.88821291 ** 2))\n"
            "v -= (m[:, None] * v).sum(0) / m.sum()\n"
            "e = capi.Engine()\n"
            "e.reax_configure(sys.argv[1] + '/ffield.reax.2', qeq_tol=1e-10)\n"
            "e.register_replica('g0', 1, capi.reax_system(sym, d['x'], d['box'], v=v))\n"
            "L = d['box'][3:6] - d['box'][:3]\n"
            "st = np.array([-3e-4 * L[0], -3e-4 * L[1], 1e-3 * L[2], 2e-5 * L[2], 0, 0])\n"
            "mk = lambda q, s, recent: capi.make_sim(q, 'g0', 1, s, nss=20, dt=0.25, temperature=300.0, strain_rate=1e-4, most_recent=recent, force_field='reax', scripts_folder=sys.argv[1])\n"
            "out = []\n"
            "a = e.strain_batch([mk(q, st * (1 + 0.2 * q), capi.QP_NONE) for q in (0, 1)])\n"
            "out += [list(o.stress) for o in a]\n"
            "a = e.strain_batch([mk(q, -st, q) for q in (0, 1)])\n"
            "out += [list(o.stress) for o in a]\n"
            "box, x, vv = e.get_state(1, 'g0', 1)\n"
            "rng = np.random.default_rng(3)\n"
            "e.set_state(0, 'g0', 1, box, x + rng.normal(0, 0.02, x.shape), vv)      # qp 0 becomes (a perturbed copy of) qp 1's state\n"
            "a = e.strain_batch([mk(q, st, q) for q in (0, 1)])\n"
            "out += [list(o.stress) for o in a]\n"
            "p = e.profile()\n"
            "print(json.dumps({'s': out, 'builds': p['neigh_builds'], 'steps': p['md_steps']}))\n")
    res = {}
    for name, env in (("keep", {}), ("nokeep", {"SCEMA_MD_KEEP_LIST": "0"})):
        pr = subprocess.run([sys.executable, "-c", code, str(d)], capture_output=True, text=True, timeout=600, cwd=root, env=dict(os.environ, **env))
        assert pr.returncode == 0, pr.stderr[-2000:]
        res[name] = json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])
    a, b = np.array(res["keep"]["s"]), np.array(res["nokeep"]["s"])
    # (the charge solve to 1e-10: what is left is the order of FP64 sums and the age of the preconditioner)
    assert np.abs(a - b).max() < 1e-7 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()
    assert res["keep"]["steps"] == res["nokeep"]["steps"]
    assert res["keep"]["builds"] <= res["nokeep"]["builds"] - 4, (res["keep"]["builds"], res["nokeep"]["builds"])


def test_a_charge_solve_that_fails_with_the_engines_preconditioner_is_repeated_with_the_references(gold, scripts, monkeypatch):
    """the approximate-inverse preconditioner of the charge equilibration is symmetrised by hand and not guaranteed positive
    definite on every geometry; a solve that does not converge with it must not end the update before the evaluation has been repeated
    once with the Jacobi preconditioner of fix qeq/reax.  The system is the H/C/N/O mixture (not polyethylene: four elements, every type
    pair) as a 2 x 2 x 2 supercell -- the 21-A cell itself is thinner than two list radii and keeps the Jacobi preconditioner anyway; the
    periodic copy has the same dynamics and therefore the oracle's stress of the single cell.  First as it is: the engine's preconditioner
    is on (few iterations per solve) and no retry is needed.  Then with a run that REPORTS a failed solve whenever that preconditioner is
    on (SCEMA_MD_TEST_QEQ_PRECOND_FAILS): the evaluation comes back from its retry, counted, within the tolerance of the oracle's stress."""
    sym1, x1, box1, v1 = _mixture(gold)
    L = box1[3:6] - box1[:3]
    shifts = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)], float) * L
    sym = sym1 * 8
    x = np.concatenate([x1 + s for s in shifts])
    v = np.concatenate([v1] * 8)
    box = np.array(box1, float)
    box[3:6] = box[:3] + 2.0 * L
    ch = gold["mixture"]["chains"][0]
    exp = np.array(ch["evals"][0]["stress"])
    strain = 2.0 * np.array(ch["evals"][0]["strain_len"])     # the same strain: lengths are in A
    res = {}
    for name, hook in (("plain", False), ("retry", True)):
        if hook:
            monkeypatch.setenv("SCEMA_MD_TEST_QEQ_PRECOND_FAILS", "1")
        e = capi.Engine()
        e.register_replica("g0", 1, capi.reax_system(sym, x, box, v=v))
        out = e.strain_batch([_sim(0, strain, gold, scripts, capi.QP_NONE)])
        res[name] = np.array(list(out[0].stress))
        st = e.reax_stats()
        its = st["qeq_iters"] / st["qeq_solves"]
        err = np.abs(res[name] - exp).max() / np.abs(exp).max()
        print(f"reax mixture 2x2x2 ({len(sym)} atoms), {name}: max rel err vs the oracle's single cell {err:.2e}, {its:.1f} CG iterations per solve, "
              f"evaluations repeated with the Jacobi preconditioner {st['precond_fallbacks']}")
        assert st["precond_fallbacks"] == (1 if hook else 0), (name, st)
        assert out[0].stress_updated and err < TOL, (name, err)
        if not hook:
            assert its < 9.0, its      # the approximate inverse is on for this system (Jacobi: 12-13 iterations per solve)
        else:
            assert its > 9.0, its      # the evaluation that counts ran with the Jacobi preconditioner
            # the engine's own setting is back after the retry: the next evaluation uses the approximate inverse again
            monkeypatch.delenv("SCEMA_MD_TEST_QEQ_PRECOND_FAILS")
            out2 = e.strain_batch([_sim(0, 0.5 * strain, gold, scripts, 0)])
            assert out2[0].stress_updated and e.reax_stats()["precond_fallbacks"] == 1
        e.close()
    # the two answers differ by the solver's tolerance, not more
    assert np.abs(res["retry"] - res["plain"]).max() < 1e-4 * np.abs(res["plain"]).max()
