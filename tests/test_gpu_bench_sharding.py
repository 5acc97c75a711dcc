"""GPU: bench.py's multi-rank path.  `python bench.py --gpus 2` must start its two ranks itself; on the one-GPU test box
the ranks share the device and the engine's collective runs over its host transport (gloo), since RCCL wants one device
per rank -- the RCCL variant runs where two devices exist and says so when it cannot."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--sims", "6", "--steps", "2", "--warmup", "1", "--nss", "10", "--cells", "4", "6", "12", "--equil-steps", "40", "--no-cpu-baseline",
          "--monotonic-updates", "0"]


def _run(cmd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
    if not ok:
        return r
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_two_rank_bench_spawns_its_ranks_and_matches_single_rank():
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + COMMON)
    two = _run([sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--share-gpus", "--full"] + COMMON)
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    c1, c2 = one["config"]["stress_zz_checksum_Pa"], two["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c2) <= 1e-8 * abs(c1), (c1, c2)      # FP64 atomics: summation order differs from run to run
    assert two["config"]["allgathers"] == 3 and two["config"]["sims_on_rank0"] == 3     # ONE collective per update (1 warm-up + 2 timed)
    for k in ("metric", "value", "unit", "ms_per_step", "roofline", "scaling", "dtype"):
        assert k in two


def test_more_gpus_than_devices_is_an_error_not_a_smaller_run():
    import torch
    n = torch.cuda.device_count() + 1
    r = _run([sys.executable, "bench.py", "--gpus", str(n)] + COMMON, ok=False)
    assert r.returncode != 0 and "n_gpus" not in r.stdout


def test_two_rank_bench_over_rccl():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("RCCL PATH WITH 2 RANKS NOT EXERCISED: this box has one GPU, and this RCCL build refuses two ranks on one device ('Duplicate GPU "
                    "detected : rank %d and rank %d both on CUDA device' is its own message; librccl of ROCm 7.2 exports no multi-rank-per-GPU entry point "
                    "such as ncclCommInitRankMulti and has no environment switch for it).  The one-rank RCCL calls run in test_gpu_multirank.py")
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + COMMON)
    two = _run([sys.executable, "bench.py", "--gpus", "2"] + COMMON)
    assert two["n_gpus"] == 2 and two["config"]["collective"].startswith("ncclAllGather")
    c1, c2 = one["config"]["stress_zz_checksum_Pa"], two["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c2) <= 1e-8 * abs(c1), (c1, c2)


def test_rccl_attach_failure_moves_every_rank_to_the_host_transport():
    """two ranks on ONE device with the RCCL data path asked for: RCCL refuses (duplicate GPU) on every rank; bench.py's attach_comm notices in its
    probe, the ranks agree over the control plane, and the run completes over the host transport with the same stresses -- and says so"""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a box where two ranks must share a device")
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + COMMON)
    two = _run([sys.executable, "bench.py", "--gpus", "2", "--share-gpus", "--comm-timeout", "120"] + COMMON)
    coll = two["config"]["collective"]
    assert coll.startswith("host transport (gloo) -- RCCL attach failed"), coll
    c1, c2 = one["config"]["stress_zz_checksum_Pa"], two["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c2) <= 1e-8 * abs(c1), (c1, c2)
    assert two["config"]["allgathers"] == 3 and two["config"]["handshakes"] == 3     # (the probe's own collective is not counted)


def test_imbalanced_batch_on_two_ranks_is_levelled_and_moves_states():
    """the ragged strain set (nts 10..100) on two ranks: after the first update the planner levels the load by MD steps,
    which makes replica states change rank (over the host transport here); the stresses equal the single-rank run's"""
    common = ["--sims", "8", "--steps", "3", "--warmup", "1", "--nss", "10", "--cells", "4", "6", "12", "--equil-steps", "40", "--no-cpu-baseline",
              "--monotonic-updates", "0", "--strain-set", "imbalanced"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + common)
    two = _run([sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--share-gpus"] + common)
    c1, c2 = one["config"]["stress_zz_checksum_Pa"], two["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c2) <= 1e-8 * abs(c1), (c1, c2)
    cfg = two["config"]
    assert cfg["allgathers"] == 4 and cfg["handshakes"] == 4            # one of each per update
    assert cfg["state_migrations"] >= 1, cfg                            # a fresh batch is dealt i % 2; levelling by cost then moves states
    assert 1 <= cfg["sims_on_rank0"] <= 7
    assert cfg["md_steps_per_eval"] > 25.0                              # ragged: more straining steps than the balanced set's 10


def test_four_rank_bench_with_the_full_576_replica_batch():
    """The code the driver starts with `--gpus 8`, minus RCCL, at the widest world a test may use on this pool (6 processes may have
    the card open and the test runner is one of them: an 8-rank run is killed by the box's process guard; the dealing at world 8
    itself runs on the CPU: test_sim_plan.py, test_stmd_sync_host.py): bench.py spawns four ranks that share the GPU, the 576-replica
    batch is dealt 144 to each, one stress collective and one handshake per update, no state changes rank, the checksum equals the
    one-rank run's, and the JSON line carries what every rank did."""
    common = ["--sims", "576", "--steps", "2", "--warmup", "1", "--nss", "10", "--cells", "4", "6", "12", "--equil-steps", "40", "--no-cpu-baseline",
              "--monotonic-updates", "0", "--reax-leg", "off"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + common)
    four = _run([sys.executable, "bench.py", "--gpus", "4", "--dist-backend", "gloo", "--share-gpus"] + common)
    c1, c4 = one["config"]["stress_zz_checksum_Pa"], four["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c4) <= 1e-8 * abs(c1), (c1, c4)
    cfg = four["config"]
    assert four["n_gpus"] == 4 and cfg["n_sims"] == 576 and cfg["sims_on_rank0"] == 144
    assert cfg["allgathers"] == 3 and cfg["handshakes"] == 3 and cfg["state_migrations"] == 0
    pr = cfg["per_rank"]
    assert [r["rank"] for r in pr] == list(range(4)) and all(r["sims"] == 144 for r in pr) and all(r["evals_per_s"] > 0 for r in pr)
    assert one["config"]["env_overrides"] == [] and "per_rank" not in one["config"]


def test_imbalanced_batch_on_four_ranks():
    """the ragged strain set at world 4: levelled by MD steps within one simulation of even, the same stresses as one rank"""
    common = ["--sims", "48", "--steps", "2", "--warmup", "1", "--nss", "10", "--cells", "4", "6", "12", "--equil-steps", "40", "--no-cpu-baseline",
              "--monotonic-updates", "0", "--strain-set", "imbalanced"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + common)
    four = _run([sys.executable, "bench.py", "--gpus", "4", "--dist-backend", "gloo", "--share-gpus"] + common)
    c1, c4 = one["config"]["stress_zz_checksum_Pa"], four["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c4) <= 1e-8 * abs(c1), (c1, c4)
    pr = four["config"]["per_rank"]
    steps = [r["md_steps"] for r in pr]
    assert sum(r["sims"] for r in pr) == 48 and min(r["sims"] for r in pr) >= 1
    assert max(steps) - min(steps) <= 2 * 110 * 2, steps     # timed updates x (nts_max + nss): within one simulation of level per update
    assert four["config"]["allgathers"] == 3


def test_reax_replica_set_bench_line():
    """bench.py --force-field reax (BASELINE config 5) at a reduced batch: the same JSON contract, roofline block of the matrix sweep"""
    out = _run([sys.executable, "bench.py", "--force-field", "reax", "--sims", "6", "--steps", "1", "--warmup", "1", "--equil-steps", "20",
                "--no-cpu-baseline", "--monotonic-updates", "0", "--full"])
    assert out["metric"] == "stress_evals_per_sec" and out["value"] > 0 and out["dtype"] == "f64"
    assert out["config"]["force_field"] == "reax" and out["config"]["atoms_per_replica"] == 1620 and "ReaxFF" in out["config"]["workload"]
    r = out["roofline"]
    assert r["bound"] == "hbm" and r["kernel"].startswith("k_rx_qeq_sweep") and r["launches"] > 0 and 0.0 < r["frac"] < 1.0
    # (the symmetric form stores a pair once, in its owner's row: half the entries of the full rows)
    assert r["symmetric"] is True and 150 < r["stored_entries_per_row"] < 550 and 2 < r["qeq_iterations_per_solve"] < 80


def test_reax_replica_set_on_two_ranks_matches_one_rank():
    """BASELINE config 5 names 8 GPUs: the ReaxFF set sharded over two ranks (sharing the one device here, host transport) gives the stresses of one rank"""
    common = ["--force-field", "reax", "--sims", "6", "--steps", "1", "--warmup", "1", "--equil-steps", "20", "--no-cpu-baseline", "--monotonic-updates", "0"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + common)
    two = _run([sys.executable, "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--share-gpus"] + common)
    assert two["n_gpus"] == 2 and two["config"]["sims_on_rank0"] == 3 and two["config"]["allgathers"] == 2
    c1, c2 = one["config"]["stress_zz_checksum_Pa"], two["config"]["stress_zz_checksum_Pa"]
    assert abs(c1 - c2) <= 1e-6 * abs(c1), (c1, c2)      # (the charge solve stops at 1e-6; summation orders differ)


def test_default_run_carries_the_reax_leg_and_reports_environment_switches():
    """the default line's second leg (BASELINE config 5 as config.reax, outside `value`), forced on for a small OPLS batch; and a run
    with a declared switch set says so in config.env_overrides (a clean run: an empty list)"""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--full", "--reax-leg", "on"] + COMMON, capture_output=True, text=True, timeout=900, cwd=ROOT,
                       env=dict(os.environ, MASTER_ADDR="127.0.0.1", SCEMA_MD_SPLIT="0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["config"]["env_overrides"] == ["SCEMA_MD_SPLIT=0"]
    x = out["config"]["reax"]
    assert "error" not in x, x
    assert x["n_sims"] == 72 and x["atoms_per_replica"] == 1620 and x["md_steps_per_eval"] == 30.0 and x["evals_per_s"] > 0
    assert abs(x["replica_steps_per_s"] - 30.0 * x["evals_per_s"]) < 1e-6 * x["replica_steps_per_s"]
    assert x["roofline"]["kernel"].startswith("k_rx_qeq_sweep") and 0.0 < x["roofline"]["frac"] < 1.0
    assert out["value"] > 0 and out["config"]["force_field"] == "opls"          # the headline is the OPLS loop's, untouched by the leg


def test_one_pass_step_tail_equals_the_three_kernels():
    """k_finish (assembly of f + fix shake + second half-kick in one pass, the default for small batches of PPPM / no k-space steps) against
    k_ewald_force + k_shake + k_final_integrate (SCEMA_MD_FUSED_TAIL=0), and the one-launch cell binning against the three-kernel
    one, on the bench's small replica set: the same stresses (FP64 atomics: summation order differs from run to run)"""
    def run(env):
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1"] + COMMON, capture_output=True, text=True, timeout=900, cwd=ROOT,
                           env=dict(os.environ, MASTER_ADDR="127.0.0.1", **env))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["config"]["stress_zz_checksum_Pa"]
    a = run({})
    for env in ({"SCEMA_MD_FUSED_TAIL": "0"}, {"SCEMA_MD_CELL_BUILD": "0"}):
        b = run(env)
        assert abs(a - b) <= 1e-8 * abs(a), (env, a, b)


def test_plain_run_is_the_headline_only_and_dumps_the_last_timed_update(tmp_path):
    """a run without --full times its steps and prints the headline, none of the extra measurements; --dump-outputs writes the stresses
    of the last timed update (float64, one row per quadrature point), the very numbers the line's checksum sums; --steps sets the timed updates"""
    args = ["--sims", "6", "--steps", "3", "--warmup", "1", "--nss", "10", "--cells", "4", "6", "12", "--equil-steps", "40"]
    out = _run([sys.executable, "bench.py", "--gpus", "1", "--dump-outputs", str(tmp_path / "o")] + args)
    assert out["steps"] == 3 and out["value"] > 0 and abs(out["value"] - 6 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    for k in ("roofline", "cpu_baseline", "box_fp64_tflops", "share8_evals_per_s"):
        assert k not in out, k
    assert "reax" not in out["config"] and "strain_set_monotonic_evals_per_s" not in out["config"]
    s = np.load(tmp_path / "o" / "stress.npy")
    assert s.dtype == np.float64 and s.shape == (6, 6) and np.isfinite(s).all()
    c = out["config"]["stress_zz_checksum_Pa"]
    assert abs(s[:, 2].sum() - c) <= 1e-12 * abs(c), (s[:, 2].sum(), c)
    # (what the plain line leaves out, --full still reports)
    full = _run([sys.executable, "bench.py", "--gpus", "1", "--full", "--no-cpu-baseline"] + args)
    assert full["roofline"]["launches"] > 0 and "box_fp64_tflops" in full
