"""bench.py's output contract and its multi-rank code path on the one GPU a test box has: --force-collective takes the world > 1 branch
(pack -> RCCL all_gather_into_tensor on a 1-rank nccl group -> unpack) and the gathered block must equal the local results bit for bit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_and_forced_collective():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--full", "--no-cpu-baseline", "--force-collective"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["dtype"] == "f64" and d["scaling"] == "weak" and d["vs_baseline"] is None
    cfg = d["config"]
    assert cfg["collective"].startswith("all_gather") and cfg["gather_matches_local_results"] is True
    assert cfg["gathered_bytes_per_step"] == 256 * (101 * 30 + 100 * 30 + 54 + 101) * 8 and len(cfg["per_rank_value"]) == 1
    assert cfg["results_finite_and_converged"] is True
    assert cfg["workload"].startswith("configs[1]")
    ss = cfg["steady_state"]          # the receding-horizon leg (warm start on the device, robots in motion): replayed inputs reproduce the recorded run bit for bit
    assert ss["replay_reproduces_the_recorded_run_bit_for_bit"] is True and ss["results_finite_and_converged"] is True and ss["value"] > 0
    assert ss["mean_abs_measured_velocity"]["joints"] > 0.01 and set(ss["kernel_ms"]) >= {"ad", "lq", "riccati", "linesearch", "wbc"}
    assert "per_rank_value_min" in cfg and cfg["slowest_rank_over_fastest"] == 1.0
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0.0 < r["frac"] < 1.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and "traffic_source" in r
    # north_star's evidence fields: matrix-core busy fraction and HBM GB/s of the roofline kernel (counters of the committed PMC passes, labelled)
    assert 0.0 < r["mfma_busy"] < 1.0 and 0.0 < r["hbm_gbps"] < 8000.0 and r["traffic"] > 0 and "profiles/" in r["traffic_source"]
    assert set(r["hbm_gbps_by_kernel"]) >= {"ad_node_kernel", "lq_node_kernel", "riccati_kernel", "wbc_kernel"}


@pytest.mark.gpu
def test_bench_scenario_every_instance_against_oracle(interface):
    """The bench's OWN scenario (bench.build_scenario: EE target from StartingPosition.h constants, schedule from qmgpu_tile_gait) -- all 256 instances of
    one cycle against the multi-threaded oracle, not only `results_finite_and_converged`."""
    import numpy as np
    import torch
    import bench
    import gpu_harness as G
    import support as S
    B, N = bench.BATCH_PER_GPU, bench.HORIZON_N
    sc = bench.build_scenario(interface, B, seed=0)
    sol = G.make_solver(interface, B, N)
    mb = G.MpcBatch(sc["x0"], sc["tt"], sc["ts"], np.full(B, sc["nev"], dtype=np.int32), np.tile(sc["ev"], (B, 1)), np.tile(sc["md"], (B, 1)), N)
    wb = G.WbcBatch(sc["rbd"], np.full(B, 0.002), np.full(B, 20.0), np.zeros((B, 30)))
    sol.cycle(mb.args, G.dev(np.zeros(B), torch.float64), wb.args)
    got = mb.results(); got.update(wb.results())
    ref = S.Oracle(interface.problem, fast=True).cycle_batch(N, sc["x0"], sc["tt"], sc["ts"], sc["nev"], sc["ev"], sc["md"], rbd=sc["rbd"])
    S.assert_parity(S.parity_report("bench_scenario_configs1_256xN100", got, ref))


def test_bench_two_ranks_on_the_emulation_path(tmp_path):
    """CPU: `python bench.py --gpus 2` without a launcher environment starts its own two ranks (torch.distributed.run on 127.0.0.1); with --emulate
    the kernels are the host-emulated ones and the collective runs over gloo.  End to end: configs[2] shards of ONE global batch, all-gather, the line,
    and rank 0's dump of what the gather delivered (every rank's instances)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--emulate", "--batch-per-gpu", "2", "--nodes", "4", "--steps", "1", "--warmup", "0",
                        "--full", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                       # rank 0 prints the one line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 1
    cfg = d["config"]
    assert cfg["workload"].startswith("configs[2]: ONE global batch of 4") and cfg["global_batch"] == 4 and cfg["batch_per_gpu"] == 2
    assert cfg["gather_matches_local_results"] is True and cfg["results_finite_and_converged"] is True
    assert len(cfg["per_rank_value"]) == 2 and cfg["collective"].startswith("all_gather")
    assert "EMULATED" in d["data"] and "cpu_baseline" not in d
    X, mode = np.load(tmp_path / "X.npy"), np.load(tmp_path / "mode.npy")
    assert X.dtype == np.float64 and X.shape == (4, 5, 30) and mode.shape == (4, 5) and np.isfinite(X).all()
    assert sorted(f.name for f in tmp_path.iterdir()) == ["U.npy", "X.npy", "mode.npy", "wbc_out.npy"]


def test_bench_eight_ranks_take_the_whole_global_batch_on_the_emulation_path():
    """CPU: the launch the driver makes on an 8-GPU node -- eight ranks, configs[2]'s ONE global batch taken WHOLE (the branch no 1- or 2-rank run reaches), contiguous
    shards, all-gather, the line -- at toy size on the host-emulated kernels over gloo (--global-batch 8: one instance per rank)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--emulate", "--batch-per-gpu", "1", "--global-batch", "8", "--nodes", "4", "--steps", "1",
                        "--warmup", "0", "--full"], capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    cfg = d["config"]
    assert d["n_gpus"] == 8 and cfg["global_batch"] == 8 and cfg["batch_per_gpu"] == 1 and len(cfg["per_rank_value"]) == 8
    assert cfg["workload"].startswith("configs[2]: ONE global batch of 8 MPC instances (all of the 8 of seed 1)")
    assert cfg["gather_matches_local_results"] is True and cfg["results_finite_and_converged"] is True


HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")
FULL_ONLY = ("roofline", "cpu_baseline")
FULL_ONLY_CONFIG = ("results_finite_and_converged", "gather_matches_local_results", "steady_state", "batch_sweep")


def test_bench_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """CPU (host-emulated kernels, one rank): without --full the line is the headline and nothing else, --steps is the number of timed steps, and
    --dump-outputs writes the last step's results as float64 .npy files -- the same numbers in two runs with the same arguments, and in a --full run."""
    import numpy as np
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--emulate", "--batch-per-gpu", "2", "--nodes", "4", "--steps", "2", "--warmup", "1"]
    dumps = []
    for i, extra in enumerate(([], [], ["--full"])):
        d_out = tmp_path / str(i)
        p = subprocess.run(cmd + extra + ["--dump-outputs", str(d_out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert all(k in d for k in HEADLINE) and d["steps"] == 2 and d["warmup"] == 1 and d["dtype"] == "f64" and d["higher_is_better"] is True
        assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-9 * d["value"]          # B instances per step over the step's milliseconds
        if extra:
            assert "roofline" in d and d["config"]["results_finite_and_converged"] is True
        else:
            assert not [k for k in FULL_ONLY if k in d] and not [k for k in FULL_ONLY_CONFIG if k in d["config"]]
        dumps.append({f.name: np.load(f) for f in d_out.iterdir()})
    assert sorted(dumps[0]) == ["T.npy", "U.npy", "X.npy", "mode.npy", "stats.npy", "wbc_input_last.npy", "wbc_out.npy", "wbc_status.npy"]
    assert dumps[0]["X.npy"].shape == (2, 5, 30) and dumps[0]["wbc_out.npy"].shape == (2, 54)
    for name, a in dumps[0].items():
        assert a.dtype == np.float64 and np.isfinite(a).all(), name
        assert np.array_equal(a, dumps[1][name]) and np.array_equal(a, dumps[2][name]), name


def test_dump_outputs_keeps_a_fixed_seeded_sample_under_the_limit(tmp_path):
    """bench.dump_outputs: above the size limit the same seeded subset of instances is taken from every array, its indices are stored next to them,
    and the files stay within the limit; below it everything is written as it is."""
    import numpy as np
    import bench
    rng = np.random.default_rng(3)
    arrays = dict(X=rng.standard_normal((1000, 11, 30)), mode=rng.integers(0, 15, (1000, 11)).astype(np.int32))
    limit = 1 << 20
    for d_out in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d_out), arrays, limit=limit)
    names = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert names == ["X.npy", "instances.npy", "mode.npy"]
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= limit
    idx = np.load(tmp_path / "a" / "instances.npy").astype(np.int64)
    assert 0 < len(idx) < 1000 and (np.diff(idx) > 0).all()
    X, mode = np.load(tmp_path / "a" / "X.npy"), np.load(tmp_path / "a" / "mode.npy")
    assert X.dtype == mode.dtype == np.float64 and np.array_equal(X, arrays["X"][idx]) and np.array_equal(mode, arrays["mode"][idx])
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    assert sorted(f.name for f in (tmp_path / "c").iterdir()) == ["X.npy", "mode.npy"] and np.array_equal(np.load(tmp_path / "c" / "X.npy"), arrays["X"])


@pytest.mark.gpu
def test_bench_plain_run_on_the_gpu(tmp_path):
    """The command every change is measured with, on the GPU: the headline only, and the dump of the last timed step (256 instances, N = 100)."""
    import numpy as np
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    d = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert all(k in d for k in HEADLINE) and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in d] and not [k for k in FULL_ONLY_CONFIG if k in d["config"]]
    X, out, status = np.load(tmp_path / "X.npy"), np.load(tmp_path / "wbc_out.npy"), np.load(tmp_path / "wbc_status.npy")
    assert X.shape == (256, 101, 30) and out.shape == (256, 54) and np.isfinite(X).all() and np.isfinite(out).all() and (status == 0).all()
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20


def test_bench_refuses_a_changed_workload_outside_the_emulation():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch-per-gpu", "8"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "BASELINE" in (p.stderr + p.stdout)


def test_a_rank_that_fails_before_the_first_barrier_ends_the_whole_job_promptly():
    """VERDICT r03 missing 1: N > 1 has never run on hardware here, so what can be checked without it is.  One of two ranks raises before the first barrier
    (QM_BENCH_FAIL_RANK): the job must exit non-zero within seconds -- not sit in dist.barrier() until a 30-minute collective timeout -- and say which rank failed."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["QM_BENCH_FAIL_RANK"] = "1"
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--emulate", "--batch-per-gpu", "2", "--nodes", "4", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    took = time.time() - t0
    assert p.returncode != 0
    assert "[bench] rank 1 of 2 failed: RuntimeError: injected failure" in p.stderr, p.stderr[-3000:]
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]          # no result line from a job that lost a rank
    assert took < 120, took


def test_rank_to_device_mapping_honours_the_visible_devices():
    """LOCAL_RANK -> device: torch.cuda.device_count() already reflects HIP_VISIBLE_DEVICES, so a launcher that starts more ranks than visible devices is
    reported as such (with the variable's value) instead of surfacing as an invalid device ordinal from the first allocation."""
    import bench
    assert [bench.device_for_rank(r, 8) for r in range(8)] == list(range(8))
    assert bench.device_for_rank(1, 2, visible="3,5") == 1                      # the SECOND visible device, whatever its physical index
    for bad in ((2, 2), (8, 8), (-1, 4), (0, 0)):
        with pytest.raises(SystemExit) as e:
            bench.device_for_rank(*bad, visible="0,1")
        assert "LOCAL_RANK" in str(e.value) and "HIP_VISIBLE_DEVICES=0,1" in str(e.value)


@pytest.mark.gpu
def test_bench_refuses_a_local_rank_without_a_device():
    """On a one-GPU box: LOCAL_RANK 1 must fail at once with the attributed message."""
    env = dict(os.environ, LOCAL_RANK="1", HIP_VISIBLE_DEVICES="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-steady-state"], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)
    assert p.returncode != 0 and "LOCAL_RANK 1 has no GPU" in (p.stderr + p.stdout)
