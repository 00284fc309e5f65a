"""bench.py's launch contract: `python bench.py --gpus N` starts N ranks itself
(one process per device, configs/trainer/ddp.yaml:8-13) and rank 0 prints ONE
JSON line carrying n_gpus == N."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_world_size_mismatch_is_refused():
    """A launcher that started a different number of ranks than --gpus must not
    silently measure something else (round-1 defect: --gpus was ignored)."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_gpus_2_spawns_two_ranks_share_gpu():
    """1-GPU box: SPT_BENCH_SHARE_GPU=1 puts both ranks on cuda:0 over gloo, so the
    N > 1 code path (spawn, scene sharding, flat gradient all-reduce, barrier,
    max-over-ranks) is executed end to end from the bare `--gpus 2` command."""
    env = dict(os.environ, SPT_BENCH_SHARE_GPU="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--settle", "1.0",      # the settle phase holds a collective per step too
                        "--scene", "T", "--full", "--no-cpu-baseline", "--no-preprocess"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2
    assert out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0
    # every line of a scaling run carries the north-star kernel's measurement (rank 0, stand-alone)
    assert out["roofline"]["achieved"] and 0 < out["roofline"]["frac"] <= 1
    assert out["cpu_baseline"] is None           # N = 1 only, by the bench contract


def test_world_size_from_the_launcher_is_taken_when_gpus_is_not_given():
    """`torchrun --nproc-per-node=2 bench.py` (no --gpus): the ranks must run, not exit on a
    mismatch with a default of 1 (here they stop at the missing GPU, a different message)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT="29999", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, BENCH, "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    msg = (r.stdout + r.stderr)
    assert "launcher started" not in msg
    assert r.returncode != 0 and "MI355X" in msg


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_module", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dumped_outputs_are_float_within_the_limit_and_the_same_sample_every_time(tmp_path):
    bench = _bench_module()
    g = torch.Generator().manual_seed(1)
    arrays = {"loss": torch.tensor(2.5), "big": torch.randn(200_000, 64, generator=g),
              "f64": torch.randn(500, 13, generator=g, dtype=torch.float64),
              "half": torch.randn(40, 4, generator=g).bfloat16(), "ids": torch.arange(7)}
    limit = 10 * 10 ** 6
    for run in ("a", "b"):
        written = bench.write_outputs(arrays, str(tmp_path / run), limit=limit)
        assert set(written) == set(arrays)
    total = 0
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == (np.float64 if t.dtype == torch.float64 else np.float32), name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= limit
    # the small arrays whole, the big one as a sample of whole rows
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(2.5)
    assert np.array_equal(np.load(tmp_path / "a" / "f64.npy"), arrays["f64"].numpy())
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.shape[1] == 64 and 0 < big.shape[0] < 200_000
    rows = {r.tobytes() for r in arrays["big"].numpy()}
    assert all(r.tobytes() in rows for r in big)


def _plain_run(out_dir, settle):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "8", "--warmup", "4",
                        "--settle", str(settle), "--scene", "T", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dumped_outputs_are_the_same_every_run(tmp_path):
    """A plain run prints the headline fields and none of the --full legs; what its last timed step
    computed (loss, gradients) is the same, to rounding, in two runs of the same step counts - the
    settle phases differ, and 12 training steps precede the last one."""
    a = _plain_run(tmp_path / "a", 0)
    b = _plain_run(tmp_path / "b", 0.5)
    for line in (a, b):
        assert line["steps"] == 8 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "Mpoints/s" and line["higher_is_better"] is True
        for leg in ("roofline", "cpu_baseline", "preprocess", "local_graph", "train_batch",
                    "ms_per_step_f32_exact", "ms_per_step_bf16", "collective"):
            assert line[leg] is None, leg
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == ["grad_flat.npy", "loss.npy"]
    assert np.load(tmp_path / "a" / "grad_flat.npy").size > 100_000        # SPT-64: 213 k parameters
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape, n
        assert np.isfinite(x).all(), n
        total += os.path.getsize(tmp_path / "a" / n)
        # float atomics in the backward: rounding of the sums, relative to the output's scale
        scale = max(float(np.abs(x).max()), 1e-30)
        assert float(np.abs(x.astype(np.float64) - y).max()) <= 1e-4 * scale, n
    assert total <= 64 * 10 ** 6
