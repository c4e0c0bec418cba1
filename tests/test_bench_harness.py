"""CPU, world_size 2, gloo: bench.py's OWN multi-rank code path -- what the driver launches on an 8-GPU node as
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...` -- run as two processes on the CPU emulation of the kernel layer
(CNR_BENCH_EMU_LIB, test infrastructure) in its BASELINE C4 form (--scaling strong: a fixed batch split over the ranks), against the
single-process run of the same batch: same rays_per_step_total, the parallelism the line reports, and the same loss after the same steps
(the ray-sharded objective equals the single-process objective; parallel.py and tests/test_sharded_gloo.py cover the pieces, this covers the
harness that assembles them)."""
import json
import os
import socket
import subprocess
import sys

import pytest

import _native as N

pytestmark = pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, rays_total, extra=(), launcher=True, scaling="strong", threads=2):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(CNR_BENCH_EMU_LIB=N.EMU_LIB, OMP_NUM_THREADS=str(threads), MASTER_ADDR="127.0.0.1")
    args = ["bench.py", "--gpus", str(world), "--steps", "2", "--warmup", "1", "--scaling", scaling, "--rays-total", str(rays_total), *extra]
    if world == 1 or not launcher:     # plain `python bench.py --gpus N`: bench.py starts its N ranks itself
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]          # rank 0 prints ONE JSON line
    return json.loads(lines[0])


_single = {}


def _one():   # the single-process run of the 16-ray batch, once per session
    if "d" not in _single:
        _single["d"] = _run(1, 16)
    return _single["d"]


def test_bench_two_ranks_strong_scaling_line_matches_single_process():
    one = _one()
    two = _run(2, 16)
    for d, w in ((one, 1), (two, 2)):
        assert d["emulation"] is True and d["n_gpus"] == w and d["scaling"] == "strong" and d["steps"] == 2 and d["warmup"] == 1
        assert d["metric"].startswith("rays/sec") and d["unit"] == "rays/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
        assert d["config"]["rays_per_step_total"] == 16 and d["config"]["rays_per_step_per_gpu"] == 16 // w
        assert d["config"]["parallelism"] == "ray-sharded dp%d" % w
        assert abs(d["value"] - 16 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-3 * d["value"] + 0.1     # value = all ranks' rays / max-over-ranks time
    assert "allreduce" in two["config"]["step"] and "allreduce" not in one["config"]["step"]
    # strong scaling: the two ranks split the single-process batch and its jitter draw, the loss terms are reduced over the ranks before
    # backward and the gradients after it -- so after the same 3 optimiser steps (1 warm-up + 2 timed) the reported loss of the last step
    # equals the single-process one up to the summation order of the reductions
    assert abs(one["config"]["final_loss"] - two["config"]["final_loss"]) <= 2e-5 * abs(one["config"]["final_loss"]), (one["config"]["final_loss"], two["config"]["final_loss"])


def test_bench_four_ranks_strong_scaling_matches_single_process():
    """The same with four ranks (the slices, the jitter rows and the two reductions do not depend on the rank count being two): the C4 form at
    8 GPUs is this code with world = 8."""
    one = _one()
    four = _run(4, 16)
    assert four["n_gpus"] == 4 and four["config"]["rays_per_step_per_gpu"] == 4 and four["config"]["parallelism"] == "ray-sharded dp4"
    assert abs(one["config"]["final_loss"] - four["config"]["final_loss"]) <= 2e-5 * abs(one["config"]["final_loss"]), (one["config"]["final_loss"], four["config"]["final_loss"])


def test_bench_eight_ranks_c4_shape_matches_single_process():
    """BASELINE C4 is EIGHT ranks splitting one batch (512 rays per GPU of 4096): the same harness with world = 8 (two rays per rank here -- the
    emulation renders ~100 rays/s -- the code path does not depend on the shard size): slices, jitter rows, the 5-float reduction before backward
    and the gradient all-reduce after it reproduce the single-process loss after 3 optimiser steps."""
    one = _one()
    eight = _run(8, 16, threads=1)
    assert eight["n_gpus"] == 8 and eight["config"]["rays_per_step_per_gpu"] == 2 and eight["config"]["parallelism"] == "ray-sharded dp8"
    assert eight["config"]["rays_per_step_total"] == 16 and "allreduce" in eight["config"]["step"]
    assert abs(one["config"]["final_loss"] - eight["config"]["final_loss"]) <= 2e-5 * abs(one["config"]["final_loss"]), (one["config"]["final_loss"], eight["config"]["final_loss"])


def test_default_invocation_carries_both_scaling_figures():
    """The driver's command is fixed (`bench.py --gpus N --full`, weak scaling): the same invocation must also yield the strong-scaling figure of BASELINE C4
    -- a `strong_scaling` object: --rays-total rays of ONE view split over the ranks, the same batch on one rank alone, speed-up and efficiency."""
    d = _run(2, 16, extra=("--rays", "8", "--full"), scaling="weak")
    assert d["scaling"] == "weak" and d["n_gpus"] == 2 and d["config"]["rays_per_step_per_gpu"] == 8 and d["config"]["rays_per_step_total"] == 16
    s = d["strong_scaling"]
    assert s["scaling"] == "strong" and s["rays_total"] == 16 and s["rays_per_gpu"] == 8 and s["unit"] == "rays/s"
    assert abs(s["value"] - 16 / (s["ms_per_step"] * 1e-3)) <= 1e-3 * s["value"] + 0.1
    one = s["one_gpu_same_batch"]
    assert abs(one["value"] - 16 / (one["ms_per_step"] * 1e-3)) <= 1e-3 * one["value"] + 0.1
    assert abs(s["speedup_vs_one_gpu_same_batch"] - one["ms_per_step"] / s["ms_per_step"]) < 2e-3 * s["speedup_vs_one_gpu_same_batch"] + 1e-3
    assert abs(s["efficiency_vs_n1_same_batch"] - s["speedup_vs_one_gpu_same_batch"] / 2) < 1e-3
    assert "strong_scaling" not in _run(1, 16, extra=("--rays", "8", "--full"), scaling="weak")     # one rank: nothing to split


def test_plain_run_times_the_headline_step_only():
    """Without --full the line holds the headline figure and nothing that takes a run of its own (here: the strong-scaling side leg at N = 2)."""
    d = _run(2, 16, extra=("--rays", "8"), scaling="weak")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and abs(d["value"] - 16 * 2 / (d["ms_per_step"] * 2e-3)) <= 1e-3 * d["value"] + 0.1
    for k in ("strong_scaling", "step_ms", "roofline", "kernel_breakdown", "small_batch", "loss_only", "inference", "c5", "torch_gpu_baseline", "cpu_baseline"):
        assert k not in d, k


def test_dump_outputs_same_arguments_same_arrays(tmp_path):
    """--dump-outputs DIR: the last timed step's loss, renderer outputs, gradients and updated parameters as float32 / float64 .npy files; two runs
    with the same arguments start from the same inputs and (on this deterministic build) write the same arrays; the 64 MB bound cuts arrays to a
    fixed sample."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    runs = []
    for i in range(2):
        folder = tmp_path / ("run%d" % i)
        d = _run(1, 16, extra=("--dump-outputs", str(folder)))
        files = sorted(os.listdir(folder))
        assert "loss.npy" in files and "out.color_fine.npy" in files
        assert any(f.startswith("grad.sdf_network.") for f in files) and any(f.startswith("param.sdf_network.") for f in files)
        arrs = {f: np.load(folder / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= bench.DUMP_LIMIT_BYTES
        assert arrs["out.color_fine.npy"].shape == (16, 3)
        assert abs(float(arrs["loss.npy"]) - d["config"]["final_loss"]) <= 1e-6 * abs(d["config"]["final_loss"])
        runs.append(arrs)
    assert runs[0].keys() == runs[1].keys()
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f
    # the bound: a small limit keeps every array within it and cuts the longest ones to the same seeded entries each time
    import torch
    g = torch.Generator().manual_seed(0)
    lin = torch.nn.Linear(64, 32)
    lin.weight.grad = torch.randn(32, 64, generator=g)
    out = {"big": torch.randn(1000, 3, generator=g), "small": torch.randn(5, generator=g)}
    cut = []
    for i in range(2):
        folder = tmp_path / ("cut%d" % i)
        bench.dump_outputs(str(folder), torch.tensor(1.5), out, lin, limit=4 * 1200)
        arrs = {f: np.load(folder / f) for f in sorted(os.listdir(folder))}
        assert sum(a.nbytes for a in arrs.values()) <= 4 * 1200
        assert arrs["out.small.npy"].shape == (5,) and arrs["param.bias.npy"].shape == (32,)
        big = out["big"].reshape(-1).numpy()
        assert np.isin(arrs["out.big.npy"], big).all() and arrs["out.big.npy"].size < big.size
        cut.append(arrs)
    for f in cut[0]:
        assert np.array_equal(cut[0][f], cut[1][f]), f


def test_plain_gpus_2_starts_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it must run TWO ranks (it used to run one and print n_gpus 1)."""
    d = _run(2, 16, launcher=False)
    assert d["n_gpus"] == 2 and d["config"]["rays_per_step_per_gpu"] == 8 and d["config"]["parallelism"] == "ray-sharded dp2"
    assert "allreduce" in d["config"]["step"]


def test_world_size_mismatch_fails():
    """--gpus that disagrees with the launcher's WORLD_SIZE is an error, never a record with the wrong GPU count."""
    env = dict(os.environ, CNR_BENCH_EMU_LIB=N.EMU_LIB, OMP_NUM_THREADS="2", MASTER_ADDR="127.0.0.1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), "bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0"]
    r = subprocess.run(cmd, cwd=ROOT, env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
