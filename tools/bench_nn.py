"""Nearest-neighbour search micro-benchmark: color_neus_amd.metrics.nearest_neighbors (cnr_nn_search) against the stock-PyTorch stand-in, a
chunked torch.cdist(...).min(1) whose distance tile is sized to a fixed scratch budget, on the same GPU, in one process, alternating.

python tools/bench_nn.py [--reps R] [--budget-mib M]

Sizes: 2^17 x 2^17, 2^20 x 2^20 and 4096 x 2^20 seeded normal clouds.  Timed with device events after one warm-up call of each side.  Per size:
the times of every repeat (median / min / max), pairs per second, the fp32 arithmetic the kernel does per pair (3 subtractions, 3
multiplications, 2 additions = 8 operations; the compare and the two selects are not counted) over the kernel time as a share of the chip's
fp32 vector peak (157.3 TFLOP/s, which counts a fused multiply-add as two operations per lane and clock: a kernel that may not fuse cannot pass
50 %), and the ratio to the stand-in.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12
OPS_PER_PAIR = 8


def standin(q, t, budget_bytes):
    """min_j |q_i - t_j| and its index by stock PyTorch: cdist tiles of at most budget_bytes, reduced tile by tile."""
    rows = max(1, budget_bytes // (4 * t.shape[0]))
    d = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    j = torch.empty(q.shape[0], dtype=torch.int64, device=q.device)
    for s in range(0, q.shape[0], rows):
        d[s:s + rows], j[s:s + rows] = torch.cdist(q[s:s + rows], t).min(dim=1)
    return d, j


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget-mib", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_nn.py needs a GPU (no fallback)")
    lib = cn.load_library()
    print(f"device {torch.cuda.get_device_name(0)}, library {lib.backend}, stand-in tile budget {a.budget_mib} MiB, {a.reps} alternating repeats")
    budget = a.budget_mib << 20
    for n, m in ((1 << 17, 1 << 17), (1 << 20, 1 << 20), (4096, 1 << 20)):
        g = torch.Generator().manual_seed(n + m)
        q, t = torch.randn(n, 3, generator=g).cuda(), torch.randn(m, 3, generator=g).cuda()
        sides = {"kernel": lambda: cn.metrics.nearest_neighbors(q, t), "standin": lambda: standin(q, t, budget)}
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                dt, out = timed(fn)
                ms[k].append(dt)
                if k == "kernel":
                    d2, idx = out
                else:
                    agree = (out[1] == idx).float().mean().item()
        med = {k: statistics.median(v) for k, v in ms.items()}
        pairs = float(n) * float(m)
        print(f"{n} x {m}: kernel {med['kernel']:.3f} ms (min {min(ms['kernel']):.3f}, max {max(ms['kernel']):.3f}), "
              f"stand-in {med['standin']:.3f} ms (min {min(ms['standin']):.3f}, max {max(ms['standin']):.3f}), "
              f"ratio stand-in / kernel {med['standin'] / med['kernel']:.2f}")
        print(f"    {pairs / (med['kernel'] * 1e-3):.3e} pairs/s, {OPS_PER_PAIR} fp32 ops/pair = {OPS_PER_PAIR * pairs / (med['kernel'] * 1e-3) / 1e12:.1f} TFLOP/s = "
              f"{100.0 * OPS_PER_PAIR * pairs / (med['kernel'] * 1e-3) / FP32_VECTOR_PEAK:.1f} % of the fp32 vector peak; "
              f"stand-in picks the same index for {100.0 * agree:.3f} % of the queries (it is not exact)")
    lib.timing_enable(True)
    cn.metrics.nearest_neighbors(q, t)
    print("    launches of the last size:", ", ".join(f"{r[0]} {r[7]:.3f} ms" for r in lib.timing_collect()))
    lib.timing_enable(False)


if __name__ == "__main__":
    main()
