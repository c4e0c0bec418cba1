"""Image-evaluation micro-benchmark: color_neus_amd.image_metrics (cnr_image_metrics) and color_neus_amd.panel (cnr_image_panel) against a
stock-PyTorch stand-in on the same GPU, in one process, alternating.

python tools/bench_image.py [--reps R] [--out profiles/image_metrics_bench.txt]

Sizes: 800 x 800 x 3 and 1200 x 1600 x 3 seeded images, in the renderer's [H, W, 3] form and in kornia's [1, 3, H, W] form.  The stand-in
computes the same numbers the way stock PyTorch offers: F.conv2d with the 3 x 3 window on the reflect-padded planes for the same five
filtered maps (x, y, x*x, y*y, x*y), element-wise ops for the SSIM map, .mean() for the two scalars; for the panel, clamp / multiply / uint8
casts, a 256-entry table lookup for the depth and torch.cat.  Both sides are timed with device events around windows of 20 whole calls (allocations
and launches included) after one warm-up call of each.  The kernel times come from the library's timing records (events around each launch), and
the share of HBM bandwidth is the bytes each launch declares (inputs read once, outputs written once) over that time and the chip's
8 TB/s.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402

HBM_PEAK = 8.0e12
W1, W0 = float.fromhex("0x1.3b3046p-2"), float.fromhex("0x1.899f76p-2")


def standin_metrics(x, y):
    """x, y [B, C, H, W] -> (mse, mean ssim) by conv2d on reflect-padded planes"""
    b, c, h, w = x.shape
    g = torch.tensor([W1, W0, W1], device=x.device)
    k = (g[:, None] * g[None, :])[None, None]
    maps = torch.cat([x, y, x * x, y * y, x * y]).reshape(5 * b * c, 1, h, w)
    mu1, mu2, e11, e22, e12 = F.conv2d(F.pad(maps, (1, 1, 1, 1), mode="reflect"), k).reshape(5, b, c, h, w)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    ssim = ((2 * m12 + 1e-4) * (2 * (e12 - m12) + 9e-4)) / (((m11 + m22) + 1e-4) * (((e11 - m11) + (e22 - m22)) + 9e-4) + 1e-12)
    return ((x - y) ** 2).mean(dtype=torch.float64), ssim.mean(dtype=torch.float64)


def standin_panel(gt, render, depth, table):
    q = lambda v: (v * 255.0).clamp(0.0, 255.0).to(torch.uint8)
    vmin, vmax = depth.min(), depth.max()
    lvl = ((depth - vmin) / (vmax - vmin) * 255.0).clamp(0.0, 255.0).to(torch.int64)
    return torch.cat([q(gt), q(render), table[lvl]], dim=1)


INNER = 20      # calls per timed window: one call is a fraction of a millisecond


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER, out


def alternate(sides, reps):
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    outs = {}
    for _ in range(reps):
        for k, fn in sides.items():
            dt, outs[k] = timed(fn)
            ms[k].append(dt)
    return ms, outs


def kernel_records(lib, fn):
    lib.timing_enable(True)
    fn()
    recs = lib.timing_collect()
    lib.timing_enable(False)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_metrics_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_image.py needs a GPU (no fallback)")
    lib = cn.load_library()
    lines = [f"image evaluation on {torch.cuda.get_device_name(0)}, library {lib.backend}: kernel = color_neus_amd.image_metrics / panel, "
             f"stand-in = stock PyTorch ops (tools/bench_image.py), {a.reps} alternating repeats of {INNER} calls, whole-call times by device events (median, min, max)",
             "kernel lines: time from the library's timing records, bytes as declared by the launch (inputs once, outputs once); images of these sizes fit in the "
             "256 MB last-level cache, so part of the declared bytes may not have come from HBM"]
    fmt = lambda v: f"{statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"
    table = cn.cmap(torch.arange(256, dtype=torch.float32, device="cuda").reshape(16, 16)).reshape(256, 3)
    for h, w in ((800, 800), (1200, 1600)):
        g = torch.Generator().manual_seed(h * w)
        gt = torch.rand(h, w, 3, generator=g).cuda()
        render = (gt + 0.05 * torch.randn(h, w, 3, generator=g).cuda()).clamp(0.0, 1.0)
        depth = (1.5 + torch.randn(h, w, generator=g)).cuda()
        x4, y4 = gt.permute(2, 0, 1)[None].contiguous(), render.permute(2, 0, 1)[None].contiguous()
        for tag, xk, yk in (("[H, W, 3]", gt, render), ("[1, 3, H, W]", x4, y4)):
            ms, outs = alternate({"kernel": lambda: cn.image_metrics(xk, yk), "standin": lambda: standin_metrics(x4, y4)}, a.reps)
            km, sm = outs["kernel"], outs["standin"]
            lines.append(f"{h} x {w} x 3 metrics {tag}: kernel {fmt(ms['kernel'])}, stand-in {fmt(ms['standin'])}, "
                         f"ratio stand-in / kernel {statistics.median(ms['standin']) / statistics.median(ms['kernel']):.2f}; "
                         f"ssim {km['ssim'].item():.9f} vs {sm[1].item():.9f}, mse {km['mse'].item():.6e} vs {sm[0].item():.6e}")
            for r in kernel_records(lib, lambda: cn.image_metrics(xk, yk)):
                lines.append(f"    {r[0]}: {r[7] * 1e3:.1f} us, {r[8] / 1e6:.2f} MB declared = {100.0 * r[8] / (r[7] * 1e-3) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s")
        ms, outs = alternate({"kernel": lambda: cn.panel(gt, render, depth), "standin": lambda: standin_panel(gt, render, depth, table)}, a.reps)
        same = (outs["kernel"] == outs["standin"]).float().mean().item()
        lines.append(f"{h} x {w} panel: kernel {fmt(ms['kernel'])}, stand-in {fmt(ms['standin'])}, "
                     f"ratio stand-in / kernel {statistics.median(ms['standin']) / statistics.median(ms['kernel']):.2f}; {100.0 * same:.4f} % of the bytes equal")
        for r in kernel_records(lib, lambda: cn.panel(gt, render, depth)):
            lines.append(f"    {r[0]}: {r[7] * 1e3:.1f} us, {r[8] / 1e6:.2f} MB declared = {100.0 * r[8] / (r[7] * 1e-3) / HBM_PEAK:.1f} % of {HBM_PEAK / 1e12:.0f} TB/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
