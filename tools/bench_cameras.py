"""What the learnable-camera step costs on the GPU (a measuring tool; bench.py does not use it).

  A   color_neus_amd.Cameras: cnr_camera_forward + cnr_camera_backward, one launch each
  B   the same computation in stock PyTorch ops (float32 on the device): index, normalise, dot, cross, stack, cat, matmul, pow, mul and their
      autograd nodes -- what the reference's Pose_Net / Focal_Net run

1. cameras alone: forward + backward of (c2w, focal) for 8 ids out of 200 cameras, 6d, everything learnable; A and B alternated in one process,
   device events around blocks of iterations after warm-up, median and spread over the blocks.
2. the IHO-style step (learnable cameras -> rays_for_training -> renderer -> fused loss -> backward -> ClipAdam over renderer + camera
   parameters) at 512 and 1024 rays with A in front and with B in front, rays/s each.  Pixels are drawn without a mask (one host randint per
   step), so that the host-side pixel choice does not hide what is being compared.

--trace-part A|B runs a fixed number of bare forward + backward iterations of one side and nothing else: run it under
`rocprofv3 --kernel-trace --stats` and divide the total number of kernel dispatches by --trace-iters for the launches per iteration.

Usage: python tools/bench_cameras.py [--out FILE] [--iters 500] [--blocks 10] [--steps 50]"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import color_neus_amd as cn  # noqa: E402
from color_neus_amd import rays as raygen, synthetic  # noqa: E402


class TorchCameras(nn.Module):
    """B: Pose_Net (6d, with init_c2w) and Focal_Net (order 2, fx and fy) in stock torch ops."""

    def __init__(self, cams):
        super().__init__()
        self.H, self.W = cams.focal_net.H, cams.focal_net.W
        self.r, self.t = (nn.Parameter(p.detach().clone()) for p in (cams.pose_net.r, cams.pose_net.t))
        self.fx, self.fy = (nn.Parameter(p.detach().clone()) for p in (cams.focal_net.fx, cams.focal_net.fy))
        self.init_c2w = nn.Parameter(cams.pose_net.init_c2w.detach().clone(), requires_grad=False)

    def forward(self, ids):
        r, t = self.r[ids], self.t[ids]
        a1, a2 = r[..., :3], r[..., 3:]
        b1 = torch.nn.functional.normalize(a1, dim=-1)
        b2 = torch.nn.functional.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
        R = torch.stack((b1, b2, torch.cross(b1, b2, dim=-1)), dim=-2)
        c2w = torch.cat([R, t.unsqueeze(-1)], dim=-1)
        c2w = torch.cat([c2w, torch.zeros_like(c2w[:, 0:1])], dim=1)
        c2w[:, 3, 3] = 1.0
        c2w = c2w @ self.init_c2w[ids]
        return c2w, torch.stack([self.fx ** 2 * self.W, self.fy ** 2 * self.H])


def make_cameras(dev, n_cams, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(n_cams, 3, generator=g), dim=-1) * 2.7
    fwd = -c / c.norm(dim=-1, keepdim=True)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)), dim=-1)
    init = torch.eye(4).repeat(n_cams, 1, 1)
    init[:, :3, 0], init[:, :3, 1], init[:, :3, 2], init[:, :3, 3] = right, torch.linalg.cross(fwd, right), fwd, c
    pose = cn.PoseNet(n_cams, True, True, pose_mode="6d", init_c2w=init)
    with torch.no_grad():
        pose.r.add_(0.01 * torch.randn(n_cams, 6, generator=g))
        pose.t.add_(0.01 * torch.randn(n_cams, 3, generator=g))
    focal = cn.FocalNet(H, W, True, False, order=2, init_focal=np.array([1.39 * W, 1.39 * H], dtype=np.float32))
    return cn.Cameras(focal, pose).to(dev)


def timed_blocks(fns, iters, blocks, warmup):
    """fns: {name: callable}; alternated block by block; returns {name: [ms per iteration of each block]}."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters)
    return out


def summary(ms):
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--n-cams", type=int, default=200)
    ap.add_argument("--trace-part", choices=["A", "B"], default=None)
    ap.add_argument("--trace-iters", type=int, default=100)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cameras needs a GPU: it measures device time (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    H = W = 400
    cams_a = make_cameras(dev, args.n_cams, H, W)
    cams_b = TorchCameras(cams_a).to(dev)
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, args.n_cams, (8,), generator=g).to(dev)
    probe, fprobe = torch.randn(8, 4, 4, generator=g).to(dev), torch.randn(2, generator=g).to(dev)

    def alone(cams):
        params = [p for p in cams.parameters() if p.requires_grad]

        def f():
            for p in params:
                p.grad = None
            c2w, focal = cams(ids)
            torch.autograd.backward([c2w, focal], [probe, fprobe])
        return f

    fa, fb = alone(cams_a), alone(cams_b)
    fa(), fb()
    torch.cuda.synchronize()
    for ka, kb in (("pose_net.r", "r"), ("pose_net.t", "t"), ("focal_net.fx", "fx"), ("focal_net.fy", "fy")):
        a, b = dict(cams_a.named_parameters())[ka].grad, dict(cams_b.named_parameters())[kb].grad
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), (ka, "A and B disagree")
    if args.trace_part:
        f = fa if args.trace_part == "A" else fb
        for _ in range(args.trace_iters):
            f()
        torch.cuda.synchronize()
        print(f"trace part {args.trace_part}: {args.trace_iters} iterations (+ 1 of each side for the agreement check)")
        return

    lines = [f"learnable cameras on {torch.cuda.get_device_name(0)}: A = Cameras (cnr_camera_forward / cnr_camera_backward), B = stock PyTorch ops",
             f"1. cameras alone, forward + backward, 8 ids of {args.n_cams} cameras, 6d, all learnable; {args.blocks} alternated blocks of {args.iters} iterations, device events",
             "   side   median us/iter   min     max"]
    res = timed_blocks({"A": fa, "B": fb}, args.iters, args.blocks, 50)
    for k in ("A", "B"):
        med, lo, hi = summary(res[k])
        lines.append(f"   {k}      {med * 1e3:10.1f}   {lo * 1e3:7.1f} {hi * 1e3:7.1f}")
    lines.append(f"   B / A = {statistics.median(res['B']) / statistics.median(res['A']):.2f}")

    # ---- the IHO-style step
    cfg = cn.RenderConfig(type="Color_NeuS", col_mode="no_view_dir", col_d_in=6, col_multires_view=0)
    image = torch.rand(8, H, W, 3, generator=g).to(dev)
    origin = torch.zeros(3)

    def make_step(which, rays):
        torch.manual_seed(0)
        renderer = synthetic.make_trained_like_(cn.ColorNeuSRenderer(cfg)).to(dev)
        cams = make_cameras(dev, args.n_cams, H, W)
        if which == "B":
            cams = TorchCameras(cams).to(dev)
        params = list(renderer._ordered_params()) + [p for p in cams.parameters() if p.requires_grad]
        opt = cn.ClipAdam(params, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=1.0, library=lib)

        def f():
            c2w, focal = cams(ids)
            o, d, near, far, rgb, _ = raygen.rays_for_training(c2w, focal, image, rays, origin, 1.0, normalize=True, library=lib)
            out = renderer(o, d, near, far)
            loss, _ = cn.compute_loss_fused(out, rgb, None, library=lib)
            for p in params:
                p.grad = None
            loss.backward()
            opt.step()
        return f

    lines.append(f"2. IHO-style step: cameras -> rays_for_training -> renderer -> fused loss -> backward -> ClipAdam (renderer + cameras); "
                 f"{args.blocks} alternated blocks of {args.steps} steps")
    lines.append("   rays  side   median ms/step   min     max     rays/s (median)")
    for rays in (512, 1024):
        torch.manual_seed(2)
        res = timed_blocks({"A": make_step("A", rays), "B": make_step("B", rays)}, args.steps, args.blocks, 10)
        for k in ("A", "B"):
            med, lo, hi = summary(res[k])
            lines.append(f"   {rays:4d}  {k}      {med:10.3f}   {lo:7.3f} {hi:7.3f}   {rays / med * 1e3:10.0f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
