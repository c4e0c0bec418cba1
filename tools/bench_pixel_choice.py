"""What choosing the pixels of a masked training batch costs, per source (a measuring tool; bench.py does not use it).

  host     rays.choose_pixels: the reference's CPU random stream -- two nonzero over the whole mask stack, randperm(#fg) and randperm(#bg) on
           the host, an index upload (the default route, unchanged)
  sampler  rays.PixelSampler.draw: cnr_choose_pixels on the pixel table of the resident mask stack (one launch, no host synchronisation)

At the shipped DTU batch shape (INCLUDE_MASK, BATCH_SIZE 8, N_RAYS 1024: a mask stack of 8 x 1200 x 1600), mask_rate 0.5 and 0.8:
1. pixel choice alone: host by wall clock around a call that ends in a device synchronise, sampler by device events around blocks of draws
2. the table build (cnr_pixel_table_build) for 8 and for 49 images, device events
3. the training step rays_for_training -> renderer -> fused loss -> backward -> ClipAdam with each source, blocks alternated, wall clock around
   blocks that end in a device synchronise (the host route is host time, so wall clock is the common measure); the sampler also feeds the
   renderer's jitter draw
Warm-up first; median, minimum and maximum over the blocks.  One GPU process; run it under a time limit.

Usage: python tools/bench_pixel_choice.py [--out FILE] [--blocks 5] [--host-steps 3] [--steps 40]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import color_neus_amd as cn  # noqa: E402
from color_neus_amd import rays as raygen, synthetic  # noqa: E402

H, W, BATCH, N_RAYS = 1200, 1600, 8, 1024


def make_masks(dev, n, seed=0):
    """[n, H, W] masks, about 30 % foreground: an ellipse per image, its centre and axes jittered."""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev), indexing="ij")
    out = torch.empty(n, H, W, device=dev)
    for i in range(n):
        cy, cx, ay, ax = (torch.rand(4, generator=g) * torch.tensor([0.1, 0.1, 0.06, 0.06]) + torch.tensor([0.45, 0.45, 0.28, 0.31])).tolist()
        out[i] = ((((y / H - cy) / ay) ** 2 + ((x / W - cx) / ax) ** 2) < 1.0).float()
    return out


def make_c2w(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1) * 2.7
    fwd = -c / c.norm(dim=-1, keepdim=True)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)), dim=-1)
    c2w = torch.eye(4).repeat(n, 1, 1)
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, torch.linalg.cross(fwd, right), fwd, c
    return c2w


def wall_blocks(fns, steps, blocks, warmup):
    """fns: {name: callable}, steps: {name: steps per block}; blocks alternated; {name: [ms per step of each block]} by wall clock around blocks
    that end in a device synchronise."""
    for k, f in fns.items():
        for _ in range(warmup[k]):
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(blocks):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps[k]):
                f()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3 / steps[k])
    return out


def event_blocks(f, iters, blocks, warmup):
    for _ in range(warmup):
        f()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def fmt(ms):
    return f"{statistics.median(ms):12.4f} {min(ms):12.4f} {max(ms):12.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixel_choice needs a GPU: it measures device time (there is no CPU fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    masks = make_masks(dev, BATCH)
    fg_share = float(masks.mean())
    lines = [f"pixel choice on {torch.cuda.get_device_name(0)}, host with {torch.get_num_threads()} torch threads: mask stack {BATCH} x {H} x {W} "
             f"({fg_share:.1%} foreground), {N_RAYS} rays",
             "   host = rays.choose_pixels (the reference's CPU stream), sampler = rays.PixelSampler.draw (cnr_choose_pixels)"]

    sampler = cn.PixelSampler(masks, seed=1)
    lines.append(f"1. pixel choice alone; host: wall clock per call incl. the device synchronise, {args.blocks} blocks of {args.host_steps} calls; "
                 f"sampler: device events, {args.blocks} blocks of 200 draws")
    lines.append("   mask_rate  source     median ms       min ms       max ms")
    for rate in (0.5, 0.8):
        torch.manual_seed(0)
        host = wall_blocks({"h": lambda: raygen.choose_pixels(N_RAYS, H * W, dev, masks, rate)}, {"h": args.host_steps}, args.blocks, {"h": 1})["h"]
        samp = event_blocks(lambda: sampler.draw(N_RAYS, rate, jitter=True), 200, args.blocks, 20)
        lines.append(f"   {rate:9.1f}  host    {fmt(host)}")
        lines.append(f"   {rate:9.1f}  sampler {fmt(samp)}")

    lines.append(f"2. table build (cnr_pixel_table_build: count, scan, scatter), device events, {args.blocks} blocks of 10 builds")
    lines.append("   images     median ms       min ms       max ms    GB/s (mask read twice + table written, median)")
    for n in (BATCH, 49):
        m = masks if n == BATCH else make_masks(dev, n, seed=3)
        s = sampler if n == BATCH else cn.PixelSampler(m, seed=1)
        ms = event_blocks(lambda: s.rebuild(m), 10, args.blocks, 3)
        lines.append(f"   {n:6d}  {fmt(ms)}   {12.0 * n * H * W / statistics.median(ms) * 1e-6:8.0f}")
        del m, s

    # ---- the training step with each source
    cfg = cn.RenderConfig(type="Color_NeuS", col_mode="no_view_dir", col_d_in=6, col_multires_view=0)
    g = torch.Generator().manual_seed(1)
    image = torch.rand(BATCH, H, W, 3, generator=g).to(dev)
    c2w, focal = make_c2w(BATCH).to(dev), torch.tensor([1.39 * W, 1.39 * H], device=dev)
    origin = torch.zeros(3)

    def make_step(source, rate):
        torch.manual_seed(0)
        renderer = synthetic.make_trained_like_(cn.ColorNeuSRenderer(cfg)).to(dev)
        params = list(renderer._ordered_params())
        opt = cn.ClipAdam(params, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=1.0, library=lib)
        smp = cn.PixelSampler(masks, seed=2) if source == "sampler" else None

        def f():
            o, d, near, far, rgb, msel = raygen.rays_for_training(c2w, focal, image, N_RAYS, origin, 1.0, normalize=True, mask=masks, mask_rate=rate,
                                                                  return_mask=True, library=lib, sampler=smp)
            if smp is not None:
                out = renderer(o, d, near, far, t_rand=smp.last_t_rand)
            else:
                out = renderer(o, d, near, far)
            loss, _ = cn.compute_loss_fused(out, rgb, msel, library=lib)
            for p in params:
                p.grad = None
            loss.backward()
            opt.step()
        return f

    lines.append(f"3. training step: rays_for_training -> renderer -> fused loss -> backward -> ClipAdam; wall clock per step over blocks ending in a "
                 f"device synchronise; {args.blocks} alternated blocks of {args.host_steps} (host) / {args.steps} (sampler) steps")
    lines.append("   mask_rate  source     median ms       min ms       max ms   rays/s (median)")
    for rate in (0.5, 0.8):
        res = wall_blocks({"host": make_step("host", rate), "sampler": make_step("sampler", rate)}, {"host": args.host_steps, "sampler": args.steps},
                          args.blocks, {"host": 2, "sampler": 10})
        for k in ("host", "sampler"):
            lines.append(f"   {rate:9.1f}  {k:7s} {fmt(res[k])}   {N_RAYS / statistics.median(res[k]) * 1e3:10.0f}")
        lines.append(f"   {rate:9.1f}  host / sampler = {statistics.median(res['host']) / statistics.median(res['sampler']):.1f}")
        if not statistics.median(res["sampler"]) < statistics.median(res["host"]):
            lines.append("   !! the step with the sampler is NOT faster than the step with the host choice")
    assert raygen.bad_index_count() == 0
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
