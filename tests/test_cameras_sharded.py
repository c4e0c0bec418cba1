"""CPU, world_size 2, gloo (the harness of tests/test_sharded_gloo.py): learnable cameras in the ray-sharded data-parallel step.

Every rank builds the rays of one batch drawn from 4 cameras and renders its half; after ``parallel.allreduce_gradients`` over the renderer's
parameters plus the cameras' every rank holds the single-process camera gradients and the renderer gradients the unchanged path gives, and the
renderer's flat gradient buffer was reduced in place: the sizes handed to ``dist.all_reduce`` are that buffer and one small gathered message."""
import os
import socket

import multiprocessing as mp
import numpy as np
import pytest
import torch
import torch.distributed as dist

import _golden as G
import _native as N

pytestmark = pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
R, H, W, N_CAMS = 32, 16, 16, 4


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup():
    import color_neus_amd as cn
    from oracle import colorneus_oracle as O
    ocfg = G.CONFIGS["tiny_sharp"]()
    renderer = N.make_renderer(ocfg, O.init_params(ocfg, seed=5, trained_like=True), N.EMU_LIB, "cpu")
    g = torch.Generator().manual_seed(0)
    c = torch.nn.functional.normalize(torch.randn(N_CAMS, 3, generator=g), dim=-1) * 2.7
    fwd = -c / c.norm(dim=-1, keepdim=True)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0]).expand_as(fwd)), dim=-1)
    init = torch.eye(4).repeat(N_CAMS, 1, 1)
    init[:, :3, 0], init[:, :3, 1], init[:, :3, 2], init[:, :3, 3] = right, torch.linalg.cross(fwd, right), fwd, c
    pose = cn.PoseNet(N_CAMS, True, True, pose_mode="6d", init_c2w=init, library=N.EMU_LIB)
    with torch.no_grad():
        pose.r.add_(0.02 * torch.randn(N_CAMS, 6, generator=g))
        pose.t.add_(0.02 * torch.randn(N_CAMS, 3, generator=g))
    cams = cn.Cameras(cn.FocalNet(H, W, True, False, init_focal=np.array([21.0, 20.0], dtype=np.float32)), pose, library=N.EMU_LIB)
    image = torch.rand(N_CAMS, H, W, 3, generator=g)
    mask = (torch.rand(N_CAMS, H, W, generator=g) < 0.7).float()
    return cn, renderer, cams, image, mask


def _step(cn, renderer, cams, image, mask, sl, n_global):
    """Cameras -> rays of the whole batch -> the rays of ``sl`` through the renderer at fixed z_vals -> fused loss -> backward."""
    from color_neus_amd import rays as raygen
    lib = cn.load_library(N.EMU_LIB)
    c2w, focal = cams([2, 0, 3, 1])
    torch.manual_seed(3)
    o, d, near, far, rgb, msel = raygen.rays_for_training(c2w, focal, image, R, torch.zeros(3), 1.0, normalize=True, mask=mask, return_mask=True, library=lib)
    with torch.no_grad():
        z = renderer(o, d, near, far, perturb_overwrite=0)["z_vals"].detach().clone()
    out = renderer(o[sl], d[sl], near[sl], far[sl], z_vals=z[sl])
    loss, _ = cn.compute_loss_fused(out, rgb[sl], msel[sl], n_rays_global=n_global, library=lib)
    loss.backward()
    return loss


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from color_neus_amd import optim, parallel
    cn, renderer, cams, image, mask = _setup()
    _step(cn, renderer, cams, image, mask, parallel.shard_slice(R, rank, world), R)
    ordered = renderer._ordered_params()
    flat = optim.flat_view_of_grads(ordered)
    n_renderer = sum(p.numel() for p in ordered)
    assert flat is not None and flat.numel() == n_renderer
    ptr, before = flat.data_ptr(), flat.clone()
    params = list(ordered) + [p for p in cams.parameters() if p.requires_grad]
    sizes, orig = [], dist.all_reduce

    def recording(t, *a, **k):
        sizes.append((t.numel(), t.data_ptr()))
        return orig(t, *a, **k)
    dist.all_reduce = recording
    try:
        parallel.allreduce_gradients(params)
    finally:
        dist.all_reduce = orig
    n_cam = sum(p.numel() for p in cams.parameters() if p.requires_grad)
    # the renderer's buffer in place (its own address, no full-size temporary) and one gathered message of the camera gradients
    assert [s for s, _ in sizes] == [n_renderer, n_cam], (sizes, n_renderer, n_cam)
    assert sizes[0][1] == ptr and ordered[0].grad.data_ptr() == ptr and not torch.equal(flat, before)
    # a list that tiles one buffer takes the one-message path it always took
    sizes.clear()
    dist.all_reduce = recording
    try:
        parallel.allreduce_gradients(list(ordered))
    finally:
        dist.all_reduce = orig
    assert sizes == [(n_renderer, ptr)], sizes
    q.put((rank, {k: p.grad.numpy().copy() for k, p in cams.named_parameters() if p.grad is not None},
           {k: (p.grad / world).numpy().copy() for k, p in renderer.named_parameters()}))      # (reduced twice above: x world)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_sharding_with_learnable_cameras():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cn, renderer, cams, image, mask = _setup()
    _step(cn, renderer, cams, image, mask, slice(0, R), None)
    want_cam = {k: p.grad for k, p in cams.named_parameters() if p.grad is not None}
    assert set(want_cam) == {"focal_net.fx", "focal_net.fy", "pose_net.r", "pose_net.t"}
    for rank, gcam, gren in got:
        assert set(gcam) == set(want_cam)
        for k, ref in want_cam.items():
            # the gate of tests/test_cameras.py without a yardstick run of its own: its floor, 1e-6 of the tensor's largest entry
            err = float((torch.from_numpy(gcam[k]) - ref).abs().max()) / float(ref.abs().max())
            print(f"rank {rank} {k}: {err:.2e}")
            assert err <= 1e-6, (rank, k, err)
        for k, p in renderer.named_parameters():
            err = float((torch.from_numpy(gren[k]) - p.grad).abs().max())
            assert err <= 1e-4 * float(p.grad.abs().max()) + 1e-12, (rank, k, err)      # the unchanged path's bound (tests/test_sharded_gloo.py)
    for k in want_cam:      # every rank holds the same bits
        assert np.array_equal(got[0][1][k], got[1][1][k]), k
