"""Inference-only early-termination compaction (prune_eps > 0): colour / relight networks run only on samples with
compositing weight >= eps.  CPU: emulation build; GPU (-m gpu): HIP build (wavefront ballot + popcount prefix)."""
import os

import pytest
import torch

import _golden as G
import _native as N


def _check(library, device, name, repeat=1):
    """``repeat``: the fixture's rays tiled that many times."""
    fx = G.load(name)
    ocfg, P = G.weights_of(name, fx)
    r = N.make_renderer(ocfg, P, library, device)
    o, d, near, far, z = (torch.cat([torch.from_numpy(fx[k])] * repeat).to(device) for k in ("rays_o", "rays_d", "jit:near", "jit:far", "jit:z_vals"))
    eps = 1e-3
    with torch.no_grad():
        full = r(o, d, near, far, z_vals=z)
        pr = r(o, d, near, far, z_vals=z, prune_eps=eps)
    keep = full["weights"] >= eps
    assert 0 < int(keep.sum()) < keep.numel(), "test needs both kept and pruned samples"
    for k in ("weights", "depth", "weight_sum", "cdf_fine", "gradients", "gradient_error"):
        assert torch.equal(full[k], pr[k]), k                       # geometry side is untouched
    # every skipped sample changes the pixel by < eps
    n_pruned = (~keep).sum(-1, keepdim=True).float()
    assert bool(((full["color_fine"] - pr["color_fine"]).abs() <= n_pruned * eps + 1e-6).all())
    assert float((full["color_fine"] - pr["color_fine"]).abs().max()) < 2e-2
    if "delta_relight" in full:
        assert torch.allclose(pr["delta_relight"][keep], full["delta_relight"][keep], atol=1e-6)
        assert float(pr["delta_relight"][~keep].abs().max()) == 0.0
    # training through a pruned forward is refused
    o2 = o.clone().requires_grad_(True)
    out = r(o2, d, near, far, z_vals=z, prune_eps=eps)
    with pytest.raises(RuntimeError, match="inference-only"):
        out["color_fine"].sum().backward()


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
@pytest.mark.parametrize("name", ["tiny_sharp", "tiny_neus_sharp"])
def test_prune_emu(name):
    _check(N.EMU_LIB, "cpu", name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_sharp", "tiny_neus_sharp", "dtu_sharp"])
def test_prune_hip(name):
    _check(None, "cuda:0", name)


@pytest.mark.gpu
def test_prune_hip_second_trip_of_the_scan():
    """prune_scan_kernel walks the rays in trips of 1024: the fixture's rays tiled to the smallest count that is at least 1025 and no multiple
    of 1024, under _check's assertions."""
    R = G.load("tiny_sharp")["rays_o"].shape[0]
    repeat = next(k for k in range(1, 2048) if k * R >= 1025 and k * R % 1024)
    assert repeat * R == 1056
    _check(None, "cuda:0", "tiny_sharp", repeat)


def _pruned_forward(library, device, n_rays, eps):
    """The forward-only render of tiny_sharp with and without prune_eps on n_rays rays (the fixture's 32 rays repeated, every origin moved by up
    to 0.01 so that the rays keep different numbers of samples), and the compaction's index list and offsets as the library left them.  They are
    read from the scratch buffer: the forward-only layout ends with index list [P], counts [R], offsets [R + 1] and the slack of 1024 floats,
    each rounded to 256 bytes (layout_ctx_infer / place_compaction in csrc/cnr_model.cpp)."""
    fx = G.load("tiny_sharp")
    ocfg, P = G.weights_of("tiny_sharp", fx)
    r = N.make_renderer(ocfg, P, library, device)
    sel = torch.arange(n_rays) % fx["rays_o"].shape[0]
    t = lambda k: torch.from_numpy(fx[k])[sel].contiguous()
    o = t("rays_o") + 0.02 * (torch.rand(n_rays, 3, generator=torch.Generator().manual_seed(11)) - 0.5)
    o, d, near, far, z = (x.to(device) for x in (o, t("rays_d"), t("jit:near"), t("jit:far"), t("jit:z_vals")))
    lib, bufs = r._lib, []
    scratch = lib.scratch

    def scratch_(bytes_fn, dev, *args, **kw):
        buf, nb = scratch(bytes_fn, dev, *args, **kw)
        if bytes_fn == "cnr_infer_scratch_bytes":
            bufs.append((buf, nb))
        return buf, nb

    with torch.no_grad():
        full = r(o, d, near, far, z_vals=z, forward_only=True)
        lib.scratch = scratch_
        try:
            pr = r(o, d, near, far, z_vals=z, prune_eps=eps, forward_only=True)
        finally:
            del lib.scratch
    (buf, nb), = bufs
    n_pts = z.numel()
    r256 = lambda count: (4 * count + 255) // 256 * 256
    off0 = nb - r256(1024) - r256(n_rays + 1)
    idx0 = off0 - r256(n_rays) - r256(n_pts)
    words = buf[:nb].cpu().view(torch.int32)
    offsets = words[off0 // 4:off0 // 4 + n_rays + 1]
    return full, pr, words[idx0 // 4:idx0 // 4 + int(offsets[-1])], offsets


@pytest.mark.gpu
@pytest.mark.parametrize("n_rays", [65, 1025])
def test_prune_scan_waves_and_trips_hip_matches_emulation(n_rays):
    """prune_scan is one workgroup of 16 waves that walks the rays in trips of 1024: 65 rays reach its second wave (the wave totals through LDS),
    1025 rays its second trip (the carry).  The index list and the offsets of the HIP build equal the emulation's and what the build's own weights
    imply (every sample with weight >= eps, in ray order; offsets = exclusive sums of the per-ray counts, the total at [R]); the outputs are held
    to the rules of _check above."""
    eps = 1e-3
    full, pr, idx, offsets = _pruned_forward(None, "cuda:0", n_rays, eps)
    _, _, idx_e, offsets_e = _pruned_forward(N.EMU_LIB, "cpu", n_rays, eps)
    keep = (full["weights"] >= eps).cpu()
    counts = keep.sum(-1)
    assert 0 < int(counts.sum()) < keep.numel() and len(set(counts.tolist())) > 2, "test needs kept and pruned samples, and rays that differ"
    expect = torch.cat([torch.zeros(1, dtype=torch.int64), counts.cumsum(0)]).int()
    assert torch.equal(offsets, expect)
    assert torch.equal(idx, keep.reshape(-1).nonzero().reshape(-1).int())
    assert torch.equal(offsets, offsets_e) and torch.equal(idx, idx_e)
    for k in ("weights", "depth", "weight_sum", "cdf_fine", "gradients", "gradient_error"):
        assert torch.equal(full[k], pr[k]), k
    n_pruned = (~keep).sum(-1, keepdim=True).float().to(full["color_fine"].device)
    assert bool(((full["color_fine"] - pr["color_fine"]).abs() <= n_pruned * eps + 1e-6).all())
    assert float((full["color_fine"] - pr["color_fine"]).abs().max()) < 2e-2
    keep_d = keep.to(pr["delta_relight"].device)
    assert torch.allclose(pr["delta_relight"][keep_d], full["delta_relight"][keep_d], atol=1e-6)
    assert float(pr["delta_relight"][~keep_d].abs().max()) == 0.0
