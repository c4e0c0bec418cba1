"""Ray generation (the producer in front of the path) through the C ABI (cnr_gen_rays / cnr_gen_rays_backward)
against the golden vectors captured from the reference's ray_utils.py; CPU-emulation build here, HIP kernels under -m gpu."""
import os

import pytest
import torch

import _golden as G
import _native as N
import color_neus_amd as cn
from color_neus_amd import rays

emu = pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")


def _multicam(library, dev):
    fx = G.load("rays")
    c2w, focal, image, mask = (torch.from_numpy(fx[k]).to(dev) for k in ("c2w", "focal", "image", "mask"))
    t = lambda k: torch.from_numpy(fx[k])
    torch.manual_seed(5)
    o, d, rgb, ms = rays.get_rays_multicam(c2w, focal, image, 40, mask=mask, mask_rate=0.7, return_mask=True, normalize=True, library=library)
    assert torch.equal(rgb.cpu(), t("m:rgb")) and torch.equal(ms.cpu(), t("m:mask"))   # identical pixel choice
    assert torch.allclose(o.cpu(), t("m:o"), atol=1e-6) and torch.allclose(d.cpu(), t("m:d"), atol=1e-6)
    torch.manual_seed(5)
    o, d, rgb, ms = rays.get_rays_multicam(c2w, focal, image, 40, mask=None, normalize=False, opengl=True, library=library)
    assert ms is None and torch.equal(rgb.cpu(), t("nm:rgb"))
    assert torch.allclose(o.cpu(), t("nm:o"), atol=1e-6) and torch.allclose(d.cpu(), t("nm:d"), atol=1e-6)


def _at_and_nearfar(library, dev):
    fx = G.load("rays")
    c2w, focal = torch.from_numpy(fx["c2w"]).to(dev), torch.from_numpy(fx["focal"]).to(dev)
    t = lambda k: torch.from_numpy(fx[k])
    o, d = rays.get_rays_at(c2w[1], focal, 12, 17, normalize=True, library=library)
    assert o.shape == (12, 17, 3)
    assert torch.allclose(o.cpu(), t("at:o"), atol=1e-6) and torch.allclose(d.cpu(), t("at:d"), atol=1e-6)
    near, far = rays.near_far_from_sphere(t("m:o"), t("m:d"))
    assert torch.allclose(near, t("nf:near"), atol=1e-6) and torch.allclose(far, t("nf:far"), atol=1e-6)
    # the fused trainer front end: same pixels, normalised origins, near / far of the normalised rays
    image, mask = t("image").to(dev), t("mask").to(dev)
    origin, radius = torch.tensor([0.1, -0.2, 0.05]), 1.7
    torch.manual_seed(5)
    o2, d2, near2, far2, rgb2, ms2 = rays.rays_for_training(c2w, focal, image, 40, origin, radius, normalize=True, mask=mask, mask_rate=0.7,
                                                            return_mask=True, library=library)
    assert torch.equal(rgb2.cpu(), t("m:rgb")) and torch.equal(ms2.cpu(), t("m:mask"))
    want_o = (t("m:o") - origin) / radius
    assert torch.allclose(o2.cpu(), want_o, atol=1e-6) and torch.allclose(d2.cpu(), t("m:d"), atol=1e-6)
    wn, wf = rays.near_far_from_sphere(want_o, t("m:d"))
    assert torch.allclose(near2.cpu(), wn, atol=2e-6) and torch.allclose(far2.cpu(), wf, atol=2e-6)


def _torch_rays(c2w, focal, idx, H, W, normalize, opengl, origin, radius):
    """plain differentiable torch formula of the same rays (float64), the autograd reference of the backward kernel"""
    cam = torch.div(idx, H * W, rounding_mode="floor")
    pix = idx - cam * H * W
    py, px = torch.div(pix, W, rounding_mode="floor").double(), (pix % W).double()
    sgn = -1.0 if opengl else 1.0
    u = torch.stack([(px - W * 0.5) / focal[0], sgn * (py - H * 0.5) / focal[1], sgn * torch.ones_like(px)], -1)
    if normalize:
        u = u / u.norm(dim=-1, keepdim=True)
    d = (u[:, None, :] * c2w[cam, :3, :3]).sum(-1)
    o = (c2w[cam, :3, 3] - origin) / radius
    mid = -(o * d).sum(-1) / (d * d).sum(-1)
    return o, d, mid - 1.0, mid + 1.0


def _backward(library, dev):
    fx = G.load("rays")
    g = torch.Generator().manual_seed(2)
    H, W, n = 12, 17, 64
    for normalize, opengl in ((True, False), (False, True)):
        c2w = torch.from_numpy(fx["c2w"]).clone()
        focal = torch.from_numpy(fx["focal"]).clone()
        idx = torch.randint(0, 3 * H * W, (n,), generator=g)
        origin, radius = torch.tensor([0.1, -0.2, 0.05]), 1.7
        co = [torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)]
        c64, f64 = c2w.double().requires_grad_(True), focal.double().requires_grad_(True)
        outs = _torch_rays(c64, f64, idx, H, W, normalize, opengl, origin.double(), radius)
        sum((a * b.double()).sum() for a, b in zip(outs, co)).backward()
        cd, fd = c2w.to(dev).requires_grad_(True), focal.to(dev).requires_grad_(True)
        lib = rays._library(library)
        o, d, _, _, near, far = rays._generate(lib, idx.to(dev), n, cd, fd, H, W, normalize, opengl, origin=origin, radius=radius, want_nearfar=True)
        for a, b in zip((o, d, near, far), outs):
            assert torch.allclose(a.detach().cpu().double(), b.detach(), atol=2e-6)
        (sum((a * b.to(dev)).sum() for a, b in zip((o, d, near, far), co))).backward()
        assert float((cd.grad.cpu().double() - c64.grad).abs().max()) < 2e-5 * float(c64.grad.abs().max())
        assert float((fd.grad.cpu().double() - f64.grad).abs().max()) < 2e-5 * float(f64.grad.abs().max())
        assert float(cd.grad[:, 3].abs().max()) == 0.0     # bottom row of the pose matrices


def _own_poses(n_cams, g):
    """camera-to-world matrices of the test's own: random rotations (QR of a Gaussian draw, determinant fixed to +1), random translations"""
    q, r = torch.linalg.qr(torch.randn(n_cams, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    q[:, :, 0] = q[:, :, 0] * torch.sign(torch.linalg.det(q))[:, None]
    assert bool((torch.linalg.det(q) > 0.999).all())
    c2w = torch.eye(4, dtype=torch.float64).repeat(n_cams, 1, 1)
    c2w[:, :3, :3], c2w[:, :3, 3] = q, torch.randn(n_cams, 3, generator=g, dtype=torch.float64)
    return c2w.float()


def _backward_wrapped(library, dev):
    """The backward beyond one trip of its ray loop: each camera's workgroup walks ALL n rays 256 at a time.  700 rays (three trips, the
    last one ragged; all four waves of a block hold non-zero partial sums) over cameras 0, 1, 2 and 4 of 5 -- camera 3 has no ray, camera 4
    only five, one in each trip and two more, so d c2w is held per camera, against that camera's own largest reference entry."""
    g = torch.Generator().manual_seed(9)
    H, W, n, n_cams = 12, 17, 700, 5
    c2w, focal = _own_poses(n_cams, g), torch.tensor([15.0, 16.5])
    origin, radius = torch.tensor([0.1, -0.2, 0.05]), 1.7
    few = torch.tensor([3, 300, 400, 600, 699])
    cam = torch.tensor([0, 1, 2])[torch.randint(0, 3, (n,), generator=g)]
    cam[few] = 4
    idx = cam * (H * W) + torch.randint(0, H * W, (n,), generator=g)
    lib = rays._library(library)

    def run(idx, co, normalize, opengl):
        cd, fd = c2w.clone().to(dev).requires_grad_(True), focal.clone().to(dev).requires_grad_(True)     # (clone: on the CPU .to() is the tensor itself)
        o, d, _, _, near, far = rays._generate(lib, idx.to(dev), idx.shape[0], cd, fd, H, W, normalize, opengl, origin=origin, radius=radius, want_nearfar=True)
        (sum((a * b.to(dev)).sum() for a, b in zip((o, d, near, far), co))).backward()
        return [t.detach().cpu() for t in (o, d, near, far)], cd.grad.cpu(), fd.grad.cpu()

    for normalize, opengl in ((True, False), (False, True)):
        co = [torch.randn(n, 3, generator=g), torch.randn(n, 3, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)]
        c64, f64 = c2w.double().requires_grad_(True), focal.double().requires_grad_(True)
        ref = _torch_rays(c64, f64, idx, H, W, normalize, opengl, origin.double(), radius)
        sum((a * b.double()).sum() for a, b in zip(ref, co)).backward()
        outs, dc, df = run(idx, co, normalize, opengl)
        for a, b in zip(outs, ref):
            assert torch.allclose(a.double(), b.detach(), atol=2e-6)
        for c in (0, 1, 2, 4):
            err, den = float((dc[c].double() - c64.grad[c]).abs().max()), float(c64.grad[c].abs().max())
            assert err < 2e-5 * den, (normalize, opengl, c, err / den)
        assert float((df.double() - f64.grad).abs().max()) < 2e-5 * float(f64.grad.abs().max())
        assert float(dc[3].abs().max()) == 0.0 and float(c64.grad[3].abs().max()) == 0.0     # the camera without rays
        assert float(dc[:, 3].abs().max()) == 0.0                                            # bottom row of the pose matrices
        # ray 256 is the first ray of the second trip: with a zero cotangent on it, the 257-ray run folds exactly what the 256-ray run folds
        co256 = [t[:256] for t in co]
        co257 = [torch.cat([t[:256], torch.zeros_like(t[256:257])]) for t in co]
        _, dc256, df256 = run(idx[:256], co256, normalize, opengl)
        _, dc257, df257 = run(idx[:257], co257, normalize, opengl)
        assert torch.equal(dc256, dc257) and torch.equal(df256, df257), (normalize, opengl)
        assert float(dc256.abs().max()) > 0.0


def _bad_indices(library, dev):
    """A caller-supplied index outside [0, n_cams * H * W): the kernel reads nothing for it (the image / mask / pose reads would be out of
    bounds), that ray's outputs are NaN, its backward contributes nothing, and every other ray is untouched."""
    fx = G.load("rays")
    H, W = 12, 17
    c2w = torch.from_numpy(fx["c2w"]).to(dev).requires_grad_(True)
    focal = torch.from_numpy(fx["focal"]).to(dev)
    image, mask = torch.from_numpy(fx["image"]).to(dev), torch.from_numpy(fx["mask"]).to(dev)
    n_cams = c2w.shape[0]
    good = torch.tensor([0, 5, H * W + 3, n_cams * H * W - 1], dtype=torch.int64)
    bad = torch.tensor([0, -1, H * W + 3, n_cams * H * W, 5, 1 << 40], dtype=torch.int64)
    lib = rays._library(library)
    og, dg, rg, mg, ng, fg = rays._generate(lib, good.to(dev), 4, c2w, focal, H, W, True, False, image=image, mask=mask, want_nearfar=True)
    assert rays.bad_index_count(dev) == 0
    rays.raise_if_bad_indices(dev)
    ob, db, rb, mb, nb, fb = rays._generate(lib, bad.to(dev), 6, c2w, focal, H, W, True, False, image=image, mask=mask, want_nearfar=True)
    with pytest.raises(IndexError, match="3 pixel"):    # the device-side error counter: raised at the caller's next synchronisation point
        rays.raise_if_bad_indices(dev)
    assert rays.bad_index_count(dev) == 0                # (reset by the check)
    for t in (ob, db, rb, mb, nb, fb):
        t = t.detach().cpu().reshape(6, -1)
        assert bool(torch.isnan(t[[1, 3, 5]]).all()) and bool(torch.isfinite(t[[0, 2, 4]]).all())
    assert torch.equal(ob[[0, 2, 4]].detach().cpu(), og[[0, 2, 1]].detach().cpu()) and torch.equal(rb[[0, 2, 4]].cpu(), rg[[0, 2, 1]].cpu())
    # backward: cotangents of the bad rays are ignored (zeroed here so that NaN x 0 does not enter through the caller's own arithmetic)
    w = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0, 0.0], device=dev)[:, None]
    (torch.nan_to_num(ob) * w).sum().backward()
    g_bad = c2w.grad.clone()
    c2w.grad = None
    og[[0, 2, 1]].sum().backward()
    assert bool(torch.isfinite(g_bad).all()) and torch.allclose(g_bad, c2w.grad, atol=1e-6)


@emu
def test_out_of_range_pixel_indices_emu():
    _bad_indices(N.EMU_LIB, "cpu")


@pytest.mark.gpu
def test_out_of_range_pixel_indices_hip():
    _bad_indices(None, "cuda:0")


@emu
def test_get_rays_multicam_same_pixels_and_values_emu():
    _multicam(N.EMU_LIB, "cpu")


@emu
def test_get_rays_at_and_near_far_emu():
    _at_and_nearfar(N.EMU_LIB, "cpu")


@emu
def test_pose_and_focal_gradients_emu():
    _backward(N.EMU_LIB, "cpu")


@emu
def test_pose_and_focal_gradients_beyond_one_trip_emu():
    _backward_wrapped(N.EMU_LIB, "cpu")


@pytest.mark.gpu
def test_pose_and_focal_gradients_beyond_one_trip_hip():
    _backward_wrapped(None, "cuda:0")


@pytest.mark.gpu
def test_ray_generation_hip():
    _multicam(None, "cuda:0")
    _at_and_nearfar(None, "cuda:0")
    _backward(None, "cuda:0")


@emu
def test_argument_checks():
    lib = cn.load_library(N.EMU_LIB)
    with pytest.raises(AssertionError):
        rays.get_rays_multicam(torch.eye(4), torch.ones(2), torch.zeros(1, 4, 4, 3), 4, library=lib)      # single pose given to the multi-camera form
    with pytest.raises(AssertionError):
        rays.get_rays_at(torch.eye(4)[None], torch.ones(2), 4, 4, library=lib)
