"""Image evaluation on the device library: PSNR, SSIM, the depth colour map and the picture of ``validate_image``.

The reference's ``NeuS_Trainer.validate_image`` (NeuS_Trainer.py:216-277) renders a view in chunks, pulls every chunk to the host, and there
computes the PSNR (lib/metrics/similarity.py:24-25), the SSIM (``kornia.metrics.ssim(img0, img1, 3)``, similarity.py:55) and the
``gt | render | depth`` picture with the depth through ``viztools.cmap`` (cv2's HOT colour map), saved as a PNG with imageio.  Here the
squared-error and SSIM sums are one kernel (``cnr_image_metrics``) and the picture another (``cnr_image_panel``, include/colorneus_render.h,
where the arithmetic is specified); the image stays on the device from ray generation to the bytes of the file.  kornia, cv2 and imageio
are not dependencies of this package.

Inputs of any float dtype and any strides are detached and converted to contiguous float32 on their own device, and the work goes to the
current stream.  CUDA tensors go through the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no CPU
fallback).  NOTHING HERE IS DIFFERENTIABLE."""
import torch

from . import _lib, meshio, parallel, rays
from ._lib import ptr, stream_of

__all__ = ["image_metrics", "psnr", "ssim", "mse2psnr", "PSNR", "SSIM", "AverageMeter", "cmap", "panel", "validate_image"]


def _library(library, dev):
    return _lib.library_for(library, dev, ("images", "evaluated"))


def _float32(x, name):
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if not x.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point tensor, got {x.dtype}")
    return x.detach().to(torch.float32)


_MAX_CHANNELS_LAST = 32      # kImgMaxCs of the library


def _is_channels_last(x):
    return x.dim() == 4 and not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)


def image_metrics(img0, img1, return_map=False, library=None):
    """``{"mse", "psnr", "ssim"}`` of two images as 0-dim float64 tensors on the inputs' device, plus ``"ssim_map"`` (float32, the inputs'
    shape) when ``return_map``.

    4-D inputs are ``[B, C, H, W]`` (kornia's layout); 3-D inputs are one ``[H, W, C]`` image (what the renderer produces).  A 4-D pair in
    torch's channels-last memory format is read as it lies, without a copy, and so is a 3-D pair.  (The channels-last kernel takes at most 32 channels; wider images of those
    forms are evaluated on a ``[B, C, H, W]`` copy.)  ``mse`` is the mean of the squared float32
    differences and ``ssim`` the mean of the SSIM map, both float64 sums (a fixed order: two calls give the same bits) divided by the element
    count; ``psnr = -10 * log10(mse)``, which is ``inf`` for identical images (the reference's ``math.log10(0)`` raises there).

    The SSIM map is what ``kornia.metrics.ssim(img0, img1, window_size=3, max_val=1.0, eps=1e-12, padding="same")`` of kornia 0.6.9 (the
    reference's requirements.txt) computes, as its documentation states it: a normalised 3 x 3 Gaussian window of sigma 1.5, reflected
    borders, every plane on its own, every float32 operation rounded separately in the order include/colorneus_render.h gives.  kornia is not
    a dependency of this package, so that equivalence is stated from its documentation and not checked by the tests.  H and W must be at
    least 2.  Not differentiable."""
    x, y = _float32(img0, "img0"), _float32(img1, "img1")
    if x.shape != y.shape:
        raise ValueError(f"image_metrics: the images differ in shape: {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise ValueError(f"img0 is on {x.device}, img1 on {y.device}")
    if x.dim() not in (3, 4):
        raise ValueError(f"image_metrics: expected [B, C, H, W] or [H, W, C] images, got {tuple(x.shape)}")
    hwc = x.dim() == 3
    if hwc and x.shape[2] > _MAX_CHANNELS_LAST:       # the channels-last kernel stages all channels of a pixel: wider images as [1, C, H, W]
        x, y = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]
    if x.dim() == 4:
        cl = _is_channels_last(x) and _is_channels_last(y) and x.shape[1] <= _MAX_CHANNELS_LAST
        if not cl:
            x, y = x.contiguous(), y.contiguous()
        (b, c, h, w) = x.shape
    else:
        x, y = x.contiguous(), y.contiguous()
        cl, b, (h, w, c) = True, 1, x.shape
    lib = _library(library, x.device)
    n = b * c * h * w
    sums = torch.empty(2, dtype=torch.float64, device=x.device)
    smap = torch.empty_like(x) if return_map else None      # empty_like keeps the memory format
    scratch, nb = lib.scratch("cnr_image_scratch_bytes", x.device, b, c, h, w, at_least=1)
    lib.call("cnr_image_metrics", ptr(x), ptr(y), b, c, h, w, int(cl), ptr(smap), ptr(sums), ptr(scratch), nb, stream_of(x))
    means = sums / torch.full((), float(n), dtype=torch.float64, device=x.device)      # tensor / tensor: a true float64 division on either device
    mse, mean_ssim = means[0], means[1]
    out = {"mse": mse, "psnr": -10.0 * torch.log10(mse), "ssim": mean_ssim}
    if return_map:
        out["ssim_map"] = smap[0].permute(1, 2, 0) if hwc and smap.dim() == 4 else smap
    return out


def psnr(img0, img1, library=None):
    """``-10 * log10(mean((img0 - img1)**2))`` as a 0-dim float64 tensor (``image_metrics``)."""
    return image_metrics(img0, img1, library=library)["psnr"]


def ssim(img0, img1, window_size=3, library=None):
    """The SSIM map of ``image_metrics`` (float32, the inputs' shape), as ``kornia.metrics.ssim(img0, img1, 3)`` returns a map.  Only
    ``window_size=3`` exists: the reference uses 3 and nothing else is built."""
    if window_size != 3:
        raise ValueError(f"ssim: only window_size=3 is built (got {window_size})")
    return image_metrics(img0, img1, return_map=True, library=library)["ssim_map"]


def mse2psnr(x):
    """``-10 * log(x) / log(10)`` (similarity.py:8) on a tensor, in its dtype."""
    x = torch.as_tensor(x)
    return -10.0 * torch.log(x) / torch.log(torch.tensor([10.0], dtype=x.dtype if x.is_floating_point() else torch.float32, device=x.device))


class AverageMeter:
    """val / sum / count / avg of the values fed (lib/metrics/basic_metric.py)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val, self.avg, self.sum, self.count = 0.0, 0.0, 0.0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class _Meter:
    name = ""

    def __init__(self, cfg=None, name="", library=None):
        self.cfg = cfg
        self.library = library
        self.avg_meter = AverageMeter()
        self.reset()

    def reset(self):
        self.avg_meter.reset()

    def get_measures(self, **kwargs):
        return {f"{self.name}": self.avg_meter.avg}

    def get_result(self):
        return self.avg_meter.avg

    def __str__(self):
        return f"{self.name}: {self.avg_meter.avg:6.4f}"


class PSNR(_Meter):
    """The reference's PSNR meter (similarity.py:11-39): ``feed(img0, img1)`` returns the PSNR of the pair as a Python float and averages
    over the feeds.  The trainer feeds ``[H, W, 3]`` images (NeuS_Trainer.py:276); any layout ``image_metrics`` takes works."""
    name = "PSNR"

    def feed(self, img0, img_1, **kwargs):
        value = float(image_metrics(img0, img_1, library=self.library)["psnr"])
        self.avg_meter.update(value, n=1)
        return value


class SSIM(_Meter):
    """The reference's SSIM meter (similarity.py:42-69): ``feed(img0, img1)`` returns the mean of the window-3 SSIM map as a Python float and
    averages over the feeds.  The trainer feeds ``[1, 3, H, W]`` images (NeuS_Trainer.py:277)."""
    name = "SSIM"

    def feed(self, img0, img_1, **kwargs):
        value = float(image_metrics(img0, img_1, library=self.library)["ssim"])
        self.avg_meter.update(value, n=1)
        return value


def _panel(gt, render, depth, library):
    d = _float32(depth, "depth")
    if d.dim() != 2:
        raise ValueError(f"depth: expected [H, W], got {tuple(d.shape)}")
    d = d.contiguous()
    h, w = d.shape
    lib = _library(library, d.device)
    colour = []
    for t, name in ((gt, "gt"), (render, "render")):
        if t is None:
            continue
        t = _float32(t, name)
        if tuple(t.shape) != (h, w, 3) or t.device != d.device:
            raise ValueError(f"{name}: expected [{h}, {w}, 3] on {d.device}, got {tuple(t.shape)} on {t.device}")
        colour.append(t.contiguous())
    out = torch.empty(h, (3 if colour else 1) * w, 3, dtype=torch.uint8, device=d.device)
    rng = torch.empty(2, dtype=torch.float32, device=d.device)
    scratch, nb = lib.scratch("cnr_image_scratch_bytes", d.device, 1, 3, h, w)
    lib.call("cnr_image_panel", ptr(colour[0] if colour else None), ptr(colour[1] if colour else None), ptr(d), h, w, ptr(out), ptr(rng),
             ptr(scratch), nb, stream_of(d))
    return out


def cmap(depth, library=None):
    """``viztools.cmap`` (lib/models/tools/viztools.py:145-162) of a ``[H, W]`` depth map: ``uint8 [H, W, 3]`` in cv2's channel order B, G, R.

    The depth is scaled to 0..255 between its minimum and maximum (NaN depths are left out of the range and come out black; a range below
    1e-10 gives level 0 everywhere) and sent through the HOT ramp ``r = clamp(2.5 u)``, ``g = clamp(2.5 u - 1)``, ``b = clamp(5 u - 4)``,
    ``u = level / 255``.  These are the three lines that OpenCV's 64-sample HOT table samples; cv2 builds its 256 entries by interpolating
    those samples, and cv2 is not a dependency of this package, so the colours can differ from ``cv2.applyColorMap``'s by a level or two
    beside the knees at 0.4 and 0.8."""
    return _panel(None, None, depth, library)


def panel(gt, render, depth, library=None):
    """The picture ``validate_image`` saves (NeuS_Trainer.py:250-263): ``uint8 [H, 3W, 3]``, ``hstack`` of the ground truth and the render
    as ``(v * 255).astype(uint8)`` and ``cmap(depth)``.  Colour values are truncated like the reference's; values outside [0, 1] are clamped
    (numpy wraps them) and NaN gives 0.  The depth part keeps cv2's B, G, R order, as the reference's picture does."""
    return _panel(gt, render, depth, library)


def validate_image(renderer, c2w, focal, image_gt, origin, radius, normalize=True, opengl=False, chunk=10000, path=None, group=None,
                   library=None, **render_kw):
    """``NeuS_Trainer.validate_image`` (NeuS_Trainer.py:216-277) for one given view: all rays of the camera (``rays.get_rays_at``), moved
    into the unit sphere (``(o - origin) / radius``), ``near_far_from_sphere``, rendered in chunks of ``chunk`` rays
    (``parallel.sharded_render_image``: the plain loop without a process group, the chunks split over the ranks with one), then
    ``image_metrics`` against ``image_gt``, the ``panel`` picture, and ``meshio.write_png(path, panel)`` when ``path`` is given.

    ``c2w`` [4, 4], ``focal`` [2], ``image_gt`` ``[H, W, 3]`` or ``[3, H, W]`` on the renderer's device; ``render_kw`` goes to the renderer
    (e.g. ``perturb_overwrite=0``).  Returns ``{"color_fine" [H, W, 3], "depth" [H, W], "psnr", "ssim", "panel"}`` (psnr / ssim Python
    floats) on rank 0 and None elsewhere.  The image never leaves the device: the only host transfers are the two scalars and, for the file,
    the bytes of the picture."""
    gt = _float32(image_gt, "image_gt")
    if gt.dim() != 3 or 3 not in (gt.shape[0], gt.shape[2]):
        raise ValueError(f"image_gt: expected [H, W, 3] or [3, H, W], got {tuple(gt.shape)}")
    if gt.shape[2] != 3:
        gt = gt.permute(1, 2, 0)
    gt = gt.contiguous()
    h, w = gt.shape[0], gt.shape[1]
    rays_o, rays_d = rays.get_rays_at(c2w, focal, h, w, normalize=normalize, opengl=opengl, library=library)
    rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    dev = rays_o.device
    rays_o = (rays_o - torch.as_tensor(origin, dtype=torch.float32, device=dev)).float()
    rays_o = (rays_o / torch.as_tensor(radius, dtype=torch.float32, device=dev)).float()
    near, far = rays.near_far_from_sphere(rays_o, rays_d)
    img = parallel.sharded_render_image(renderer, rays_o, rays_d, near, far, chunk=chunk, group=group, **render_kw)
    if img is None:
        return None
    color = img["color_fine"].reshape(h, w, 3)
    depth = img["depth"].reshape(h, w)
    m = image_metrics(color, gt, library=library)
    pic = panel(gt, color, depth, library=library)
    if path is not None:
        meshio.write_png(path, pic)
    return {"color_fine": color, "depth": depth, "psnr": float(m["psnr"]), "ssim": float(m["ssim"]), "panel": pic}
