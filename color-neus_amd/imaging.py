"""Image evaluation on the device library: PSNR, SSIM, the depth colour map and the picture of ``validate_image``.

The reference's ``NeuS_Trainer.validate_image`` (NeuS_Trainer.py:216-277) renders a view in chunks, pulls every chunk to the host, and there
computes the PSNR (lib/metrics/similarity.py:24-25), the SSIM (``kornia.metrics.ssim(img0, img1, 3)``, similarity.py:55) and the
``gt | render | depth`` picture with the depth through ``viztools.cmap`` (cv2's HOT colour map), saved as a PNG with imageio.  Here the
squared-error and SSIM sums are one kernel (``cnr_image_metrics``) and the picture another (``cnr_image_panel``, include/colorneus_render.h,
where the arithmetic is specified); the image stays on the device from ray generation to the bytes of the file.  kornia, cv2 and imageio
are not dependencies of this package.

``rasterize_mesh`` and ``mesh_view_metrics`` look at the product of a run, the extracted mesh with its vertex colours, from a camera
(``cnr_mesh_raster``): the reference has no counterpart, it shows its meshes in third-party viewers.

Inputs of any float dtype and any strides are detached and converted to contiguous float32 on their own device, and the work goes to the
current stream.  CUDA tensors go through the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no CPU
fallback).  NOTHING HERE IS DIFFERENTIABLE."""
import numpy as np
import torch

from . import _lib, meshio, parallel, rays
from ._lib import ptr, stream_of

__all__ = ["image_metrics", "psnr", "ssim", "mse2psnr", "PSNR", "SSIM", "AverageMeter", "cmap", "panel", "validate_image", "rasterize_mesh",
           "mesh_view_metrics"]


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


def _on(x, dtype, dev, name, shape):
    """``x`` (tensor, numpy array or sequence) as a contiguous ``dtype`` tensor of ``shape`` (-1: any) on ``dev``."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    x = x.detach().to(device=dev, dtype=dtype).contiguous()
    if x.dim() != len(shape) or any(want not in (-1, have) for want, have in zip(shape, x.shape)):
        raise ValueError(f"{name}: expected shape {list(shape)} (-1: any), got {list(x.shape)}")
    return x


def rasterize_mesh(vertices, triangles, c2w, focal, H, W, colors=None, opengl=False, origin=None, radius=1.0, z_near=1e-3, background=None,
                   library=None):
    """The mesh seen from one camera (``cnr_mesh_raster``, include/colorneus_render.h, where the arithmetic is specified): a z-buffer of
    opaque triangles with per-vertex colours, pixel ``(i, j)`` sampled where the ray of ``rays.get_rays_at`` leaves the camera.

    ``vertices`` [V, 3], ``triangles`` [F, 3], ``colors`` [V, 3] or None: tensors or numpy arrays of any float / integer dtype
    (``extract_geometry`` and ``extract_color`` return float64 / int64 numpy), converted to contiguous float32 / int32.  The device is that
    of ``vertices`` when it is a tensor, else that of ``c2w`` when it is one, else the CPU; everything else is moved there.  ``c2w`` [4, 4],
    ``focal`` [2]; ``origin`` [3] / ``radius`` move the camera centre into the mesh's frame, ``(c2w[:3, 3] - origin) / radius``, as the
    trainer normalises its rays (without ``origin``, ``radius`` must be 1).  The rotation of ``c2w`` is taken as orthonormal.  A triangle with
    a vertex at or behind ``z_near`` (or projected beyond 2^21 pixels) is dropped whole: there is no polygon clipping.

    Returns ``{"rgb" [H, W, 3] (only with colors), "depth" [H, W] (camera depth; NaN where nothing is covered), "tri_id" [H, W] int64 (-1:
    nothing), "mask" [H, W] bool, "dropped": {"behind_or_far": int, "bad_index": int}}``; uncovered pixels of ``rgb`` are ``background``
    (3 floats, default black).  Reading ``dropped`` is the call's one host synchronisation.  Results are bitwise reproducible.
    CUDA tensors use the HIP library; CPU tensors need an explicit emulation ``library=``.  Not differentiable."""
    dev = vertices.device if torch.is_tensor(vertices) else (c2w.device if torch.is_tensor(c2w) else torch.device("cpu"))
    lib = _lib.library_for(library, dev, ("a mesh", "rasterised"))
    H, W = int(H), int(W)
    v = _on(vertices, torch.float32, dev, "vertices", (-1, 3))
    idx = torch.as_tensor(np.asarray(triangles)) if not torch.is_tensor(triangles) else triangles
    if idx.is_floating_point() or idx.dtype == torch.bool:
        raise ValueError(f"triangles: expected an integer dtype, got {idx.dtype}")
    t = _on(idx, torch.int32, dev, "triangles", (-1, 3))
    col = _on(colors, torch.float32, dev, "colors", (v.shape[0], 3)) if colors is not None else None
    if col is not None and col.shape[0] == 0:      # (an empty tensor has no address; colors / rgb are NULL together in the ABI)
        col = torch.zeros(1, 3, dtype=torch.float32, device=dev)
    cam = _on(c2w, torch.float32, dev, "c2w", (4, 4))
    foc = _on(torch.as_tensor(focal).reshape(-1) if torch.is_tensor(focal) else np.asarray(focal).reshape(-1), torch.float32, dev, "focal", (2,))
    org = _on(origin, torch.float32, dev, "origin", (3,)) if origin is not None else None
    if org is None and float(radius) != 1.0:
        raise ValueError("rasterize_mesh: radius without origin (pass origin=[0, 0, 0] to scale only)")
    if H < 1 or W < 1:
        raise ValueError(f"rasterize_mesh: H and W must be at least 1 (got {H} x {W})")
    rgb = torch.empty(H, W, 3, dtype=torch.float32, device=dev) if col is not None else None
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    tri_id = torch.empty(H, W, dtype=torch.int32, device=dev)
    dropped = torch.empty(2, dtype=torch.int32, device=dev)
    bg = _lib.float3(background) if background is not None else None
    scratch, nb = lib.scratch("cnr_mesh_raster_scratch_bytes", dev, v.shape[0], t.shape[0], H, W, at_least=1)
    lib.call("cnr_mesh_raster", ptr(v if v.shape[0] else None), v.shape[0], ptr(t if t.shape[0] else None), t.shape[0], ptr(col), ptr(cam),
             ptr(foc), H, W, int(bool(opengl)), ptr(org), float(radius), float(z_near), bg, ptr(rgb), ptr(depth), ptr(tri_id), ptr(dropped),
             ptr(scratch), nb, stream_of(dev))
    out = {}
    if col is not None:
        out["rgb"] = rgb
    out["depth"] = depth
    out["tri_id"] = tri_id.to(torch.int64)
    out["mask"] = tri_id >= 0
    n_far, n_bad = (int(x) for x in dropped.tolist())      # the one host read, last
    out["dropped"] = {"behind_or_far": n_far, "bad_index": n_bad}
    return out


def mesh_view_metrics(vertices, triangles, colors, c2w, focal, image_gt, mask=None, opengl=False, origin=None, radius=1.0, background=None,
                      path=None, library=None):
    """The product (mesh and vertex colours) scored against one image: ``rasterize_mesh`` into the image's size, then ``image_metrics``
    against ``image_gt`` (``[H, W, 3]`` or ``[3, H, W]``), so PSNR and SSIM have the definitions of ``validate_image``.

    With a ``mask`` ``[H, W]`` the ground truth is composited onto ``background`` (default black) outside ``mask > 0`` before scoring, and
    ``iou`` is added: intersection over union of ``mask > 0`` with the raster's mask, from integer counts (1.0 when both are empty).  With
    ``path`` the picture ``gt | mesh render | mesh depth`` is saved through ``panel`` and ``meshio.write_png``.  Returns a dict of Python
    floats ``{"psnr", "ssim"[, "iou"]}``.  Not differentiable."""
    gt = _float32(image_gt, "image_gt")
    if gt.dim() != 3 or 3 not in (gt.shape[0], gt.shape[2]):
        raise ValueError(f"image_gt: expected [H, W, 3] or [3, H, W], got {tuple(gt.shape)}")
    if gt.shape[2] != 3:
        gt = gt.permute(1, 2, 0)
    h, w = gt.shape[0], gt.shape[1]
    if colors is None:
        raise ValueError("mesh_view_metrics: colors are required")
    r = rasterize_mesh(vertices, triangles, c2w, focal, h, w, colors=colors, opengl=opengl, origin=origin, radius=radius, background=background,
                       library=library)
    dev = r["depth"].device
    gt = gt.to(dev).contiguous()
    out = {}
    if mask is not None:
        m = (mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))).to(dev)
        if tuple(m.shape) != (h, w):
            raise ValueError(f"mask: expected [{h}, {w}], got {tuple(m.shape)}")
        m = m > 0
        bg = torch.tensor([float(x) for x in background] if background is not None else [0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        gt = torch.where(m[..., None], gt, bg.expand(h, w, 3)).contiguous()
        inter, union = int((m & r["mask"]).sum()), int((m | r["mask"]).sum())
        out["iou"] = inter / union if union else 1.0
    s = image_metrics(r["rgb"], gt, library=library)
    out["psnr"], out["ssim"] = float(s["psnr"]), float(s["ssim"])
    if path is not None:
        meshio.write_png(path, panel(gt, r["rgb"], r["depth"], library=library))
    return out
