"""Ray tools of the caller side of the render path: drop-in counterparts of the reference's
``get_rays_multicam`` / ``get_rays_at`` / ``near_far_from_sphere`` (lib/models/tools/ray_utils.py:7-119) on the device library.

The reference builds directions and origins for ALL N*H*W pixels of the batch (about 184 MB per step at DTU size) and gathers
n_rays of them.  Here the pixels are chosen first and one kernel (cnr_gen_rays) builds rays, colours and mask values only for
those; ``rays_for_training`` also folds in what NeuS_Trainer.render does next (origin / radius normalisation, near / far).
Learnable poses and focal lengths (config/Color_NeuS_iho.yml:18-20) get their gradients from cnr_gen_rays_backward; the parameters
behind them (pose_net.r / .t, focal_net.fx / .fy) and the step from those gradients to theirs are in cameras.py.

Pixel choice has two sources.  The default (``choose_pixels``) consumes the torch CPU generator exactly like the reference (same calls, same
order), so a seeded run picks the same pixels: that part stays in torch -- it IS the reference's random stream -- and it costs what the
reference's costs: two nonzero over the whole mask stack and permutations of all its pixels on the host, every step.  The opt-in source
(``PixelSampler``, passed as ``sampler=``) keeps the sampling semantics (a share of the batch from the foreground, the rest from the background,
both without replacement, shuffled) on a counter-based stream of its own on the device (cnr_pixel_table_build / cnr_choose_pixels): no host
synchronisation, no per-step allocation, capturable in a HIP graph, and a function of (seed, step) alone, so the ranks of a ray-sharded run
draw the same batch without talking.  It does NOT reproduce the reference's pixels."""
import ctypes as C
import os
import warnings

import torch

from ._lib import dense_f32, grad_f32, library_for, ptr, save_named, saved_named, stream_of
from ._lib import resolve_library as _library


def choose_pixels(n_rays, pixels_per_image, device, mask=None, mask_rate=0.9):
    """Flat pixel indices (camera * H * W + row * W + column) of one training batch.

    Without a mask: uniform draws over ONE image's pixels, as the reference does (its indices never leave camera 0,
    ray_utils.py:58).  With a mask: a share ``mask_rate`` of the batch from the foreground pixels, the rest from the background,
    both without replacement, then shuffled.  Random-number consumption: randint | randperm(#fg), randperm(#bg), randperm(n)."""
    if mask is None:
        return torch.randint(0, pixels_per_image, (n_rays,)).to(device)
    flat = mask.reshape(-1)
    fg = torch.nonzero(flat > 0, as_tuple=True)[0]
    fg_order = torch.randperm(fg.shape[0])
    want_fg = int(mask_rate * n_rays)
    if want_fg > fg.shape[0]:
        warnings.warn(f"only {fg.shape[0]} foreground pixels for {want_fg} requested rays")
        want_fg = fg.shape[0]
    bg = torch.nonzero(flat == 0, as_tuple=True)[0]
    bg_order = torch.randperm(bg.shape[0])
    chosen = torch.cat([fg[fg_order[:want_fg]], bg[bg_order[:n_rays - want_fg]]], dim=-1)
    return chosen[torch.randperm(chosen.shape[0])]


class PixelSampler:
    """Pixel choice on the device: the pixel table of a mask stack and a {seed, step} random state (include/colorneus_render.h, "on-device
    pixel choice").  Not the reference's random stream -- the same sampling semantics on a Philox stream of its own.

    ``masks``: the DEVICE mask stack [N, H, W] (or [N, H * W]) the batches are drawn from -- a resident dataset's, built once; callers that
    upload a fresh batch stack per step call ``rebuild``.  Without masks (``n_images`` and ``pixels_per_image`` given) the draws are uniform
    with replacement, like the reference's unmasked route.  The sampler owns its state and its output buffers; the buffers are sized on first
    use and keep their addresses, and a draw neither allocates nor touches the host, so it may run inside graph.GraphedStep.  What ``draw``
    returns ARE those buffers: the next draw of the same size overwrites them (clone what must outlive it; a backward pass through the rays of a
    batch runs before the next draw).
    """

    def __init__(self, masks=None, *, n_images=None, pixels_per_image=None, seed=0, library=None, device=None):
        if masks is not None:
            if masks.dim() not in (2, 3):
                raise ValueError("masks [N, H, W] (or [N, H * W]) expected")
            device = masks.device
            n_images, pixels_per_image = masks.shape[0], masks[0].numel()
        elif n_images is None or pixels_per_image is None:
            raise ValueError("PixelSampler needs a mask stack, or n_images and pixels_per_image")
        if device is None:
            device = "cuda" if _library(library).backend.startswith("hip") else "cpu"
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = library_for(library, self.device, ("pixels", "chosen"))
        self.n_images, self.pixels_per_image = int(n_images), int(pixels_per_image)
        self.mask_shape = None
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)           # {seed, step}
        self.want_fg_buffer = torch.zeros(1, dtype=torch.int32, device=self.device)  # draw(mask_rate=None) reads the foreground count here
        self.order = self.fg_count = self.bg_count = self._scratch = None
        self._out, self._cams = {}, {}
        self._counts = torch.zeros(2, dtype=torch.int32, device=self.device)
        self.last_cams = self.last_idx = self.last_t_rand = None    # device views of the last draw: its images, indices, jitter
        self.seed(seed)
        if masks is not None:
            self.rebuild(masks)

    def seed(self, s, step=0):
        """Set the state: the same (seed, step) draws the same batch on every rank.  (A host-to-device copy: not inside a captured step.)"""
        wrap = lambda v: ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)
        self.state.copy_(torch.tensor([wrap(s), wrap(step)], dtype=torch.int64))

    @property
    def last_counts(self):
        """Device int32 [2] of the last masked draw: foreground draws made, background draws served."""
        return self._counts

    def rebuild(self, masks):
        """Build the pixel table of ``masks`` (same shape as before) into the sampler's buffers: three launches, no allocation after the first."""
        if masks.device != self.device:
            raise ValueError(f"masks are on {masks.device} but the sampler is on {self.device}")
        if masks.shape[0] != self.n_images or masks[0].numel() != self.pixels_per_image or (self.mask_shape not in (None, tuple(masks.shape))):
            raise ValueError(f"mask stack {tuple(masks.shape)} does not match the sampler's "
                             f"{self.mask_shape or (self.n_images, self.pixels_per_image)}")
        m = dense_f32(masks)
        if self.order is None:
            n = self.n_images
            self.order = torch.empty(n, self.pixels_per_image, dtype=torch.int32, device=self.device)
            self.fg_count, self.bg_count = (torch.zeros(n, dtype=torch.int32, device=self.device) for _ in range(2))
            self._scratch = self.lib.scratch("cnr_pixel_table_scratch_bytes", self.device, n, self.pixels_per_image, at_least=256)
        self.lib.call("cnr_pixel_table_build", ptr(m), self.n_images, self.pixels_per_image, ptr(self.order), ptr(self.fg_count), ptr(self.bg_count),
                      ptr(self._scratch[0]), self._scratch[1], stream_of(self.device))
        self.mask_shape = tuple(masks.shape)

    def check_stacks(self, image, mask=None):
        """The image [N, H, W, 3] / mask [N, H, W] stacks that go to the ray kernel with this sampler's (global) indices must be the stacks it
        was built on: same number of images, same H x W."""
        for name, t in (("image", image), ("mask", mask)):
            if t is None:
                continue
            hw = tuple(t.shape[1:3])
            ok = t.shape[0] == self.n_images and hw[0] * hw[1] == self.pixels_per_image
            if ok and self.mask_shape is not None and len(self.mask_shape) == 3:
                ok = hw == self.mask_shape[1:]
            if not ok:
                raise ValueError(f"{name} stack {tuple(t.shape)} is not the stack the sampler was built on: "
                                 f"{self.mask_shape or (self.n_images, self.pixels_per_image)}")

    def draw(self, n_rays, mask_rate=0.9, images=None, images_per_step=None, jitter=False, span=None):
        """One batch: int64 [n_rays] global pixel indices (image * H * W + pixel; -1 where the background cannot serve a draw), and with
        ``jitter`` the renderer's ``t_rand`` [n_rays, 1] as well (it is drawn either way: ``last_t_rand``).  Advances the step by one.

        ``mask_rate``: the foreground share, want_fg = int(mask_rate * n_rays) as the reference forms it; None: want_fg is read from
        ``want_fg_buffer`` on the device (a captured step following the MASK_RATE schedule).  ``images``: int32 device tensor of the images
        of this step, or ``images_per_step`` = B for B images chosen by the stream (default: all).  ``span`` (unmasked draws only): the
        index range, default one image's pixels as in the reference."""
        n = int(n_rays)
        cam_ids = None
        if images is not None:
            cam_ids = torch.as_tensor(images, dtype=torch.int32, device=self.device).contiguous()
            B = cam_ids.numel()
        else:
            B = self.n_images if images_per_step is None else int(images_per_step)
        table = self.order is not None
        out = self._out.get(n)
        if out is None:
            out = self._out[n] = (torch.empty(max(n, 0), dtype=torch.int64, device=self.device), torch.empty(max(n, 0), 1, dtype=torch.float32, device=self.device))
        cams = self._cams.get(B)
        if cams is None:
            cams = self._cams[B] = torch.empty(max(B, 1), dtype=torch.int32, device=self.device)
        want_dev = self.want_fg_buffer if (table and mask_rate is None) else None
        want_fg = int(mask_rate * n) if (table and mask_rate is not None) else 0
        self.lib.call("cnr_choose_pixels", ptr(self.state), n, want_fg, ptr(want_dev), ptr(cam_ids), B, self.n_images, self.pixels_per_image,
                      ptr(self.order), ptr(self.fg_count), ptr(self.bg_count), int(span or 0), ptr(out[0]), ptr(cams), ptr(self._counts),
                      ptr(out[1]), stream_of(self.device))
        self.last_cams, self.last_idx, self.last_t_rand = cams[:B], out[0], out[1]
        return (out[0], out[1]) if jitter else out[0]


_CHECK_INDICES = os.environ.get("CNR_CHECK_INDICES", "0") not in ("", "0")
_BAD = {}   # device -> int32 counter written by the ray kernel: pixel indices outside [0, n_cams * H * W) since the last check


def _bad_counter(dev):
    t = _BAD.get(dev)
    if t is None:
        t = _BAD[dev] = torch.zeros(1, dtype=torch.int32, device=dev)
    return t


def bad_index_count(device=None):
    """Out-of-range pixel indices the ray kernel has met on ``device`` (default: every device used) since the last call; resets the counter.
    Reads device memory, i.e. synchronises -- call it where the step synchronises anyway (next to the loss' .item())."""
    n = 0
    for dev, t in _BAD.items():
        if device is None or torch.device(device) == dev:
            n += int(t.item())
            t.zero_()
    return n


def raise_if_bad_indices(device=None):
    """The reference's torch indexing raises IndexError on an out-of-range pixel index (ray_utils.py:63-76); the ray kernel cannot raise -- it
    makes that ray NaN and counts it.  Call this at the step's synchronisation point (before the optimiser step, if NaN gradients must not
    reach the optimiser state): raises IndexError like the reference, one step late at most."""
    n = bad_index_count(device)
    if n:
        raise IndexError(f"{n} pixel index/indices outside [0, n_cams * H * W) reached cnr_gen_rays since the last check (their rays are NaN)")


class _GenRays(torch.autograd.Function):
    """autograd edge around cnr_gen_rays / cnr_gen_rays_backward."""

    @staticmethod
    def forward(ctx, lib, pix_idx, n, c2w, focal, H, W, normalize, opengl, image, mask, origin, radius, want_nearfar):
        dev = c2w.device
        c2w_c = dense_f32(c2w, -1, 4, 4)
        focal_c = dense_f32(focal, -1).to(dev)
        # every operand is dereferenced on c2w's device.  The image / mask stacks must already live there: moving a host-resident stack
        # (about 1 GB for DTU) on every step would be a silent per-step upload, so that is an error like the device mismatch the reference's
        # torch ops would raise; the small operands (focal, origin, the index list) are moved.
        for name, t in (("image", image), ("mask", mask)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} is on {t.device} but c2w is on {dev}: keep the image / mask stacks on the device that generates the rays")
        img, msk = dense_f32(image), dense_f32(mask)
        org = dense_f32(origin, -1).to(dev) if origin is not None else None
        idx = pix_idx.to(dev).contiguous().to(torch.int64) if pix_idx is not None else None
        n_cams = c2w_c.shape[0]
        for name, t in (("image", img), ("mask", msk)):
            if t is not None and t.shape[0] != n_cams:
                raise ValueError(f"{name} holds {t.shape[0]} cameras but c2w holds {n_cams}")
        # range of the indices: the ray kernel checks every index on the device (an index outside [0, n_cams * H * W) reads nothing and makes
        # that ray's outputs NaN; its backward contributes nothing) -- no host cost, no out-of-bounds access.  The host-side check below
        # raises like the reference's torch indexing would, but costs two device-to-host syncs: on request only (CNR_CHECK_INDICES=1);
        # the indices of choose_pixels, the only producer inside this module, are in range by construction
        if idx is not None and idx.numel() > 0 and _CHECK_INDICES:
            lo, hi = int(idx.min()), int(idx.max())
            if lo < 0 or hi >= n_cams * H * W:
                raise IndexError(f"pixel index range [{lo}, {hi}] outside [0, {n_cams * H * W})")
        f32 = dict(dtype=torch.float32, device=dev)
        rays_o, rays_d = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
        rgb = torch.empty(n, 3, **f32) if img is not None else None
        msel = torch.empty(n, **f32) if msk is not None else None
        near = torch.empty(n, **f32) if want_nearfar else None
        far = torch.empty(n, **f32) if want_nearfar else None
        lib.call("cnr_gen_rays", ptr(idx), n, ptr(c2w_c), c2w_c.shape[0], ptr(focal_c), H, W, int(normalize), int(opengl), ptr(img), ptr(msk),
                 ptr(org), float(radius), ptr(rays_o), ptr(rays_d), ptr(rgb), ptr(msel), ptr(near), ptr(far),
                 ptr(_bad_counter(dev)) if idx is not None else C.c_void_p(0), stream_of(c2w_c))
        ctx.lib, ctx.meta = lib, (n, H, W, int(normalize), int(opengl), float(radius), c2w.shape, focal.shape)
        save_named(ctx, idx=idx, c2w=c2w_c, focal=focal_c, origin=org)
        ctx.mark_non_differentiable(*[t for t in (rgb, msel) if t is not None])
        ctx.n_extra = (rgb is not None, msel is not None, want_nearfar)
        return (rays_o, rays_d, rgb if rgb is not None else torch.empty(0, device=dev), msel if msel is not None else torch.empty(0, device=dev),
                near if near is not None else torch.empty(0, device=dev), far if far is not None else torch.empty(0, device=dev))

    @staticmethod
    def backward(ctx, d_o, d_d, _d_rgb, _d_mask, d_near, d_far):
        sv, _ = saved_named(ctx)
        idx, c2w_c, focal_c, org = sv["idx"], sv["c2w"], sv["focal"], sv["origin"]
        n, H, W, normalize, opengl, radius, c2w_shape, focal_shape = ctx.meta
        dev = c2w_c.device
        need = ctx.needs_input_grad
        if not (need[3] or need[4]):
            return (None,) * 14
        d_o, d_d = grad_f32(d_o), grad_f32(d_d)
        has_nf = ctx.n_extra[2] and d_near is not None and d_far is not None and d_near.numel() == n
        d_near = grad_f32(d_near) if has_nf else None
        d_far = grad_f32(d_far) if has_nf else None
        d_c2w = torch.empty_like(c2w_c)
        d_focal = torch.empty(2, dtype=torch.float32, device=dev)
        scratch, nb = ctx.lib.scratch("cnr_gen_rays_backward", dev, nbytes=c2w_c.shape[0] * 2 * 4)   # n_cams * 2 floats: the header's formula
        ctx.lib.call("cnr_gen_rays_backward", ptr(idx), n, ptr(c2w_c), c2w_c.shape[0], ptr(focal_c), H, W, normalize, opengl,
                     ptr(org), radius, ptr(d_o), ptr(d_d), ptr(d_near), ptr(d_far), ptr(d_c2w), ptr(d_focal),
                     ptr(scratch), nb, stream_of(c2w_c))
        return (None, None, None, d_c2w.reshape(c2w_shape) if need[3] else None, d_focal.reshape(focal_shape) if need[4] else None,
                None, None, None, None, None, None, None, None, None)


def _generate(lib, pix_idx, n, c2w, focal, H, W, normalize, opengl, image=None, mask=None, origin=None, radius=1.0, want_nearfar=False):
    o, d, rgb, msel, near, far = _GenRays.apply(lib, pix_idx, n, c2w, focal, H, W, normalize, opengl, image, mask, origin, radius, want_nearfar)
    return o, d, (rgb if image is not None else None), (msel if mask is not None else None), (near if want_nearfar else None), (far if want_nearfar else None)


def _pixels(sampler, n_rays, H, W, device, image, mask, mask_rate):
    """The batch's pixel indices: the reference's CPU stream, or the draw of a PixelSampler built on these very stacks."""
    if sampler is None:
        return choose_pixels(n_rays, H * W, device, mask, mask_rate)
    sampler.check_stacks(image, mask)
    return sampler.draw(n_rays, mask_rate)


def get_rays_multicam(c2w, focal, image, n_rays, normalize=False, mask=None, mask_rate=0.9, return_mask=False, opengl=False, library=None,
                      sampler=None):
    """Random n rays in world space from N cameras: the reference's signature and return values (ray_utils.py:16-87).  ``sampler``: a
    PixelSampler built on the ``mask`` stack (image / mask must be the stacks it was built on) draws the pixels on the device instead."""
    assert c2w.dim() == 3 and image.dim() == 4, "c2w [N,4,4] and image [N,H,W,3] expected (multi-camera form)"
    H, W = image.shape[1], image.shape[2]
    idx = _pixels(sampler, n_rays, H, W, c2w.device, image, mask, mask_rate)
    if return_mask:
        assert mask is not None
    o, d, rgb, msel, _, _ = _generate(_library(library), idx, idx.shape[0], c2w, focal, H, W, normalize, opengl, image=image,
                                      mask=mask if return_mask else None)
    return o, d, rgb, msel


def get_rays_at(c2w, focal, H, W, normalize=False, opengl=False, library=None):
    """All rays of one camera, [H, W, 3] each (ray_utils.py:90-119)."""
    assert c2w.dim() == 2, "c2w [4,4] expected (single-camera form)"
    o, d, _, _, _, _ = _generate(_library(library), None, H * W, c2w, focal, H, W, normalize, opengl)
    return o.reshape(H, W, 3), d.reshape(H, W, 3)


def rays_for_training(c2w, focal, image, n_rays, origin, radius, normalize=False, mask=None, mask_rate=0.9, return_mask=False, opengl=False,
                      library=None, sampler=None):
    """What NeuS_Trainer.render does in front of the renderer call (NeuS_Trainer.py:104-120) in one launch: pixel choice, rays,
    (rays_o - origin) / radius, near / far from the unit sphere, colours and mask values of the chosen pixels.
    Returns rays_o, rays_d, near, far, rgb_gt, mask_select (None unless return_mask).  ``sampler``: as in get_rays_multicam; a draw the
    background could not serve is a NaN ray that bad_index_count() counts."""
    assert c2w.dim() == 3 and image.dim() == 4
    H, W = image.shape[1], image.shape[2]
    idx = _pixels(sampler, n_rays, H, W, c2w.device, image, mask, mask_rate)
    o, d, rgb, msel, near, far = _generate(_library(library), idx, idx.shape[0], c2w, focal, H, W, normalize, opengl, image=image,
                                           mask=mask if return_mask else None, origin=torch.as_tensor(origin, dtype=torch.float32), radius=float(radius),
                                           want_nearfar=True)
    return o, d, near, far, rgb, msel


def near_far_from_sphere(rays_o, rays_d):
    """near / far of the unit sphere along each ray (ray_utils.py:7-13); differentiable torch ops on [n, 3] tensors (callers that
    already hold rays; rays_for_training gets the same values from the ray kernel)."""
    a = (rays_d * rays_d).sum(-1)
    mid = -(rays_o * rays_d).sum(-1) / a
    return mid - 1.0, mid + 1.0
