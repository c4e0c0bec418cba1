"""N_OUTSIDE > 0: the NeRF++ background of NeuS (lib/models/renderers/NeuS.py:95-134, 313-369; NeRF, fields.py:192-274) on the device library.

No shipped configuration enables it (N_OUTSIDE is absent from every config/*.yml, NeuS.py:82).  Everything arithmetic runs behind the C ABI
(include/colorneus_render.h, "N_OUTSIDE > 0"): this module holds the background network's PARAMETERS under the reference's names
(``nerf.pts_linears.0.weight`` ...: reference checkpoints load with strict=True) and the three autograd edges around the library calls

    OutsideZ        cnr_outside_z / cnr_outside_z_backward                        z_vals_outside, sorted z_vals_feed          NeuS.py:315-338, 353-355
    Background      cnr_background_forward / cnr_background_backward              render_core_outside: alpha, sigmoid(rgb)    NeuS.py:95-134
    CompositeBg     cnr_composite_background_forward / ..._backward               render_core's mixing + compositing          NeuS.py:236-292, Color_NeuS.py:66-138

The foreground fields (sdf, normals, colours per sample) come from the render call's per-sample outputs and take their gradients back through
it (renderer._RenderFunction).  No tensor arithmetic of the path is done in torch here; without the library the module fails loudly."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import dense_f32, grad_f32, param_array, ptr, save_named, saved_named, stream_of


class NeRF(nn.Module):
    """Parameter storage of the reference's NeRF background network with its defaults (NeuS.__init__ falls back to NeRF() for every cfg,
    NeuS.py:87-91): 8 x 256 ReLU layers on PE-10 of the 4-vector (x / r, 1 / r), skip at 4, view branch on PE-4 (fields.py:215-231)."""

    def __init__(self, D=8, W=256, d_in=4, d_in_view=3, multires=10, multires_view=4, skips=(4,)):
        super().__init__()
        self.D, self.W, self.multires, self.multires_view, self.skips = D, W, multires, multires_view, tuple(skips)
        ch = d_in * (1 + 2 * multires)
        ch_view = d_in_view * (1 + 2 * multires_view)
        self.pts_linears = nn.ModuleList([nn.Linear(ch, W)] + [nn.Linear(W + ch, W) if i in self.skips else nn.Linear(W, W) for i in range(D - 1)])
        self.views_linears = nn.ModuleList([nn.Linear(ch_view + W, W // 2)])
        self.feature_linear = nn.Linear(W, W)
        self.alpha_linear = nn.Linear(W, 1)
        self.rgb_linear = nn.Linear(W // 2, 3)
        self._order = None

    def config(self):
        mask = 0
        for i in self.skips:
            mask |= 1 << i
        return _lib.CnrNerfConfig(D=self.D, W=self.W, multires=self.multires, multires_view=self.multires_view, skip_mask=mask)

    def ordered_params(self, lib):
        """Parameters in the library's canonical order (cnr_nerf_param_info), checked against this module's own names and shapes."""
        if self._order is None:
            inv = lib.param_inventory(self.config(), "cnr_nerf_param_count", "cnr_nerf_param_info")
            self._order = _lib.ordered_names(inv, dict(self.named_parameters()))
        named = dict(self.named_parameters())
        return [named[k] for k in self._order]

    def forward(self, *a, **k):
        raise RuntimeError("the background network is evaluated by the render library (background.Background), not by this module")


class OutsideZ(torch.autograd.Function):
    """z_vals_feed = sort(cat(z_vals, far / flip(zz) + 1 / n_samples)) and the source index of every entry."""

    @staticmethod
    def forward(ctx, lib, far, t_rand, z_vals, n_samples, n_outside):
        R, M = z_vals.shape
        dev = z_vals.device
        far_c, z_c = dense_f32(far, -1), dense_f32(z_vals)
        t_c = dense_f32(t_rand.to(dev)) if t_rand is not None else None
        z_feed = torch.empty(R, M + n_outside, dtype=torch.float32, device=dev)
        src = torch.empty(R, M + n_outside, dtype=torch.int32, device=dev)
        lib.call("cnr_outside_z", ptr(far_c), ptr(t_c), ptr(z_c), R, M, n_outside, n_samples, ptr(z_feed), ptr(src), stream_of(z_c))
        ctx.lib, ctx.meta = lib, (R, M, n_samples, n_outside, far.shape)
        save_named(ctx, src=src, t_rand=t_c)
        ctx.mark_non_differentiable(src)
        return z_feed, src

    @staticmethod
    def backward(ctx, d_z_feed, _d_src):
        sv, _ = saved_named(ctx)
        R, M, n_samples, n_outside, far_shape = ctx.meta
        dz = grad_f32(d_z_feed)
        d_far = torch.empty(R, dtype=torch.float32, device=dz.device)
        d_z = torch.empty(R, M, dtype=torch.float32, device=dz.device) if ctx.needs_input_grad[3] else None
        ctx.lib.call("cnr_outside_z_backward", ptr(sv["t_rand"]), ptr(sv["src"]), ptr(dz), R, M, n_outside, n_samples, ptr(d_far), ptr(d_z),
                     stream_of(dz))
        return None, d_far.reshape(far_shape), None, d_z, None, None


class Background(torch.autograd.Function):
    """render_core_outside (NeuS.py:95-134): per-sample alpha and colour of the background network at z_feed."""

    @staticmethod
    def forward(ctx, lib, ncfg, sample_dist, rays_o, rays_d, z_feed, *params):
        R, MF = z_feed.shape
        dev = z_feed.device
        o, d, zf = dense_f32(rays_o), dense_f32(rays_d), dense_f32(z_feed)
        plist = [dense_f32(p) for p in params]
        alpha = torch.empty(R, MF, dtype=torch.float32, device=dev)
        color = torch.empty(R, MF, 3, dtype=torch.float32, device=dev)
        buf, nb = lib.scratch("cnr_background_ctx_bytes", dev, C.byref(ncfg), R, MF)
        lib.call("cnr_background_forward", C.byref(ncfg), param_array(plist), ptr(o), ptr(d), ptr(zf), R, MF, float(sample_dist), ptr(alpha),
                 ptr(color), ptr(buf), nb, stream_of(zf))
        ctx.lib, ctx.ncfg, ctx.meta = lib, ncfg, (R, MF, float(sample_dist))
        save_named(ctx, plist, o=o, d=d, zf=zf, color=color, buf=buf)
        ctx.set_materialize_grads(False)
        return alpha, color

    @staticmethod
    def backward(ctx, d_alpha, d_color):
        lib, ncfg = ctx.lib, ctx.ncfg
        R, MF, sample_dist = ctx.meta
        sv, plist = saved_named(ctx)
        o, d, zf, color, buf = (sv[k] for k in ("o", "d", "zf", "color", "buf"))
        dev = zf.device
        da, dc = grad_f32(d_alpha), grad_f32(d_color)
        flat, gviews, garr = _lib.flat_grads(plist, dev)
        d_o, d_d = torch.empty(R, 3, dtype=torch.float32, device=dev), torch.empty(R, 3, dtype=torch.float32, device=dev)
        d_zf = torch.empty(R, MF, dtype=torch.float32, device=dev)
        scratch, nb = lib.scratch("cnr_background_bwd_scratch_bytes", dev, C.byref(ncfg), R, MF)
        lib.call("cnr_background_backward", C.byref(ncfg), param_array(plist), ptr(o), ptr(d), ptr(zf), R, MF, sample_dist, ptr(buf), buf.numel(),
                 ptr(color), ptr(da), ptr(dc), garr, ptr(d_o), ptr(d_d), ptr(d_zf), ptr(scratch), nb, stream_of(zf))
        res = (None, None, None, d_o, d_d, d_zf, *gviews)
        del gviews, flat   # (_lib.flat_grads: the views go to autograd without a second reference)
        return res


_COMP_OUT = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "weights", "gradient_error", "depth", "global_color"]


def composite_output_names(has_gc):
    """(differentiable names, non-differentiable names) of the tuple CompositeBg returns, in its order; ``has_gc``: global_color_samples were
    given (Color_NeuS).  The one place that order is stated: forward, backward and the renderer all name the tuple through it."""
    return [k for k in _COMP_OUT if has_gc or k != "global_color"], ["inside_sphere", "eik_sums"]


class CompositeBg(torch.autograd.Function):
    """The tail of render_core with a background: S-density alpha, inside / outside mixing, compositing over M + N_OUTSIDE samples."""

    @staticmethod
    def forward(ctx, lib, sample_dist, cos_anneal_ratio, background_rgb, rays_o, rays_d, z_vals, z_feed, sdf, grads, color, gcolor, bg_alpha, bg_color,
                variance):
        R, M = z_vals.shape
        MF = z_feed.shape[1]
        dev = z_vals.device
        f32 = dict(dtype=torch.float32, device=dev)
        c = dense_f32
        t = dict(rays_o=c(rays_o), rays_d=c(rays_d), z_vals=c(z_vals), z_feed=c(z_feed), sdf=c(sdf), grads=c(grads), color=c(color), gcolor=c(gcolor),
                 bg_alpha=c(bg_alpha), bg_color=c(bg_color), variance=c(variance, -1), bg=c(background_rgb))
        out = dict(color_fine=torch.empty(R, 3, **f32), s_val=torch.empty(R, 1, **f32), cdf_fine=torch.empty(R, M, **f32), weight_sum=torch.empty(R, 1, **f32),
                   weight_max=torch.empty(R, 1, **f32), weights=torch.empty(R, MF, **f32), gradient_error=torch.empty((), **f32),
                   inside_sphere=torch.empty(R, M, **f32), depth=torch.empty(R, **f32), global_color=torch.empty(R, 3, **f32) if gcolor is not None else None,
                   eik_sums=torch.empty(2, **f32))
        cin = CompositeBg._cin(t, R, M, MF, sample_dist, cos_anneal_ratio)
        cout = _lib.CnrOutputs(**{k: ptr(out.get(k)) for k in _lib.OUTPUT_FIELDS})
        scratch, nb = lib.scratch("cnr_composite_background_scratch_bytes", dev, R)
        lib.call("cnr_composite_background_forward", C.byref(cin), C.byref(cout), ptr(scratch), nb, stream_of(t["z_vals"]))
        ctx.lib, ctx.meta = lib, (R, M, MF, float(sample_dist), float(cos_anneal_ratio), gcolor is not None, variance.shape)
        save_named(ctx, **t, weights=out["weights"], eik_sums=out["eik_sums"])
        ctx.set_materialize_grads(False)
        diff, non_diff = composite_output_names(gcolor is not None)
        ctx.mark_non_differentiable(*[out[k] for k in non_diff])
        return tuple(out[k] for k in diff + non_diff)

    @staticmethod
    def _cin(t, R, M, MF, sample_dist, cos_anneal_ratio):
        return _lib.CnrBgCompositeIn(rays_o=ptr(t["rays_o"]), rays_d=ptr(t["rays_d"]), z_vals=ptr(t["z_vals"]), z_feed=ptr(t["z_feed"]), n_rays=R, n_z=M,
                                     n_feed=MF, sample_dist=float(sample_dist), sdf_samples=ptr(t["sdf"]), gradients=ptr(t["grads"]),
                                     color_samples=ptr(t["color"]), global_color_samples=ptr(t["gcolor"]), bg_alpha=ptr(t["bg_alpha"]),
                                     bg_color=ptr(t["bg_color"]), variance=ptr(t["variance"]), cos_anneal_ratio=float(cos_anneal_ratio),
                                     background_rgb=ptr(t["bg"]))

    @staticmethod
    def backward(ctx, *gouts):
        lib = ctx.lib
        R, M, MF, sample_dist, car, has_gc, var_shape = ctx.meta
        t, _ = saved_named(ctx)
        weights, eik_sums = t["weights"], t["eik_sums"]
        dev = weights.device
        f32 = dict(dtype=torch.float32, device=dev)
        g = {k: grad_f32(v) for k, v in zip(composite_output_names(has_gc)[0], gouts)}
        go = _lib.CnrOutGrads(**{k: ptr(g.get(k)) for k in _lib.OUT_GRAD_FIELDS})
        cin = CompositeBg._cin(t, R, M, MF, sample_dist, car)
        cout = _lib.CnrOutputs(**{k: ptr({"weights": weights, "eik_sums": eik_sums}.get(k)) for k in _lib.OUTPUT_FIELDS})
        # (composite_bg_args checks the forward output pointers: the backward only reads weights and eik_sums, the rest may be any valid buffers)
        dummyR = torch.empty(R, max(M, 3), **f32)
        for k in ("color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "inside_sphere", "depth", "gradient_error", "global_color"):
            setattr(cout, k, ptr(dummyR))
        d = dict(d_sdf_samples=torch.empty(R, M, **f32), d_gradients=torch.empty(R, M, 3, **f32), d_color_samples=torch.empty(R, M, 3, **f32),
                 d_global_color_samples=torch.empty(R, M, 3, **f32) if has_gc else None, d_bg_alpha=torch.empty(R, MF, **f32),
                 d_bg_color=torch.empty(R, MF, 3, **f32), d_variance=torch.empty(1, **f32), d_rays_d=torch.empty(R, 3, **f32),
                 d_z_vals=torch.zeros(R, M, **f32), d_z_feed=torch.empty(R, MF, **f32))
        gi = _lib.CnrBgCompositeGrads(**{k: ptr(v) for k, v in d.items()})
        scratch, nb = lib.scratch("cnr_composite_background_scratch_bytes", dev, R)
        lib.call("cnr_composite_background_backward", C.byref(cin), C.byref(cout), C.byref(go), C.byref(gi), ptr(scratch), nb, stream_of(weights))
        need = ctx.needs_input_grad
        return (None, None, None, None, None, d["d_rays_d"] if need[5] else None, d["d_z_vals"] if need[6] else None, d["d_z_feed"] if need[7] else None,
                d["d_sdf_samples"], d["d_gradients"], d["d_color_samples"], d["d_global_color_samples"], d["d_bg_alpha"], d["d_bg_color"],
                d["d_variance"].reshape(var_shape))
