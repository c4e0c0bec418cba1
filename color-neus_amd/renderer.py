"""Drop-in renderer modules: same constructor argument (the MODEL.RENDERER cfg sub-tree), same ``forward`` signature and
return dict, same parameter names/shapes as the reference's ``NeuS`` / ``Color_NeuS`` classes
(lib/models/renderers/NeuS.py:68-420, Color_NeuS.py:10-138) -- so reference checkpoints load with strict=True --
but every tensor operation of the path runs in the HIP library behind the C ABI (include/colorneus_render.h).

PyTorch is used for: parameter storage, device memory allocation, the autograd graph edge, stream selection."""
import ctypes as C
import math

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import dense_f32, grad_f32, param_array, ptr, save_named, saved_named, stream_of
from .config import RenderConfig, config_from_node

_OUT_DIFF = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error", "depth",
             "global_color", "delta_relight"]
_SAMPLE_OUT = ["sdf_samples", "color_samples", "global_color_samples"]   # per-sample network outputs (only with want_samples)
_NON_DIFF_OUT = ["inside_sphere", "z_vals", "eik_sums"]
_RETURN_KEYS = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error", "inside_sphere",
                "depth", "global_color", "delta_relight_ray_sum", "delta_relight", "z_vals", "eik_sums"]   # of NeuSRenderer.forward's dict


def _output_shapes(color_type, mode, R=0, M=0):
    """The shape of every output of one render call, keyed by _lib.OUTPUT_FIELDS' names (None: not produced, passed as NULL).  ``mode``:
    "saving" (the training dict), "loss_only" (what compute_loss needs: no [R][M][3] tensors, the relight term as per-ray sums),
    "with_samples" (the dict plus the per-sample network outputs for the N_OUTSIDE mixing) or "forward_only" (same entries as "saving")."""
    color = color_type == "Color_NeuS"
    loss_only, samples = mode == "loss_only", mode == "with_samples"
    return dict(color_fine=(R, 3), s_val=(R, 1), cdf_fine=(R, M), weight_sum=(R, 1), weight_max=(R, 1),
                gradients=None if loss_only else (R, M, 3), weights=(R, M), gradient_error=(), inside_sphere=(R, M), depth=(R,),
                global_color=(R, 3) if color else None, delta_relight=(R, M, 3) if (color and not loss_only) else None,
                delta_relight_ray_sum=(R,) if (color and loss_only) else None, z_vals=(R, M), eik_sums=(2,),
                sdf_samples=(R, M) if samples else None, color_samples=(R, M, 3) if samples else None,
                global_color_samples=(R, M, 3) if (samples and color) else None)


def _alloc_outputs(cfg, R, device, mode):
    """The output tensors of one render call: an uninitialised float32 tensor for every entry of _output_shapes, None for the others."""
    return {k: None if shape is None else torch.empty(shape, dtype=torch.float32, device=device)
            for k, shape in _output_shapes(cfg.type, mode, R, cfg.n_total).items()}


def _render_output_names(color_type, mode):
    """(differentiable names, per-sample names, non-differentiable names) of the tuple _RenderFunction returns, in its order: the outputs
    _output_shapes says the call produces.  The one place that order is stated: whoever names the tuple's entries does it through here."""
    made = {k for k, shape in _output_shapes(color_type, mode).items() if shape is not None}
    return ([k for k in _OUT_DIFF + ["delta_relight_ray_sum"] if k in made], [k for k in _SAMPLE_OUT if k in made], list(_NON_DIFF_OUT))


def _render(owner, mode, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio, prune_eps, params):
    """_RenderFunction.apply in ``mode`` ("saving", "with_samples" or "loss_only"): its outputs as {name: tensor}."""
    want = {"saving": False, "with_samples": True, "loss_only": "loss_only"}[mode]   # the edge's want_samples argument
    res = _RenderFunction.apply(owner, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio, prune_eps, want, *params)
    return dict(zip(sum(_render_output_names(owner.rcfg.type, mode), []), res))


def _rays_f32(rays_o, rays_d, near, far):
    """The four ray inputs as the contiguous float32 tensors the library reads (near / far flattened)."""
    return dense_f32(rays_o), dense_f32(rays_d), dense_f32(near, -1), dense_f32(far, -1)


def _inputs(rays_o, rays_d, near, far, t_rand=None, z_override=None, background_rgb=None, cos_anneal_ratio=0.0, prune_eps=0.0):
    """CnrInputs of contiguous float32 tensors (``z_override``: the z_vals output buffer that already holds the given positions, or None)."""
    return _lib.CnrInputs(rays_o=ptr(rays_o), rays_d=ptr(rays_d), near_=ptr(near), far_=ptr(far), t_rand=ptr(t_rand),
                          z_vals_override=ptr(z_override) if z_override is not None else None, background_rgb=ptr(background_rgb),
                          n_rays=rays_o.shape[0], cos_anneal_ratio=float(cos_anneal_ratio), prune_eps=float(prune_eps))


def _forward_call(owner, entry, bytes_fn, mode, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio, prune_eps, params):
    """What cnr_render_forward and cnr_render_forward_only share: (outputs, float32 ray inputs, detached parameters, context / scratch buffer)."""
    lib, ccfg, cfg = owner._lib, owner._ccfg, owner.rcfg
    R = rays_o.shape[0]
    rays = _rays_f32(rays_o, rays_d, near, far)
    out = _alloc_outputs(cfg, R, rays_o.device, mode)
    if z_override is not None:
        out["z_vals"].copy_(z_override.detach().reshape(R, cfg.n_total))
    plist = [p.detach().contiguous() for p in params]
    cin = _inputs(*rays, t_rand, out["z_vals"] if z_override is not None else None, background_rgb, cos_anneal_ratio, prune_eps)
    cout = _lib.CnrOutputs(**{k: ptr(out[k]) for k in _lib.OUTPUT_FIELDS})
    buf, nbytes = lib.scratch(bytes_fn, rays_o.device, C.byref(ccfg), R)
    lib.call(entry, C.byref(ccfg), param_array(plist), C.byref(cin), C.byref(cout), ptr(buf), nbytes, stream_of(rays_o))
    return out, rays, plist, buf


class _RenderFunction(torch.autograd.Function):
    """autograd edge around cnr_render_forward / cnr_render_backward."""

    @staticmethod
    def forward(ctx, owner, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio, prune_eps, want_samples, *params):
        cfg = owner.rcfg
        # want_samples: False / True (per-sample network outputs for the N_OUTSIDE mixing) / "loss_only" (the training outputs compute_loss
        # needs: no [R][M][3] dict tensors, the relight term as per-ray sums)
        mode = "loss_only" if want_samples == "loss_only" else "with_samples" if want_samples is True else "saving"
        out, (rays_o_c, rays_d_c, near_c, far_c), plist, ctx_buf = _forward_call(
            owner, "cnr_render_forward", "cnr_ctx_bytes", mode, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio,
            prune_eps, params)
        ctx.owner = owner
        # tensors go through save_for_backward (outputs held in a plain attribute would form an uncollectable
        # tensor -> grad_fn -> ctx -> tensor cycle and leak the multi-GB context buffer every step)
        ctx.cfg_aux = (float(cos_anneal_ratio), z_override is not None, float(prune_eps))
        save_named(ctx, plist, rays_o=rays_o_c, rays_d=rays_d_c, near=near_c, far=far_c, z_vals=out["z_vals"], gradients=out["gradients"],
                   ctx_buf=ctx_buf, t_rand=t_rand, background_rgb=background_rgb)
        ctx.rays_need_grad = rays_o.requires_grad or rays_d.requires_grad
        # z is an affine function of near / far only without importance sampling (NeuS.py:311-313; with it z is built under no_grad, :343)
        ctx.nearfar_need_grad = (near.requires_grad or far.requires_grad) and cfg.n_importance == 0 and z_override is None
        ctx.nearfar_shapes = (near.shape, far.shape)
        ctx.set_materialize_grads(False)   # outputs the loss does not use arrive as None in backward (which passes NULL), not as zero tensors
        diff, samples, non_diff = _render_output_names(cfg.type, mode)
        ctx.mark_non_differentiable(*[out[k] for k in non_diff])
        ctx.grad_names = diff + samples   # the outputs whose gradients backward receives, in the tuple's order
        return tuple(out[k] for k in diff + samples + non_diff)

    @staticmethod
    def backward(ctx, *gouts):
        lib, ccfg = ctx.owner._lib, ctx.owner._ccfg
        car, had_override, prune_eps = ctx.cfg_aux
        if prune_eps > 0:
            raise RuntimeError("prune_eps > 0 is inference-only (early-termination compaction); call under torch.no_grad()")
        sv, plist = saved_named(ctx)
        rays_o, rays_d, near, far, z_vals, ctx_buf = (sv[k] for k in ("rays_o", "rays_d", "near", "far", "z_vals", "ctx_buf"))
        R = rays_o.shape[0]
        gmap = {}
        for k, g in zip(ctx.grad_names, gouts):
            if k == "delta_relight_ray_sum":   # d loss / d (sum_jc delta[r, j, c]) = the per-ray gradient of every delta[r, j, c]
                if g is not None:
                    gmap["delta_relight_per_ray"] = grad_f32(g.reshape(-1))
                continue
            if k == "delta_relight" and g is not None and g.dim() == 3 and g.stride(1) == 0 and g.stride(2) == 0:
                # a gradient that is constant along each ray and over rgb (what the relight loss term produces, loss.compute_loss_fused
                # hands it over as an expanded view): pass the per-ray vector, never materialise [R][M][3]
                gmap["delta_relight_per_ray"] = grad_f32(g[:, 0, 0])
                continue
            gmap[k] = grad_f32(g)
        cg = _lib.CnrOutGrads(**{k: ptr(gmap.get(k)) for k in _lib.OUT_GRAD_FIELDS})
        flat, dparams, darr = _lib.flat_grads(plist, rays_o.device)
        d_o = torch.empty_like(rays_o) if ctx.rays_need_grad else None
        d_d = torch.empty_like(rays_d) if ctx.rays_need_grad else None
        d_near = torch.empty_like(near) if ctx.nearfar_need_grad else None
        d_far = torch.empty_like(far) if ctx.nearfar_need_grad else None
        gin = _lib.CnrInGrads(d_params=C.cast(darr, C.POINTER(C.c_void_p)), d_rays_o=ptr(d_o), d_rays_d=ptr(d_d),
                              d_near=ptr(d_near), d_far=ptr(d_far))
        cin = _inputs(rays_o, rays_d, near, far, sv["t_rand"], z_vals if had_override else None, sv["background_rgb"], car)
        cout = _lib.CnrOutputs(z_vals=ptr(z_vals), gradients=ptr(sv["gradients"]))   # the only forward outputs backward reads (gradients: NULL = kept in the context buffer)
        scratch, nbytes = lib.scratch("cnr_bwd_scratch_bytes", rays_o.device, C.byref(ccfg), R)
        lib.call("cnr_render_backward", C.byref(ccfg), param_array(plist), C.byref(cin), C.byref(cout), ptr(ctx_buf), ctx_buf.numel(),
                 C.byref(cg), C.byref(gin), ptr(scratch), nbytes, stream_of(rays_o))
        if d_near is not None:
            d_near, d_far = d_near.reshape(ctx.nearfar_shapes[0]), d_far.reshape(ctx.nearfar_shapes[1])
        res = (None, d_o, d_d, d_near, d_far, None, None, None, None, None, None) + tuple(dparams)
        del dparams, flat   # (_lib.flat_grads: the views go to autograd without a second reference)
        return res


def _render_forward_only(owner, rays_o, rays_d, near, far, t_rand, z_override, background_rgb, cos_anneal_ratio, prune_eps, params):
    """cnr_render_forward_only: the inference use of the path (NeuS_Trainer.validate_image, NeuS_Trainer.py:236-245; evaluation.py).  Same
    outputs, bit-identical values; nothing is kept for a backward pass and the scratch buffer is about half of the training context (14.1 GB against 29.7 GB at 8192 rays)."""
    return _forward_call(owner, "cnr_render_forward_only", "cnr_infer_scratch_bytes", "forward_only", rays_o, rays_d, near, far, t_rand,
                         z_override, background_rgb, cos_anneal_ratio, prune_eps, params)[0]


def sample_pdf(bins, weights, n_samples, det=False, library=None):
    """ray_utils.sample_pdf(bins, weights, n_samples, det=False) (lib/models/tools/ray_utils.py:121-154; same default as the reference) on the
    device: the hierarchical sampler's own kernel (cnr_sample_pdf; NeuS.up_sample passes det=True, NeuS.py:180).  det=False: the uniform draws come
    from torch.rand on the CPU generator with the reference's shape and call order (ray_utils.py:135-136), the inversion runs in the same kernel."""
    lib = _lib.resolve_library(library)
    bins, weights = dense_f32(bins), dense_f32(weights)
    n = bins.shape[-1]
    assert weights.shape[-1] == n - 1 and bins.shape[:-1] == weights.shape[:-1]
    R = bins.numel() // n
    out = torch.empty(*bins.shape[:-1], n_samples, dtype=torch.float32, device=bins.device)
    if det:
        lib.call("cnr_sample_pdf", ptr(bins), ptr(weights), R, n, int(n_samples), ptr(out), stream_of(bins))
    else:
        u = torch.rand(list(bins.shape[:-1]) + [int(n_samples)]).to(bins.device).contiguous()
        lib.call("cnr_sample_pdf_u", ptr(bins), ptr(weights), ptr(u), R, n, int(n_samples), ptr(out), stream_of(bins))
    return out


# --------------------------------------------------------------------------------------------------------------------
# parameter containers with the reference's state_dict names
# --------------------------------------------------------------------------------------------------------------------
class _WNLinear(nn.Module):
    """nn.utils.weight_norm(nn.Linear) parameter triple: bias, weight_g (out,1), weight_v (out,in)."""

    def __init__(self, weight, bias):
        super().__init__()
        self.bias = nn.Parameter(bias)
        self.weight_g = nn.Parameter(weight.norm(dim=1, keepdim=True))
        self.weight_v = nn.Parameter(weight)


class _Linear(nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(bias)


def _default_linear(i, o):
    lin = nn.Linear(i, o)   # kaiming-uniform default init, like the reference's freshly built nn.Linear
    return lin.weight.detach().clone(), lin.bias.detach().clone()


def _wrap(w, b, weight_norm):
    return _WNLinear(w, b) if weight_norm else _Linear(w, b)


def _embed_dim(multires, d=3):
    return d * (1 + 2 * multires) if multires > 0 else d


# Points per library call of an SDF point query: a larger query is split into calls of at most this many points, fewer when the context
# and backward scratch of that many points (cnr_sdf_query_ctx_bytes + cnr_sdf_query_bwd_scratch_bytes) would exceed _QUERY_MAX_BYTES.
_QUERY_MAX_POINTS = 1 << 20
_QUERY_MAX_BYTES = 16 << 30


class _Binding:
    """A renderer's one link to the library: the lazily resolved ``library`` argument, the C config, the parameter inventory, and the calls
    that the renderer and its ``sdf_network`` both make.  Held as a plain attribute of both (not a module, no parameters or buffers:
    state_dict and named_parameters stay those of the reference); a deepcopy shares it, since it holds nothing of the copied module."""

    def __init__(self, library, rcfg):
        self._library_arg = library
        self._lib_obj = None
        self.ccfg = _lib.c_config(rcfg)
        self.d_out = rcfg.sdf_d_out
        self._inventory = self._names = None
        self._max_pts = {}

    def __deepcopy__(self, memo):
        return self

    @property
    def lib(self):
        if self._lib_obj is None:
            self._lib_obj = _lib.resolve_library(self._library_arg)
        return self._lib_obj

    def inventory(self):
        """[(name, rows, cols)] of the configuration's parameters in the library's canonical order."""
        if self._inventory is None:
            self._inventory = self.lib.param_inventory(self.ccfg)
        return self._inventory

    def names(self):
        """(number of canonical parameters, sdf_network parameter names in canonical order, without the prefix)."""
        if self._names is None:
            inv = self.inventory()
            self._names = (len(inv), [n[len("sdf_network."):] for n, _, _ in inv if n.startswith("sdf_network.")])
        return self._names

    def max_points(self, want_grad):
        """Points per call (see _QUERY_MAX_POINTS), from the library's size functions: fixed part + per-point part at two sizes."""
        if want_grad not in self._max_pts:
            L, wg = self.lib.lib, int(want_grad)
            size = lambda n: L.cnr_sdf_query_ctx_bytes(C.byref(self.ccfg), n, wg) + L.cnr_sdf_query_bwd_scratch_bytes(C.byref(self.ccfg), n, wg)
            n0 = 1 << 16
            per_pt = (size(2 * n0) - size(n0)) / n0
            fixed = size(n0) - per_pt * n0
            fit = int((_QUERY_MAX_BYTES - fixed) / per_pt) // 128 * 128
            self._max_pts[want_grad] = max(128, min(_QUERY_MAX_POINTS, fit))
        return self._max_pts[want_grad]

    def param_array(self, tensors):
        """The canonical inventory as a pointer array: the sdf_network entries (the leading ones) from ``tensors``, NULL for the others."""
        return param_array(tensors, self.names()[0])

    def forward(self, x, params, want_grad, want_feat, keep_ctx):
        """cnr_sdf_query_forward on the float32 [n, 3] points x (0 < n): (sdf [n, 1], feat [n, F] or None, grad [n, 3] or None, ctx or None)."""
        L, n, dev = self.lib, x.shape[0], x.device
        f32 = dict(dtype=torch.float32, device=dev)
        sdf = torch.empty(n, 1, **f32)
        feat = torch.empty(n, self.d_out - 1, **f32) if want_feat else None
        grad = torch.empty(n, 3, **f32) if want_grad else None
        cbuf, nb = L.scratch("cnr_sdf_query_ctx_bytes", dev, C.byref(self.ccfg), n, int(want_grad))
        L.call("cnr_sdf_query_forward", C.byref(self.ccfg), self.param_array(params), ptr(x), n, int(want_grad), ptr(sdf), ptr(feat),
               ptr(grad), ptr(cbuf), nb, stream_of(x))
        return sdf, feat, grad, (cbuf if keep_ctx else None)

    def evaluate(self, entry, bytes_fn, size_args, params, dev, *args, at_least=0):
        """An evaluation entry point ``entry(cfg, params, *args, scratch, scratch_bytes, stream)`` on ``dev``: ``params`` (the canonical
        inventory, or its leading sdf_network entries) are detached and go as the pointer array, the scratch is what the size function
        ``bytes_fn(cfg, *size_args)`` asks for."""
        plist = [p.detach().contiguous() for p in params]
        scratch, nb = self.lib.scratch(bytes_fn, dev, C.byref(self.ccfg), *size_args, at_least=at_least)
        self.lib.call(entry, C.byref(self.ccfg), self.param_array(plist), *args, ptr(scratch), nb, stream_of(dev))

    def sdf_eval(self, x, params, sign=1.0):
        """cnr_sdf_eval: sign * sdf [n, 1] at the float32 points x [n, 3] (0 < n), nothing kept for a backward pass."""
        n = x.shape[0]
        out = torch.empty(n, 1, dtype=torch.float32, device=x.device)
        self.evaluate("cnr_sdf_eval", "cnr_sdf_eval_scratch_bytes", (n,), params, x.device, ptr(x), n, float(sign), ptr(out))
        return out


class _SdfQueryFunction(torch.autograd.Function):
    """autograd edge around cnr_sdf_query_forward / cnr_sdf_query_backward: outputs sdf [n, 1], then feat [n, F] (want_feat), then
    grad = d sdf / d x [n, 3] (want_grad).  The backward is the library's complete first- and second-order SDF backward, run once with
    whatever cotangents arrived; it is not itself differentiable (third order)."""

    @staticmethod
    def forward(ctx, binding, want_grad, want_feat, x, *params):
        plist = [p.detach().contiguous() for p in params]
        sdf, feat, grad, cbuf = binding.forward(x.detach(), plist, want_grad, want_feat, keep_ctx=True)
        ctx.binding, ctx.want_grad, ctx.want_feat = binding, want_grad, want_feat
        save_named(ctx, plist, x=x.detach(), cbuf=cbuf)
        ctx.set_materialize_grads(False)   # unused outputs arrive as None and go to the library as NULL
        return tuple(t for t in (sdf, feat, grad) if t is not None)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        binding, L = ctx.binding, ctx.binding.lib
        sv, plist = saved_named(ctx)
        x, cbuf = sv["x"], sv["cbuf"]
        gouts = list(gouts)
        d_sdf = grad_f32(gouts.pop(0))
        d_feat = grad_f32(gouts.pop(0)) if ctx.want_feat else None
        d_grad = grad_f32(gouts.pop(0)) if ctx.want_grad else None
        n, dev = x.shape[0], x.device
        need_x, need_p = ctx.needs_input_grad[3], any(ctx.needs_input_grad[4:])
        d_x = torch.empty(n, 3, dtype=torch.float32, device=dev) if need_x else None
        dparams, flat, darr = [None] * len(plist), None, None
        if need_p:
            # one flat buffer of the sdf_network parameters in canonical order: a step with point losses only hands optim.flat_view_of_grads
            # one buffer; when the step also renders, this backward runs first (its node is newer), autograd adopts these views as the sdf
            # .grad tensors and adds the render's sdf gradients into them, while the colour / relight gradients stay in the render's buffer:
            # flat_view_of_grads over all parameters is then None and the all-reduce takes its gathered-copy path (same values, one copy)
            flat, dparams, darr = _lib.flat_grads(plist, dev, binding.names()[0])
        if need_x or need_p:
            wg = int(ctx.want_grad)
            scratch, nb = L.scratch("cnr_sdf_query_bwd_scratch_bytes", dev, C.byref(binding.ccfg), n, wg)
            L.call("cnr_sdf_query_backward", C.byref(binding.ccfg), binding.param_array(plist), ptr(x), n, wg, ptr(d_sdf), ptr(d_feat),
                   ptr(d_grad), ptr(cbuf), cbuf.numel(), darr, ptr(d_x), ptr(scratch), nb, stream_of(x))
        res = (None, None, None, d_x) + tuple(d if need else None for d, need in zip(dparams, ctx.needs_input_grad[4:]))
        del dparams, flat   # (_lib.flat_grads: the views go to autograd without a second reference)
        return res


class _SDFNet(nn.Module):
    """SDFNetwork (fields.py:12-115): its parameters with the geometric initialisation (fields.py:31-75), and its methods forward / sdf /
    sdf_hidden_appearance / gradient evaluated by the library (cnr_sdf_query_*, differentiable to second order in the parameters and the
    points).  The renderer attaches the library binding after construction."""

    def __init__(self, c: RenderConfig):
        super().__init__()
        d0 = _embed_dim(c.sdf_multires)
        dims = [d0] + [c.sdf_d_hidden] * c.sdf_n_layers + [c.sdf_d_out]
        n = len(dims)
        for l in range(n - 1):
            out_dim = dims[l + 1] - d0 if (l + 1) in c.sdf_skip_in else dims[l + 1]
            w, b = _default_linear(dims[l], out_dim)
            if c.sdf_geometric_init:
                if l == n - 2:
                    sign = -1.0 if c.sdf_inside_outside else 1.0
                    nn.init.normal_(w, mean=sign * math.sqrt(math.pi) / math.sqrt(dims[l]), std=0.0001)
                    b.fill_(-sign * c.sdf_bias)
                elif c.sdf_multires > 0 and l == 0:
                    b.zero_()
                    w[:, 3:].zero_()
                    nn.init.normal_(w[:, :3], 0.0, math.sqrt(2) / math.sqrt(out_dim))
                elif c.sdf_multires > 0 and l in c.sdf_skip_in:
                    b.zero_()
                    nn.init.normal_(w, 0.0, math.sqrt(2) / math.sqrt(out_dim))
                    w[:, -(d0 - 3):].zero_()
                else:
                    b.zero_()
                    nn.init.normal_(w, 0.0, math.sqrt(2) / math.sqrt(out_dim))
            setattr(self, f"lin{l}", _wrap(w, b, c.sdf_weight_norm))
        self._query = None   # the renderer's _Binding, set by it

    # -- the reference's methods (fields.py:81-115) ------------------------------------------------------------------------------------------
    def _query_params(self):
        named = dict(self.named_parameters())
        return [named[k] for k in self._query.names()[1]]

    def _run(self, x, want_grad, want_feat):
        """(sdf [n, 1], feat [n, F] or None, grad [n, 3] or None) at the float32 points x [n, 3], through the autograd function when a
        gradient can flow, as a plain query otherwise; split into calls of at most max_points points."""
        if self._query is None:
            raise RuntimeError("sdf_network has no library binding (it is built by NeuSRenderer / ColorNeuSRenderer)")
        q = self._query
        params = self._query_params()
        n, dev = x.shape[0], x.device
        if n == 0:   # (the C ABI takes n_points > 0)
            e = lambda w: torch.zeros(0, w, dtype=torch.float32, device=dev)
            return e(1), (e(q.d_out - 1) if want_feat else None), (e(3) if want_grad else None)
        track = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
        step = q.max_points(want_grad)
        parts = []
        for s0 in range(0, n, step):
            xs = x[s0:s0 + step]
            if track:
                outs = list(_SdfQueryFunction.apply(q, want_grad, want_feat, xs, *params))
                parts.append((outs.pop(0), outs.pop(0) if want_feat else None, outs.pop(0) if want_grad else None))
            else:
                with torch.no_grad():
                    parts.append(q.forward(xs.detach().contiguous(), [p.detach().contiguous() for p in params], want_grad, want_feat,
                                           keep_ctx=False)[:3])
        if len(parts) == 1:
            return parts[0]
        cat = lambda i: torch.cat([p[i] for p in parts]) if parts[0][i] is not None else None
        return cat(0), cat(1), cat(2)

    @staticmethod
    def _points(x):
        return x.reshape(-1, 3).to(torch.float32).contiguous()

    def forward(self, inputs):
        """[n, d_out]: sdf (= h_top[0] / scale) followed by the d_out - 1 features (fields.py:81-96)."""
        sdf, feat, _ = self._run(self._points(inputs), False, True)
        return torch.cat([sdf, feat], dim=-1)

    def sdf(self, x):
        """[n, 1] (fields.py:98-99); without a gradient to form it is the library's plain sdf evaluation (cnr_sdf_eval)."""
        x = self._points(x)
        if self._query is not None and x.shape[0] > 0 and not (torch.is_grad_enabled() and
                                                               (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return self._query.sdf_eval(x, self._query_params())
        return self._run(x, False, False)[0]

    def sdf_hidden_appearance(self, x):
        return self.forward(x)

    def gradient(self, x):
        """[n, 1, 3]: d sdf / d x (fields.py:105-115), differentiable in the points and the parameters (the eikonal term's double
        backward); like the reference it sets x.requires_grad."""
        x.requires_grad_(True)
        return self._run(self._points(x), True, False)[2].unsqueeze(1)


class _ColorNet(nn.Module):
    def __init__(self, c: RenderConfig):
        super().__init__()
        d0 = c.col_d_in + c.col_d_feature
        if c.col_multires_view > 0:
            d0 += _embed_dim(c.col_multires_view) - 3
        dims = [d0] + [c.col_d_hidden] * c.col_n_layers + [c.col_d_out]
        for l in range(len(dims) - 1):
            w, b = _default_linear(dims[l], dims[l + 1])
            setattr(self, f"lin{l}", _wrap(w, b, c.col_weight_norm))


class _VarianceNet(nn.Module):
    def __init__(self, c: RenderConfig):
        super().__init__()
        self.variance = nn.Parameter(torch.tensor(float(c.init_val)))


class _RelightNet(nn.Module):
    def __init__(self, c: RenderConfig):
        super().__init__()
        d_in = c.rel_d_in + (3 if c.rel_include_grad else 0)
        if c.rel_multires_view > 0:
            d_in += _embed_dim(c.rel_multires_view) - 3
        H = c.rel_d_hidden
        self.in_layer = _Linear(*_default_linear(d_in, H))
        layers = []
        for i in range(c.rel_n_layers):
            if i == c.rel_y_in_layer - 1 and c.rel_y_in_layer == c.rel_n_layers:
                layers.append(_Linear(*_default_linear(3 + H, c.rel_d_out)))
            elif i == c.rel_y_in_layer - 1:
                layers.append(_Linear(*_default_linear(3 + H, H)))
            elif i == c.rel_n_layers - 1:
                layers.append(_Linear(*_default_linear(H, c.rel_d_out)))
            else:
                layers.append(_Linear(*_default_linear(H, H)))
        self.rl_mlp = nn.ModuleList(layers)


class NeuSRenderer(nn.Module):
    """MI355X-native counterpart of the reference ``NeuS`` renderer class (NeuS.py:68-420)."""

    TYPE = "NeuS"

    def __init__(self, cfg, library=None):
        super().__init__()
        self.name = type(self).__name__
        self.cfg = cfg
        rcfg = cfg if isinstance(cfg, RenderConfig) else config_from_node(cfg)
        rcfg.type = self.TYPE   # the class, not cfg.TYPE, decides (as in the reference registry)
        rcfg.validate()
        self.rcfg = rcfg
        self.sdf_network = _SDFNet(rcfg)
        self.deviation_network = _VarianceNet(rcfg)
        self.color_network = _ColorNet(rcfg)
        self.n_samples, self.n_importance = rcfg.n_samples, rcfg.n_importance
        self.n_outside, self.up_sample_steps, self.perturb, self.N = rcfg.n_outside, rcfg.up_sample_steps, rcfg.perturb, rcfg.N
        if self.n_outside > 0:   # NeRF++ background (NeuS.py:87-91): parameters here, arithmetic in the library (background.py)
            from .background import NeRF
            self.nerf = NeRF()
        self._order = None
        self._binding = self.sdf_network._query = _Binding(library, rcfg)   # (a plain attribute: no child module, no state)

    # -- library plumbing -------------------------------------------------------------------------------------------
    _lib = property(lambda self: self._binding.lib)      # the RenderLibrary and the CnrConfig, as the edges, tests and tools read them
    _ccfg = property(lambda self: self._binding.ccfg)

    def _ordered_params(self):
        """Parameters in the library's canonical order (names = reference state_dict names)."""
        if self._order is None:
            # nerf.*: the background network has its own inventory (cnr_nerf_param_info)
            self._order = _lib.ordered_names(self._binding.inventory(), dict(self.named_parameters()), exempt_prefix="nerf.")
        named = dict(self.named_parameters())
        return [named[k] for k in self._order]

    def _jitter_to_device(self, t_cpu, dev):
        """H2D copy of the per-ray jitter without stalling the host: a plain .to(device) from pageable memory blocks until the
        stream has drained, i.e. once per step.  Two pinned staging buffers are used alternately; an event per buffer guards reuse."""
        if dev.type != "cuda":
            return t_cpu.to(dev)
        n = t_cpu.shape[0]
        st = getattr(self, "_jit_stage", None)
        if st is None or st["n"] != n or st["dev"] != dev:
            st = {"n": n, "dev": dev, "i": 0, "buf": [torch.empty(n, 1, pin_memory=True) for _ in range(2)], "ev": [None, None]}
            self._jit_stage = st
        i = st["i"]
        st["i"] = 1 - i
        if st["ev"][i] is not None:
            st["ev"][i].synchronize()          # the copy issued two calls ago
        st["buf"][i].copy_(t_cpu)
        out = st["buf"][i].to(dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        st["ev"][i] = ev
        return out

    # -- NeuS.forward (NeuS.py:294-408) -------------------------------------------------------------------------------
    def forward(self, rays_o, rays_d, near, far, perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0, z_vals=None,
                prune_eps=0.0, training_outputs="dict", forward_only=None, **kwargs):
        """input: rays_o [n_rays,3], rays_d [n_rays,3], near/far [n_rays].  Extra kwarg ``z_vals`` (not in the reference)
        overrides the sampler so that render_core can be checked at fixed sample positions; ``prune_eps`` > 0 (inference only, not in the
        reference) skips the colour / relight networks for samples whose compositing weight is below it (NeuS_Trainer.validate_image
        consumes only color_fine and depth, :244-245).  ``training_outputs="loss_only"`` (not in the reference; default "dict" = the reference's
        return dict): the two [n_rays, M, 3] entries `gradients` and `delta_relight` are not materialised; the dict carries
        `delta_relight_ray_sum` [n_rays] instead, which is all compute_loss needs (loss.compute_loss_fused accepts either form).
        ``forward_only`` (not in the reference): None = automatic -- the call takes the forward-only entry point of the library
        (cnr_render_forward_only: identical values, nothing kept for a backward pass) whenever no gradient can be asked of it, i.e. under
        torch.no_grad() or when neither a parameter nor an input requires grad; False forces the saving forward, True the forward-only one."""
        if training_outputs not in ("dict", "loss_only"):
            raise ValueError("training_outputs must be 'dict' or 'loss_only'")
        loss_only = training_outputs == "loss_only"
        if loss_only and (self.n_outside > 0 or prune_eps > 0):
            raise ValueError("training_outputs='loss_only' is for the plain training step (no background samples, no pruning)")
        n_rays = len(rays_o)
        dev = rays_d.device
        if n_rays == 0:
            return self._empty_batch(dev, background_rgb, cos_anneal_ratio)
        perturb = self.perturb
        if perturb_overwrite >= 0:
            perturb = perturb_overwrite
        t_rand = None
        t_given = kwargs.get("t_rand")        # extra kwarg (not in the reference): the jitter draw of THESE rays, e.g. a rank's rows of the
        if perturb > 0 and (z_vals is None or self.n_outside > 0):   # whole batch's draw in ray-sharded training (parallel.draw_jitter)
            if t_given is not None:
                if t_given.numel() != n_rays:
                    raise ValueError(f"t_rand must hold one draw per ray ({n_rays}), got {tuple(t_given.shape)}")
                t_cpu = t_given.detach().reshape(n_rays, 1).float()
            else:
                t_cpu = torch.rand([n_rays, 1])   # CPU generator, exactly like NeuS.py:325 (drawn even under a z override when the
            if z_vals is None:                    # background draw follows, so that the stream stays the reference's)
                t_rand = self._jitter_to_device(t_cpu, dev) if t_cpu.device.type == "cpu" else t_cpu.to(dev).contiguous()
        bg = None
        if background_rgb is not None:
            bg = torch.as_tensor(background_rgb, dtype=torch.float32, device=dev).reshape(-1)[:3].contiguous()
        params = self._ordered_params()
        if self.n_outside > 0:
            return self._forward_with_background(rays_o, rays_d, near, far, perturb, t_rand, bg, cos_anneal_ratio, params, z_vals)
        if forward_only is None:
            forward_only = not loss_only and not (torch.is_grad_enabled() and (any(p.requires_grad for p in params) or any(
                torch.is_tensor(t) and t.requires_grad for t in (rays_o, rays_d, near, far))))
        if forward_only:
            if loss_only:
                raise ValueError("training_outputs='loss_only' belongs to the training step, not to a forward-only call")
            out = _render_forward_only(self, rays_o, rays_d, near, far, t_rand, z_vals, bg, cos_anneal_ratio, prune_eps, params)
        else:
            out = _render(self, "loss_only" if loss_only else "saving", rays_o, rays_d, near, far, t_rand, z_vals, bg, cos_anneal_ratio, prune_eps,
                          params)
        # the reference's dict in its key order, then the extra keys (not in the reference dict): z_vals, and eik_sums =
        # {sum relax*(|g|-1)^2, sum relax}, needed by ray-sharded training
        return {k: out[k] for k in _RETURN_KEYS if out.get(k) is not None}

    def _empty_batch(self, dev, background_rgb, cos_anneal_ratio):
        """No rays (the reference runs its torch ops on empty tensors): the C ABI takes n_rays > 0, so one dummy ray is rendered without
        jitter and every output is cut to zero rows -- right shapes and dtypes, gradient_error = 0 / 1e-5 = 0, and exactly-zero gradients for
        every parameter (the CPU generator is not consumed, as torch.rand([0, 1]) consumes nothing)."""
        o = torch.tensor([[0.0, 0.0, -3.0]], device=dev)
        d = torch.tensor([[0.0, 0.0, 1.0]], device=dev)
        one = self.forward(o, d, torch.full((1, 1), 2.0, device=dev), torch.full((1, 1), 4.0, device=dev), perturb_overwrite=0,
                           background_rgb=background_rgb, cos_anneal_ratio=cos_anneal_ratio)
        return {k: (v * 0.0 if v.dim() == 0 or k == "eik_sums" else v[:0]) for k, v in one.items()}

    def up_sample(self, rays_o, rays_d, z_vals, sdf, n_importance, inv_s):
        """NeuS.up_sample (NeuS.py:136-181): n_importance new sample positions per ray from the current z / sdf."""
        z = dense_f32(z_vals)
        R, n = z.shape
        out = torch.empty(R, int(n_importance), dtype=torch.float32, device=z.device)
        self._lib.call("cnr_up_sample", ptr(dense_f32(rays_o)), ptr(dense_f32(rays_d)), ptr(z), ptr(dense_f32(sdf, R, n)), R, n,
                       int(n_importance), float(inv_s), ptr(out), stream_of(z))
        return out

    # -- N_OUTSIDE > 0 (NeuS.py:313-369): four library calls chained by autograd (background.py); no tensor arithmetic here ------------
    def _forward_with_background(self, rays_o, rays_d, near, far, perturb, t_rand, bg, cos_anneal_ratio, params, z_override):
        from . import background as B
        rc, lib = self.rcfg, self._lib
        R = len(rays_o)
        dev = rays_o.device
        # second draw of the CPU generator, like NeuS.py:335
        t_out = torch.rand([R, self.n_outside]).to(dev) if perturb > 0 else None
        if z_override is None:
            z_vals = self._sample_z(rays_o, rays_d, near, far, t_rand)      # (built under no_grad in the reference when N_IMPORTANCE > 0, NeuS.py:343)
        else:
            z_vals = z_override.detach().reshape(R, rc.n_total).float()
        sample_dist = 2.0 / self.n_samples
        z_feed, _src = B.OutsideZ.apply(lib, far, t_out, z_vals, int(self.n_samples), int(self.n_outside))
        nparams = self.nerf.ordered_params(lib)
        bg_alpha, bg_color = B.Background.apply(lib, self.nerf.config(), sample_dist, rays_o, rays_d, z_feed, *nparams)
        f = _render(self, "with_samples", rays_o, rays_d, near, far, None, z_vals, None, 0.0, 0.0, params)
        color = rc.type == "Color_NeuS"
        cres = B.CompositeBg.apply(lib, sample_dist, float(cos_anneal_ratio), bg, rays_o, rays_d, z_vals, z_feed, f["sdf_samples"], f["gradients"],
                                   f["color_samples"], f.get("global_color_samples"), bg_alpha, bg_color, self.deviation_network.variance)
        c = dict(zip(sum(B.composite_output_names(color), []), cres))
        out = {k: c[k] for k in ("color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max")}
        out.update(gradients=f["gradients"], weights=c["weights"], gradient_error=c["gradient_error"], inside_sphere=c["inside_sphere"], depth=c["depth"])
        if color:
            out["global_color"] = c["global_color"]
            out["delta_relight"] = f["delta_relight"]
        out["z_vals"] = z_vals
        out["eik_sums"] = c["eik_sums"]
        return out

    def _sample_z(self, rays_o, rays_d, near, far, t_rand):
        """The hierarchical sampler on its own (cnr_sample_z): final z_vals [R, M], no gradient (NeuS.py:343)."""
        rc, dev = self.rcfg, rays_o.device
        R = len(rays_o)
        rays = _rays_f32(rays_o, rays_d, near, far)
        z = torch.empty(R, rc.n_total, dtype=torch.float32, device=dev)
        cin = _inputs(*rays, t_rand)
        self._binding.evaluate("cnr_sample_z", "cnr_ctx_bytes", (R,), self._ordered_params(), dev, C.byref(cin), ptr(z))
        return z

    # -- evaluation paths (NeuS.py:14-64, 410-420) ---------------------------------------------------------------------
    def _param_array(self):
        """(detached ordered parameters, their pointer array) for a direct call of an entry point (the methods below go through evaluate)."""
        plist = [p.detach().contiguous() for p in self._ordered_params()]
        return plist, param_array(plist)

    def sdf(self, pts, sign=1.0):
        """sdf_network.sdf(pts) (fields.py:99) on the device, any number of points."""
        pts = dense_f32(pts, -1, 3)
        if pts.shape[0] == 0:   # (the C ABI takes n_points > 0)
            return torch.empty(0, 1, dtype=torch.float32, device=pts.device)
        return self._binding.sdf_eval(pts, self._ordered_params(), sign)

    def extract_fields(self, bound_min, bound_max, device, resolution):
        """u = -sdf on linspace(bound_min, bound_max, resolution)^3 (NeuS.py:14-28); stays on the device, one D2H at the end."""
        bmin, bmax = _lib.float3(bound_min), _lib.float3(bound_max)
        u = torch.empty(resolution, resolution, resolution, dtype=torch.float32, device=torch.device(device))
        self._binding.evaluate("cnr_sdf_grid", "cnr_sdf_grid_scratch_bytes", (resolution,), self._ordered_params(), u.device, bmin, bmax,
                               resolution, ptr(u))
        return u

    def extract_fields_slab(self, bound_min, bound_max, device, resolution, x_begin, x_end):
        """Rows x in [x_begin, x_end) of extract_fields' lattice (same values): the unit of the sharded evaluation (parallel.sharded_extract_fields)."""
        bmin, bmax = _lib.float3(bound_min), _lib.float3(bound_max)
        u = torch.empty(x_end - x_begin, resolution, resolution, dtype=torch.float32, device=torch.device(device))
        self._binding.evaluate("cnr_sdf_grid_slab", "cnr_sdf_grid_slab_scratch_bytes", (resolution, x_begin, x_end), self._ordered_params(),
                               u.device, bmin, bmax, resolution, x_begin, x_end, ptr(u), at_least=1)
        return u

    def marching_cubes(self, u, bound_min, bound_max, threshold=0.0):
        """Iso-surface of a device-resident lattice u[x][y][z] (cnr_mc_count / cnr_mc_emit): returns device tensors
        (vertices [V, 3] float32 in world coordinates, triangles [F, 3] int32)."""
        u = dense_f32(u)
        res = u.shape[0]
        assert u.shape == (res, res, res)
        lib = self._lib
        scratch, nb = lib.scratch("cnr_mc_scratch_bytes", u.device, res)
        totals = torch.empty(2, dtype=torch.int32, device=u.device)
        lib.call("cnr_mc_count", ptr(u), res, float(threshold), ptr(scratch), nb, ptr(totals), stream_of(u))
        nv, nt = (int(x) for x in totals.tolist())     # the one host round trip: the caller owns the output buffers
        verts = torch.empty(max(nv, 1), 3, dtype=torch.float32, device=u.device)
        tris = torch.empty(max(nt, 1), 3, dtype=torch.int32, device=u.device)
        bmin, bmax = _lib.float3(bound_min), _lib.float3(bound_max)
        lib.call("cnr_mc_emit", ptr(u), res, float(threshold), bmin, bmax, ptr(scratch), nb, ptr(verts), ptr(tris), stream_of(u))
        return verts[:nv], tris[:nt]

    def _clean(self, verts, tris, clean):
        """The opt-in clean-up of an extracted mesh (meshops.clean_mesh on the renderer's library): ``clean`` is "largest" or a dict of
        clean_mesh's keyword arguments (keep, min_faces, min_ratio)."""
        from . import meshops
        kw = {"keep": clean} if isinstance(clean, str) else dict(clean)
        verts, tris, _, _ = meshops.clean_mesh(verts, tris, library=self._lib, **kw)
        return verts, tris

    def extract_geometry(self, bound_min, bound_max, device, resolution, threshold=0.0, clean=None, cull=None):
        """NeuS.extract_geometry (NeuS.py:31-40): -sdf on the lattice, iso-surface at ``threshold``; (vertices np (V,3), triangles np (F,3)).
        The lattice stays in HBM and the surface is extracted there (the reference copies 512 MiB to the host for PyMCubes).
        ``clean`` (default None: the raw iso-surface, as the reference returns it): "largest" or a dict of ``meshops.clean_mesh`` keyword
        arguments removes floaters on the device before the copy to the host.  ``cull`` (default None): a ``meshops.MeshCuller``, applied
        BEFORE ``clean``: what the views never constrained goes first, then the components are chosen among what is left."""
        u = self.extract_fields(bound_min, bound_max, device, resolution)
        verts, tris = self.marching_cubes(u, bound_min, bound_max, threshold)
        if cull is not None:
            verts, tris, _, _ = cull(verts, tris)
        if clean is not None:
            verts, tris = self._clean(verts, tris, clean)
        return verts.cpu().numpy().astype(np.float64), tris.cpu().numpy().astype(np.int64)

    def vertex_colors(self, vertices):
        """extract_color on device tensors: ``vertices`` [V, 3] on the renderer's device -> rgb [V, 3] float32 there, no host round trip."""
        pts = dense_f32(vertices, -1, 3)
        n = pts.shape[0]
        rgb = torch.empty(n, 3, dtype=torch.float32, device=pts.device)
        if n > 0:
            self._binding.evaluate("cnr_vertex_color", "cnr_vertex_color_scratch_bytes", (n,), self._ordered_params(), pts.device, ptr(pts), n,
                                   ptr(rgb))
        return rgb

    def extract_color(self, vertices, device):
        """Per-vertex colour = color_network(pts, g, -g, feat) (NeuS.py:44-64); returns np (V,3)."""
        pts = torch.as_tensor(np.asarray(vertices), dtype=torch.float32, device=torch.device(device))
        return self.vertex_colors(pts).cpu().numpy()

    def render_mesh_view(self, bound_min, bound_max, resolution, c2w, focal, H, W, threshold=0.0, opengl=False, origin=None, radius=1.0,
                         z_near=1e-3, background=None, clean=None, cull=None):
        """The extracted, coloured mesh seen from a camera without leaving the device: extract_fields -> marching_cubes -> vertex colours
        (cnr_vertex_color) -> imaging.rasterize_mesh.  ``c2w`` [4, 4] on the renderer's device decides the device.  Returns rasterize_mesh's
        dict plus ``"vertices"``, ``"triangles"`` and ``"colors"`` (device tensors).  ``clean`` as in ``extract_geometry``: the floaters are
        removed BEFORE the colours are evaluated, so the colour network does not run on debris; ``cull`` (a ``meshops.MeshCuller``, with
        views of its own) likewise, before ``clean``.  Not differentiable."""
        from . import imaging
        u = self.extract_fields(bound_min, bound_max, c2w.device, resolution)
        verts, tris = self.marching_cubes(u, bound_min, bound_max, threshold)
        if cull is not None:
            verts, tris, _, _ = cull(verts, tris)
        if clean is not None:
            verts, tris = self._clean(verts, tris, clean)
        colors = self.vertex_colors(verts)
        out = imaging.rasterize_mesh(verts, tris, c2w, focal, H, W, colors=colors, opengl=opengl, origin=origin, radius=radius, z_near=z_near,
                                     background=background, library=self._lib)
        out.update(vertices=verts, triangles=tris, colors=colors)
        return out


class ColorNeuSRenderer(NeuSRenderer):
    """MI355X-native counterpart of the reference ``Color_NeuS`` class (Color_NeuS.py:10-138)."""

    TYPE = "Color_NeuS"

    def __init__(self, cfg, library=None):
        if not isinstance(cfg, RenderConfig):
            mode = cfg.COLOR.MODE if hasattr(cfg, "COLOR") else cfg["COLOR"]["MODE"]
            assert mode == "no_view_dir"   # Color_NeuS.py:14
        super().__init__(cfg, library)
        assert self.rcfg.type == "Color_NeuS"
        self.relight_network = _RelightNet(self.rcfg)


# --------------------------------------------------------------------------------------------------------------------
# registry look-alike (lib/utils/builder.py:50-309) so that cfg-driven construction reads like the reference
# --------------------------------------------------------------------------------------------------------------------
class _Registry:
    def __init__(self, name):
        self.name = name
        self._module_dict = {}

    def get(self, key):
        return self._module_dict.get(key, None)

    def register_module(self, name=None, force=False, module=None):
        def _reg(cls):
            key = name or cls.__name__
            if not force and key in self._module_dict:
                raise KeyError(f"{key} is already registered in {self.name}")
            self._module_dict[key] = cls
            return cls
        return _reg(module) if module is not None else _reg


RENDERER = _Registry("renderer")
RENDERER.register_module(name="NeuS", module=NeuSRenderer)
RENDERER.register_module(name="Color_NeuS", module=ColorNeuSRenderer)


def build_renderer(cfg, **kwargs):
    """build_from_cfg(cfg, RENDERER) (builder.py:9-47): cfg.TYPE selects the class, which is called as cls(cfg)."""
    typ = cfg.get("TYPE", None) if hasattr(cfg, "get") else getattr(cfg, "TYPE", None)
    if typ is None:
        raise AssertionError("cfg.TYPE is required")
    cls = RENDERER.get(typ)
    if cls is None:
        raise KeyError(f"{typ} is not in the {RENDERER.name} registry")
    return cls(cfg, **kwargs)


def register_into(registry, force=True):
    """Override the reference's own RENDERER entries ("NeuS", "Color_NeuS") with the native classes:
    ``register_into(lib.utils.builder.RENDERER)`` before ``build_model_init`` keeps train.py / evaluation.py unchanged."""
    registry.register_module(name="NeuS", force=force, module=NeuSRenderer)
    registry.register_module(name="Color_NeuS", force=force, module=ColorNeuSRenderer)
