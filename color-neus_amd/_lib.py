"""ctypes binding of the C ABI declared in include/colorneus_render.h.

The product library is ``libcolorneus_hip.so`` next to this file (built by ``__graft_entry__.build()`` /
``make -C color-neus_amd/csrc hip``).  There is NO fallback: if it is missing, loading raises."""
import ctypes as C
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))


class CnrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("type", "n_samples", "n_importance", "up_sample_steps", "sdf_d_hidden", "sdf_n_layers",
                                         "sdf_d_out", "sdf_multires", "sdf_skip_mask", "sdf_weight_norm")] + \
               [("sdf_scale", C.c_float)] + \
               [(n, C.c_int32) for n in ("col_mode", "col_d_feature", "col_d_hidden", "col_n_layers", "col_multires_view",
                                         "col_weight_norm", "col_squeeze_out", "rel_d_hidden", "rel_n_layers", "rel_y_in_layer",
                                         "rel_multires_view", "rel_include_grad", "rel_inv_sigmoid")]


_FP = C.c_void_p


class CnrInputs(C.Structure):
    _fields_ = [("rays_o", _FP), ("rays_d", _FP), ("near_", _FP), ("far_", _FP), ("t_rand", _FP), ("z_vals_override", _FP),
                ("background_rgb", _FP), ("n_rays", C.c_int64), ("cos_anneal_ratio", C.c_float), ("prune_eps", C.c_float)]


OUTPUT_FIELDS = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error",
                 "inside_sphere", "depth", "global_color", "delta_relight", "z_vals", "eik_sums", "sdf_samples", "color_samples",
                 "global_color_samples", "delta_relight_ray_sum"]
OUT_GRAD_FIELDS = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error",
                   "depth", "global_color", "delta_relight", "sdf_samples", "color_samples", "global_color_samples",
                   "delta_relight_per_ray"]


class CnrOutputs(C.Structure):
    _fields_ = [(n, _FP) for n in OUTPUT_FIELDS]


class CnrOutGrads(C.Structure):
    _fields_ = [(n, _FP) for n in OUT_GRAD_FIELDS]


class CnrNerfConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("D", "W", "multires", "multires_view", "skip_mask")]


class CnrBgCompositeIn(C.Structure):
    _fields_ = [("rays_o", _FP), ("rays_d", _FP), ("z_vals", _FP), ("z_feed", _FP), ("n_rays", C.c_int64), ("n_z", C.c_int32), ("n_feed", C.c_int32),
                ("sample_dist", C.c_float), ("sdf_samples", _FP), ("gradients", _FP), ("color_samples", _FP), ("global_color_samples", _FP),
                ("bg_alpha", _FP), ("bg_color", _FP), ("variance", _FP), ("cos_anneal_ratio", C.c_float), ("background_rgb", _FP)]


class CnrBgCompositeGrads(C.Structure):
    _fields_ = [(n, _FP) for n in ("d_sdf_samples", "d_gradients", "d_color_samples", "d_global_color_samples", "d_bg_alpha", "d_bg_color",
                                   "d_variance", "d_rays_d", "d_z_vals", "d_z_feed")]


class CnrKernelTiming(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("kind", C.c_int32), ("nt", C.c_int32), ("P", C.c_int64), ("N", C.c_int32),
                ("K", C.c_int32), ("pairs", C.c_int32), ("ms", C.c_float), ("bytes", C.c_double)]


class CnrLossConfig(C.Structure):
    _fields_ = [("lambda_fine", C.c_float), ("lambda_eikonal", C.c_float), ("lambda_mask", C.c_float), ("lambda_relight", C.c_float),
                ("rgb_l1", C.c_int32), ("include_mask", C.c_int32)]


class CnrAdamConfig(C.Structure):
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("max_norm", C.c_float),
                ("step", C.c_int32), ("hyper_dev", C.c_void_p)]


class CnrInGrads(C.Structure):
    _fields_ = [("d_params", C.POINTER(_FP)), ("d_rays_o", _FP), ("d_rays_d", _FP), ("d_near", _FP), ("d_far", _FP)]


class CnrCameraConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_cams", "pose_mode", "focal_order", "fx_only", "H", "W", "has_init_c2w")]


_MODE = {"idr": 0, "no_view_dir": 1, "no_normal": 2}


def c_config(cfg) -> CnrConfig:
    mask = 0
    for l in cfg.sdf_skip_in:
        mask |= 1 << int(l)
    return CnrConfig(type=1 if cfg.type == "Color_NeuS" else 0, n_samples=cfg.n_samples, n_importance=cfg.n_importance,
                     up_sample_steps=cfg.up_sample_steps, sdf_d_hidden=cfg.sdf_d_hidden, sdf_n_layers=cfg.sdf_n_layers,
                     sdf_d_out=cfg.sdf_d_out, sdf_multires=cfg.sdf_multires, sdf_skip_mask=mask,
                     sdf_weight_norm=int(cfg.sdf_weight_norm), sdf_scale=float(cfg.sdf_scale), col_mode=_MODE[cfg.col_mode],
                     col_d_feature=cfg.col_d_feature, col_d_hidden=cfg.col_d_hidden, col_n_layers=cfg.col_n_layers,
                     col_multires_view=cfg.col_multires_view, col_weight_norm=int(cfg.col_weight_norm),
                     col_squeeze_out=int(cfg.col_squeeze_out), rel_d_hidden=cfg.rel_d_hidden, rel_n_layers=cfg.rel_n_layers,
                     rel_y_in_layer=cfg.rel_y_in_layer, rel_multires_view=cfg.rel_multires_view,
                     rel_include_grad=int(cfg.rel_include_grad), rel_inv_sigmoid=int(cfg.rel_inv_sigmoid))


_int, _i32, _i64, _f32, _size = C.c_int, C.c_int32, C.c_int64, C.c_float, C.c_size_t
_PP = C.POINTER(_FP)              # const float* const* params / float* const* d_params
_F3 = C.POINTER(C.c_float)        # host float[3] bounds
_cfg, _ncfg, _lcfg = C.POINTER(CnrConfig), C.POINTER(CnrNerfConfig), C.POINTER(CnrLossConfig)
_in, _out, _gout = C.POINTER(CnrInputs), C.POINTER(CnrOutputs), C.POINTER(CnrOutGrads)
_bgin = C.POINTER(CnrBgCompositeIn)
_info = [_int, C.c_char_p, _int, C.POINTER(_int), C.POINTER(_int)]   # index, name, name_len, rows, cols

# Every export of include/colorneus_render.h, in the header's order: name -> (restype, argtypes).  tests/test_binding.py holds the arity of
# each entry against the header's prototype.
SIGNATURES = {
    # per-launch timing
    "cnr_timing_enable": (None, [_int]),
    "cnr_timing_collect": (_int, [C.POINTER(CnrKernelTiming), _int]),
    # loss of the training step
    "cnr_loss_scratch_bytes": (_size, [_i64]),
    "cnr_loss_sums": (_int, [_lcfg, _FP, _FP, _FP, _FP, _FP, _i64, _i32, _FP, _FP, _size, _FP]),
    "cnr_loss_sums_ray": (_int, [_lcfg, _FP, _FP, _FP, _FP, _FP, _i64, _i32, _FP, _FP, _size, _FP]),
    "cnr_loss_grads": (_int, [_lcfg, _FP, _FP, _FP, _FP, _i64, _i32, _FP, _FP, _FP, _FP, _FP]),
    "cnr_loss_combine": (_int, [_lcfg, _FP, _FP, _f32, _i32, _i32, _i32, _FP, _FP]),
    "cnr_loss_coef": (_int, [_lcfg, _FP, _FP, _f32, _i32, _i32, _i32, _FP, _FP]),
    "cnr_loss_forward": (_int, [_lcfg, _FP, _FP, _FP, _i32, _FP, _FP, _FP, _i64, _i32, _f32, _i32, _i32, _FP, _FP, _FP, _size, _FP]),
    "cnr_loss_backward": (_int, [_lcfg, _FP, _FP, _FP, _FP, _i64, _i32, _FP, _FP, _FP, _f32, _i32, _i32, _FP, _FP, _FP, _FP, _FP]),
    "cnr_loss_shard_stats": (_int, [_lcfg, _FP, _FP, _FP, _i32, _FP, _FP, _FP, _i64, _i32, _FP, _FP, _size, _FP]),
    "cnr_loss_shard_combine": (_int, [_lcfg, _FP, _f32, _i32, _i32, _i32, _FP, _FP]),
    # ray generation, on-device pixel choice, learnable cameras
    "cnr_gen_rays": (_int, [_FP, _i64, _FP, _i32, _FP, _i32, _i32, _i32, _i32, _FP, _FP, _FP, _f32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    "cnr_gen_rays_backward": (_int, [_FP, _i64, _FP, _i32, _FP, _i32, _i32, _i32, _i32, _FP, _f32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _size, _FP]),
    "cnr_pixel_table_scratch_bytes": (_size, [_i32, _i64]),
    "cnr_pixel_table_build": (_int, [_FP, _i32, _i64, _FP, _FP, _FP, _FP, _size, _FP]),
    "cnr_choose_pixels": (_int, [_FP, _i64, _i32, _FP, _FP, _i32, _i32, _i64, _FP, _FP, _FP, _i64, _FP, _FP, _FP, _FP, _FP]),
    "cnr_camera_forward": (_int, [C.POINTER(CnrCameraConfig), _FP, _FP, _FP, _FP, _FP, _FP, _i64, _FP, _FP, _FP]),
    "cnr_camera_backward": (_int, [C.POINTER(CnrCameraConfig), _FP, _FP, _FP, _FP, _FP, _FP, _i64, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    # optimiser step
    "cnr_clip_adam_scratch_bytes": (_size, [_i32, C.POINTER(_i64)]),
    "cnr_clip_adam_step": (_int, [C.POINTER(CnrAdamConfig), _i32, C.POINTER(_i64), _PP, _PP, _FP, _FP, _FP, _size, _FP]),
    # identification, parameter inventory
    "cnr_abi_version": (_int, []),
    "cnr_backend_name": (C.c_char_p, []),
    "cnr_last_error": (C.c_char_p, []),
    "cnr_param_count": (_int, [_cfg]),
    "cnr_param_info": (_int, [_cfg] + _info),
    # the render path
    "cnr_ctx_bytes": (_size, [_cfg, _i64]),
    "cnr_bwd_scratch_bytes": (_size, [_cfg, _i64]),
    "cnr_render_forward": (_int, [_cfg, _PP, _in, _out, _FP, _size, _FP]),
    "cnr_infer_scratch_bytes": (_size, [_cfg, _i64]),
    "cnr_render_forward_only": (_int, [_cfg, _PP, _in, _out, _FP, _size, _FP]),
    "cnr_sample_z": (_int, [_cfg, _PP, _in, _FP, _FP, _size, _FP]),
    "cnr_render_backward": (_int, [_cfg, _PP, _in, _out, _FP, _size, _gout, C.POINTER(CnrInGrads), _FP, _size, _FP]),
    "cnr_sample_pdf": (_int, [_FP, _FP, _i64, _i32, _i32, _FP, _FP]),
    "cnr_sample_pdf_u": (_int, [_FP, _FP, _FP, _i64, _i32, _i32, _FP, _FP]),
    "cnr_up_sample": (_int, [_FP, _FP, _FP, _FP, _i64, _i32, _i32, _f32, _FP, _FP]),
    # SDF evaluation, point queries, lattice, iso-surface
    "cnr_sdf_eval_scratch_bytes": (_size, [_cfg, _i64]),
    "cnr_sdf_eval": (_int, [_cfg, _PP, _FP, _i64, _f32, _FP, _FP, _size, _FP]),
    "cnr_sdf_query_ctx_bytes": (_size, [_cfg, _i64, _i32]),
    "cnr_sdf_query_bwd_scratch_bytes": (_size, [_cfg, _i64, _i32]),
    "cnr_sdf_query_forward": (_int, [_cfg, _PP, _FP, _i64, _i32, _FP, _FP, _FP, _FP, _size, _FP]),
    "cnr_sdf_query_backward": (_int, [_cfg, _PP, _FP, _i64, _i32, _FP, _FP, _FP, _FP, _size, _PP, _FP, _FP, _size, _FP]),
    "cnr_sdf_grid_scratch_bytes": (_size, [_cfg, _i32]),
    "cnr_sdf_grid": (_int, [_cfg, _PP, _F3, _F3, _i32, _FP, _FP, _size, _FP]),
    "cnr_sdf_grid_slab_scratch_bytes": (_size, [_cfg, _i32, _i32, _i32]),
    "cnr_sdf_grid_slab": (_int, [_cfg, _PP, _F3, _F3, _i32, _i32, _i32, _FP, _FP, _size, _FP]),
    "cnr_mc_scratch_bytes": (_size, [_i32]),
    "cnr_mc_count": (_int, [_FP, _i32, _f32, _FP, _size, _FP, _FP]),
    "cnr_mc_emit": (_int, [_FP, _i32, _f32, _F3, _F3, _FP, _size, _FP, _FP, _FP]),
    # nearest neighbours, image evaluation, vertex colours
    "cnr_nn_scratch_bytes": (_size, [_i64, _i64]),
    "cnr_nn_search": (_int, [_FP, _i64, _FP, _i64, _FP, _FP, _FP, _size, _FP]),
    "cnr_image_scratch_bytes": (_size, [_i64, _int, _int, _int]),
    "cnr_image_metrics": (_int, [_FP, _FP, _i64, _int, _int, _int, _int, _FP, _FP, _FP, _size, _FP]),
    "cnr_image_panel": (_int, [_FP, _FP, _FP, _int, _int, _FP, _FP, _FP, _size, _FP]),
    "cnr_vertex_color_scratch_bytes": (_size, [_cfg, _i64]),
    "cnr_vertex_color": (_int, [_cfg, _PP, _FP, _i64, _FP, _FP, _size, _FP]),
    # mesh rasteriser
    "cnr_mesh_raster_scratch_bytes": (_size, [_i64, _i64, _i32, _i32]),
    "cnr_mesh_raster": (_int, [_FP, _i64, _FP, _i64, _FP, _FP, _FP, _i32, _i32, _i32, _FP, _f32, _f32, _F3, _FP, _FP, _FP, _FP, _FP, _size, _FP]),
    # mesh connected components, selection, compaction
    "cnr_mesh_components": (_int, [_FP, _i64, _i64, _FP, _FP, _FP, _FP, _FP, _FP]),
    "cnr_mesh_select": (_int, [_FP, _i64, _i64, _FP, _FP, _FP, _i32, _i32, _f32, _FP, _FP, _FP, _FP, _FP, _FP]),
    "cnr_mesh_compact": (_int, [_FP, _FP, _FP, _i64, _i64, _FP, _FP, _FP, _FP, _FP, _FP]),
    # mesh surface sampling, exact point-to-mesh distance
    "cnr_mesh_area_cdf": (_int, [_FP, _i64, _FP, _i64, _FP, _FP, _FP]),
    "cnr_mesh_sample": (_int, [_FP, _i64, _FP, _i64, _FP, _i64, _i64, _FP, _FP, _FP, _FP]),
    "cnr_point_mesh_distance": (_int, [_FP, _i64, _FP, _i64, _FP, _i64, _FP, _FP, _FP, _FP, _FP]),
    # culling a mesh against the views: packed dilated masks, per-vertex votes, selection
    "cnr_mask_dilate": (_int, [_FP, _i64, _i32, _i32, _i32, _FP, _FP, _FP]),
    "cnr_mesh_view_votes": (_int, [_FP, _i64, _FP, _FP, _FP, _f32, _f32, _i32, _i64, _i32, _i32, _FP, _FP, _f32, _FP, _FP]),
    "cnr_mesh_cull_select": (_int, [_FP, _i64, _i64, _FP, _i32, _i32, _i32, _i32, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    # ICP registration to a cloud or a mesh
    "cnr_icp": (_int, [_FP, _i64, _FP, _i64, _FP, _i64, _FP, _i32, _f32, _i32, _i32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP]),
    # one plain fully-connected layer
    "cnr_linear_scratch_bytes": (_size, [_i64, _i32, _i32, _i32]),
    "cnr_linear_forward": (_int, [_FP, _i64, _i32, _FP, _FP, _i32, _i32, _FP, _FP, _size, _FP]),
    "cnr_linear_backward": (_int, [_FP, _FP, _FP, _i64, _i32, _FP, _i32, _i32, _FP, _FP, _FP, _FP, _size, _FP]),
    # N_OUTSIDE > 0: the NeRF++ background
    "cnr_nerf_param_count": (_int, [_ncfg]),
    "cnr_nerf_param_info": (_int, [_ncfg] + _info),
    "cnr_outside_z": (_int, [_FP, _FP, _FP, _i64, _i32, _i32, _i32, _FP, _FP, _FP]),
    "cnr_outside_z_backward": (_int, [_FP, _FP, _FP, _i64, _i32, _i32, _i32, _FP, _FP, _FP]),
    "cnr_background_ctx_bytes": (_size, [_ncfg, _i64, _i32]),
    "cnr_background_bwd_scratch_bytes": (_size, [_ncfg, _i64, _i32]),
    "cnr_background_forward": (_int, [_ncfg, _PP, _FP, _FP, _FP, _i64, _i32, _f32, _FP, _FP, _FP, _size, _FP]),
    "cnr_background_backward": (_int, [_ncfg, _PP, _FP, _FP, _FP, _i64, _i32, _f32, _FP, _size, _FP, _FP, _FP, _PP, _FP, _FP, _FP, _FP, _size, _FP]),
    "cnr_composite_background_scratch_bytes": (_size, [_i64]),
    "cnr_composite_background_forward": (_int, [_bgin, _out, _FP, _size, _FP]),
    "cnr_composite_background_backward": (_int, [_bgin, _out, _gout, C.POINTER(CnrBgCompositeGrads), _FP, _size, _FP]),
}
EXPORTS = list(SIGNATURES)
ABI_VERSION = 9


class RenderLibrary:
    def __init__(self, path):
        if not os.path.isfile(path):
            raise RuntimeError(
                f"Color-NeuS HIP library not found at {path}. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C color-neus_amd/csrc hip`. There is no CPU/PyTorch fallback for the render path.")
        self.path = path
        self.lib = C.CDLL(path)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(self.lib, name)      # (CDLL keeps the function object as an attribute of self.lib from here on)
            fn.restype, fn.argtypes = restype, argtypes
        if self.lib.cnr_abi_version() != ABI_VERSION:
            raise RuntimeError("colorneus library ABI mismatch")

    @property
    def backend(self) -> str:
        return self.lib.cnr_backend_name().decode()

    def check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.lib.cnr_last_error().decode()}")

    def call(self, name, *args):
        """Call the status-returning entry point ``name``; a non-zero status raises with that name and cnr_last_error()."""
        if getattr(self.lib, name)(*args) != 0:
            raise RuntimeError(f"{name} failed: {self.lib.cnr_last_error().decode()}")

    def scratch(self, bytes_fn, device, *args, at_least=0, zero=False, nbytes=None):
        """(uninitialised uint8 tensor on ``device``, nbytes) for the size function ``bytes_fn(*args)``; the tensor holds at least
        ``at_least`` bytes (a valid pointer where the size can be 0), nbytes is what the size function said.  ``nbytes``: the byte count
        itself, for an entry point whose scratch size the header states as a formula (``bytes_fn`` then names that entry point).
        ``zero``: the buffer comes zero-filled (the loss scratch's contract: zero before the first use, left zero by every call).
        Every context / scratch buffer of the package is allocated here (tests/_guard.py substitutes this one method)."""
        nb = getattr(self.lib, bytes_fn)(*args) if nbytes is None else int(nbytes)
        alloc = torch.zeros if zero else torch.empty
        return alloc(max(nb, at_least), dtype=torch.uint8, device=device), nb

    def timing_enable(self, on: bool):
        self.lib.cnr_timing_enable(1 if on else 0)

    def timing_collect(self, max_records=65536):
        """Per-launch records [(name, kind, nt, P, N, K, pairs, ms, bytes)] since the last collect (synchronises the events)."""
        buf = (CnrKernelTiming * max_records)()
        n = self.lib.cnr_timing_collect(buf, max_records)
        return [(buf[i].name.decode(), buf[i].kind, buf[i].nt, buf[i].P, buf[i].N, buf[i].K, buf[i].pairs, buf[i].ms, buf[i].bytes)
                for i in range(min(n, max_records))]

    def param_inventory(self, ccfg, count="cnr_param_count", info="cnr_param_info"):
        """[(name, rows, cols)] of a configuration in the library's canonical order; ``count`` / ``info`` name the pair of entry points
        (the renderer's by default, cnr_nerf_param_* for the background network's CnrNerfConfig)."""
        n = getattr(self.lib, count)(C.byref(ccfg))
        if n < 0:
            raise RuntimeError(f"unsupported renderer configuration: {self.lib.cnr_last_error().decode()}")
        out = []
        buf = C.create_string_buffer(128)
        r, c = C.c_int(), C.c_int()
        for i in range(n):
            self.call(info, C.byref(ccfg), i, buf, 128, C.byref(r), C.byref(c))
            out.append((buf.value.decode(), r.value, c.value))
        return out


def ptr(t):
    """Device (or host) address of a tensor for a pointer argument; None gives NULL."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream_of(x):
    """The current stream of a tensor's device, or of a torch.device, as the ABI's stream argument (NULL on the CPU)."""
    dev = x if isinstance(x, torch.device) else x.device
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else C.c_void_p(0)


def points3(x, name, dev=None, rows=None):
    """``x`` (a tensor, or anything numpy reads as an array) of shape (N, 3) and any float dtype and strides as a detached contiguous float32
    tensor on ``dev`` (its own device when None); ``rows``: the N it must have.  Anything else raises ValueError under ``name``."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point (N, 3) tensor, got {tuple(x.shape)} {x.dtype}")
    if rows is not None and x.shape[0] != rows:
        raise ValueError(f"{name}: expected {rows} rows, got {x.shape[0]}")
    return x.detach().to(device=dev, dtype=torch.float32).contiguous()


def dense_f32(t, *shape):
    """``t`` as the detached contiguous float32 tensor the library reads, reshaped to ``shape`` when one is given; None stays None.  For a
    contiguous float32 tensor that is the same storage and no launch.  It does not move ``t``: a ``.to(device)`` stays with the caller."""
    if t is None:
        return None
    t = t.detach()
    return (t.reshape(*shape) if shape else t).contiguous().float()


def grad_f32(g):
    """A backward pass's incoming gradient as a contiguous float32 tensor (dense_f32 without the detach); None (unused output) stays None."""
    return g.contiguous().float() if g is not None else None


def save_named(ctx, tail=(), **tensors):
    """ctx.save_for_backward of the named tensors that are not None, then of the list ``tail`` (the parameters).  Which names are present
    is recorded on ``ctx``, so that an absent tensor needs no placeholder and a real zero-element tensor is not taken for one.  Everything
    goes through save_for_backward: a tensor held in a plain ctx attribute would form an uncollectable tensor -> grad_fn -> ctx -> tensor
    cycle."""
    ctx.saved_names = tuple(tensors)
    ctx.saved_present = tuple(t is not None for t in tensors.values())
    ctx.save_for_backward(*[t for t in tensors.values() if t is not None], *tail)


def saved_named(ctx):
    """What save_named saved: ({name: tensor, or None for an absent one}, tail list)."""
    it = iter(ctx.saved_tensors)
    named = {k: (next(it) if here else None) for k, here in zip(ctx.saved_names, ctx.saved_present)}
    return named, list(it)


def param_array(tensors, n=None):
    """The addresses of ``tensors`` as a ``void*[n]`` (n: len(tensors) unless given); a None entry and every slot past the list are NULL."""
    return (C.c_void_p * (len(tensors) if n is None else n))(*[t.data_ptr() if t is not None else None for t in tensors])


def flat_grads(plist, device, n=None):
    """Gradients of the parameters ``plist`` as views into ONE flat float32 buffer (in this order): a ray-sharded run all-reduces it as is
    and the fused optimiser step (optim.ClipAdam, optim.flat_view_of_grads) streams it -- no torch.cat, no copy back.  Returns
    (flat, views, param_array(views, n)).

    A backward pass must hand the views over WITHOUT keeping a second reference (``del views, flat`` before it returns): autograd then
    installs them as p.grad as they are (it clones a gradient that something else still references), so p.grad aliases the flat buffer."""
    sizes = [p.numel() for p in plist]
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=device)
    views, off = [], 0
    for p, size in zip(plist, sizes):
        views.append(flat[off:off + size].view(p.shape))
        off += size
    return flat, views, param_array(views, n)


def float3(v):
    """A host ``float[3]`` (bound_min / bound_max arguments)."""
    return (C.c_float * 3)(*[float(x) for x in v])


def ordered_names(inventory, named, exempt_prefix=None):
    """The names of a library inventory [(name, rows, cols)] in its order, checked against a module's ``dict(named_parameters())``: every
    entry exists with rows * cols elements, and the module has no parameter beyond them other than those under ``exempt_prefix``."""
    order = []
    for name, rows, cols in inventory:
        if name not in named:
            raise RuntimeError(f"library expects parameter {name!r} which this module does not have")
        if named[name].numel() != rows * cols:
            raise RuntimeError(f"parameter {name}: expected {rows}x{cols}, have {tuple(named[name].shape)}")
        order.append(name)
    extra = [k for k in named if k not in order and not (exempt_prefix and k.startswith(exempt_prefix))]
    if extra:
        raise RuntimeError(f"parameter inventory mismatch between module and library: {extra[:3]}")
    return order


def resolve_library(library=None):
    """``library`` as a RenderLibrary: the object itself, the build at a path, or (None) the HIP library next to this file."""
    return library if isinstance(library, RenderLibrary) else load_library(library)


def library_for(library, dev, what):
    """The library that serves tensors on ``dev``: CUDA tensors use the HIP library, CPU tensors only an explicitly passed CPU-emulation
    ``library=``.  There is no CPU fallback: a mismatch raises.  ``what`` words the message ("points ... searched", "images ... evaluated")."""
    lib = resolve_library(library)
    if lib.backend.startswith("hip") != (dev.type == "cuda"):
        raise RuntimeError(f"{what[0]} on '{dev}' cannot be {what[1]} by the '{lib.backend}' library: CUDA tensors use the HIP library, CPU tensors "
                           "need an explicitly passed CPU-emulation library= (there is no CPU fallback)")
    return lib


def library_path() -> str:
    return os.path.join(_HERE, "libcolorneus_hip.so")


_cached = {}


def load_library(path=None) -> RenderLibrary:
    """Load the HIP library (default) or an explicitly given build (tests pass the CPU-emulation build explicitly)."""
    path = os.path.abspath(path or library_path())
    if path not in _cached:
        _cached[path] = RenderLibrary(path)
    return _cached[path]
