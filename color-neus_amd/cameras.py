"""Learnable cameras on the device library: the reference's ``Focal_Net`` and ``Pose_Net`` (lib/models/tools/camera_net.py:8-109), the two
calls every training step starts with (``focal = self.focal_net()``, ``c2w = self.pose_net(img_ids)``, NeuS_Trainer.py:183-184).

``FocalNet`` and ``PoseNet`` keep the reference's constructor arguments, parameter names, shapes, initial values and ``requires_grad`` flags,
so that the ``focal_net.*`` / ``pose_net.*`` entries of a reference trainer checkpoint load into ``Cameras`` with ``strict=True``.  The
arithmetic is one kernel forward (``cnr_camera_forward``) and one backward (``cnr_camera_backward``, include/colorneus_render.h) behind ONE
``autograd.Function`` for both outputs; the outputs feed ``rays.rays_for_training / get_rays_multicam / get_rays_at`` unchanged.

Parameters on ``cuda`` use the HIP library; CPU parameters need an explicitly passed CPU-emulation ``library=``; there is no torch fallback.

Rotations.  ``pose_mode="6d"`` is pytorch3d's ``rotation_6d_to_matrix`` (Zhou et al. 2019): ``b1 = a1 / max(|a1|, 1e-12)``,
``b2 = normalize(a2 - (b1 . a2) b1)``, ``b3 = b1 x b2``, the ROWS of R.  ``"3d"`` is the axis-angle exponential map (pytorch3d's
``axis_angle_to_matrix``), evaluated with its series below ``|r| = 1e-2`` so that value and gradient are right at ``r = 0``, the initial
value.  pytorch3d is not a dependency of this package: both equivalences are stated from its documentation and not checked by the tests
(which pin the formulas against a float64 restatement and scipy's ``Rotation.from_rotvec``).

One difference from the reference: ``focal`` is always the flat ``[2]`` (with one-entry ``(1,)`` parameters the reference returns ``[2, 1]``;
the ray functions flatten it anyway)."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import dense_f32, ptr, save_named, saved_named, stream_of

__all__ = ["FocalNet", "PoseNet", "Cameras", "cameras_from_state_dict"]

_POSE_MODE = {"3d": 0, "6d": 1}


def _library(library, dev):
    return _lib.library_for(library, dev, ("camera parameters", "evaluated"))


class _CameraFunction(torch.autograd.Function):
    """autograd edge around cnr_camera_forward / cnr_camera_backward: (c2w [B,4,4], focal [2]) from (r, t, fx, fy); the pose part is left out
    when ``r`` is None, the focal part when ``fx`` is None (the unused output is an empty tensor)."""

    @staticmethod
    def forward(ctx, lib, meta, ids, r, t, init_c2w, fx, fy):
        num_cams, pose_mode, order, fx_only, H, W = meta
        dev = (r if r is not None else fx).device
        f32 = dict(dtype=torch.float32, device=dev)
        rc, tc = dense_f32(r), dense_f32(t if r is not None else None)
        ic = dense_f32(init_c2w if r is not None else None)
        fxc = dense_f32(fx, -1)
        fyc = dense_f32(fy if fx is not None else None, -1)
        B = (ids.shape[0] if ids is not None else num_cams) if r is not None else 0
        c2w = torch.empty(B, 4, 4, **f32) if r is not None else None
        focal = torch.empty(2, **f32) if fx is not None else None
        cfg = _lib.CnrCameraConfig(num_cams=num_cams, pose_mode=pose_mode, focal_order=order, fx_only=int(fx_only), H=H, W=W,
                                   has_init_c2w=int(ic is not None))
        if B > 0 or focal is not None:
            pose = B > 0
            lib.call("cnr_camera_forward", C.byref(cfg), ptr(rc if pose else None), ptr(tc if pose else None), ptr(ic if pose else None),
                     ptr(fxc), ptr(fyc), ptr(ids if pose else None), B, ptr(c2w if pose else None), ptr(focal), stream_of(dev))
        ctx.lib, ctx.cfg, ctx.B = lib, cfg, B
        ctx.shapes = (fx.shape if fx is not None else None, fy.shape if fy is not None else None)
        save_named(ctx, ids=ids, r=rc, t=tc, init_c2w=ic, fx=fxc, fy=fyc)
        ctx.set_materialize_grads(False)
        return (c2w if c2w is not None else torch.empty(0, 4, 4, **f32)), (focal if focal is not None else torch.empty(0, **f32))

    @staticmethod
    def backward(ctx, d_c2w, d_focal):
        sv, _ = saved_named(ctx)
        ids, rc, tc, ic, fxc, fyc = (sv[k] for k in ("ids", "r", "t", "init_c2w", "fx", "fy"))
        need_r, need_t, need_fx, need_fy = (ctx.needs_input_grad[i] for i in (3, 4, 6, 7))
        B = ctx.B
        pose = (need_r or need_t) and B > 0 and d_c2w is not None
        focal = (need_fx or need_fy) and fxc is not None and d_focal is not None
        if not (pose or focal):
            return (None,) * 8
        dev = (rc if rc is not None else fxc).device
        f32 = dict(dtype=torch.float32, device=dev)
        d_r = torch.empty_like(rc) if pose and need_r else None
        d_t = torch.empty_like(tc) if pose and need_t else None
        d_fx = torch.empty(1, **f32) if focal and need_fx else None
        d_fy = torch.empty(1, **f32) if focal and need_fy and fyc is not None else None
        if focal and d_fx is None and d_fy is None:
            focal = False
        if pose or focal:
            g_c = dense_f32(d_c2w) if pose else None
            g_f = dense_f32(d_focal) if focal else None
            ctx.lib.call("cnr_camera_backward", C.byref(ctx.cfg), ptr(rc if pose else None), ptr(tc if pose else None),
                         ptr(ic if pose else None), ptr(fxc if focal else None), ptr(fyc if focal else None), ptr(ids if pose else None), B,
                         ptr(g_c), ptr(g_f), ptr(d_r), ptr(d_t), ptr(d_fx), ptr(d_fy), stream_of(dev))
        sx, sy = ctx.shapes
        return (None, None, None, d_r, d_t, None, d_fx.reshape(sx) if d_fx is not None else None, d_fy.reshape(sy) if d_fy is not None else None)


def _camera_ids(cam_ids, num_cams, dev, check_ids):
    """int64 ids on ``dev`` (None: all cameras in order).  Host-side ids (a Python sequence or a CPU tensor, what ``batch['img_ids']`` is) are
    range-checked like torch indexing (IndexError outside [-num_cams, num_cams); negative ids count from the end); a device tensor is not read
    back."""
    if cam_ids is None:
        return None
    host = not torch.is_tensor(cam_ids) or cam_ids.device.type == "cpu"
    ids = torch.as_tensor(cam_ids).reshape(-1)
    if ids.is_floating_point() or ids.dtype == torch.bool:
        raise IndexError(f"camera ids must be integers, got {ids.dtype}")
    ids = ids.to(torch.int64)
    if (host if check_ids is None else check_ids) and ids.numel() > 0:
        lo, hi = int(ids.min()), int(ids.max())
        if lo < -num_cams or hi >= num_cams:
            raise IndexError(f"camera id range [{lo}, {hi}] is out of bounds for {num_cams} cameras")
        ids = torch.where(ids < 0, ids + num_cams, ids)
    return ids.to(dev).contiguous()


def _apply(library, focal_net, pose_net, cam_ids, check_ids=None):
    """The one entry to the autograd function: (c2w or None, focal or None) for the modules given."""
    ref = pose_net.r if pose_net is not None else focal_net.fx
    lib = _library(library, ref.device)
    ids = r = t = init = fx = fy = None
    num_cams = pose_mode = 0
    order, fx_only, H, W = 2, False, 1, 1
    if pose_net is not None:
        num_cams, pose_mode = pose_net.num_cams, _POSE_MODE[pose_net.pose_mode]
        ids = _camera_ids(cam_ids, num_cams, ref.device, check_ids)
        r, t, init = pose_net.r, pose_net.t, pose_net.init_c2w
    if focal_net is not None:
        order, fx_only, H, W = focal_net.order, focal_net.fx_only, focal_net.H, focal_net.W
        fx, fy = focal_net.fx, (None if fx_only else focal_net.fy)
        if fx.device != ref.device:
            raise ValueError(f"focal_net is on {fx.device} but pose_net is on {ref.device}")
    c2w, focal = _CameraFunction.apply(lib, (num_cams, pose_mode, order, fx_only, H, W), ids, r, t, init, fx, fy)
    return (c2w if pose_net is not None else None), (focal if focal_net is not None else None)


def _focal_init(init_focal, size, order):
    """sqrt(init_focal / size) (order 2) or init_focal / size (order 1), numpy arithmetic in init_focal's dtype, then float32."""
    a = np.asarray(init_focal)
    if not np.issubdtype(a.dtype, np.floating):
        a = a.astype(np.float64)
    q = a / np.asarray(size, dtype=a.dtype)
    return torch.from_numpy(np.asarray(np.sqrt(q) if order == 2 else q)).float().clone()


class FocalNet(nn.Module):
    """``Focal_Net`` (camera_net.py:8-66): ``focal_net()`` -> ``[2]`` = ``(fx*fx*W, fy*fy*H)`` (order 2) or ``(fx*W, fy*H)`` (order 1); with
    ``fx_only`` there is no ``fy`` and both entries are the first.  ``req_grad`` sets ``requires_grad`` of the parameters.

    ``init_focal``: None (parameters 1.0, 0-dim); a 0-dim or ONE-entry array (what the datasets pass with FX_ONLY; the parameters take its
    shape, ``()`` or ``(1,)``); or, only with ``fx_only=False`` and ``order=2``, a TWO-entry array ``(focal_x, focal_y)`` (0-dim parameters).
    A two-entry array with ``fx_only=True`` or ``order=1`` makes two-element parameters and a ``[2, 2]`` focal in the reference, which no
    caller can use: ValueError here.  The output is always the flat ``[2]`` (the reference returns ``[2, 1]`` for ``(1,)`` parameters)."""

    def __init__(self, H, W, req_grad, fx_only, order=2, init_focal=None, library=None):
        super().__init__()
        if order not in (1, 2):
            raise ValueError(f"focal order must be 1 or 2, got {order}")
        self.H, self.W, self.fx_only, self.order, self.library = int(H), int(W), bool(fx_only), int(order), library
        if init_focal is None:
            cx, cy = torch.tensor(1.0, dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32)
        else:
            a = np.asarray(init_focal)
            if a.ndim > 1 or a.size not in (1, 2):
                raise ValueError(f"init_focal: expected one or two entries, got shape {a.shape}")
            if a.size == 2:
                if self.fx_only or self.order != 2:
                    raise ValueError("a two-entry init_focal needs fx_only=False and order=2 (the reference builds two-element parameters and a "
                                     "[2, 2] focal from it otherwise, which nothing can use)")
                cx, cy = _focal_init(a[0], self.W, 2), _focal_init(a[1], self.H, 2)
            else:
                cx, cy = _focal_init(a, self.W, self.order), _focal_init(a, self.H, self.order)
        self.fx = nn.Parameter(cx, requires_grad=bool(req_grad))
        if not self.fx_only:
            self.fy = nn.Parameter(cy, requires_grad=bool(req_grad))

    def forward(self, i=None):   # (the reference's unused argument)
        return _apply(self.library, self, None, None)[1]


class PoseNet(nn.Module):
    """``Pose_Net`` (camera_net.py:70-109): ``pose_net(cam_ids)`` -> ``c2w [B, 4, 4]`` = ``[[R(r[cam]), t[cam]], [0 0 0 1]] @ init_c2w[cam]``
    (without the product when ``init_c2w`` is None).  ``r`` is ``[num_cams, 6]`` initialised to ``[1,0,0,0,1,0]`` (``pose_mode="6d"``) or
    ``[num_cams, 3]`` zeros (``"3d"``, axis-angle), ``t`` is ``[num_cams, 3]`` zeros; ``init_c2w [num_cams, 4, 4]`` is a frozen parameter
    (it is in the ``state_dict``).

    ``cam_ids``: duplicates allowed, any order; None: all cameras in order.  A Python sequence or CPU tensor is range-checked here
    (IndexError, like torch indexing); a device tensor is not read back: an out-of-range slot gets a NaN ``c2w`` and contributes nothing to the
    backward pass.  ``check_ids`` overrides that choice (True: check, reading a device tensor back; False: never).
    Gradients of ``r`` / ``t`` are dense: rows of cameras not in ``cam_ids`` are exactly 0, duplicates add up in slot order (bitwise reproducible)."""

    def __init__(self, num_cams, learn_R, learn_t, pose_mode="3d", init_c2w=None, library=None):
        super().__init__()
        if pose_mode not in _POSE_MODE:
            raise ValueError(f"pose mode must be one of 3d or 6d, but got {pose_mode}")
        self.num_cams, self.pose_mode, self.library = int(num_cams), pose_mode, library
        self.init_c2w = None
        if init_c2w is not None:
            init_c2w = torch.as_tensor(init_c2w)
            if tuple(init_c2w.shape) != (self.num_cams, 4, 4):
                raise ValueError(f"init_c2w: expected ({self.num_cams}, 4, 4), got {tuple(init_c2w.shape)}")
            self.init_c2w = nn.Parameter(init_c2w, requires_grad=False)
        if pose_mode == "3d":
            r0 = torch.zeros(self.num_cams, 3, dtype=torch.float32)
        else:
            r0 = torch.tensor([[1, 0, 0, 0, 1, 0]], dtype=torch.float32).repeat(self.num_cams, 1)
        self.r = nn.Parameter(r0, requires_grad=bool(learn_R))
        self.t = nn.Parameter(torch.zeros(self.num_cams, 3, dtype=torch.float32), requires_grad=bool(learn_t))

    def forward(self, cam_ids=None, check_ids=None):
        return _apply(self.library, None, self, cam_ids, check_ids)[0]


class Cameras(nn.Module):
    """``focal_net`` and ``pose_net`` under the attribute names of the reference trainer, so that ``state_dict()`` holds exactly the camera
    keys of a trainer checkpoint.  ``cameras(cam_ids) -> (c2w [B, 4, 4], focal [2])``: one launch forward, one backward, for both outputs."""

    def __init__(self, focal_net, pose_net, library=None):
        super().__init__()
        self.focal_net, self.pose_net = focal_net, pose_net
        self.library = library if library is not None else (pose_net.library if pose_net.library is not None else focal_net.library)

    def forward(self, cam_ids=None, check_ids=None):
        return _apply(self.library, self.focal_net, self.pose_net, cam_ids, check_ids)


def cameras_from_state_dict(sd, H, W, focal_order=2, library=None):
    """A ``Cameras`` from the ``focal_net.*`` / ``pose_net.*`` entries of a reference trainer ``state_dict`` (other keys are ignored):
    ``num_cams`` and ``pose_mode`` from the shape of ``pose_net.r``, ``fx_only`` from the absence of ``focal_net.fy``, ``init_c2w`` from its
    presence; the focal parameters keep the shapes they are stored with (``()`` or ``(1,)``).  All parameters come out frozen
    (``requires_grad`` is not part of a state_dict): set it on those to be refined."""
    cam = {k: v for k, v in sd.items() if k.startswith(("focal_net.", "pose_net."))}
    for k in ("focal_net.fx", "pose_net.r", "pose_net.t"):
        if k not in cam:
            raise KeyError(f"{k} is not in the state_dict")
    r = cam["pose_net.r"]
    if r.dim() != 2 or r.shape[1] not in (3, 6):
        raise ValueError(f"pose_net.r: expected [num_cams, 3 or 6], got {tuple(r.shape)}")
    fx_only = "focal_net.fy" not in cam
    focal_net = FocalNet(H, W, False, fx_only, order=focal_order, library=library)
    for name in ("fx",) if fx_only else ("fx", "fy"):
        v = cam["focal_net." + name]
        if v.numel() != 1:
            raise ValueError(f"focal_net.{name}: expected one entry, got shape {tuple(v.shape)}")
        setattr(focal_net, name, nn.Parameter(torch.empty(v.shape, dtype=torch.float32), requires_grad=False))
    init = cam.get("pose_net.init_c2w")
    pose_net = PoseNet(r.shape[0], False, False, pose_mode="6d" if r.shape[1] == 6 else "3d",
                       init_c2w=torch.empty_like(init) if init is not None else None, library=library)
    cams = Cameras(focal_net, pose_net, library=library)
    cams.load_state_dict(cam, strict=True)
    return cams
