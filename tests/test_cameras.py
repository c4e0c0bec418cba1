"""Learnable cameras (color_neus_amd.cameras: FocalNet / PoseNet / Cameras on cnr_camera_forward / cnr_camera_backward).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The yardsticks are written here in
plain torch and use nothing from the library:

  F64     the specification (include/colorneus_render.h) in float64 with autograd, on the float32 inputs: focal table, 6d Gram-Schmidt rows,
          the exponential map with its series below theta^2 = 1e-4 (branching on theta^2 BEFORE the square root, so that it is differentiable
          at r = 0), [[R, t], [0 0 0 1]] @ init_c2w.  The same code run in float32 gives the yardstick's own float32-to-float64 distance.
  scipy   Rotation.from_rotvec for the 3d matrices: an exponential map that is not ours.
  golden  tests/golden/cameras.npz: the reference's Focal_Net / Pose_Net run in float32 and float64 (tools/gen_camera_golden.py; the two
          pytorch3d functions were stand-ins there, so the golden pins everything AROUND the rotation formula, F64 pins the formula).

Error measure: largest absolute error of a tensor over its largest absolute entry, every entry counts.  Tolerance per tensor:
min(1e-5, max(1e-6, 4 x the yardstick's own float32-to-float64 distance on that tensor)); the reference's own float32 run is 1.5e-7 (c2w),
2.4e-7 (d r), 4e-8 (d t) from its float64 run on the input family used here, so 1e-6 is about 4x its worst error."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _golden as G
import _native as N
import color_neus_amd as cn
from color_neus_amd import _lib, cameras as cams_mod, rays as raygen
from oracle import colorneus_oracle as O

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
SERIES_THETA2 = 1e-4


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _golden():
    return G.load("cameras")


# ---------------------------------------------------------------------------------------------------------------------------------------
# F64: the specification in plain torch (dtype follows the inputs)
# ---------------------------------------------------------------------------------------------------------------------------------------
def _normalize(x, eps=1e-12):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(eps)


def _rot6d(r):
    a1, a2 = r[..., :3], r[..., 3:]
    b1 = _normalize(a1)
    b2 = _normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
    b3 = torch.cross(b1, b2, dim=-1)
    return torch.stack((b1, b2, b3), dim=-2)


def _hat(r):
    z = torch.zeros_like(r[..., 0])
    return torch.stack([z, -r[..., 2], r[..., 1], r[..., 2], z, -r[..., 0], -r[..., 1], r[..., 0], z], -1).reshape(r.shape[:-1] + (3, 3))


def _expmap(r, half_angle=True):
    x = (r * r).sum(-1)
    small = x < SERIES_THETA2
    xs = torch.where(small, torch.ones_like(x), x)
    th = xs.sqrt()
    A = torch.where(small, 1 - x / 6, torch.sin(th) / th)
    B = torch.where(small, 0.5 - x / 24, (2 * torch.sin(th / 2) ** 2 if half_angle else 1 - torch.cos(th)) / xs)
    K = _hat(r)
    return torch.eye(3, dtype=r.dtype).expand(K.shape) + A[..., None, None] * K + B[..., None, None] * (K @ K)


def f64_c2w(r, t, init, ids, mode):
    R = _rot6d(r[ids]) if mode == "6d" else _expmap(r[ids])
    M = torch.cat([R, t[ids].unsqueeze(-1)], dim=-1)
    last = torch.tensor([0, 0, 0, 1], dtype=r.dtype).expand(M.shape[0], 1, 4)
    M = torch.cat([M, last], dim=1)
    return M @ init[ids] if init is not None else M


def f64_focal(fx, fy, H, W, order, fx_only):
    fx, fy = fx.reshape(()), (fx if fx_only else fy).reshape(())
    sy = W if fx_only else H
    return torch.stack([fx * fx * W, fy * fy * sy]) if order == 2 else torch.stack([fx * W, fy * sy])


def _err(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double(), torch.as_tensor(ref).detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def _tol(ref32, ref64):
    return min(1e-5, max(1e-6, 4.0 * _err(ref32, ref64)))


def _check(name, got, ref32, ref64, tol=None):
    e, lim = _err(got, ref64), (_tol(ref32, ref64) if tol is None else tol)
    print(f"{name}: error {e:.2e}, yardstick float32 {_err(ref32, ref64):.2e}, tolerance {lim:.2e}")
    assert e <= lim, (name, e, lim)


def _yardstick(r, t, init, ids, mode, probe, dtype):
    """(c2w, d r, d t) of sum(c2w * probe) by autograd in ``dtype`` on the float32 inputs."""
    r_, t_ = r.detach().clone().to(dtype).requires_grad_(True), t.detach().clone().to(dtype).requires_grad_(True)
    c2w = f64_c2w(r_, t_, init.to(dtype) if init is not None else None, ids, mode)
    (c2w * probe.to(dtype)).sum().backward()
    return c2w.detach(), r_.grad, t_.grad


def _pose_inputs(seed, mode, n_cams=49, n_ids=8, with_init=True):
    """The input family of the value / gradient gate: r near the identity (6d: |a1| and |b2'| away from 0), moderate rotations (3d), small
    translations, init_c2w = random rotations with translations of a few units; ids drawn with replacement."""
    from scipy.spatial.transform import Rotation
    g = torch.Generator().manual_seed(seed)
    if mode == "6d":
        r = torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(n_cams, 1) + 0.2 * torch.randn(n_cams, 6, generator=g)
    else:
        r = 0.3 * torch.randn(n_cams, 3, generator=g)
    t = 0.1 * torch.randn(n_cams, 3, generator=g)
    init = None
    if with_init:
        init = torch.eye(4).repeat(n_cams, 1, 1)
        init[:, :3, :3] = torch.from_numpy(Rotation.random(n_cams, random_state=seed).as_matrix()).float()
        init[:, :3, 3] = 3 * torch.randn(n_cams, 3, generator=g)
    ids = torch.randint(0, n_cams, (n_ids,), generator=g)
    probe = torch.randn(n_ids, 4, 4, generator=g)
    return r, t, init, ids, probe


def _pose_net(lib, dev, mode, r, t, init, learn_R=True, learn_t=True):
    net = cn.PoseNet(r.shape[0], learn_R, learn_t, pose_mode=mode, init_c2w=init.clone() if init is not None else None, library=lib)
    with torch.no_grad():
        net.r.copy_(r)
        net.t.copy_(t)
    return net.to(dev)


def _run_pose(net, ids, probe, dev, **kw):
    net.zero_grad(set_to_none=True)
    c2w = net(ids, **kw)
    (c2w * probe.to(dev)).sum().backward()
    return c2w.detach(), net.r.grad, net.t.grad


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. reference interface
# ---------------------------------------------------------------------------------------------------------------------------------------
def _focal_case_args(fx, name):
    _, o, fo, init = name.split(":")
    H, W = (int(v) for v in fx[name + ":HW"])
    return H, W, fo == "fxonly", int(o[1]), (fx[name + ":init_focal"] if init != "none" else None)


def _assert_inventory(module, fx, name):
    sd = module.state_dict()
    flags = {k: p.requires_grad for k, p in module.named_parameters()}
    assert list(sd.keys()) == list(fx[name + ":keys"]), (name, list(sd.keys()))
    assert [str(tuple(v.shape)) for v in sd.values()] == list(fx[name + ":shapes"]), name
    assert [str(v.dtype) for v in sd.values()] == list(fx[name + ":dtypes"]), name
    assert [flags[k] for k in sd] == list(fx[name + ":requires_grad"]), name


def test_reference_interface_of_the_modules():
    fx = _golden()
    assert list(fx["stand_ins"]) == ["pytorch3d.transforms.rotation_6d_to_matrix", "pytorch3d.transforms.axis_angle_to_matrix"]
    assert len(fx["focal_cases"]) == 9 and len(fx["pose_cases"]) == 4
    for name in fx["focal_cases"]:
        H, W, fx_only, order, init_focal = _focal_case_args(fx, name)
        net = cn.FocalNet(H, W, bool(fx[name + ":req_grad"]), fx_only, order=order, init_focal=init_focal)
        _assert_inventory(net, fx, name)
        for k, v in net.state_dict().items():      # initial values: the bits of the reference's numpy arithmetic
            assert np.array_equal(v.numpy().view(np.int32), fx[f"{name}:init:{k}"].view(np.int32)), (name, k)
    for name in fx["pose_cases"]:
        mode, with_init = name.split(":")[1], name.endswith(":init")
        learn_R, learn_t = (bool(v) for v in fx[name + ":learn"])
        n_cams = fx[name + ":r"].shape[0]
        net = cn.PoseNet(n_cams, learn_R, learn_t, pose_mode=mode, init_c2w=torch.from_numpy(fx[name + ":init_c2w"]) if with_init else None)
        _assert_inventory(net, fx, name)
        for k in ("r", "t"):
            assert np.array_equal(net.state_dict()[k].numpy(), fx[f"{name}:init:{k}"]), (name, k)
        # Cameras: the camera keys of a trainer checkpoint, and a state_dict assembled from the golden loads with strict=True
        fname = "focal:o2:fxonly:one" if with_init else "focal:o2:fxfy:two"
        H, W, fx_only, order, init_focal = _focal_case_args(fx, fname)
        both = cn.Cameras(cn.FocalNet(H, W, True, fx_only, order=order, init_focal=init_focal), net)
        want = ["focal_net." + k for k in fx[fname + ":keys"]] + ["pose_net." + k for k in fx[name + ":keys"]]
        assert list(both.state_dict().keys()) == want
        sd = {"focal_net." + k: torch.from_numpy(fx[f"{fname}:run:{k}"]) for k in fx[fname + ":keys"]}
        sd.update({"pose_net." + k: torch.from_numpy(fx[f"{name}:{k}"]) for k in fx[name + ":keys"]})
        both.load_state_dict(sd, strict=True)
        assert torch.equal(both.pose_net.r.detach(), torch.from_numpy(fx[name + ":r"]))
    with pytest.raises(ValueError):
        cn.PoseNet(3, True, True, pose_mode="quat")
    two = np.array([61.5, 44.75], dtype=np.float32)
    for fx_only, order in ((True, 2), (True, 1), (False, 1)):      # two-element parameters and a [2, 2] focal in the reference
        with pytest.raises(ValueError, match="two-entry"):
            cn.FocalNet(48, 64, True, fx_only, order=order, init_focal=two)
    assert cn.cameras.Cameras is cn.Cameras and cn.cameras_from_state_dict is cams_mod.cameras_from_state_dict


@pytest.mark.parametrize("backend", BACKENDS)
def test_cameras_from_state_dict_reproduces_the_golden(backend):
    """A trainer state_dict (renderer.* keys are ignored) -> Cameras -> the golden's c2w / focal; focal parameter shapes () and (1,) both."""
    lib, dev = _lib_and_dev(backend)
    fx = _golden()
    for name, fname in (("pose:6d:init", "focal:o2:fxonly:one"), ("pose:3d:noinit", "focal:o2:fxfy:two"), ("pose:6d:noinit", "focal:o1:fxfy:one"),
                        ("pose:3d:init", "focal:o1:fxonly:none")):
        H, W, fx_only, order, _ = _focal_case_args(fx, fname)
        sd = {"focal_net." + k: torch.from_numpy(fx[f"{fname}:run:{k}"]) for k in fx[fname + ":keys"]}
        sd.update({"pose_net." + k: torch.from_numpy(fx[f"{name}:{k}"]) for k in fx[name + ":keys"]})
        sd["renderer.deviation_network.variance"] = torch.tensor([0.3])
        cams = cn.cameras_from_state_dict(sd, H, W, focal_order=order, library=lib).to(dev)
        assert cams.pose_net.pose_mode == name.split(":")[1] and cams.focal_net.fx_only == fx_only and cams.pose_net.num_cams == 12
        assert (cams.pose_net.init_c2w is not None) == name.endswith(":init")
        assert [tuple(p.shape) for p in cams.focal_net.parameters()] == [tuple(fx[f"{fname}:run:{k}"].shape) for k in fx[fname + ":keys"]]
        assert not any(p.requires_grad for p in cams.parameters())
        c2w, focal = cams(torch.from_numpy(fx[name + ":ids"]))
        assert c2w.shape == (8, 4, 4) and focal.shape == (2,) and c2w.dtype == focal.dtype == torch.float32 and c2w.device.type == torch.device(dev).type
        assert c2w.grad_fn is None and focal.grad_fn is None
        _check(f"{name} c2w", c2w, fx[name + ":f32:c2w"], fx[name + ":f64:c2w"])
        _check(f"{fname} focal", focal, fx[fname + ":f32:focal"], fx[fname + ":f64:focal"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. values and gradients
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_values_and_gradients_against_the_golden(backend):
    lib, dev = _lib_and_dev(backend)
    fx = _golden()
    t_ = lambda k: torch.from_numpy(fx[k])
    for name in fx["pose_cases"]:
        mode, with_init = name.split(":")[1], name.endswith(":init")
        net = _pose_net(lib, dev, mode, t_(name + ":r"), t_(name + ":t"), t_(name + ":init_c2w") if with_init else None)
        c2w, d_r, d_t = _run_pose(net, t_(name + ":ids"), t_(name + ":probe"), dev)
        for k, got in (("c2w", c2w), ("d_r", d_r), ("d_t", d_t)):
            _check(f"{name} {k}", got, fx[f"{name}:f32:{k}"], fx[f"{name}:f64:{k}"])
        # F64 on the same inputs agrees with the golden's float64 run (the restatement here IS what the reference computes around the formula)
        y = _yardstick(t_(name + ":r"), t_(name + ":t"), t_(name + ":init_c2w") if with_init else None, t_(name + ":ids"), mode, t_(name + ":probe"),
                       torch.float64)
        for k, v in zip(("c2w", "d_r", "d_t"), y):
            assert _err(v, fx[f"{name}:f64:{k}"]) < 1e-12, (name, k)
    for name in fx["focal_cases"]:
        H, W, fx_only, order, init_focal = _focal_case_args(fx, name)
        net = cn.FocalNet(H, W, True, fx_only, order=order, init_focal=init_focal, library=lib)
        net.load_state_dict({k: t_(f"{name}:run:{k}") for k in fx[name + ":keys"]})
        net = net.to(dev)
        focal = net()
        assert focal.shape == (2,)
        (focal * t_(name + ":probe").to(dev)).sum().backward()
        _check(f"{name} focal", focal, fx[name + ":f32:focal"], fx[name + ":f64:focal"])
        for k, p in net.named_parameters():
            assert p.grad.shape == p.shape
            _check(f"{name} d_{k}", p.grad, fx[f"{name}:f32:d_{k}"], fx[f"{name}:f64:d_{k}"])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["6d", "3d"])
def test_values_and_gradients_against_f64_on_fresh_inputs(backend, mode):
    """49 cameras, 8 ids drawn with replacement, 5 seeds, with and without init_c2w; cameras(ids) for both outputs at once."""
    lib, dev = _lib_and_dev(backend)
    for seed in range(5):
        r, t, init, ids, probe = _pose_inputs(100 + seed, mode, with_init=seed != 3)
        g = torch.Generator().manual_seed(seed)
        fxy = 0.8 + 0.5 * torch.rand(2, generator=g)
        fprobe = torch.randn(2, generator=g)
        order, fx_only = (2, 1)[seed % 2], seed == 2
        fnet = cn.FocalNet(48, 64, True, fx_only, order=order)
        with torch.no_grad():
            fnet.fx.fill_(float(fxy[0]))
            if not fx_only:
                fnet.fy.fill_(float(fxy[1]))
        cams = cn.Cameras(fnet, _pose_net(lib, "cpu", mode, r, t, init), library=lib).to(dev)
        c2w, focal = cams(ids)
        ((c2w * probe.to(dev)).sum() + (focal * fprobe.to(dev)).sum()).backward()
        y32, y64 = (_yardstick(r, t, init, ids, mode, probe, dt) for dt in (torch.float32, torch.float64))
        for k, got, a, b in zip(("c2w", "d r", "d t"), (c2w, cams.pose_net.r.grad, cams.pose_net.t.grad), y32, y64):
            _check(f"{mode} seed {seed} {k}", got, a, b)
        f = {}
        for dt in (torch.float32, torch.float64):
            x, y = fxy[0].to(dt).requires_grad_(True), fxy[1].to(dt).requires_grad_(True)
            out = f64_focal(x, y, 48, 64, order, fx_only)
            (out * fprobe.to(dt)).sum().backward()
            f[dt] = (out.detach(), x.grad, y.grad)
        _check(f"seed {seed} focal", focal, f[torch.float32][0], f[torch.float64][0])
        _check(f"seed {seed} d fx", cams.focal_net.fx.grad, f[torch.float32][1], f[torch.float64][1])
        if not fx_only:
            _check(f"seed {seed} d fy", cams.focal_net.fy.grad, f[torch.float32][2], f[torch.float64][2])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["6d", "3d"])
def test_the_initial_state_is_the_initial_pose(backend, mode):
    """r as constructed (6d identity rows, 3d zeros), t = 0: c2w == init_c2w, gradients finite and equal to F64's."""
    lib, dev = _lib_and_dev(backend)
    _, _, init, ids, probe = _pose_inputs(7, mode)
    net = cn.PoseNet(49, True, True, pose_mode=mode, init_c2w=init.clone(), library=lib).to(dev)
    r0, t0 = net.r.detach().cpu().clone(), net.t.detach().cpu().clone()
    c2w, d_r, d_t = _run_pose(net, ids, probe, dev)
    y32, y64 = (_yardstick(r0, t0, init, ids, mode, probe, dt) for dt in (torch.float32, torch.float64))
    assert bool(torch.isfinite(d_r).all()) and bool(torch.isfinite(d_t).all()) and float(d_r.abs().max()) > 0
    _check(f"{mode} initial c2w against init_c2w", c2w, y32[0], init[ids].double())
    for k, got, a, b in zip(("c2w", "d r", "d t"), (c2w, d_r, d_t), y32, y64):
        _check(f"{mode} initial {k}", got, a, b)


def _axis_rows():
    th = np.sqrt(np.float32(SERIES_THETA2))
    lo, hi = np.nextafter(th, np.float32(0)), np.nextafter(th, np.float32(1))
    mags = [0.0, 1e-8, 1e-4, 1e-3, 1e-2, 0.05, 0.3, 1.0, 3.1, float(lo), float(hi)]
    axis = torch.tensor([1.0, 2.0, -2.0], dtype=torch.float64) / 3.0
    rows = [(axis * m).float() for m in mags]
    rows += [torch.tensor([0.0, float(m), 0.0]) for m in (lo, th, hi)]     # along a coordinate axis theta^2 is exact: both sides of the threshold
    r = torch.stack(rows)
    x = (r * r).sum(-1)
    assert bool((x < SERIES_THETA2).any()) and bool((x[-3:] < np.float32(SERIES_THETA2)).any()) and bool((x[-3:] >= np.float32(SERIES_THETA2)).any())
    return r


@pytest.mark.parametrize("backend", BACKENDS)
def test_axis_angle_from_zero_to_pi(backend):
    """3d rows along a fixed axis with |r| from 0 to 3.1 and around the series threshold: matrices against scipy, gradients against F64, both
    at a flat 1e-6 (a plain float32 torch evaluation of the half-angle form stays below 2e-7 on these rows; the 1 - cos form fails it, which
    is intended: see the last assertion)."""
    from scipy.spatial.transform import Rotation
    lib, dev = _lib_and_dev(backend)
    r = _axis_rows()
    n = r.shape[0]
    g = torch.Generator().manual_seed(11)
    probe = torch.randn(n, 4, 4, generator=g)
    net = _pose_net(lib, dev, "3d", r, torch.zeros(n, 3), None)
    c2w, d_r, _ = _run_pose(net, None, probe, dev)
    R_scipy = torch.from_numpy(Rotation.from_rotvec(r.double().numpy()).as_matrix())
    for i in range(n):      # per row: every rotation matrix has entries of size 1
        _check(f"|r| = {float(r[i].norm()):.3e} R against scipy", c2w[i, :3, :3], c2w[i, :3, :3], R_scipy[i], tol=1e-6)
    y64 = _yardstick(r, torch.zeros(n, 3), None, torch.arange(n), "3d", probe, torch.float64)
    assert _err(y64[0][:, :3, :3], R_scipy) < 1e-9      # F64 itself against scipy (series truncation at the threshold: 8e-11)
    _check("d r along the axis", d_r, d_r, y64[1], tol=1e-6)
    for i in range(n):
        _check(f"|r| = {float(r[i].norm()):.3e} d r", d_r[i], d_r[i], y64[1][i], tol=1e-6)
    # the yardstick separates the two forms: 1 - cos in float32 is outside the gate on these rows
    r32 = r.clone().requires_grad_(True)
    (_expmap(r32, half_angle=False) * probe[:, :3, :3]).sum().backward()
    assert max(_err(r32.grad[i], y64[1][i]) for i in range(n)) > 1e-6


@pytest.mark.parametrize("backend", BACKENDS)
def test_axis_angle_jacobian_at_zero_is_the_generators(backend):
    """The known answer at the initial value r = 0: dR/dr_k = [e_k]x, entry by entry."""
    lib, dev = _lib_and_dev(backend)
    net = cn.PoseNet(2, True, False, pose_mode="3d", library=lib).to(dev)
    J = torch.zeros(3, 3, 3)
    for i in range(3):
        for j in range(3):
            net.zero_grad(set_to_none=True)
            c2w = net([1])
            assert torch.equal(c2w[0].cpu(), torch.eye(4))
            c2w[0, i, j].backward()
            assert net.t.grad is None and float(net.r.grad[0].abs().max()) == 0.0
            J[i, j] = net.r.grad[1].cpu()
    want = torch.stack([_hat(e) for e in torch.eye(3)], dim=-1)      # [i, j, k] = [e_k]x[i, j]
    assert torch.equal(J, want), (J, want)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. dense, ordered, deterministic     4. bad ids
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["6d", "3d"])
def test_gradients_are_dense_ordered_and_deterministic(backend, mode):
    lib, dev = _lib_and_dev(backend)
    r, t, init, _, _ = _pose_inputs(3, mode, n_cams=9)
    g = torch.Generator().manual_seed(5)
    probe = torch.randn(4, 4, 4, generator=g)
    ids = [3, 0, 3, 6]
    net = _pose_net(lib, dev, mode, r, t, init)
    c2w, d_r, d_t = _run_pose(net, ids, probe, dev)
    d_r, d_t = d_r.clone(), d_t.clone()
    assert d_r.shape == r.shape and d_t.shape == t.shape
    rest = [c for c in range(9) if c not in ids]
    assert not d_r[rest].any() and not d_t[rest].any()      # exactly 0.0, not merely small
    assert torch.equal(c2w[0], c2w[2])
    # row 3 is the sum of its two slots (in slot order), rows 0 and 6 are their single slots
    single = {}
    for s, cam in enumerate(ids):
        _, a, b = _run_pose(net, [cam], probe[s:s + 1], dev)
        single[s] = (a[cam].clone(), b[cam].clone())
    assert torch.equal(d_r[0], single[1][0]) and torch.equal(d_r[6], single[3][0]) and torch.equal(d_t[6], single[3][1])
    assert torch.equal(d_r[3], single[0][0] + single[2][0]) and torch.equal(d_t[3], single[0][1] + single[2][1])
    y32, y64 = (_yardstick(r, t, init, torch.tensor(ids), mode, probe, dt) for dt in (torch.float32, torch.float64))
    _check("d r with duplicates", d_r, y32[1], y64[1])
    _check("d t with duplicates", d_t, y32[2], y64[2])
    # two runs are bitwise equal
    c2, a2, b2 = _run_pose(net, ids, probe, dev)
    assert torch.equal(c2, c2w) and torch.equal(a2, d_r) and torch.equal(b2, d_t)
    # ids as a tuple, a CPU tensor and a device tensor of another integer type are the same call
    for same in (tuple(ids), torch.tensor(ids), torch.tensor(ids, dtype=torch.int32).to(dev), [3, 0, -6, 6]):
        assert torch.equal(net(same), c2w)
    # cam_ids=None is arange(num_cams)
    full = torch.randn(9, 4, 4, generator=g)
    ca, ra, ta = (x.clone() for x in _run_pose(net, None, full, dev))
    cb, rb, tb = _run_pose(net, torch.arange(9), full, dev)
    assert torch.equal(ca, cb) and torch.equal(ra, rb) and torch.equal(ta, tb)


@pytest.mark.parametrize("backend", BACKENDS)
def test_frozen_parameters_get_no_gradient_and_no_launch(backend):
    lib, dev = _lib_and_dev(backend)
    L = cn.load_library(lib)
    r, t, init, ids, probe = _pose_inputs(4, "6d", n_cams=9)
    full = _run_pose(_pose_net(lib, dev, "6d", r, t, init), ids, probe, dev)
    for learn_R, learn_t in ((True, False), (False, True)):
        net = _pose_net(lib, dev, "6d", r, t, init, learn_R, learn_t)
        c2w, d_r, d_t = _run_pose(net, ids, probe, dev)
        assert (d_r is None) == (not learn_R) and (d_t is None) == (not learn_t) and net.init_c2w.grad is None
        assert torch.equal(c2w, full[0])
        assert torch.equal(d_r, full[1]) if learn_R else torch.equal(d_t, full[2])
    fnet = cn.FocalNet(48, 64, True, False)
    fnet.fy.requires_grad_(False)
    cams = cn.Cameras(fnet, _pose_net(lib, "cpu", "6d", r, t, init, False, False), library=lib).to(dev)
    c2w, focal = cams(ids)
    assert c2w.grad_fn is not None     # (one function for both outputs: only fx asks for a gradient)
    focal.sum().backward()
    assert float(cams.focal_net.fx.grad) == 2.0 * 64 and cams.focal_net.fy.grad is None and cams.pose_net.r.grad is None
    # everything frozen: no graph, hence no backward launch
    cams.focal_net.fx.requires_grad_(False)
    if dev != "cpu":
        L.timing_enable(True)
        L.timing_collect()
    c2w, focal = cams(ids)
    assert c2w.grad_fn is None and focal.grad_fn is None and not c2w.requires_grad and not focal.requires_grad
    if dev != "cpu":
        names = [rec[0] for rec in L.timing_collect()]
        L.timing_enable(False)
        assert names == ["camera_fwd"], names


@pytest.mark.parametrize("backend", BACKENDS)
def test_bad_ids(backend):
    lib, dev = _lib_and_dev(backend)
    r, t, init, _, _ = _pose_inputs(6, "6d", n_cams=9)
    net = _pose_net(lib, dev, "6d", r, t, init)
    # host-side ids (a Python sequence or a CPU tensor, what batch['img_ids'] is) raise like torch indexing
    for bad in ([0, 9], [-10, 1], torch.tensor([3, 100]), np.array([9])):
        with pytest.raises(IndexError):
            net(bad)
    with pytest.raises(IndexError):
        net([0.5])
    # ids that the host does not look at (a device tensor; the emulation library has no device, so the check is switched off by hand): an
    # out-of-range slot is NaN, the other slots and the gradients of the in-range slots are those of the same call without that slot
    g = torch.Generator().manual_seed(1)
    probe = torch.randn(5, 4, 4, generator=g)
    good = torch.tensor([2, 7, 2])
    bad = torch.tensor([2, 9, 7, -1, 2])
    kw = dict(check_ids=False) if dev == "cpu" else {}
    cg, rg, tg = (x.clone() for x in _run_pose(net, good.to(dev), probe[[0, 2, 4]], dev, **kw))
    net.zero_grad(set_to_none=True)
    cb = net(bad.to(dev), **kw)
    assert bool(torch.isnan(cb[[1, 3]]).all()) and torch.equal(cb[[0, 2, 4]].detach(), cg)
    (torch.nan_to_num(cb) * probe.to(dev)).sum().backward()      # (nan_to_num: NaN x 0 must not enter through the test's own arithmetic)
    assert bool(torch.isfinite(net.r.grad).all()) and torch.equal(net.r.grad, rg) and torch.equal(net.t.grad, tg)
    if dev != "cpu":
        with pytest.raises(IndexError):
            net(bad.to(dev), check_ids=True)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 5. ABI argument checks
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_abi_argument_checks():
    lib = cn.load_library(N.EMU_LIB)
    L = lib.lib
    assert L.cnr_abi_version() == 9
    p = lambda x: C.c_void_p(x.data_ptr())
    r, t, init = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 3), torch.zeros(3, 3), torch.eye(4).repeat(3, 1, 1)
    fx, fy, ids = torch.ones(1), torch.ones(1), torch.tensor([2, 0])
    c2w, focal, g = torch.empty(2, 4, 4), torch.empty(2), torch.ones(2, 4, 4)
    d_r, d_t, d_fx, d_fy = torch.empty(3, 6), torch.empty(3, 3), torch.empty(1), torch.empty(1)

    def cfg(**kw):
        base = dict(num_cams=3, pose_mode=1, focal_order=2, fx_only=0, H=4, W=6, has_init_c2w=1)
        base.update(kw)
        return C.byref(_lib.CnrCameraConfig(**base))

    fwd = lambda c, *a: L.cnr_camera_forward(c, *a, None)
    bwd = lambda c, *a: L.cnr_camera_backward(c, *a, None)
    assert fwd(cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)) == 0
    assert torch.equal(c2w, init[[2, 0]]) and focal.tolist() == [6.0, 4.0]
    assert fwd(cfg(fx_only=1), None, None, None, p(fx), None, None, 0, None, p(focal)) == 0 and focal.tolist() == [6.0, 6.0]      # focal part only
    assert fwd(cfg(has_init_c2w=0), p(r), p(t), None, None, None, None, 3, p(torch.empty(3, 4, 4)), None) == 0                 # pose part only
    assert bwd(cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal), p(d_r), p(d_t), p(d_fx), p(d_fy)) == 0
    assert not d_r[1].any() and d_t.tolist() == [[1.0] * 3, [0.0] * 3, [1.0] * 3]
    assert bwd(cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), None, None, p(d_t), None, None) == 0                  # skipped outputs
    bad_fwd = [((cfg(), None, p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "null"),
               ((cfg(), p(r), None, p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "null"),
               ((cfg(), p(r), p(t), p(init), None, p(fy), p(ids), 2, p(c2w), p(focal)), "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), None, p(ids), 2, p(c2w), p(focal)), "null"),
               ((None, p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, None, None), "null"),
               ((cfg(), p(r), p(t), None, p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "init_c2w"),
               ((cfg(has_init_c2w=0), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "init_c2w"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 0, p(c2w), p(focal)), "B"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), -1, p(c2w), p(focal)), "B"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), None, 2, p(c2w), p(focal)), "B"),
               ((cfg(num_cams=0), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "num_cams"),
               ((cfg(pose_mode=2), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "pose_mode"),
               ((cfg(focal_order=3), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "focal_order"),
               ((cfg(W=0), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(c2w), p(focal)), "H, W")]
    for args, msg in bad_fwd:
        assert fwd(*args) < 0
        assert msg in L.cnr_last_error().decode(), (msg, L.cnr_last_error().decode())
    tail = (p(d_r), p(d_t), p(d_fx), p(d_fy))
    bad_bwd = [((cfg(), None, p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal)) + tail, "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, None, None) + tail, "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal), None, None, p(d_fx), p(d_fy)), "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal), p(d_r), p(d_t), None, None), "null"),
               ((cfg(), p(r), p(t), p(init), p(fx), p(fy), p(ids), 0, p(g), p(focal)) + tail, "B"),
               ((cfg(num_cams=-3), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal)) + tail, "num_cams"),
               ((cfg(pose_mode=-1), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal)) + tail, "pose_mode"),
               ((cfg(focal_order=0), p(r), p(t), p(init), p(fx), p(fy), p(ids), 2, p(g), p(focal)) + tail, "focal_order")]
    for args, msg in bad_bwd:
        assert bwd(*args) < 0
        assert msg in L.cnr_last_error().decode(), (msg, L.cnr_last_error().decode())


def test_cpu_parameters_need_an_emulation_library():
    """No torch fallback: CPU parameters with the HIP library (the default) are an error."""
    if not os.path.isfile(cn.library_path()):
        pytest.skip("HIP library not built")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.PoseNet(3, True, True)([0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.FocalNet(4, 4, True, True)()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 6. end to end: Cameras -> rays_for_training -> renderer -> compute_loss_fused -> backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def _look_at(n_cams, seed, radius=2.7):
    """Cameras on a sphere around the origin looking at it: columns right / down / forward / centre (synthetic.synthetic_camera's convention)."""
    g = torch.Generator().manual_seed(seed)
    c = torch.nn.functional.normalize(torch.randn(n_cams, 3, generator=g, dtype=torch.float64), dim=-1) * radius
    fwd = -c / c.norm(dim=-1, keepdim=True)
    right = torch.nn.functional.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(fwd)), dim=-1)
    down = torch.linalg.cross(fwd, right)
    c2w = torch.eye(4, dtype=torch.float64).repeat(n_cams, 1, 1)
    c2w[:, :3, 0], c2w[:, :3, 1], c2w[:, :3, 2], c2w[:, :3, 3] = right, down, fwd, c
    return c2w.float()


def _f64_rays(c2w, focal, idx, H, W, origin, radius):
    """The ray formula of rays_for_training(normalize=True) in the dtype of c2w, differentiable (tests/test_rays.py::_torch_rays)."""
    cam = torch.div(idx, H * W, rounding_mode="floor")
    pix = idx - cam * H * W
    py, px = torch.div(pix, W, rounding_mode="floor").to(c2w.dtype), (pix % W).to(c2w.dtype)
    u = torch.stack([(px - W * 0.5) / focal[0], (py - H * 0.5) / focal[1], torch.ones_like(px)], -1)
    u = u / u.norm(dim=-1, keepdim=True)
    d = (u[:, None, :] * c2w[cam, :3, :3]).sum(-1)
    o = (c2w[cam, :3, 3] - origin.to(c2w.dtype)) / radius
    mid = -(o * d).sum(-1) / (d * d).sum(-1)
    return o, d, mid - 1.0, mid + 1.0


CAM_KEYS = ("pose_net.r", "pose_net.t", "focal_net.fx", "focal_net.fy")


def _e2e_setup(lib, dev, ocfg, H, W, n_cams=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    P = O.init_params(ocfg, seed=5, trained_like=True)
    renderer = N.make_renderer(ocfg, P, lib, dev)
    init = _look_at(n_cams, seed + 1)
    r = torch.tensor([1.0, 0, 0, 0, 1, 0]).repeat(n_cams, 1) + 0.02 * torch.randn(n_cams, 6, generator=g)
    t = 0.02 * torch.randn(n_cams, 3, generator=g)
    fnet = cn.FocalNet(H, W, True, False, order=2, init_focal=np.array([1.3 * W, 1.25 * H], dtype=np.float32))
    cams = cn.Cameras(fnet, _pose_net(lib, "cpu", "6d", r, t, init), library=lib).to(dev)
    ids = torch.tensor([3, 0, 9, 5, 1, 8, 2, 6])      # 8 of the 10 cameras, in no order: cameras 4 and 7 get zero rows
    image = torch.rand(8, H, W, 3, generator=g)
    mask = (torch.rand(8, H, W, generator=g) < 0.7).float()
    return P, renderer, cams, ids, image, mask


def _e2e_native(lib, dev, renderer, cams, ids, image, mask, R, origin, radius, seed):
    """One training-step front: returns the loss, the camera and renderer gradients, the pixel indices, z_vals, and the renderer gradients of
    the same step fed with the same ray tensors as detached leaves."""
    library = cn.load_library(lib)
    image, mask = image.to(dev), mask.to(dev)
    H, W = image.shape[1], image.shape[2]
    torch.manual_seed(seed)
    idx = raygen.choose_pixels(R, H * W, "cpu", mask.cpu(), 0.9)
    params = list(renderer.parameters()) + list(cams.parameters())

    def step(leaves, z):
        for p in params:
            p.grad = None
        c2w, focal = cams(ids)
        torch.manual_seed(seed)
        o, d, near, far, rgb, msel = raygen.rays_for_training(c2w, focal, image, R, origin, radius, normalize=True, mask=mask, return_mask=True,
                                                              library=library)
        if z is None:
            with torch.no_grad():
                torch.manual_seed(seed + 1)
                return renderer(o, d, near, far)["z_vals"].detach().clone(), None, None
        if leaves:
            o, d, near, far = (x.detach().clone().requires_grad_(True) for x in (o, d, near, far))
        out = renderer(o, d, near, far, z_vals=z)
        loss, _ = cn.compute_loss_fused(out, rgb, msel, library=library)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in cams.named_parameters() if p.grad is not None}, \
            {k: p.grad.detach().clone() for k, p in renderer.named_parameters()}

    z, _, _ = step(False, None)      # fixed z_vals from a first call: gate G2's way of taking the sampler out
    loss, gcam, gren = step(False, z)
    _, gcam_leaf, gren_leaf = step(True, z)
    assert not gcam_leaf      # (leaves: nothing reaches the cameras)
    return loss, gcam, gren, gren_leaf, idx, z, (image, mask)


def _e2e_oracle(P, ocfg, cams, ids, idx, z, image, mask, origin, radius, dtype):
    sd = {k: v.detach().cpu().to(dtype) for k, v in cams.state_dict().items()}
    leaves = {k: sd[k].clone().requires_grad_(True) for k in CAM_KEYS}
    H, W = image.shape[1], image.shape[2]
    c2w = f64_c2w(leaves["pose_net.r"], leaves["pose_net.t"], sd["pose_net.init_c2w"], ids, "6d")
    focal = f64_focal(leaves["focal_net.fx"], leaves["focal_net.fy"], H, W, 2, False)
    o, d, near, far = _f64_rays(c2w, focal, idx, H, W, origin, radius)
    Pd = {k: v.to(dtype) for k, v in P.items()}
    out = O.render(Pd, ocfg, o, d, near, far, z_vals=z.cpu().to(dtype))
    rgb = image.cpu().reshape(-1, 3)[idx].to(dtype)
    msel = mask.cpu().reshape(-1)[idx].to(dtype)
    loss, _ = O.compute_loss(out, rgb, msel)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in leaves.items()}


def _e2e(backend, ocfg, R, H, W):
    lib, dev = _lib_and_dev(backend)
    P, renderer, cams, ids, image, mask = _e2e_setup(lib, dev, ocfg, H, W)
    origin, radius = torch.tensor([0.05, -0.03, 0.02]), 1.1
    loss, gcam, gren, gren_leaf, idx, z, (image_d, mask_d) = _e2e_native(lib, dev, renderer, cams, ids, image, mask, R, origin, radius, seed=3)
    assert len(set((idx // (H * W)).tolist())) == 8      # every selected camera owns rays
    l64, g64 = _e2e_oracle(P, ocfg, cams, ids, idx, z, image, mask, origin, radius, torch.float64)
    l32, g32 = _e2e_oracle(P, ocfg, cams, ids, idx, z, image, mask, origin, radius, torch.float32)
    print(f"loss {float(loss):.8f}, oracle float64 {float(l64):.8f}, oracle float32 {float(l32):.8f}")
    assert abs(float(loss) - float(l64)) < 2e-4 * abs(float(l64))
    assert set(gcam) == set(CAM_KEYS)
    bad = []
    for k in CAM_KEYS:
        spread = _err(g32[k], g64[k])
        lim = G.scalar_tolerance(spread) if k.startswith("focal_net") else G.grad_tolerance(spread, strict=True)
        e = _err(gcam[k], g64[k])
        print(f"{k}: error {e:.2e}, float32 oracle {spread:.2e}, tolerance {lim:.2e}")
        if not e <= lim:
            bad.append((k, e, spread, lim))
    assert not bad, bad
    assert not gcam["pose_net.r"][[4, 7]].any() and not gcam["pose_net.t"][[4, 7]].any()
    # the camera path does not perturb the render path: same kernels on the same bits, only the producer of the rays differs
    assert len(gren) == len(gren_leaf) == len(P)
    for k in gren:
        assert torch.equal(gren[k], gren_leaf[k]), k


def test_end_to_end_tiny_emu():
    _e2e("emu", G.CONFIGS["tiny_sharp"](), 64, 16, 16)


@pytest.mark.gpu
def test_end_to_end_dtu_512_rays_hip():
    ocfg = O.dtu_config()
    assert len(O.init_params(ocfg, seed=5, trained_like=True)) == 53
    _e2e("hip", ocfg, 512, 64, 64)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 7. optimiser
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_clip_adam_steps_the_camera_parameters_like_clip_and_adam(backend):
    """One ClipAdam over the renderer's parameters plus the trainable camera parameters against per-tensor clip_grad_norm_ + torch.optim.Adam on
    copies fed the same gradients (the comparison of tests/test_clip_adam.py), over three real steps."""
    lib, dev = _lib_and_dev(backend)
    ocfg = G.CONFIGS["tiny_sharp"]()
    H = W = 16
    P, renderer, cams, ids, image, mask = _e2e_setup(lib, dev, ocfg, H, W)
    library = cn.load_library(lib)
    image, mask = image.to(dev), mask.to(dev)
    ours = list(renderer._ordered_params()) + [p for p in cams.parameters() if p.requires_grad]
    names = [k for k, p in cams.named_parameters() if p.requires_grad]
    assert names == ["focal_net.fx", "focal_net.fy", "pose_net.r", "pose_net.t"]
    ref = [p.detach().clone().requires_grad_(True) for p in ours]
    max_norm = 0.05
    o_our = cn.ClipAdam(ours, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=max_norm, library=library)
    o_ref = torch.optim.Adam(ref, lr=5e-4, betas=(0.9, 0.99), eps=1e-8)
    start = [p.detach().clone() for p in ours[-4:]]
    for it in range(3):
        for p in ours:
            p.grad = None
        torch.manual_seed(it)
        c2w, focal = cams(ids)
        o, d, near, far, rgb, msel = raygen.rays_for_training(c2w, focal, image, 64, torch.zeros(3), 1.0, normalize=True, mask=mask, return_mask=True,
                                                              library=library)
        loss, _ = cn.compute_loss_fused(renderer(o, d, near, far), rgb, msel, library=library)
        loss.backward()
        for p, q in zip(ours, ref):
            q.grad = p.grad.detach().clone()
            torch.nn.utils.clip_grad_norm_(q, max_norm, 2)
        with torch.no_grad():      # (the reference copies follow their own trajectory: keep the inputs of the next step identical)
            for p, q in zip(ours, ref):
                q.copy_(p)
        o_our.step()
        o_ref.step()
        for k, p, q in zip(["renderer"] * (len(ours) - 4) + names, ours, ref):
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(q.detach().abs().max())), (it, k)
    assert all(float((p.detach() - v).abs().max()) > 0 for p, v in zip(ours[-4:], start))      # r, t, fx, fy all moved
    for p, v in zip(ours[-2:], start[-2:]):      # rows of the cameras no step selected: zero gradients, zero moments, no movement
        assert torch.equal(p.detach()[[4, 7]], v[[4, 7]])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 9. GPU only
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_launch_forward_and_one_backward():
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    L = cn.load_library()
    r, t, init, ids, probe = _pose_inputs(8, "6d", n_cams=200)
    cams = cn.Cameras(cn.FocalNet(48, 64, True, False), _pose_net(None, "cpu", "6d", r, t, init)).to(dev)
    ids_d, probe_d = ids.to(dev), probe.to(dev)
    torch.cuda.synchronize()
    L.timing_enable(True)
    L.timing_collect()
    c2w, focal = cams(ids_d)
    ((c2w * probe_d).sum() + focal.sum()).backward()
    torch.cuda.synchronize()
    names = [rec[0] for rec in L.timing_collect()]
    L.timing_enable(False)
    assert names == ["camera_fwd", "camera_bwd"], names
    assert all(p.grad is not None for p in cams.parameters() if p.requires_grad)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.gpu
def test_hip_matches_the_emulation_bitwise_in_6d():
    """focal, and c2w and all gradients in 6d mode: both libraries compile the same bodies with -ffp-contract=off, and the 6d path uses only
    + - * / and sqrt, which hipcc rounds correctly by default.  (3d goes through sin / cos, whose device and host implementations differ in
    the last bit: held to the value / gradient gate only.)"""
    assert torch.cuda.is_available(), "needs a GPU"
    for seed, with_init in ((0, True), (1, False), (2, True)):
        r, t, init, ids, probe = _pose_inputs(200 + seed, "6d", with_init=with_init)
        res = []
        for lib, dev in ((N.EMU_LIB, "cpu"), (None, "cuda:0")):
            fnet = cn.FocalNet(48, 64, True, seed == 1, order=2 if seed != 2 else 1, init_focal=np.array([57.25], dtype=np.float32))
            cams = cn.Cameras(fnet, _pose_net(lib, "cpu", "6d", r, t, init), library=lib).to(dev)
            c2w, focal = cams(ids)
            ((c2w * probe.to(dev)).sum() + (focal * torch.tensor([0.3, -1.7], device=dev)).sum()).backward()
            res.append([c2w, focal] + [p.grad for p in cams.parameters() if p.requires_grad])
        assert len(res[0]) == len(res[1]) >= 5
        for a, b in zip(*res):
            assert torch.equal(_bits(a), _bits(b)), (seed, a.shape, int((_bits(a) != _bits(b)).sum()))


@pytest.mark.gpu
def test_graph_capture_and_replay_equal_the_eager_result():
    """cameras + rays + backward captured once (the pattern of tests/test_graph_step.py), replayed after an in-place change of r."""
    assert torch.cuda.is_available(), "needs a GPU"
    from color_neus_amd.graph import GraphedStep
    dev = "cuda:0"
    lib = cn.load_library()
    H = W = 32
    R = 256
    r, t, init, _, _ = _pose_inputs(9, "6d", n_cams=10)
    g = torch.Generator().manual_seed(4)
    wo, wd, wn = (torch.randn(s, generator=g).to(dev) for s in ((R, 3), (R, 3), (R,)))
    delta = (0.01 * torch.randn(10, 6, generator=g)).to(dev)
    idx_all = torch.randint(0, 8 * H * W, (R,), generator=g)

    def make():
        cams = cn.Cameras(cn.FocalNet(H, W, True, False, init_focal=np.array([40.0, 38.0], dtype=np.float32)), _pose_net(None, "cpu", "6d", r, t, _look_at(10, 2))).to(dev)
        params = [p for p in cams.parameters() if p.requires_grad]

        def fn(ids, idx):
            c2w, focal = cams(ids)
            o, d, _, _, near, far = raygen._generate(lib, idx, R, c2w, focal, H, W, True, False, origin=None, radius=1.0, want_nearfar=True)
            loss = (o * wo).sum() + (d * wd).sum() + (near * wn).sum() + (far * wn).sum()
            for p in params:
                p.grad = None
            loss.backward()
            return loss
        return cams, params, fn

    static = {"ids": torch.tensor([3, 0, 9, 5, 1, 8, 2, 6], device=dev), "idx": idx_all.to(dev)}
    cams_e, params_e, fn_e = make()
    with torch.no_grad():
        cams_e.pose_net.r.add_(delta)
    loss_e = fn_e(**static).detach().clone()
    grads_e = [p.grad.clone() for p in params_e]
    cams_g, params_g, fn_g = make()
    graph = GraphedStep(fn_g, static, warmup=2)
    first = graph.replay().clone()
    with torch.no_grad():
        cams_g.pose_net.r.add_(delta)
    loss_g = graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(first, loss_g)
    assert torch.equal(_bits(loss_g), _bits(loss_e))
    for a, b in zip(params_g, grads_e):
        assert torch.equal(_bits(a.grad), _bits(b))
