"""Differentiable SDF point queries: renderer.sdf_network.forward / .sdf / .sdf_hidden_appearance / .gradient (SDFNetwork,
fields.py:81-115) through cnr_sdf_query_forward / cnr_sdf_query_backward.

Every check runs twice: on the CPU-emulation library with the tiny and mid networks, and (marked gpu) on the HIP library at the DTU widths,
where the fused SDF-backward launches run.  The references: the reference SDFNetwork's own values and float32 / float64 gradients of one
fixed loss through its create_graph double backward (sdf_query.npz, tools/gen_sdf_query_golden.py), and the float64 oracle
(oracle.sdf_forward with its analytic gradient, differentiated by torch autograd) for everything else."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import color_neus_amd as cn
from color_neus_amd import _lib
import _golden as G
import _native as N
from oracle import colorneus_oracle as O

EMU_CONFIGS = {"tiny": O.tiny_config, "mid": G.mid_config}


def _lib_and_dev(backend):
    if backend == "emu":
        if not os.path.isfile(N.EMU_LIB):
            pytest.skip("emulation library not built")
        return N.EMU_LIB, "cpu"
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return None, "cuda:0"


def _setup(ocfg, backend, seed=3):
    lib, dev = _lib_and_dev(backend)
    P64 = O.init_params(ocfg, seed=seed, dtype=torch.float64, trained_like=True)
    r = N.make_renderer(ocfg, {k: v.float() for k, v in P64.items()}, lib, dev)
    return r, P64, dev


def _points(n, seed=0, radius=1.3):
    """n points, uniform in a ball of the given radius (so some lie outside the unit sphere)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    rr = torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0) * radius
    return d * rr


def _cotangents(n, F, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, F, generator=g, dtype=torch.float64) * 0.1,
            torch.randn(n, 3, generator=g, dtype=torch.float64))


TERMS = {"sdf": ("a",), "feat": ("B",), "grad": ("c", "eik"), "all": ("a", "B", "c", "eik")}


def _loss(sdf, feat, g, cot, terms):
    a, B, c = cot
    L = sdf.sum() * 0.0
    if "a" in terms:
        L = L + (a.to(sdf.device, sdf.dtype) * sdf.reshape(-1)).sum()
    if "B" in terms:
        L = L + (B.to(feat.device, feat.dtype) * feat).sum()
    if "c" in terms:
        L = L + (c.to(g.device, g.dtype) * g).sum()
    if "eik" in terms:
        L = L + ((g.norm(dim=-1) - 1.0) ** 2).sum()
    return L


def _oracle_grads(P, ocfg, x, cot, terms, dtype, x_grad=True, dev="cpu"):
    """The oracle on `dev` (the GPU tests run it there: DTU widths at 2^18 points), results on the CPU."""
    Pd = {k: v.detach().to(dev, dtype).clone().requires_grad_(k.startswith("sdf_network.")) for k, v in P.items()}
    xd = x.detach().to(dev, dtype).clone().requires_grad_(x_grad)
    sdf, feat, g = O.sdf_forward(Pd, ocfg.sdf, xd, want_grad=True)
    _loss(sdf, feat, g, tuple(t.to(dev) for t in cot), terms).backward()
    out = {k: v.grad.cpu() for k, v in Pd.items() if k.startswith("sdf_network.")}
    if x_grad:
        out["x"] = xd.grad.cpu()
    return out, (sdf.detach().cpu(), feat.detach().cpu(), g.detach().cpu())


def _native_grads(r, x, cot, terms, x_grad=True):
    r.zero_grad(set_to_none=True)
    xn = x.detach().float().to(next(r.parameters()).device).clone().requires_grad_(x_grad)
    out = r.sdf_network(xn)
    g = r.sdf_network.gradient(xn)[:, 0] if ("c" in terms or "eik" in terms) else torch.zeros(xn.shape[0], 3, device=xn.device)
    _loss(out[:, :1], out[:, 1:], g, cot, terms).backward()
    got = {k: p.grad.detach().cpu() for k, p in r.named_parameters() if k.startswith("sdf_network.")}
    if x_grad:
        got["x"] = xn.grad.detach().cpu()
    return got


def _check_backward(ocfg, backend, n, terms, x_grad=True, seed=0):
    r, P, dev = _setup(ocfg, backend)
    x = _points(n, seed)
    cot = _cotangents(n, ocfg.sdf.d_out - 1, seed + 1)
    ref64, _ = _oracle_grads(P, ocfg, x, cot, terms, torch.float64, x_grad, dev)
    ref32, _ = _oracle_grads(P, ocfg, x, cot, terms, torch.float32, x_grad, dev)
    got = _native_grads(r, x, cot, terms, x_grad)
    assert set(got) == set(ref64)
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    bad = G.check_grads_full(ref64, ref32, got, strict=True)
    assert not bad, bad


def _check_forward(ocfg, backend, n, seed=0):
    r, P, dev = _setup(ocfg, backend)
    x = _points(n, seed)
    _, (sdf64, feat64, g64) = _oracle_grads(P, ocfg, x, _cotangents(n, ocfg.sdf.d_out - 1), ("a",), torch.float64, False)
    xn = x.float().to(dev)
    out = r.sdf_network(xn)
    assert out.shape == (n, ocfg.sdf.d_out)
    s = r.sdf_network.sdf(xn)
    assert s.shape == (n, 1)
    xg = x.float().to(dev)
    g = r.sdf_network.gradient(xg)
    assert g.shape == (n, 1, 3) and xg.requires_grad
    h = r.sdf_network.sdf_hidden_appearance(xn)
    assert torch.equal(h, out)
    for got, ref in ((out[:, :1], sdf64), (out[:, 1:], feat64), (s, sdf64), (g[:, 0], g64)):
        got = got.detach().cpu()
        assert torch.isfinite(got).all()
        assert G.relerr(got, ref) < 1e-4, G.relerr(got, ref)


# ---------------------------------------------------------------------------------------------------------------------------------------
# emulation library: tiny and mid networks
@pytest.mark.parametrize("name", list(EMU_CONFIGS))
def test_forward_matches_oracle_emu(name):
    _check_forward(EMU_CONFIGS[name](), "emu", 100)


@pytest.mark.parametrize("name", list(EMU_CONFIGS))
@pytest.mark.parametrize("terms", list(TERMS))
def test_backward_matches_oracle_emu(name, terms):
    _check_backward(EMU_CONFIGS[name](), "emu", 96, TERMS[terms])


@pytest.mark.parametrize("x_grad", [False, True])
def test_backward_points_not_requiring_grad_emu(x_grad):
    _check_backward(G.mid_config(), "emu", 64, TERMS["all"], x_grad=x_grad)


def _reference_fixture(backend, tag):
    """The reference's own SDFNetwork outputs (functions.npz: forward and gradient captured from the reference by tools/gen_golden.py)."""
    lib, dev = _lib_and_dev(backend)
    fx = G.load("functions")
    ocfg = O.tiny_config() if tag == "tiny" else G.mid_config()
    r = N.make_renderer(ocfg, G.prefixed(fx, tag + "w:"), lib, dev)
    pts = torch.from_numpy(fx[f"{tag}:pts"]).to(dev)
    assert G.relerr(r.sdf_network(pts).detach().cpu(), fx[f"{tag}:sdf_out"]) < 1e-4
    assert G.relerr(r.sdf_network.sdf(pts).detach().cpu(), fx[f"{tag}:sdf_out"][:, :1]) < 1e-4
    if f"{tag}:sdf_grad" in fx:
        assert G.relerr(r.sdf_network.gradient(pts.clone())[:, 0].detach().cpu(), fx[f"{tag}:sdf_grad"]) < 1e-4


@pytest.mark.parametrize("tag", ["tiny", "mid"])
def test_forward_matches_reference_fixture_emu(tag):
    _reference_fixture("emu", tag)


GOLDEN_NETS = {"tiny": O.tiny_config, "mid": G.mid_config, "tiny_nown_skip2": G.CONFIGS["tiny_nown_skip2"],
               "tiny_twoskip": G.CONFIGS["tiny_twoskip"], "dtu": O.dtu_config}


def _reference_golden(backend, tag):
    """sdf_query.npz (tools/gen_sdf_query_golden.py): the reference SDFNetwork's forward / gradient values and the float32 / float64 parameter
    and point gradients of L = sum a sdf + sum B feat + sum c g + sum (|g| - 1)^2 through its create_graph double backward."""
    lib, dev = _lib_and_dev(backend)
    fx = G.load("sdf_query")
    ocfg = GOLDEN_NETS[tag]()
    P = O.init_params(ocfg, seed=int(fx[f"{tag}:weight_seed"]), dtype=torch.float32, trained_like=True)
    cs = O.params_checksum(P)
    assert abs(cs - float(fx[f"{tag}:weight_checksum"])) <= 1e-9 * abs(cs), "weight recipe drifted from the fixture"
    r = N.make_renderer(ocfg, P, lib, dev)
    x = torch.from_numpy(fx[f"{tag}:x"]).to(dev).requires_grad_(True)
    a, B, c = (torch.from_numpy(fx[f"{tag}:{k}"]).to(dev) for k in ("a", "B", "c"))
    out = r.sdf_network(x)
    g = r.sdf_network.gradient(x)[:, 0]
    assert G.relerr(out.detach().cpu(), fx[f"{tag}:forward"]) < 1e-4
    assert G.relerr(r.sdf_network.sdf(x).detach().cpu(), fx[f"{tag}:forward"][:, :1]) < 1e-4
    assert G.relerr(g.detach().cpu(), fx[f"{tag}:gradient"]) < 1e-4
    ((a * out[:, 0]).sum() + (B * out[:, 1:]).sum() + (c * g).sum() + ((g.norm(dim=-1) - 1.0) ** 2).sum()).backward()
    stride = int(fx[f"{tag}:stride"])
    got, r64, r32 = {"x": x.grad.detach().cpu()}, {"x": torch.from_numpy(fx[f"{tag}:f64:x_grad"])}, {"x": torch.from_numpy(fx[f"{tag}:f32:x_grad"])}
    for k, p in r.named_parameters():
        if k.startswith("sdf_network."):
            ref = fx[f"{tag}:f64:{k}"]
            v = p.grad.detach().cpu().reshape(-1)
            got[k] = v if v.numel() == ref.size else v[::stride]
            r64[k], r32[k] = torch.from_numpy(ref), torch.from_numpy(fx[f"{tag}:f32:{k}"])
    assert len(got) == len([k for k in fx if k.startswith(f"{tag}:f64:sdf_network.")]) + 1
    bad = G.check_grads_full(r64, r32, got, strict=True)
    assert not bad, bad


@pytest.mark.parametrize("tag", ["tiny", "mid", "tiny_nown_skip2", "tiny_twoskip"])
def test_matches_reference_golden_emu(tag):
    _reference_golden("emu", tag)


def test_point_loss_gradients_tile_one_buffer_emu():
    """A step with point losses only: the sdf_network gradients are views into one flat buffer in canonical order."""
    from color_neus_amd import optim
    r, P, dev = _setup(G.mid_config(), "emu")
    x = _points(50).float()
    ((r.sdf_network.gradient(x)[:, 0].norm(dim=-1) - 1.0) ** 2).sum().backward()
    names = r.sdf_network._query.names()[1]
    named = dict(r.sdf_network.named_parameters())
    assert optim.flat_view_of_grads([named[k] for k in names]) is not None


def _parameters_without_grad(ocfg, backend, n):
    """Only the points require grad (projection onto the surface): no weight-gradient launches, d x as the oracle."""
    r, P, dev = _setup(ocfg, backend)
    for p in r.parameters():
        p.requires_grad_(False)
    x = _points(n)
    cot = _cotangents(n, ocfg.sdf.d_out - 1)
    ref64, _ = _oracle_grads(P, ocfg, x, cot, TERMS["all"], torch.float64, True, dev)
    ref32, _ = _oracle_grads(P, ocfg, x, cot, TERMS["all"], torch.float32, True, dev)
    xn = x.float().to(dev).clone().requires_grad_(True)
    out = r.sdf_network(xn)
    g = r.sdf_network.gradient(xn)[:, 0]
    _loss(out[:, :1], out[:, 1:], g, cot, TERMS["all"]).backward()
    bad = G.check_grads_full({"x": ref64["x"]}, {"x": ref32["x"]}, {"x": xn.grad.cpu()}, strict=True)
    assert not bad, bad


def test_parameters_without_grad_emu():
    _parameters_without_grad(G.mid_config(), "emu", 64)


@pytest.mark.parametrize("n", [1, 31, 33, 127, 129, 600])
def test_ragged_sizes_emu(n):
    _check_backward(G.mid_config(), "emu", n, TERMS["all"], seed=n)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the C ABI: sentinel-filled oversized buffers, nothing is written past row n
def _abi_sentinel(backend, ocfg, n):
    libpath, dev = _lib_and_dev(backend)
    lib = cn.load_library(libpath)
    ccfg = _lib.c_config(N.render_config_from_oracle(ocfg))
    P = O.init_params(ocfg, seed=5, trained_like=True)
    inv = lib.param_inventory(ccfg)
    params = [P[name].float().contiguous().to(dev) if name.startswith("sdf_network.") else None for name, _, _ in inv]
    parr = (C.c_void_p * len(inv))(*[p.data_ptr() if p is not None else None for p in params])
    F, pad, S = ocfg.sdf.d_out - 1, 7, 12345.0
    f32 = dict(dtype=torch.float32, device=dev)
    x = torch.full((n + pad, 3), S, **f32)
    x[:n] = _points(n).float().to(dev)
    sdf, feat, grad = torch.full((n + pad,), S, **f32), torch.full((n + pad, F), S, **f32), torch.full((n + pad, 3), S, **f32)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if dev != "cpu" else C.c_void_p(0)
    nb = lib.lib.cnr_sdf_query_ctx_bytes(C.byref(ccfg), n, 1)
    ctx = torch.empty(nb, dtype=torch.uint8, device=dev)
    lib.check(lib.lib.cnr_sdf_query_forward(C.byref(ccfg), parr, C.c_void_p(x.data_ptr()), n, 1, C.c_void_p(sdf.data_ptr()),
                                            C.c_void_p(feat.data_ptr()), C.c_void_p(grad.data_ptr()), C.c_void_p(ctx.data_ptr()), nb, stream),
              "forward")
    cot = [t.float().to(dev) for t in _cotangents(n, F)]
    dsdf, dfeat, dgrad = [torch.cat([t, torch.full((pad,) + tuple(t.shape[1:]), S, **f32)]) for t in cot]
    d_params = [torch.full(p.shape, float("nan"), **f32) if p is not None else None for p in params]   # NaN: finite afterwards = overwritten
    darr = (C.c_void_p * len(inv))(*[p.data_ptr() if p is not None else None for p in d_params])
    d_x = torch.full((n + pad, 3), S, **f32)
    nbs = lib.lib.cnr_sdf_query_bwd_scratch_bytes(C.byref(ccfg), n, 1)
    scratch = torch.full((nbs,), 255, dtype=torch.uint8, device=dev)
    lib.check(lib.lib.cnr_sdf_query_backward(C.byref(ccfg), parr, C.c_void_p(x.data_ptr()), n, 1, C.c_void_p(dsdf.data_ptr()),
                                             C.c_void_p(dfeat.data_ptr()), C.c_void_p(dgrad.data_ptr()), C.c_void_p(ctx.data_ptr()), nb,
                                             C.cast(darr, C.POINTER(C.c_void_p)), C.c_void_p(d_x.data_ptr()), C.c_void_p(scratch.data_ptr()), nbs,
                                             stream), "backward")
    if dev != "cpu":
        torch.cuda.synchronize()
    for t in (sdf, feat, grad, d_x):
        assert torch.isfinite(t[:n]).all()
        assert (t[n:] == S).all()
    for p in d_params:
        if p is not None:
            assert torch.isfinite(p).all()
    # and a backward that asks for the gradient path on a context the forward wrote without it poisons its outputs (NaN), it is never
    # silently wrong
    nb0 = lib.lib.cnr_sdf_query_ctx_bytes(C.byref(ccfg), n, 0)
    ctx0 = torch.empty(max(nb0, nb), dtype=torch.uint8, device=dev)
    lib.check(lib.lib.cnr_sdf_query_forward(C.byref(ccfg), parr, C.c_void_p(x.data_ptr()), n, 0, C.c_void_p(sdf.data_ptr()), None, None,
                                            C.c_void_p(ctx0.data_ptr()), ctx0.numel(), stream), "forward")
    lib.check(lib.lib.cnr_sdf_query_backward(C.byref(ccfg), parr, C.c_void_p(x.data_ptr()), n, 1, C.c_void_p(dsdf.data_ptr()), None,
                                             C.c_void_p(dgrad.data_ptr()), C.c_void_p(ctx0.data_ptr()), ctx0.numel(), None,
                                             C.c_void_p(d_x.data_ptr()), C.c_void_p(scratch.data_ptr()), nbs, stream), "backward")
    if dev != "cpu":
        torch.cuda.synchronize()
    assert torch.isnan(d_x[:n]).all() and (d_x[n:] == S).all()


@pytest.mark.parametrize("n", [1, 33, 129])
def test_abi_writes_nothing_past_row_n_emu(n):
    _abi_sentinel("emu", G.mid_config(), n)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _determinism(ocfg, backend, n):
    r, P, dev = _setup(ocfg, backend)
    x = _points(n).float().to(dev).requires_grad_(True)
    cot = _cotangents(n, ocfg.sdf.d_out - 1)
    out = r.sdf_network(x)
    g = r.sdf_network.gradient(x)[:, 0]
    L = _loss(out[:, :1], out[:, 1:], g, cot, TERMS["all"])
    res = []
    for _ in range(3):
        r.zero_grad(set_to_none=True)
        x.grad = None
        L.backward(retain_graph=True)
        res.append([p.grad.clone() for p in r.sdf_network.parameters()] + [x.grad.clone()])
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b)
    for a, b in zip(res[0], res[2]):
        assert torch.equal(a, b)


def test_determinism_and_retain_graph_emu():
    _determinism(G.mid_config(), "emu", 200)


def _render_agreement(ocfg, backend, R):
    r, P, dev = _setup(ocfg, backend)
    g = torch.Generator().manual_seed(7)
    o = (torch.rand(R, 3, generator=g) - 0.5) * 0.4
    d = torch.randn(R, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    near, far = torch.full((R, 1), 0.3), torch.full((R, 1), 1.9)
    o, d, near, far = o.to(dev), d.to(dev), near.to(dev), far.to(dev)
    with torch.no_grad():
        out = r(o, d, near, far, perturb_overwrite=0)
    z = out["z_vals"]
    M = z.shape[1]
    dist = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), 2.0 / ocfg.n_samples, device=dev)], dim=1)
    mid = z + dist * 0.5
    pts = (o[:, None, :] + d[:, None, :] * mid[..., None]).reshape(-1, 3)
    with torch.no_grad():
        gq = r.sdf_network.gradient(pts.clone())[:, 0].reshape(R, M, 3)
        fq = r.sdf_network(pts)          # (the query forward; sdf() itself is cnr_sdf_eval here, the function r.sdf calls)
    assert G.relerr(gq.cpu(), out["gradients"].cpu()) < 1e-5
    assert G.relerr(fq[:, :1].cpu(), r.sdf(pts).cpu()) < 1e-5
    # and with the context kept (autograd path)
    x = pts.clone().requires_grad_(True)
    sg = r.sdf_network.sdf(x)
    assert G.relerr(sg.detach().cpu(), r.sdf(pts).cpu()) < 1e-5


def test_agrees_with_render_path_emu():
    _render_agreement(O.tiny_config(), "emu", 16)


# ---------------------------------------------------------------------------------------------------------------------------------------
def _training_step(ocfg, backend, R, n_eik):
    """loss = compute_loss(render) + 0.1 * mean((|g(x)| - 1)^2), x uniform in the unit ball: every SDF parameter gradient as the float64
    oracle of the same combined loss; the colour / relight gradients bitwise those of the render-only loss; ClipAdam steps."""
    lib, dev = _lib_and_dev(backend)
    fx = G.load("tiny_sharp")
    r, P, dev = _setup(ocfg, backend)
    R = min(R, fx["rays_o"].shape[0])
    o, d = torch.from_numpy(fx["rays_o"][:R]), torch.from_numpy(fx["rays_d"][:R])
    near, far = (torch.from_numpy(fx[f"jit:{k}"][:R]) for k in ("near", "far"))
    gt, mask = torch.from_numpy(fx["rgb_gt"][:R]), torch.from_numpy(fx["mask"][:R])
    with torch.no_grad():   # the samples this network's own sampler picks, then fixed for the native runs and the oracle
        z = r(o.to(dev), d.to(dev), near.to(dev), far.to(dev), perturb_overwrite=0)["z_vals"].cpu()
    xe = _points(n_eik, seed=11, radius=1.0)
    odev = dev   # (the float64 oracle runs where the native code runs: DTU widths on the GPU)

    def native(with_eik):
        r.zero_grad(set_to_none=True)
        out = r(o.to(dev), d.to(dev), near.to(dev), far.to(dev), z_vals=z.to(dev))
        loss, _ = cn.compute_loss(out, gt.to(dev), mask.to(dev))
        if with_eik:
            g = r.sdf_network.gradient(xe.float().to(dev))[:, 0]
            loss = loss + 0.1 * ((g.norm(dim=-1) - 1.0) ** 2).mean()
        loss.backward()
        return {k: p.grad.detach().clone().cpu() for k, p in r.named_parameters()}

    def oracle(dtype):
        Pd = {k: v.detach().to(odev, dtype).clone().requires_grad_(True) for k, v in P.items()}
        out = O.render(Pd, ocfg, o.to(odev, dtype), d.to(odev, dtype), near.to(odev, dtype), far.to(odev, dtype), z_vals=z.to(odev, dtype))
        loss = O.compute_loss(out, gt.to(odev, dtype), mask.to(odev, dtype))[0]
        _, _, g = O.sdf_forward(Pd, ocfg.sdf, xe.to(odev, dtype), want_grad=True)
        loss = loss + 0.1 * ((g.norm(dim=-1) - 1.0) ** 2).mean()
        loss.backward()
        return {k: v.grad.cpu() for k, v in Pd.items() if k.startswith("sdf_network.")}

    base = native(False)
    got = native(True)
    for k in got:
        if not k.startswith("sdf_network."):
            assert torch.equal(got[k], base[k]), k
    bad = G.check_grads_full(oracle(torch.float64), oracle(torch.float32), got, strict=True)
    assert not bad, bad
    opt = cn.ClipAdam(r.parameters(), lr=1e-4, library=lib)
    before = [p.detach().clone() for p in r.parameters()]
    opt.step()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, r.parameters()))


def test_training_step_with_point_eikonal_emu():
    _training_step(O.tiny_config(), "emu", 16, 256)


# ---------------------------------------------------------------------------------------------------------------------------------------
def test_module_hygiene():
    lib, _ = _lib_and_dev("emu")
    rc = N.render_config_from_oracle(O.tiny_config())
    r = cn.ColorNeuSRenderer(rc, library=lib)
    ref_keys = list(cn.ColorNeuSRenderer(rc, library=lib).state_dict().keys())
    assert list(r.sdf_network.children()) == [m for _, m in r.sdf_network.named_children()]
    assert all(n.startswith("lin") for n, _ in r.sdf_network.named_children())
    assert list(r.sdf_network.buffers()) == []
    x = _points(40).float()
    before = r.sdf_network(x).detach()
    assert list(r.state_dict().keys()) == ref_keys
    assert all(n.startswith("lin") for n, _ in r.sdf_network.named_children())
    # strict loading of a reference-named state dict still works
    r.load_state_dict(copy.deepcopy(r.state_dict()), strict=True)
    # a deepcopy queries its own parameters
    r2 = copy.deepcopy(r)
    with torch.no_grad():
        for p in r2.sdf_network.parameters():
            p.mul_(0.5)
    assert torch.equal(r.sdf_network(x).detach(), before)
    assert not torch.equal(r2.sdf_network(x).detach(), before)
    # empty queries keep the shapes
    e = torch.zeros(0, 3)
    assert r.sdf_network(e).shape == (0, rc.sdf_d_out) and r.sdf_network.sdf(e).shape == (0, 1)
    assert r.sdf_network.gradient(e.clone()).shape == (0, 1, 3)


def test_third_order_raises():
    lib, _ = _lib_and_dev("emu")
    r = cn.ColorNeuSRenderer(N.render_config_from_oracle(O.tiny_config()), library=lib)
    x = _points(20).float()
    g = r.sdf_network.gradient(x)
    L = ((g.norm(dim=-1) - 1) ** 2).sum()
    gp = torch.autograd.grad(L, list(r.sdf_network.parameters()), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiate twice"):
        sum(t.sum() for t in gp).backward()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the HIP library at the DTU widths (the fused SDF-backward launches)
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["tiny", "mid"])
def test_forward_matches_reference_fixture_gpu(tag):
    _reference_fixture("hip", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(GOLDEN_NETS))
def test_matches_reference_golden_gpu(tag):
    _reference_golden("hip", tag)


@pytest.mark.gpu
def test_forward_matches_oracle_gpu():
    _check_forward(O.dtu_config(), "hip", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("terms", list(TERMS))
def test_backward_matches_oracle_gpu(terms):
    _check_backward(O.dtu_config(), "hip", 4096, TERMS[terms])


@pytest.mark.gpu
@pytest.mark.parametrize("x_grad", [False, True])
def test_backward_points_not_requiring_grad_gpu(x_grad):
    _check_backward(O.dtu_config(), "hip", 2048, TERMS["all"], x_grad=x_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 31, 33, 127, 129, 4097, (1 << 18) + 1])
def test_ragged_sizes_gpu(n):
    _check_backward(O.dtu_config(), "hip", n, TERMS["all"], seed=n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 33, 4097])
def test_abi_writes_nothing_past_row_n_gpu(n):
    _abi_sentinel("hip", O.dtu_config(), n)


@pytest.mark.gpu
def test_determinism_and_retain_graph_gpu():
    _determinism(O.dtu_config(), "hip", 8192)


@pytest.mark.gpu
def test_agrees_with_render_path_gpu():
    _render_agreement(O.dtu_config(), "hip", 256)


@pytest.mark.gpu
def test_training_step_with_point_eikonal_gpu():
    _training_step(O.dtu_config(), "hip", 32, 1 << 14)


@pytest.mark.gpu
def test_parameters_without_grad_gpu():
    _parameters_without_grad(O.dtu_config(), "hip", 4096)


@pytest.mark.gpu
def test_query_backward_takes_the_fused_launches_gpu():
    """At 2^16 points with the DTU widths a query backward runs the fused SDF-backward launches a render backward runs: the fused
    layer + weight-gradient launch (layer_dw), the first layer's sweep (sweep0_dw) and the one-pass first-layer backward (narrow_bwd)."""
    r, P, dev = _setup(O.dtu_config(), "hip")
    x = _points(1 << 16).float().to(dev).requires_grad_(True)
    g = r.sdf_network.gradient(x)[:, 0]
    L = ((g.norm(dim=-1) - 1.0) ** 2).sum() + r.sdf_network.sdf(x).sum()
    lib = r._lib
    torch.cuda.synchronize()
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        L.backward()
        torch.cuda.synchronize()
        names = {rec[0] for rec in lib.timing_collect()}
    finally:
        lib.timing_enable(False)
    for k in ("layer_dw", "sweep0_dw", "narrow_bwd"):
        assert k in names, (k, sorted(names))
