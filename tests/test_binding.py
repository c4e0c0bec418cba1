"""CPU: the Python binding layer above the C ABI (color_neus_amd._lib): the signature table against the header's prototypes, the one call
path and its error text, the pointer-array, flat-gradient-buffer and inventory helpers, the output allocation of a render call, and what the
autograd edges share: the coercion, the saving of optional tensors, the names of the render outputs."""
import ctypes as C
import os
import re

import pytest
import torch

import _golden as G
import _native as N
import color_neus_amd as cn
from color_neus_amd import _lib, optim, renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return cn.load_library(N.EMU_LIB)


def header_prototypes():
    """name -> number of parameters, from include/colorneus_render.h with its comments stripped."""
    src = open(os.path.join(ROOT, "include", "colorneus_render.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    protos = {}
    for name, params in re.findall(r"(cnr_\w+)\s*\(([^()]*)\)\s*;", src):
        assert name not in protos, name
        protos[name] = 0 if params.strip() in ("", "void") else params.count(",") + 1
    return protos


def test_signature_table_has_the_arity_of_the_header(lib):
    protos = header_prototypes()
    assert set(protos) == set(_lib.EXPORTS) == set(_lib.SIGNATURES), set(protos) ^ set(_lib.EXPORTS)
    assert _lib.EXPORTS == list(_lib.SIGNATURES)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        assert argtypes is not None, name
        assert len(argtypes) == protos[name], (name, len(argtypes), protos[name])
        if name.endswith("_bytes"):
            assert restype is C.c_size_t, name
        # ... and the loaded library carries exactly the table
        fn = getattr(lib.lib, name)
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes) and fn.restype is restype, name


def test_a_failing_call_raises_with_the_entry_point_and_the_library_message(lib):
    ccfg = _lib.c_config(cn.RenderConfig(col_mode="no_view_dir", col_d_in=6, col_multires_view=0))
    buf, r, c = C.create_string_buffer(128), C.c_int(), C.c_int()
    with pytest.raises(RuntimeError) as e:
        lib.call("cnr_param_info", C.byref(ccfg), 10 ** 6, buf, 128, C.byref(r), C.byref(c))
    msg = lib.lib.cnr_last_error().decode()
    assert msg and "cnr_param_info" in str(e.value) and msg in str(e.value), (str(e.value), msg)
    scratch, nb = lib.scratch("cnr_mc_scratch_bytes", "cpu", 4)
    assert scratch.dtype == torch.uint8 and scratch.numel() == nb > 0
    with pytest.raises(RuntimeError) as e:      # a null lattice
        lib.call("cnr_mc_count", None, 4, 0.0, _lib.ptr(scratch), nb, None, None)
    msg = lib.lib.cnr_last_error().decode()
    assert msg and "cnr_mc_count" in str(e.value) and msg in str(e.value), (str(e.value), msg)
    assert lib.call("cnr_param_info", C.byref(ccfg), 0, buf, 128, C.byref(r), C.byref(c)) is None and r.value * c.value > 0


def test_scratch_keeps_a_minimum_allocation(lib):
    t, nb = lib.scratch("cnr_loss_scratch_bytes", "cpu", 5)
    assert t.numel() == nb == lib.lib.cnr_loss_scratch_bytes(5)
    t, nb2 = lib.scratch("cnr_loss_scratch_bytes", "cpu", 5, at_least=nb + 7)
    assert nb2 == nb and t.numel() == nb + 7


def test_flat_grads_views_tile_one_buffer():
    plist = [torch.zeros(3, 5), torch.zeros(1), torch.zeros(4, 1)]
    flat, views, arr = _lib.flat_grads(plist, torch.device("cpu"))
    assert flat.dtype == torch.float32 and flat.shape == (15 + 1 + 4,)
    assert [v.shape for v in views] == [p.shape for p in plist]
    assert all(v.is_contiguous() for v in views)
    assert views[0].data_ptr() == flat.data_ptr()
    for a, b in zip(views, views[1:]):
        assert b.data_ptr() - a.data_ptr() == 4 * a.numel()
    assert len(arr) == 3 and [arr[i] for i in range(3)] == [v.data_ptr() for v in views]
    params = [torch.nn.Parameter(p) for p in plist]
    for p, v in zip(params, views):
        p.grad = v
    got = optim.flat_view_of_grads(params)
    assert got is not None and got.data_ptr() == flat.data_ptr() and got.shape == flat.shape
    flat.copy_(torch.arange(20.0))
    assert torch.equal(got, flat) and torch.equal(params[2].grad.reshape(-1), torch.arange(16.0, 20.0))
    _, views5, arr5 = _lib.flat_grads(plist, torch.device("cpu"), 5)      # trailing NULL entries (the SDF-query inventory)
    assert len(arr5) == 5 and [arr5[i] for i in range(5)] == [v.data_ptr() for v in views5] + [None, None]


def test_param_array_gives_null_for_none_and_for_the_tail():
    a, b = torch.zeros(2), torch.zeros(3)
    arr = _lib.param_array([a, None, b])
    assert len(arr) == 3 and [arr[i] for i in range(3)] == [a.data_ptr(), None, b.data_ptr()]
    arr = _lib.param_array([a, None, b], 6)
    assert len(arr) == 6 and [arr[i] for i in range(6)] == [a.data_ptr(), None, b.data_ptr(), None, None, None]
    assert len(_lib.param_array([])) == 0
    assert _lib.ptr(None).value is None and _lib.ptr(a).value == a.data_ptr()
    assert _lib.stream_of(a).value is None and _lib.stream_of(torch.device("cpu")).value is None
    f3 = _lib.float3([1, 2.5, -3])
    assert len(f3) == 3 and list(f3) == [1.0, 2.5, -3.0]


def test_inventory_check_messages():
    named = {"a.weight": torch.zeros(4, 3), "a.bias": torch.zeros(4)}
    inv = [("a.bias", 4, 1), ("a.weight", 4, 3)]
    assert _lib.ordered_names(inv, named) == ["a.bias", "a.weight"]
    with pytest.raises(RuntimeError, match=r"library expects parameter 'b\.bias' which this module does not have"):
        _lib.ordered_names(inv + [("b.bias", 4, 1)], named)
    with pytest.raises(RuntimeError, match=r"parameter a\.weight: expected 4x4, have \(4, 3\)"):
        _lib.ordered_names([("a.bias", 4, 1), ("a.weight", 4, 4)], named)
    extra = dict(named, **{"nerf.x": torch.zeros(1)})
    with pytest.raises(RuntimeError, match=r"parameter inventory mismatch between module and library: \['nerf\.x'\]"):
        _lib.ordered_names(inv, extra)
    with pytest.raises(RuntimeError, match="parameter inventory mismatch between module and library"):
        _lib.ordered_names(inv, extra, exempt_prefix="other.")
    assert _lib.ordered_names(inv, extra, exempt_prefix="nerf.") == ["a.bias", "a.weight"]


def test_inventories_of_both_networks_go_through_param_inventory(lib):
    from color_neus_amd.background import NeRF
    net = NeRF()
    inv = lib.param_inventory(net.config(), "cnr_nerf_param_count", "cnr_nerf_param_info")
    assert sorted(n for n, _, _ in inv) == sorted(dict(net.named_parameters()))
    assert [p.numel() for p in net.ordered_params(lib)] == [r * c for _, r, c in inv]


R, M = 3, 10      # rays, samples per ray (n_samples 6 + n_importance 4)
_F32 = torch.float32
# the output tensors of a render call per (renderer type, mode): name -> shape, None = not produced.  Key order is the dict's order.
_COMMON = {"color_fine": (R, 3), "s_val": (R, 1), "cdf_fine": (R, M), "weight_sum": (R, 1), "weight_max": (R, 1), "gradients": (R, M, 3),
           "weights": (R, M), "gradient_error": (), "inside_sphere": (R, M), "depth": (R,), "global_color": (R, 3), "delta_relight": (R, M, 3),
           "delta_relight_ray_sum": None, "z_vals": (R, M), "eik_sums": (2,), "sdf_samples": None, "color_samples": None,
           "global_color_samples": None}
OUTPUT_TABLE = {
    ("Color_NeuS", "saving"): dict(_COMMON),
    ("Color_NeuS", "forward_only"): dict(_COMMON),
    ("Color_NeuS", "loss_only"): dict(_COMMON, gradients=None, delta_relight=None, delta_relight_ray_sum=(R,)),
    ("Color_NeuS", "with_samples"): dict(_COMMON, sdf_samples=(R, M), color_samples=(R, M, 3), global_color_samples=(R, M, 3)),
    ("NeuS", "saving"): dict(_COMMON, global_color=None, delta_relight=None),
    ("NeuS", "forward_only"): dict(_COMMON, global_color=None, delta_relight=None),
    ("NeuS", "loss_only"): dict(_COMMON, gradients=None, global_color=None, delta_relight=None),
    ("NeuS", "with_samples"): dict(_COMMON, global_color=None, delta_relight=None, sdf_samples=(R, M), color_samples=(R, M, 3)),
}


@pytest.mark.parametrize("typ,mode", sorted(OUTPUT_TABLE))
def test_output_allocation_per_mode(typ, mode):
    cfg = cn.RenderConfig(type=typ, n_samples=6, n_importance=4)
    out = renderer._alloc_outputs(cfg, R, torch.device("cpu"), mode)
    want = OUTPUT_TABLE[(typ, mode)]
    assert list(out) == list(want) and set(out) == set(_lib.OUTPUT_FIELDS)
    for k, shape in want.items():
        if shape is None:
            assert out[k] is None, k
        else:
            assert out[k] is not None and tuple(out[k].shape) == shape and out[k].dtype == _F32 and out[k].device.type == "cpu", k


# ---------------------------------------------------------------------------------------------------------------------
# the autograd edges' shared bookkeeping: output names, optional saved tensors, no reference cycle
# ---------------------------------------------------------------------------------------------------------------------
def _tiny(name, lib):
    """(renderer on the CPU emulation library, [rays_o, rays_d, near, far], ground-truth colours, mask) of a tiny fixture"""
    fx = G.load(name)
    ocfg, P = G.weights_of(name, fx)
    rays = [torch.from_numpy(fx[k]) for k in ("rays_o", "rays_d", "jit:near", "jit:far")]
    return N.make_renderer(ocfg, P, lib, "cpu"), rays, torch.from_numpy(fx["rgb_gt"]), torch.from_numpy(fx["mask"])


_FIXTURE = {("NeuS", False): "tiny_neus_sharp", ("NeuS", True): "tiny_neus_outside", ("Color_NeuS", False): "tiny_sharp",
            ("Color_NeuS", True): "tiny_outside"}      # (type, N_OUTSIDE > 0)


@pytest.mark.parametrize("mode", ["saving", "loss_only", "with_samples"])
@pytest.mark.parametrize("typ", ["NeuS", "Color_NeuS"])
def test_output_names_against_shapes_and_the_returned_dict(lib, monkeypatch, typ, mode):
    """The tuple of _RenderFunction.apply has one entry per name of _render_output_names, each with the shape _alloc_outputs gives that name,
    and NeuSRenderer.forward's dict holds under every key the very tensor of that name's position -- in "with_samples" mode (N_OUTSIDE > 0)
    through CompositeBg and composite_output_names, with and without global_color."""
    from color_neus_amd import background as B
    r, rays, _, _ = _tiny(_FIXTURE[(typ, mode == "with_samples")], lib)
    seen = {}

    def spy(cls, key):
        orig = cls.apply

        def apply(*args):
            seen[key] = (args, orig(*args))
            return seen[key][1]
        monkeypatch.setattr(cls, "apply", apply)
    spy(renderer._RenderFunction, "render")
    spy(B.CompositeBg, "composite")
    out = r(*rays, perturb_overwrite=0, training_outputs="loss_only" if mode == "loss_only" else "dict")
    _, res = seen["render"]
    names = sum(renderer._render_output_names(typ, mode), [])
    assert len(set(names)) == len(names) == len(res)
    shapes = renderer._alloc_outputs(r.rcfg, len(rays[0]), torch.device("cpu"), mode)
    assert sorted(names) == sorted(k for k, t in shapes.items() if t is not None)
    for k, t in zip(names, res):
        assert t.shape == shapes[k].shape and t.dtype == _F32, k
    at = lambda k: res[names.index(k)].data_ptr()
    if mode != "with_samples":
        assert "composite" not in seen
        assert set(out) == set(names) & set(renderer._RETURN_KEYS)
        for k, t in out.items():
            assert t.data_ptr() == at(k), k
        return
    cargs, cres = seen["composite"]
    has_gc = typ == "Color_NeuS"
    cnames = sum(B.composite_output_names(has_gc), [])
    assert len(set(cnames)) == len(cnames) == len(cres) and ("global_color" in cnames) == has_gc
    # what the renderer hands to CompositeBg by name: sdf, grads, color, gcolor (arguments 8 .. 11)
    for i, k in ((8, "sdf_samples"), (9, "gradients"), (10, "color_samples"), (11, "global_color_samples")):
        assert (cargs[i].data_ptr() == at(k)) if k in names else (cargs[i] is None), k
    z_vals, MF = cargs[6], cargs[7].shape[1]
    cshape = dict(color_fine=(len(z_vals), 3), s_val=(len(z_vals), 1), cdf_fine=z_vals.shape, weight_sum=(len(z_vals), 1), weight_max=(len(z_vals), 1),
                  weights=(len(z_vals), MF), gradient_error=(), depth=(len(z_vals),), global_color=(len(z_vals), 3), inside_sphere=z_vals.shape,
                  eik_sums=(2,))
    for k, t in zip(cnames, cres):
        assert tuple(t.shape) == tuple(cshape[k]), k
    for k, t in out.items():
        want = cres[cnames.index(k)] if k in cnames else z_vals if k == "z_vals" else res[names.index(k)]
        assert t.data_ptr() == want.data_ptr(), k
    assert set(out) == set(cnames) | {"z_vals", "gradients"} | ({"delta_relight"} if has_gc else set())


class _StubCtx:
    """What save_named / saved_named use of an autograd context."""

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors


def test_saved_named_keeps_absent_and_empty_apart():
    ctx = _StubCtx()
    a, empty, b = torch.arange(3.0), torch.empty(0, 3), torch.ones(2, dtype=torch.int64)
    tail = [torch.zeros(1), torch.zeros(2), torch.empty(0)]
    _lib.save_named(ctx, tail, a=a, gone=None, empty=empty, also_gone=None, b=b)
    assert len(ctx.saved_tensors) == 3 + 3        # nothing stands in for the absent ones
    named, got_tail = _lib.saved_named(ctx)
    assert list(named) == ["a", "gone", "empty", "also_gone", "b"]
    assert named["a"] is a and named["b"] is b
    assert named["empty"] is empty and named["empty"].numel() == 0      # a real zero-element tensor comes back as itself
    assert named["gone"] is None and named["also_gone"] is None
    assert len(got_tail) == 3 and all(x is y for x, y in zip(got_tail, tail))
    _lib.save_named(ctx, x=None)                  # no tail, nothing present
    assert ctx.saved_tensors == () and _lib.saved_named(ctx) == ({"x": None}, [])


def test_dense_f32_is_a_view_of_a_dense_float32_tensor():
    t = torch.arange(6.0).reshape(2, 3).requires_grad_(True)
    d = _lib.dense_f32(t)
    assert d.data_ptr() == t.data_ptr() and not d.requires_grad and _lib.dense_f32(None) is None and _lib.grad_f32(None) is None
    assert _lib.dense_f32(t, -1).shape == (6,) and _lib.dense_f32(t, -1).data_ptr() == t.data_ptr()
    h = _lib.dense_f32(t.double().t(), 3, 2)
    assert h.dtype == _F32 and h.is_contiguous() and torch.equal(h, t.detach().t())
    g = _lib.grad_f32(t.t())
    assert g.is_contiguous() and g.requires_grad and torch.equal(g, t.t())


def test_no_edge_keeps_its_buffers_in_a_reference_cycle(lib, monkeypatch):
    """Every context / scratch buffer the edges take dies by reference counting alone (gc disabled, no gc.collect()) once the outputs, the
    loss and the gradients' owners are gone: nothing of an edge sits in a tensor -> grad_fn -> ctx -> tensor cycle.  The fused loss'
    scratch is left out: loss._loss_scratch keeps it per stream on purpose."""
    import gc
    import weakref
    refs = []
    orig = _lib.RenderLibrary.scratch

    def scratch(self, bytes_fn, *args, **kw):
        buf, nb = orig(self, bytes_fn, *args, **kw)
        if bytes_fn != "cnr_loss_scratch_bytes":
            refs.append((bytes_fn, weakref.ref(buf)))
        return buf, nb
    monkeypatch.setattr(_lib.RenderLibrary, "scratch", scratch)

    def alive():
        return [name for name, ref in refs if ref() is not None]
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        r, rays, gt, mask = _tiny("tiny_sharp", lib)          # a Color_NeuS step
        out = r(*rays)
        loss, loss_dict = cn.compute_loss_fused(out, gt, mask, library=lib)
        loss.backward()
        del out, loss, loss_dict, r
        assert {"cnr_ctx_bytes", "cnr_bwd_scratch_bytes"} <= {name for name, _ in refs} and not alive(), alive()
        r, rays, gt, mask = _tiny("tiny_sharp", lib)          # a forward whose backward never runs: the context buffer goes with the outputs
        out = r(*rays, training_outputs="loss_only")
        assert alive() == ["cnr_ctx_bytes"]
        del out
        assert not alive(), alive()
        n = len(refs)
        r, rays, gt, mask = _tiny("tiny_outside", lib)        # the background edges
        out = r(*rays)
        loss, loss_dict = cn.compute_loss(out, gt, mask)
        loss.backward()
        del out, loss, loss_dict
        assert {"cnr_background_ctx_bytes", "cnr_composite_background_scratch_bytes"} <= {name for name, _ in refs[n:]} and not alive(), alive()
        x = torch.rand(9, 3, generator=torch.Generator().manual_seed(1)) - 0.5
        g = r.sdf_network.gradient(x)                         # a point query with a backward
        held = alive()
        (g.norm(dim=-1) - 1.0).pow(2).mean().backward()
        del g, x, r
        assert held == ["cnr_sdf_query_ctx_bytes"] and not alive(), (held, alive())
    finally:
        if was_enabled:
            gc.enable()
