"""CPU: the Python binding layer above the C ABI (color_neus_amd._lib): the signature table against the header's prototypes, the one call
path and its error text, the pointer-array, flat-gradient-buffer and inventory helpers, and the output allocation of a render call."""
import ctypes as C
import os
import re

import pytest
import torch

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
