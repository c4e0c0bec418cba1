"""Image evaluation (color_neus_amd.imaging on cnr_image_metrics / cnr_image_panel, meshio.write_png).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  No fixture from the reference is
possible (kornia and cv2 are not installed), so the yardsticks are written here and use nothing from the library:

  R32   the arithmetic specified in include/colorneus_render.h restated in float32 torch on the CPU as separate element-wise operations on
        slices of the reflect-padded planes (each is one IEEE rounding, so this is the specification bit for bit).  The SSIM map must match
        it BITWISE; the two sums must be within 1e-9 relative of the float64 sums of its elements (the library adds N <= 2^23 float64 terms
        of magnitude <= 1 in some fixed order: N * 2^-53 < 1e-9).
  R64   the same in float64.
  RC    an independent float64 form: F.conv2d with the 3 x 3 outer-product window on F.pad(..., mode="reflect").
  the quantisation, the depth levels and the HOT ramp restated in numpy float32.
"""
import ctypes as C
import functools
import math
import os
import struct
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import color_neus_amd as cn
import _golden as G
import _native as N

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
LAYOUTS = ["nchw", "nhwc"]
W1, W0 = float.fromhex("0x1.3b3046p-2"), float.fromhex("0x1.899f76p-2")


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


# ---- yardsticks -------------------------------------------------------------------------------------------------------------------------
def _filt(p):
    """rows first: h = (w1*p[c-1] + w0*p[c]) + w1*p[c+1], then the same down the columns; reflected border; dtype of p"""
    w1, w0 = torch.tensor(W1, dtype=p.dtype), torch.tensor(W0, dtype=p.dtype)
    q = F.pad(p, (1, 1, 1, 1), mode="reflect")
    h = (w1 * q[..., :, :-2] + w0 * q[..., :, 1:-1]) + w1 * q[..., :, 2:]
    return (w1 * h[..., :-2, :] + w0 * h[..., 1:-1, :]) + w1 * h[..., 2:, :]


def _ssim_ref(x, y, dtype):
    """The SSIM map of [B, C, H, W] images by the specified operations in `dtype` (R32 / R64)."""
    x, y = x.detach().cpu().to(dtype), y.detach().cpu().to(dtype)
    c1, c2, eps, two = (torch.tensor(v, dtype=dtype) for v in (np.float32(1e-4), np.float32(9e-4), np.float32(1e-12), 2.0))
    mu1, mu2 = _filt(x), _filt(y)
    e11, e22, e12 = _filt(x * x), _filt(y * y), _filt(x * y)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s1, s2, s12 = e11 - m11, e22 - m22, e12 - m12
    num = (two * m12 + c1) * (two * s12 + c2)
    den = ((m11 + m22) + c1) * ((s1 + s2) + c2)
    return num / (den + eps)


def _ssim_conv(x, y):
    """RC: float64 conv2d with the outer-product window on reflect-padded planes."""
    x, y = x.detach().cpu().double(), y.detach().cpu().double()
    b, c, h, w = x.shape
    g = torch.tensor([W1, W0, W1], dtype=torch.float64)
    k = (g[:, None] * g[None, :])[None, None]
    f = lambda p: F.conv2d(F.pad(p.reshape(b * c, 1, h, w), (1, 1, 1, 1), mode="reflect"), k).reshape(b, c, h, w)
    c1, c2, eps = float(np.float32(1e-4)), float(np.float32(9e-4)), float(np.float32(1e-12))
    mu1, mu2 = f(x), f(y)
    s1, s2, s12 = f(x * x) - mu1 * mu1, f(y * y) - mu2 * mu2, f(x * y) - mu1 * mu2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2) + eps)


# ---- inputs ([B, C, H, W] float32 on the CPU; computed once, never modified) -------------------------------------------------------------
def _smooth(h=37, w=67):
    i, j = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    ch = [0.5 + 0.4 * torch.sin(0.07 * i + p) * torch.cos(0.05 * j - p) for p in (0.0, 1.0, 2.0)]
    return torch.stack(ch)[None].contiguous()


@functools.lru_cache(maxsize=None)
def _case(name):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == "A":
        x = torch.rand(1, 3, 37, 67, generator=g)
        return x, (x + 0.05 * torch.randn(1, 3, 37, 67, generator=g)).clamp(0.0, 1.0)
    if name == "B":
        x = _smooth()
        return x, x + 0.01 * torch.randn(1, 3, 37, 67, generator=g)
    if name == "C":
        return _smooth(), _smooth()
    if name == "D":
        return torch.full((1, 3, 37, 67), 0.7), torch.full((1, 3, 37, 67), 0.7)
    if name == "E":
        return torch.ones(1, 3, 37, 67), torch.zeros(1, 3, 37, 67)
    if name == "F":
        x = torch.rand(1, 3, 2, 2, generator=g)
        return x, (x + 0.05 * torch.randn(1, 3, 2, 2, generator=g)).clamp(0.0, 1.0)
    shape = {"G1": (2, 1, 2, 130), "G2": (2, 1, 130, 2)}[name]
    x = torch.rand(shape, generator=g)
    return x, (x + 0.05 * torch.randn(shape, generator=g)).clamp(0.0, 1.0)


CASES = ["A", "B", "C", "D", "E", "F", "G1", "G2"]


@functools.lru_cache(maxsize=None)
def _r32(name):
    x, y = _case(name)
    d = x - y
    return _ssim_ref(x, y, torch.float32), d * d


def _raw_nhwc(lib, dev, x, y):
    """cnr_image_metrics with channels_last = 1 on the [B][H][W][C] copies of [B, C, H, W] tensors (the one form image_metrics cannot be
    handed when C == 1, where both layouts are the same memory) -> (sums [2] float64, map as [B, C, H, W])."""
    b, c, h, w = x.shape
    lib = cn.load_library(lib)
    L = lib.lib
    xd, yd = (t.permute(0, 2, 3, 1).contiguous().to(dev) for t in (x, y))
    sums, smap = torch.empty(2, dtype=torch.float64, device=dev), torch.empty_like(xd)
    nb = L.cnr_image_scratch_bytes(b, c, h, w)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if xd.is_cuda else None
    lib.check(L.cnr_image_metrics(p(xd), p(yd), b, c, h, w, 1, p(smap), p(sums), p(scratch), nb, stream), "cnr_image_metrics")
    return sums, smap.permute(0, 3, 1, 2)


def _metrics(backend, x, y, layout):
    """image_metrics of [B, C, H, W] CPU tensors on the backend in the given memory layout -> (mse, ssim, psnr as floats, map [B, C, H, W] on the CPU)"""
    lib, dev = _lib_and_dev(backend)
    b, c = x.shape[:2]
    if layout == "nchw":
        m = cn.image_metrics(x.to(dev), y.to(dev), return_map=True, library=lib)
        smap = m["ssim_map"]
    elif b == 1:
        m = cn.image_metrics(x[0].permute(1, 2, 0).contiguous().to(dev), y[0].permute(1, 2, 0).contiguous().to(dev), return_map=True, library=lib)
        smap = m["ssim_map"].permute(2, 0, 1)[None]
    else:
        sums, smap = _raw_nhwc(lib, dev, x, y)
        means = sums / torch.full((), float(x.numel()), dtype=torch.float64, device=dev)
        m = {"mse": means[0], "ssim": means[1], "psnr": -10.0 * torch.log10(means[0])}
    for k in ("mse", "ssim", "psnr"):
        assert m[k].dtype == torch.float64 and m[k].dim() == 0 and m[k].device.type == torch.device(dev).type and m[k].grad_fn is None
    assert smap.dtype == torch.float32 and tuple(smap.shape) == tuple(x.shape)
    return m["mse"].item(), m["ssim"].item(), m["psnr"].item(), smap.cpu().contiguous()


# ---- 1 / 2: the map is the specification, the scalars are its float64 means ----------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", CASES)
def test_map_is_the_specification_and_scalars_are_its_means(name, layout, backend):
    x, y = _case(name)
    ref_map, ref_sq = _r32(name)
    mse, ssim, psnr, smap = _metrics(backend, x, y, layout)
    assert torch.equal(_bits(smap), _bits(ref_map)), int((_bits(smap) != _bits(ref_map)).sum())     # every pixel, border included
    ref_mse, ref_ssim = ref_sq.double().mean().item(), ref_map.double().mean().item()
    print(f"{name} {layout}: mse {mse:.17g} (R32 {ref_mse:.17g}), ssim {ssim:.17g} (R32 {ref_ssim:.17g}), psnr {psnr:.12f}, R32 map min {ref_map.min().item():.7f}")
    assert abs(mse - ref_mse) <= 1e-9 * ref_mse
    assert abs(ssim - ref_ssim) <= 1e-9 * abs(ref_ssim)
    if name in ("C", "D"):          # identical images
        assert mse == 0.0 and psnr == math.inf
    else:
        ref_psnr = -10.0 * math.log10(ref_mse)
        # what the 1e-9 relative bound on mse gives: d psnr = 10 / ln(10) * d mse / mse (an absolute 1e-9 on psnr would not follow from it)
        assert abs(psnr - ref_psnr) <= 10.0 / math.log(10.0) * 1e-9
    if name == "C":                 # what float32 leaves of e11 - m11 where the image is flat: R32 itself is this far from 1
        assert abs(ssim - 1.0) <= 2e-5
    if name == "E":
        assert mse == 1.0 and psnr == 0.0 and abs(ssim - 9.999e-5) < 1e-8


# ---- 3: independent form ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["A", "B", "F"])
def test_mean_ssim_against_the_conv2d_form(name, backend):
    x, y = _case(name)
    rc = _ssim_conv(x, y).mean().item()
    r64 = _ssim_ref(x, y, torch.float64).mean().item()
    r32 = _r32(name)[0].double().mean().item()
    _, ssim, _, _ = _metrics(backend, x, y, "nchw")
    print(f"{name}: library - RC {ssim - rc:.3e}, R32 - R64 {r32 - r64:.3e}, R64 - RC {r64 - rc:.3e}")
    assert abs(r64 - rc) <= 1e-12
    assert abs(ssim - rc) <= 2e-6


# ---- 4: planes are independent -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_planes_are_independent(layout, backend):
    for name in ("G1", "G2"):
        x, y = _case(name)
        whole = _metrics(backend, x, y, layout)[3]
        alone = _metrics(backend, x[1:], y[1:], layout)[3]
        assert torch.equal(_bits(whole[1:]), _bits(alone))
    x, y = _case("A")
    perm = [2, 0, 1]
    base = _metrics(backend, x, y, layout)[3]
    permuted = _metrics(backend, x[:, perm].contiguous(), y[:, perm].contiguous(), layout)[3]
    assert torch.equal(_bits(permuted), _bits(base[:, perm]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_channels_last_memory_format_is_read_in_place(backend):
    """a 4-D pair in torch's channels-last memory format: the same numbers, the map in that format too"""
    lib, dev = _lib_and_dev(backend)
    x, y = (torch.cat([t, t.flip(1)]).to(dev).contiguous(memory_format=torch.channels_last) for t in _case("A"))
    assert not x.is_contiguous()
    m = cn.image_metrics(x, y, return_map=True, library=lib)
    assert m["ssim_map"].is_contiguous(memory_format=torch.channels_last) and not m["ssim_map"].is_contiguous()
    ref = _r32("A")[0]
    assert torch.equal(_bits(m["ssim_map"]), _bits(torch.cat([ref, ref.flip(1)])))
    # any other strides / dtype: the contiguous float32 copy is evaluated; no graph
    xs = torch.zeros(1, 3, 37, 134, device=dev)[..., ::2]
    xs.copy_(_case("A")[0])
    m2 = cn.image_metrics(xs.double().requires_grad_(True), _case("A")[1].to(dev), return_map=True, library=lib)
    assert torch.equal(_bits(m2["ssim_map"]), _bits(ref)) and m2["ssim"].grad_fn is None and not m2["ssim_map"].requires_grad
    # more than 32 channels in a channels-last form: evaluated on a [B, C, H, W] copy, the map in the caller's shape
    wide_x, wide_y = (torch.cat([t] * 11, 1)[0].permute(1, 2, 0).contiguous().to(dev) for t in _case("A"))      # [37, 67, 33]
    m3 = cn.image_metrics(wide_x, wide_y, return_map=True, library=lib)
    assert tuple(m3["ssim_map"].shape) == (37, 67, 33)
    assert torch.equal(_bits(m3["ssim_map"].permute(2, 0, 1)), _bits(torch.cat([ref] * 11, 1)[0]))
    m4 = cn.image_metrics(wide_x.permute(2, 0, 1)[None], wide_y.permute(2, 0, 1)[None], return_map=True, library=lib)   # channels-last strides, 33 channels
    assert torch.equal(_bits(m4["ssim_map"]), _bits(torch.cat([ref] * 11, 1))) and m4["ssim"].item() == m3["ssim"].item()
    with pytest.raises(ValueError):
        cn.image_metrics(x, y[:, :, :-1], library=lib)
    with pytest.raises(ValueError):
        cn.image_metrics(x[0, 0], y[0, 0], library=lib)


# ---- 5: reproducible ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_calls_give_the_same_bits(layout, backend):
    x, y = _case("A")
    a, b = _metrics(backend, x, y, layout), _metrics(backend, x, y, layout)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(_bits(a[3]), _bits(b[3]))


# ---- 6: the reference's meter classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_meter_classes(backend):
    lib, dev = _lib_and_dev(backend)
    (xa, ya), (xb, yb) = ((t.to(dev) for t in _case(n)) for n in ("A", "B"))
    hwc = lambda t: t[0].permute(1, 2, 0).contiguous()
    P, S = cn.PSNR(None, library=lib), cn.SSIM(cfg=None, name="", library=lib)
    assert P.name == "PSNR" and S.name == "SSIM"
    p1 = P.feed(hwc(xa), hwc(ya))                 # NeuS_Trainer.py:276 feeds [H, W, 3]
    s1 = S.feed(xa, ya)                           # :277 feeds [1, 3, H, W]
    assert type(p1) is float and type(s1) is float
    assert p1 == cn.image_metrics(hwc(xa), hwc(ya), library=lib)["psnr"].item() == cn.psnr(hwc(xa), hwc(ya), library=lib).item()
    assert s1 == cn.image_metrics(xa, ya, library=lib)["ssim"].item()
    assert P.get_result() == p1 and S.get_measures() == {"SSIM": s1}
    p2, s2 = P.feed(hwc(xb), hwc(yb)), S.feed(xb, yb)
    assert P.get_measures() == {"PSNR": (p1 + p2) / 2} and S.get_result() == (s1 + s2) / 2
    assert str(P) == "PSNR: %6.4f" % ((p1 + p2) / 2) and str(S) == "SSIM: %6.4f" % ((s1 + s2) / 2)
    P.reset()
    assert P.feed(hwc(xb), hwc(yb)) == p2 and P.get_result() == p2
    smap = cn.ssim(xa, ya, window_size=3, library=lib)
    assert torch.equal(_bits(smap), _bits(_r32("A")[0]))
    with pytest.raises(ValueError):
        cn.ssim(xa, ya, window_size=5, library=lib)
    mse = torch.tensor(0.01, dtype=torch.float64)
    assert abs(cn.mse2psnr(mse).item() - 20.0) < 1e-12


# ---- 7: quantisation, depth colour map, panel ------------------------------------------------------------------------------------------------------
def _quant_np(v):
    t = np.asarray(v, dtype=np.float32) * np.float32(255.0)
    t = np.where(t > np.float32(0.0), t, np.float32(0.0))            # max(., 0) that sends NaN to 0
    t = np.where(t < np.float32(255.0), t, np.float32(255.0))
    return t.astype(np.int32).astype(np.uint8)


def _levels_np(d):
    d = np.asarray(d, dtype=np.float32)
    if np.isnan(d).all():
        return np.zeros(d.shape, np.int32)
    vmin, vmax = np.nanmin(d), np.nanmax(d)
    rng = np.float32(vmax - vmin)
    if not rng >= np.float32(1e-10):
        return np.zeros(d.shape, np.int32)
    with np.errstate(invalid="ignore"):
        t = (d - vmin) / rng * np.float32(255.0)
        t = np.where(t > np.float32(0.0), t, np.float32(0.0))
        t = np.where(t < np.float32(255.0), t, np.float32(255.0))
    return t.astype(np.int32)


def _hot_np(v):
    """levels -> uint8 [..., 3] in B, G, R order"""
    u = np.asarray(v).astype(np.float32) / np.float32(255.0)
    r = np.clip(np.float32(2.5) * u, np.float32(0.0), np.float32(1.0))
    g = np.clip(np.float32(2.5) * u - np.float32(1.0), np.float32(0.0), np.float32(1.0))
    b = np.clip(np.float32(5.0) * u - np.float32(4.0), np.float32(0.0), np.float32(1.0))
    return np.stack([(np.float32(255.0) * c + np.float32(0.5)).astype(np.int32).astype(np.uint8) for c in (b, g, r)], axis=-1)


def _cmap_np(d):
    return _hot_np(_levels_np(d))


@pytest.mark.parametrize("backend", BACKENDS)
def test_quantise_cmap_panel(backend):
    lib, dev = _lib_and_dev(backend)
    vals = np.array([-0.1, 0.0, 0.5 / 255.0, 0.999, 1.0, 1.3, float("nan")], dtype=np.float32)
    assert _quant_np(vals).tolist() == [0, 0, 0, 254, 255, 255, 0]
    gt = torch.from_numpy(np.resize(vals, (5, 7, 3)).copy())
    render = torch.from_numpy(np.resize(vals[::-1], (5, 7, 3)).copy())
    # a ramp of 256 distinct depths that hits every level: 0, k + 0.5 (k = 1 .. 254), 255
    ramp = np.arange(256, dtype=np.float32) + np.float32(0.5)
    ramp[0], ramp[255] = 0.0, 255.0
    assert len(set(ramp.tolist())) == 256 and _levels_np(ramp).tolist() == list(range(256))
    table = cn.cmap(torch.from_numpy(ramp.reshape(16, 16)).to(dev), library=lib)
    assert table.dtype == torch.uint8 and tuple(table.shape) == (16, 16, 3) and table.device.type == torch.device(dev).type
    table = table.cpu().numpy().reshape(256, 3)
    assert np.array_equal(table, _hot_np(np.arange(256)))
    assert table[0].tolist() == [0, 0, 0] and table[255].tolist() == [255, 255, 255]
    assert table[102].tolist() == [0, 0, 255] and table[204].tolist() == [0, 255, 255]      # B, G, R: red saturates at 0.4, green at 0.8
    # a constant depth: all zero
    assert not cn.cmap(torch.full((5, 7), 1.25, device=dev), library=lib).any()
    # one NaN: left out of the range, its pixel black
    rng = np.random.default_rng(3)
    d = rng.uniform(0.5, 3.0, (5, 7)).astype(np.float32)
    d[2, 3] = np.nan
    got = cn.cmap(torch.from_numpy(d).to(dev), library=lib).cpu().numpy()
    assert np.array_equal(got, _cmap_np(d)) and got[2, 3].tolist() == [0, 0, 0] and got.max() == 255
    # the panel: hstack of the three parts
    pic = cn.panel(gt.to(dev), render.to(dev), torch.from_numpy(d).to(dev), library=lib)
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (5, 21, 3)
    assert np.array_equal(pic.cpu().numpy(), np.hstack([_quant_np(gt.numpy()), _quant_np(render.numpy()), _cmap_np(d)]))
    h, w = 33, 130
    g_, r_ = (rng.uniform(-0.2, 1.2, (h, w, 3)).astype(np.float32) for _ in range(2))
    d_ = rng.normal(0.0, 2.0, (h, w)).astype(np.float32)
    pic = cn.panel(torch.from_numpy(g_).to(dev), torch.from_numpy(r_).to(dev), torch.from_numpy(d_).to(dev), library=lib)
    assert pic.dtype == torch.uint8 and tuple(pic.shape) == (h, 3 * w, 3)
    assert np.array_equal(pic.cpu().numpy(), np.hstack([_quant_np(g_), _quant_np(r_), _cmap_np(d_)]))
    # float64 / strided inputs: their contiguous float32 copies
    pic2 = cn.panel(torch.from_numpy(g_).to(dev).double(), torch.from_numpy(np.ascontiguousarray(r_.transpose(1, 0, 2))).to(dev).transpose(0, 1),
                    torch.from_numpy(d_).to(dev), library=lib)
    assert torch.equal(pic2, pic)


# ---- 8: PNG ----------------------------------------------------------------------------------------------------------------------------------------
def _read_png(path):
    """A reader for what write_png promises: signature, IHDR / IDAT / IEND with correct lengths and CRCs, 8 bit, RGB or grey, filter 0."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(raw):
        (n,) = struct.unpack(">I", raw[at:at + 4])
        tag, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        assert len(data) == n
        (crc,) = struct.unpack(">I", raw[at + 8 + n:at + 12 + n])
        assert crc == (zlib.crc32(tag + data) & 0xffffffff), tag
        chunks.append((tag, data))
        at += 12 + n
    assert at == len(raw) and [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    w, h, depth, ctype, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, interlace) == (8, 0, 0, 0) and ctype in (0, 2)
    nch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(h, 1 + w * nch)
    assert not rows[:, 0].any()          # filter type 0 on every row
    img = rows[:, 1:]
    return img.reshape(h, w, 3) if nch == 3 else img.reshape(h, w)


def _check_png(path, img):
    got = _read_png(path)
    assert got.shape == img.shape and np.array_equal(got, img)
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.array_equal(np.asarray(Image.open(path)), img)


def test_write_png(tmp_path):
    rng = np.random.default_rng(8)
    for name, shape in (("rgb.png", (5, 7, 3)), ("grey.png", (33, 130))):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        cn.write_png(str(tmp_path / name), img)
        _check_png(str(tmp_path / name), img)
    cn.meshio.write_png(str(tmp_path / "t.png"), torch.from_numpy(img))
    _check_png(str(tmp_path / "t.png"), img)
    with pytest.raises(ValueError):
        cn.write_png(str(tmp_path / "bad.png"), img.astype(np.float32))


# ---- 9: validate_image end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_validate_image_end_to_end(backend, tmp_path):
    lib, dev = _lib_and_dev(backend)
    fx = G.load("tiny_sharp")
    ocfg, P = G.weights_of("tiny_sharp", fx)
    r = N.make_renderer(ocfg, P, lib, dev)
    h, w = 12, 10
    c2w, focal, image, _ = cn.synthetic.synthetic_camera(height=h, width=w, device=dev)
    origin, radius = torch.tensor([0.1, -0.05, 0.02]), 1.1
    path = str(tmp_path / "view.png")
    res = cn.validate_image(r, c2w[0], focal, image[0], origin, radius, normalize=True, chunk=32, path=path, library=lib, perturb_overwrite=0)
    assert set(res) == {"color_fine", "depth", "psnr", "ssim", "panel"}
    assert tuple(res["color_fine"].shape) == (h, w, 3) and tuple(res["depth"].shape) == (h, w) and res["color_fine"].device.type == torch.device(dev).type
    # one renderer call on all 120 rays (four chunks of 32, the last one partial: a ray renders identically in every chunk size)
    o, d = cn.rays.get_rays_at(c2w[0], focal, h, w, normalize=True, library=lib)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    o = (o - origin.to(dev)) / torch.tensor(radius, device=dev)
    near, far = cn.rays.near_far_from_sphere(o, d)
    with torch.no_grad():
        out = r(o, d, near, far, perturb_overwrite=0)
    assert torch.equal(_bits(res["color_fine"]), _bits(out["color_fine"].reshape(h, w, 3)))
    assert torch.equal(_bits(res["depth"]), _bits(out["depth"].reshape(h, w)))
    assert res["color_fine"].std().item() > 1e-3          # a picture, not a constant
    m = cn.image_metrics(res["color_fine"], image[0], library=lib)
    assert type(res["psnr"]) is float and res["psnr"] == m["psnr"].item() and res["ssim"] == m["ssim"].item()
    pic = cn.panel(image[0], res["color_fine"], res["depth"], library=lib)
    assert torch.equal(res["panel"], pic) and tuple(pic.shape) == (h, 3 * w, 3)
    _check_png(path, pic.cpu().numpy())
    # [3, H, W] ground truth, no file
    res2 = cn.validate_image(r, c2w[0], focal, image[0].permute(2, 0, 1), origin, radius, chunk=32, library=lib, perturb_overwrite=0)
    assert res2["psnr"] == res["psnr"] and torch.equal(res2["panel"], pic)


# ---- 10 / 11: the C ABI's argument checks; no CPU fallback ---------------------------------------------------------------------------------------------
def test_abi_argument_checks():
    lib = cn.load_library(N.EMU_LIB)
    L = lib.lib
    assert L.cnr_abi_version() == 9
    x = torch.rand(1, 3, 4, 5)
    smap, sums = torch.empty_like(x), torch.full((2,), 7.0, dtype=torch.float64)
    nb = L.cnr_image_scratch_bytes(1, 3, 4, 5)
    assert nb >= 3 * 16 and L.cnr_image_scratch_bytes(0, 3, 4, 5) == 0
    s = torch.empty(nb, dtype=torch.uint8)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert L.cnr_image_metrics(p(x), p(x), 1, 3, 4, 5, 0, p(smap), p(sums), p(s), nb, None) == 0
    assert sums[0].item() == 0.0 and sums[1].item() > 59.9
    assert L.cnr_image_metrics(p(x), p(x), 1, 3, 4, 5, 1, None, p(sums), p(s), nb, None) == 0          # no map
    sums.fill_(7.0)
    assert L.cnr_image_metrics(None, None, 0, 3, 4, 5, 0, None, p(sums), None, 0, None) == 0 and sums.tolist() == [0.0, 0.0]   # n_images == 0
    for args, msg in (((p(x), p(x), 1, 3, 1, 5, 0, p(smap), p(sums), p(s), nb, None), "at least 2"),
                      ((p(x), p(x), 1, 3, 4, 1, 0, p(smap), p(sums), p(s), nb, None), "at least 2"),
                      ((p(x), p(x), 1, 0, 4, 5, 0, p(smap), p(sums), p(s), nb, None), "channels"),
                      ((None, p(x), 1, 3, 4, 5, 0, p(smap), p(sums), p(s), nb, None), "null"),
                      ((p(x), None, 1, 3, 4, 5, 0, p(smap), p(sums), p(s), nb, None), "null"),
                      ((p(x), p(x), 1, 3, 4, 5, 0, p(smap), None, p(s), nb, None), "null"),
                      ((p(x), p(x), 1, 3, 4, 5, 0, p(smap), p(sums), None, nb, None), "null"),
                      ((p(x), p(x), 1, 3, 4, 5, 0, p(smap), p(sums), p(s), nb - 1, None), "scratch"),
                      ((p(x), p(x), 1 << 20, 3, 32, 32, 0, p(smap), p(sums), p(s), nb, None), "2^31"),
                      ((p(x), p(x), 1, 33, 4, 5, 1, p(smap), p(sums), p(s), nb, None), "channels")):
        assert L.cnr_image_metrics(*args) < 0
        assert msg in L.cnr_last_error().decode(), L.cnr_last_error().decode()
    g, d = torch.rand(4, 5, 3), torch.rand(4, 5)
    pic, rng = torch.empty(4, 15, 3, dtype=torch.uint8), torch.empty(2)
    assert L.cnr_image_panel(p(g), p(g), p(d), 4, 5, p(pic), p(rng), p(s), nb, None) == 0
    assert rng.tolist() == [d.min().item(), d.max().item()]
    for args, msg in (((p(g), p(g), None, 4, 5, p(pic), p(rng), p(s), nb, None), "null"), ((p(g), None, p(d), 4, 5, p(pic), p(rng), p(s), nb, None), "null"),
                      ((p(g), p(g), p(d), 4, 5, None, p(rng), p(s), nb, None), "null"), ((p(g), p(g), p(d), 4, 5, p(pic), p(rng), p(s), 4, None), "scratch"),
                      ((p(g), p(g), p(d), 0, 5, p(pic), p(rng), p(s), nb, None), "at least 1"),
                      ((p(g), p(g), p(d), 1 << 15, 1 << 15, p(pic), p(rng), p(s), nb, None), "2^31")):
        assert L.cnr_image_panel(*args) < 0
        assert msg in L.cnr_last_error().decode(), L.cnr_last_error().decode()


def test_cpu_images_need_an_emulation_library():
    """No CPU fallback: CPU tensors with the HIP library (the default) are an error, not a torch computation."""
    if not os.path.isfile(cn.library_path()):
        pytest.skip("HIP library not built")
    x, y = _case("A")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.image_metrics(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.panel(x[0].permute(1, 2, 0), y[0].permute(1, 2, 0), x[0, 0])


# ---- 12: HIP against the emulation at 800 x 800 ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_matches_the_emulation_at_800x800():
    """[1, 3, 800, 800] seeded rand against rand + noise, both layouts: the HIP map bits equal the emulation library's (computed on the CPU
    here), the scalars agree within 1e-9 relative (the two builds order the float64 additions differently), one call on a non-default
    stream gives the same bits; the 800 x 800 panel is bit-identical too."""
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator().manual_seed(800)
    x = torch.rand(1, 3, 800, 800, generator=g)
    y = (x + 0.05 * torch.randn(1, 3, 800, 800, generator=g)).clamp(0.0, 1.0)
    for form in (lambda t: t, lambda t: t[0].permute(1, 2, 0).contiguous()):
        xe, ye = form(x), form(y)
        emu = cn.image_metrics(xe, ye, return_map=True, library=N.EMU_LIB)
        xd, yd = xe.cuda(), ye.cuda()
        hip = cn.image_metrics(xd, yd, return_map=True)
        assert torch.equal(_bits(hip["ssim_map"]), _bits(emu["ssim_map"])), int((_bits(hip["ssim_map"]) != _bits(emu["ssim_map"])).sum())
        for k in ("mse", "ssim", "psnr"):
            a, b = hip[k].item(), emu[k].item()
            print(f"{k}: hip {a:.17g} emu {b:.17g} relative {abs(a - b) / abs(b):.2e}")
            assert abs(a - b) <= 1e-9 * abs(b)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            again = cn.image_metrics(xd, yd, return_map=True)
        side.synchronize()
        assert torch.equal(_bits(again["ssim_map"]), _bits(emu["ssim_map"]))
        assert again["mse"].item() == hip["mse"].item() and again["ssim"].item() == hip["ssim"].item()
    gt, render = x[0].permute(1, 2, 0).contiguous(), y[0].permute(1, 2, 0).contiguous()
    depth = 1.5 + torch.randn(800, 800, generator=g)
    depth[17, 400] = float("nan")
    pe = cn.panel(gt, render, depth, library=N.EMU_LIB)
    ph = cn.panel(gt.cuda(), render.cuda(), depth.cuda())
    assert tuple(ph.shape) == (800, 2400, 3) and torch.equal(ph.cpu(), pe)
    assert torch.equal(cn.cmap(depth.cuda()).cpu(), pe[:, 1600:])
