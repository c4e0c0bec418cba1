"""Culling an extracted mesh against the views (cnr_mask_dilate / cnr_mesh_view_votes / cnr_mesh_cull_select; color_neus_amd.meshops
dilate_masks / view_votes / cull_mesh / MeshCuller, NeuSRenderer.extract_geometry / render_mesh_view with ``cull=``).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The reference project has no
counterpart, so the yardsticks are written here and use nothing from the library:

  NP    the specification of include/colorneus_render.h restated in numpy: the box dilation from a summed-area table, the packing by shifts,
        the votes with float32 for the float steps (every numpy operation on float32 arrays is one IEEE rounding) and int64 for the integer
        steps -- the recipe of tests/test_mesh_raster.py's S32 --, the selection with boolean indexing.  Everything is compared BITWISE.
  MP    F.max_pool2d(fg, 2 r + 1, 1, r) > 0: torch's own box dilation.
  F64   the votes' classification in float64 from the project's rays.get_rays_at camera model, compared away from the rounding boundaries.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import color_neus_amd as cn
from color_neus_amd import _lib, meshops
import _golden as G
import _guard
import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
f32 = np.float32
SCAN_CHUNK = 8192      # cnr_meshcc.h: kMeshScanThreads * kMeshScanPer, one trip of the carried scan both selections share
ALL, ANY = 0, 1


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return cn.load_library(N.EMU_LIB), "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return cn.load_library(), "cuda:0"


def _np(t):
    return t.detach().cpu().contiguous().numpy()


# ---- NP: masks -----------------------------------------------------------------------------------------------------------------------------
def _np_dilate(fg, r):
    """fg bool [N, H, W] -> bool [N, H, W]: a pixel is set iff its (2 r + 1)^2 box, clipped to the image, holds a foreground pixel"""
    n, H, W = fg.shape
    S = np.zeros((n, H + 1, W + 1), np.int64)
    S[:, 1:, 1:] = fg.astype(np.int64).cumsum(1).cumsum(2)
    j, i = np.arange(H), np.arange(W)
    j0, j1 = np.maximum(j - r, 0), np.minimum(j + r, H - 1) + 1
    i0, i1 = np.maximum(i - r, 0), np.minimum(i + r, W - 1) + 1
    box = S[:, j1][:, :, i1] - S[:, j0][:, :, i1] - S[:, j1][:, :, i0] + S[:, j0][:, :, i0]
    return box > 0


def _np_pack(b):
    """bool [N, H, W] -> uint64 [N, H, Wq]: bit b of word k is pixel 64 k + b, the pad bits zero"""
    n, H, W = b.shape
    Wq = (W + 63) // 64
    p = np.zeros((n, H, Wq * 64), np.uint64)
    p[:, :, :W] = b
    return (p.reshape(n, H, Wq, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def _raw_dilate(lib, dev, masks, r, guard):
    """cnr_mask_dilate on exact-size poisoned guarded buffers; returns the packed result as uint64 [N, H, Wq]"""
    m = torch.from_numpy(np.ascontiguousarray(masks, f32)).to(dev)
    n, H, W = m.shape
    Wq = (W + 63) // 64
    src = guard.copy(m)
    row_bits, bits = guard.empty((n, H, Wq), torch.int64, dev), guard.empty((n, H, Wq), torch.int64, dev)
    lib.call("cnr_mask_dilate", guard.addr(src), n, H, W, r, guard.addr(row_bits), guard.addr(bits), _lib.stream_of(torch.device(dev)))
    guard.check()
    return _np(bits).view(np.uint64)


def _mask_inputs(n, H, W):
    """the stacks of one shape: single foreground pixels at the word borders and the image's corners (image 0), a random 2 % stack, and one
    with values that are background (-1, NaN, -0.0, 0) or foreground (+inf, 1e-30) by the rule mask > 0"""
    g = np.random.default_rng(1000 * n + 10 * H + W)
    out = []
    for k, c in enumerate(sorted({c for c in (0, 63, 64, W - 1) if c < W})):
        m = np.zeros((n, H, W), f32)
        m[0, (0, H - 1)[k % 2], c] = 1.0
        out.append(("pixel r%d c%d" % ((0, H - 1)[k % 2], c), m))
    m = np.zeros((n, H, W), f32)
    m[0, H - 1, 0] = 2.0
    m[0, 0, W - 1] = 0.5
    out.append(("corners", m))
    out.append(("random", (g.random((n, H, W)) < 0.02).astype(f32)))
    vals = np.array([-1.0, np.nan, np.inf, 1e-30, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], f32)
    flat = vals[np.arange(n * H * W) % len(vals)]                    # every kind is present from 4 pixels on; shuffled where there is room
    out.append(("special", (g.permutation(flat) if flat.size >= 2 * len(vals) else flat).reshape(n, H, W)))
    return out


@pytest.mark.parametrize("W", [5, 63, 64, 65, 70, 129])
@pytest.mark.parametrize("backend", BACKENDS)
def test_dilation_is_the_box_of_the_definition(backend, W):
    """word for word, pad bits included, against NP and MP; image 1 of a stack of three stays empty when image 0 holds a pixel in its last
    row; the guards of row_bits and bits are intact (checked inside _raw_dilate)"""
    lib, dev = _lib_and_dev(backend)
    for H in (1, 3, 17):
        for n in (1, 3):
            for name, m in _mask_inputs(n, H, W):
                with np.errstate(invalid="ignore"):
                    fg = m > 0
                if name == "special":
                    assert fg.any() and np.isnan(m).any() and (m < 0).any() and fg.sum() == (np.isinf(m) | (m == f32(1e-30))).sum()
                for r in (0, 1, 2, 63, 64, 65, W, W + 70):
                    what = (name, n, H, W, r)
                    want = _np_dilate(fg, r)
                    mp = F.max_pool2d(torch.from_numpy(fg.astype(f32)), 2 * r + 1, 1, r).numpy() > 0
                    assert np.array_equal(want, mp), what
                    got = _raw_dilate(lib, dev, m, r, _guard.Guard(0xFF if (r + n) % 2 else 0x00))
                    assert got.dtype == np.uint64 and np.array_equal(got, _np_pack(want)), what
                    if r == 0:
                        assert np.array_equal(got, _np_pack(fg)), what
                    if n == 3 and not fg[1].any():
                        assert not got[1].any(), what
                    vm = meshops.dilate_masks(torch.from_numpy(m).to(dev), r, library=lib)
                    assert np.array_equal(_np(vm.bits).view(np.uint64), got) and np.array_equal(_np(vm.to_bool()), want), what


# ---- NP: votes -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere(levels=2, radius=0.5):
    """An octahedron subdivided `levels` times onto the sphere of `radius`: (66 vertices, 128 triangles) at 2, (4098, 8192) at 5"""
    V = [np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    Fc = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = V[a] + V[b]
                V.append(m / np.linalg.norm(m))
                cache[k] = len(V) - 1
            return cache[k]
        for a, b, c in Fc:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        Fc = nf
    V, Fc = (np.array(V) * radius).astype(f32), np.array(Fc, dtype=np.int32)
    V.setflags(write=False)
    Fc.setflags(write=False)
    return V, Fc


def _camera(seed, opengl=False, dist=3.0):
    """c2w (float32 [4, 4]) on the sphere of radius `dist`, looking at the origin, a random orthonormal rotation from a seeded QR"""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    c2w = np.eye(4)
    c2w[:3, 3] = -dist * Q[:, 2]
    if opengl:
        Q = Q * np.array([1.0, -1.0, -1.0])
    c2w[:3, :3] = Q
    return c2w.astype(f32)


def _look_at(eye, up=(0.0, 0.0, 1.0)):
    """c2w (float32) of a camera at `eye` looking at the origin; columns right / down / forward"""
    eye = np.asarray(eye, float)
    fwd = -eye / np.linalg.norm(eye)
    up = np.asarray(up, float) if abs(fwd @ np.asarray(up, float)) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return c2w.astype(f32)


def _np_votes(V, c2w, focal, H, W, opengl=False, origin=None, radius=1.0, z_near=1e-3, mask=None, depth=None, tol=0.0):
    """counts int32 [V, 4] and the per-view `usable` flags of the header's definition.  c2w [n, 4, 4], focal [n, 2], mask bool [n, H, W] or
    None, depth float32 [n, H, W] or None"""
    V, c2w, focal = np.asarray(V, f32).reshape(-1, 3), np.asarray(c2w, f32), np.asarray(focal, f32)
    counts = np.zeros((len(V), 4), np.int64)
    usable_all = []
    for n in range(len(c2w)):
        R, t = c2w[n, :3, :3], c2w[n, :3, 3]
        if origin is not None:
            t = (t - np.asarray(origin, f32)) / f32(radius)
        fx, fy = focal[n]
        with np.errstate(all="ignore"):
            d = V - t
            xc, yc, zc = [(R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2] for k in range(3)]
            if opengl:
                yc, zc = -yc, -zc
            u = (fx * xc) / zc + f32(W) * f32(0.5)
            v = (fy * yc) / zc + f32(H) * f32(0.5)
            usable = (zc > f32(z_near)) & (np.abs(u) < f32(2 ** 21)) & (np.abs(v) < f32(2 ** 21))
            X = np.where(usable, np.rint(np.where(usable, u, 0) * f32(256)), 0).astype(np.int64)
            Y = np.where(usable, np.rint(np.where(usable, v, 0) * f32(256)), 0).astype(np.int64)
        i, j = (X + 128) >> 8, (Y + 128) >> 8
        seen = usable & (i >= 0) & (i < W) & (j >= 0) & (j < H)
        ic, jc = np.clip(i, 0, W - 1), np.clip(j, 0, H - 1)
        inside = seen & (mask[n, jc, ic] if mask is not None else True)
        if depth is not None:
            with np.errstate(all="ignore"):
                hidden = zc > depth[n, jc, ic] * (f32(1.0) + f32(tol))
            visible = seen & ~hidden
        else:
            visible = seen
        counts += np.stack([np.ones(len(V), bool), seen, inside, visible], 1)
        usable_all.append(usable)
    return counts.astype(np.int32), np.array(usable_all)


def _raw_votes(lib, dev, V, c2w, focal, H, W, opengl=False, origin=None, radius=1.0, z_near=1e-3, bits=None, depth=None, tol=0.0, guard=None,
               counts=None, n_vertices=None):
    """cnr_mesh_view_votes on guarded inputs; `counts`: a guarded tensor to add to (made here, zeroed, when None).  Returns that tensor."""
    guard = guard if guard is not None else _guard.Guard()
    t = lambda a, dt=f32: guard.copy(torch.from_numpy(np.ascontiguousarray(a, dt)).to(dev))
    v, cam, foc = t(np.asarray(V, f32).reshape(-1, 3)), t(c2w), t(focal)
    org = t(origin) if origin is not None else None
    b = guard.copy(torch.from_numpy(np.ascontiguousarray(bits).view(np.int64)).to(dev)) if bits is not None else None
    d = t(depth) if depth is not None else None
    if counts is None:
        counts = guard.empty((v.shape[0], 4), torch.int32, dev)
        counts.zero_()
    a = lambda x: guard.addr(x) if x is not None else C.c_void_p(0)
    lib.call("cnr_mesh_view_votes", a(v), v.shape[0] if n_vertices is None else n_vertices, a(cam), a(foc), a(org), float(radius), float(z_near),
             int(opengl), cam.shape[0], H, W, a(b), a(d), float(tol), guard.addr(counts), _lib.stream_of(torch.device(dev)))
    guard.check()
    return counts


def _vote_scene(H, W, opengl, with_origin):
    """the 66-vertex sphere, four vertices no camera 0 can use, 5 cameras, a random mask stack and depth maps with NaN pixels"""
    g = np.random.default_rng(7 * H + W + opengl)
    origin, radius = ((0.05, -0.02, 0.03), 1.25) if with_origin else (None, 1.0)
    c2w = np.stack([_camera(s, opengl) for s in (1, 2, 3, 4, 5)])
    if with_origin:      # the cameras stay where they were in the mesh's frame: centre' = centre * radius + origin
        c2w[:, :3, 3] = c2w[:, :3, 3] * f32(radius) + np.asarray(origin, f32)
    focal = np.stack([(150.0 + 3 * k, 140.0 - 2 * k) for k in range(5)]).astype(f32) * f32(min(H, W) / 72.0)
    sph, _ = _sphere()
    eye = (c2w[0, :3, 3].astype(float) - (np.asarray(origin) if with_origin else 0.0)) / radius
    fwd = c2w[0, :3, 2].astype(float) * (-1.0 if opengl else 1.0)
    right = c2w[0, :3, 0].astype(float)
    extra = np.array([[np.nan, 0.0, 0.0], eye - fwd, eye + 0.5e-3 * fwd, eye + 1e-2 * fwd + 1e4 * right, [0.0, np.inf, 0.0]], f32)
    V = np.concatenate([sph, extra])
    mask = g.random((5, H, W)) < 0.5
    depth = g.uniform(2.4, 3.6, (5, H, W)).astype(f32)
    depth[g.random((5, H, W)) < 0.2] = np.nan
    return V, c2w, focal, origin, radius, mask, depth


@pytest.mark.parametrize("with_origin", [False, True])
@pytest.mark.parametrize("opengl", [False, True])
@pytest.mark.parametrize("shape", [(72, 96), (7, 70)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_votes_are_the_bits_of_the_definition(backend, shape, opengl, with_origin):
    lib, dev = _lib_and_dev(backend)
    H, W = shape
    V, c2w, focal, origin, radius, mask, depth = _vote_scene(H, W, opengl, with_origin)
    kw = dict(opengl=opengl, origin=origin, radius=radius)
    tol = 0.01
    want, usable = _np_votes(V, c2w, focal, H, W, mask=mask, depth=depth, tol=tol, **kw)
    assert not usable[0, 66:].any() and usable[:, :66].all()                  # the four special vertices and the two non-finite ones
    assert (want[:66, 1] > 0).all() and len(np.unique(want[:66, 2])) > 2 and len(np.unique(want[:66, 3])) > 2
    got = _raw_votes(lib, dev, V, c2w, focal, H, W, bits=_np_pack(mask), depth=depth, tol=tol, **kw)
    assert got.dtype == torch.int32 and np.array_equal(_np(got), want)
    # two calls with disjoint view subsets into one counts = one call; the rows of a second region stay as they were
    guard = _guard.Guard()
    counts = guard.empty((len(V) + 9, 4), torch.int32, dev)
    counts[:len(V)].zero_()
    counts[len(V):].fill_(-77)
    for sl in (slice(0, 2), slice(2, 5)):
        _raw_votes(lib, dev, V, c2w[sl], focal[sl], H, W, bits=_np_pack(mask[sl]), depth=depth[sl], tol=tol, guard=guard, counts=counts,
                   n_vertices=len(V), **kw)
    assert np.array_equal(_np(counts)[:len(V)], want) and (_np(counts)[len(V):] == -77).all()
    # without masks and depth maps columns 1, 2 and 3 are equal
    plain = _np(_raw_votes(lib, dev, V, c2w, focal, H, W, **kw))
    assert np.array_equal(plain, _np_votes(V, c2w, focal, H, W, **kw)[0])
    assert np.array_equal(plain[:, 1], plain[:, 2]) and np.array_equal(plain[:, 1], plain[:, 3]) and (plain[:, 0] == 5).all()
    # each alone
    only_mask = _np(_raw_votes(lib, dev, V, c2w, focal, H, W, bits=_np_pack(mask), **kw))
    assert np.array_equal(only_mask, _np_votes(V, c2w, focal, H, W, mask=mask, **kw)[0]) and np.array_equal(only_mask[:, 1], only_mask[:, 3])
    only_depth = _np(_raw_votes(lib, dev, V, c2w, focal, H, W, depth=depth, tol=tol, **kw))
    assert np.array_equal(only_depth, _np_votes(V, c2w, focal, H, W, depth=depth, tol=tol, **kw)[0])
    # the Python entry gives the same counts
    vm = meshops.ViewMasks(torch.from_numpy(_np_pack(mask).view(np.int64)).to(dev), H, W, 0)
    py = meshops.view_votes(torch.from_numpy(V).to(dev), torch.from_numpy(c2w).to(dev), torch.from_numpy(focal).to(dev), H, W, masks=vm,
                            depth=torch.from_numpy(depth).to(dev), depth_tol=tol, library=lib, **kw)
    assert np.array_equal(_np(py), want)


@pytest.mark.parametrize("shape", [(72, 96), (7, 70)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rounding_and_image_bounds(backend, shape):
    """the identity camera with focal 128 projects ((U - W / 2) z / 128, (Vp - H / 2) z / 128, z) exactly onto (U, Vp) at z = 2: pixel centres
    sit at integers, so -0.5 rounds to pixel 0 (seen), -0.5 - 1/128 to -1 (not), W - 0.5 - 1/256 to W - 1 (seen), W - 0.5 to W (not)"""
    lib, dev = _lib_and_dev(backend)
    H, W = shape
    us = [(-0.5, True), (-0.5 - 1 / 128, False), (W - 0.5 - 1 / 256, True), (W - 0.5, False), (W / 2 + 0.25, True)]
    vs = [(-0.5, True), (-0.5 - 1 / 128, False), (H - 0.5 - 1 / 256, True), (H - 0.5, False), (H / 2 - 0.25, True)]
    pts, seen, pix = [], [], []
    for u, uok in us:
        for v, vok in vs:
            pts.append([(u - W * 0.5) * 2.0 / 128.0, (v - H * 0.5) * 2.0 / 128.0, 2.0])
            seen.append(uok and vok)
            pix.append((int(np.floor(v + 0.5)), int(np.floor(u + 0.5))))
    pts = np.array(pts, f32)
    assert np.array_equal(pts.astype(float), np.array(pts, float))
    c2w, focal = np.eye(4, dtype=f32)[None], np.array([[128.0, 128.0]], f32)
    got = _np(_raw_votes(lib, dev, pts, c2w, focal, H, W))
    assert np.array_equal(got[:, 1], np.array(seen, np.int32)) and np.array_equal(got, _np_votes(pts, c2w, focal, H, W)[0])
    # the mask bit read is the one of that pixel: a mask with exactly the seen vertices' pixels cleared
    mask = np.ones((1, H, W), bool)
    for (j, i), s in zip(pix, seen):
        if s:
            mask[0, j, i] = False
    got = _np(_raw_votes(lib, dev, pts, c2w, focal, H, W, bits=_np_pack(mask)))
    assert np.array_equal(got[:, 1], np.array(seen, np.int32)) and not got[:, 2].any()
    got = _np(_raw_votes(lib, dev, pts, c2w, focal, H, W, bits=_np_pack(~mask)))
    assert np.array_equal(got[:, 2], np.array(seen, np.int32))
    # a NaN depth pixel hides nothing; a depth just below z / (1 + tol) hides, the depth z itself does not
    for d, vis in ((np.nan, True), (2.0, True), (1.7, False), (2.0 / 1.125 + 1e-3, True), (2.0 / 1.125 - 1e-3, False)):
        got = _np(_raw_votes(lib, dev, pts, c2w, focal, H, W, depth=np.full((1, H, W), d, f32), tol=0.125))
        assert np.array_equal(got[:, 3], np.array(seen, np.int32) * int(vis)), d


@pytest.mark.parametrize("backend", BACKENDS)
def test_votes_against_float64_rays(backend):
    """F64.  get_rays_at(normalize=False) gives the rays o, d(i, j) of a pinhole camera: d is affine in (i, j), so three rays give
    d = d00 + i di + j dj, and P - o = s (d00 + u di + v dj) is a 3 x 3 linear system for (s, s u, s v): the pixel coordinates (u, v) and the
    camera depth s of P in float64, with nothing of the rasteriser's vertex stage.  The library snaps to 1/256 pixel from float32 (error
    below 1/512 + 1e-3 pixel), so vertices further than 1/64 pixel from a rounding boundary (u + 0.5 or v + 0.5 an integer) in both axes must
    classify the same; with a uniform fractional part 2 * 2/64 = 6 % of them lie nearer, and at most 10 % may.  The depth maps hold 0.5 or
    2 times the scene's depth: far from the threshold whatever the rounding."""
    lib, dev = _lib_and_dev(backend)
    H, W = 72, 96
    g = np.random.default_rng(5)
    pts = g.normal(size=(600, 3))
    pts = (pts / np.linalg.norm(pts, axis=1, keepdims=True) * g.uniform(0.0, 1.0, (600, 1)) ** (1 / 3) * 1.1).astype(f32)
    for seed, opengl in ((11, False), (12, True), (13, False)):
        c2w = _camera(seed, opengl)
        focal = np.array([130.0, 120.0], f32)
        o, d = cn.rays.get_rays_at(torch.from_numpy(c2w), torch.from_numpy(focal), H, W, normalize=False, opengl=opengl, library=N.EMU_LIB)
        o, d = o.double().numpy(), d.double().numpy()
        M = np.stack([d[0, 0], d[0, 1] - d[0, 0], d[1, 0] - d[0, 0]], 1)      # d[j][i]: columns d00, di, dj
        sol = np.linalg.solve(M, (pts.astype(float) - o[0, 0]).T).T
        s, u, v = sol[:, 0], sol[:, 1] / sol[:, 0], sol[:, 2] / sol[:, 0]
        near = lambda x: np.abs((x + 0.5) - np.rint(x + 0.5)) <= 1 / 64
        left_out = near(u) | near(v)
        assert left_out.mean() <= 0.10, left_out.mean()
        i, j = np.floor(u + 0.5).astype(int), np.floor(v + 0.5).astype(int)
        seen = (s > 1e-3) & (i >= 0) & (i < W) & (j >= 0) & (j < H)
        assert 0.3 < seen.mean() < 0.98
        mask = g.random((1, H, W)) < 0.5
        depth = (3.0 * np.where(g.random((1, H, W)) < 0.5, 0.5, 2.0)).astype(f32)
        ic, jc = np.clip(i, 0, W - 1), np.clip(j, 0, H - 1)
        want = np.stack([np.ones(600, bool), seen, seen & mask[0, jc, ic], seen & ~(s > depth[0, jc, ic].astype(float) * 1.01)], 1).astype(np.int32)
        got = _np(_raw_votes(lib, dev, pts, c2w[None], focal[None], H, W, opengl=opengl, bits=_np_pack(mask), depth=depth, tol=0.01))
        assert np.array_equal(got[~left_out], want[~left_out])
        assert 0 < want[:, 2].sum() < want[:, 1].sum() and 0 < want[:, 3].sum() < want[:, 1].sum()


# ---- the visual hull and the visibility test on scenes with a known answer -------------------------------------------------------------------------
HULL_H, HULL_W, HULL_F = 72, 96, 120.0


@functools.lru_cache(maxsize=None)
def _hull_scene():
    """the small sphere (radius 0.1 around (0.55, 0.55, 0)) FIRST, then the sphere of radius 0.5: a result that equals the big sphere is
    renumbered.  Six cameras on the axes at distance 3.  From +-z the small sphere projects 31 pixels from the centre, the big one's
    silhouette has a radius of 20.3: more than 6 pixels of background between them."""
    bv, bt = _sphere()
    sv = (bv * f32(0.2) + np.array([0.55, 0.55, 0.0], f32)).astype(f32)
    V, T = np.concatenate([sv, bv]), np.concatenate([bt, bt + 66]).astype(np.int32)
    c2w = np.stack([_look_at(e) for e in ((3, 0, 0), (-3, 0, 0), (0, 3, 0), (0, -3, 0), (0, 0, 3), (0, 0, -3))])
    return V, T, bv, bt, c2w


def _silhouettes(lib, dev, bv, bt, c2w, H, W, focal):
    foc = torch.tensor([focal, focal], device=dev)
    return torch.stack([cn.rasterize_mesh(torch.from_numpy(bv.copy()).to(dev), torch.from_numpy(bt.copy()).to(dev), torch.from_numpy(c).to(dev), foc, H, W,
                                          library=lib)["tri_id"] >= 0 for c in c2w])


@pytest.mark.parametrize("backend", BACKENDS)
def test_visual_hull_keeps_the_object_and_drops_what_is_beside_it(backend):
    lib, dev = _lib_and_dev(backend)
    V, T, bv, bt, c2w = _hull_scene()
    masks = _silhouettes(lib, dev, bv, bt, c2w, HULL_H, HULL_W, HULL_F)
    assert masks.dtype == torch.bool and 0.1 < float(masks.float().mean()) < 0.5
    tv, tt, cams = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(c2w).to(dev)
    col = torch.from_numpy(np.random.default_rng(3).random((132, 3)).astype(f32)).to(dev)
    ov, ot, oc, info = meshops.cull_mesh(tv, tt, cams, [HULL_F, HULL_F], HULL_H, HULL_W, masks=masks, colors=col, dilation=2, max_outside=0,
                                         library=lib)
    kv = _np(info["keep_vertex"])
    assert kv[66:].all() and not kv[:66].any() and _np(info["keep_face"])[128:].all() and not _np(info["keep_face"])[:128].any()
    assert np.array_equal(_np(ov).view(np.int32), bv.view(np.int32)) and np.array_equal(_np(ot), bt) and ot.dtype == torch.int32
    assert np.array_equal(_np(oc).view(np.int32), _np(col)[66:].view(np.int32))
    assert info["n_vertices"] == 66 and info["n_faces"] == 128 and info["dropped"] == 0 and info["n_views"] == 6
    counts = _np(info["counts"])
    assert (counts[:, 0] == 6).all() and (counts[66:, 1] == 6).all() and (counts[66:, 2] == 6).all() and (counts[:66, 1] > counts[:66, 2]).all()
    # a prepared culler with resident masks gives the same result, for this mesh and again
    culler = meshops.MeshCuller(cams, [HULL_F, HULL_F], HULL_H, HULL_W, masks=meshops.dilate_masks(masks, 2, library=lib), library=lib)
    for _ in range(2):
        cv, ct, cc, cinfo = culler(tv, tt, col)
        assert torch.equal(cv, ov) and torch.equal(ct, ot) and torch.equal(cc, oc) and torch.equal(cinfo["counts"], info["counts"])

    # dilation 0: the silhouette vertices round to pixels outside the undilated masks; "any" keeps at least what "all" keeps, and every
    # face obeys its rule against the counts
    kept = {}
    for rule in ("all", "any"):
        _, rt, _, rinfo = meshops.cull_mesh(tv, tt, cams, [HULL_F, HULL_F], HULL_H, HULL_W, masks=masks, dilation=0, faces=rule, library=lib)
        c = _np(rinfo["counts"])
        passes = (c[:, 1] >= 1) & (c[:, 1] - c[:, 2] <= 0)
        per_face = passes[T]
        want = per_face.all(1) if rule == "all" else per_face.any(1)
        assert np.array_equal(_np(rinfo["keep_face"]), want) and rt.shape[0] == want.sum() == rinfo["n_faces"]
        used = np.zeros(132, bool)
        used[T[want].reshape(-1)] = True
        assert np.array_equal(_np(rinfo["keep_vertex"]), used)
        kept[rule] = int(want.sum())
    assert 0 < kept["all"] < kept["any"] <= 128


VIS_H, VIS_W, VIS_F, VIS_D, VIS_R, VIS_TOL = 144, 192, 300.0, 3.0, 0.5, 0.02


@pytest.mark.parametrize("backend", BACKENDS)
def test_visibility_against_the_facing_of_a_sphere(backend):
    """One camera at distance D = 3 from the sphere of radius R = 0.5 (4098 vertices, a convex polyhedron inscribed in it), focal f = 300,
    depth_tol = 0.02.  g = n . (cam - v) / |cam - v|, n = v / |v|, in float64.  The band around g = 0 in which nothing is asserted:

      a   = (sqrt(2) / 2) (D + R) / f (1 + 2 R / (D - R)): the largest distance between a vertex and the ray through its nearest pixel
            centre (half a pixel's diagonal at the largest depth), with the allowance 2 R a / z for treating that ray and the vertex's own
            ray as parallel across the sphere
      front, g >= band must PASS.  The polyhedron lies inside the ball, so the depth the z-buffer holds at the pixel is at least the depth at
            which the pixel's ray enters the ball.  In the plane of the two rays the ball is a circle of radius R' <= R on which the vertex
            has a cosine g' >= g; the entry depth of a ray displaced by a is sqrt(R'^2 g'^2 + 2 a R') - R' g' <= a / g' <= a / g nearer than
            the vertex.  The vertex passes when a / g <= depth_tol (D - R):   g >= a / (depth_tol (D - R))
      back, g <= -band must FAIL.  The vertex's own ray has crossed the ball on a chord of 2 R |g|; the displaced ray enters at most a / |g|
            later, and the polyhedron at most s / |g| behind the ball, s = e^2 / (2 R) bounding the sagitta of a facet whose longest edge is e
            (measured on the mesh below).  The vertex fails when 2 R |g| - (a + s) / |g| > depth_tol (D + R), the right side bounding
            depth_tol times the z-buffer's depth:   |g| >= (T + sqrt(T^2 + 8 R (a + s))) / (4 R),  T = depth_tol (D + R)
    The band is the larger of the two; at most 25 % of the vertices may lie in it (g is close to uniform on [-1, 1])."""
    lib, dev = _lib_and_dev(backend)
    V, T = _sphere(5)
    assert V.shape == (4098, 3)
    Vd = V.astype(float)
    e = max(np.linalg.norm(Vd[T[:, a]] - Vd[T[:, b]], axis=1).max() for a, b in ((0, 1), (1, 2), (2, 0)))
    D, R, tol = VIS_D, VIS_R, VIS_TOL
    a = np.sqrt(0.5) * (D + R) / VIS_F * (1 + 2 * R / (D - R))
    s = e * e / (2 * R)
    Tz = tol * (D + R)
    band = max(a / (tol * (D - R)), (Tz + np.sqrt(Tz * Tz + 8 * R * (a + s))) / (4 * R))
    eye = np.array([1.0, 2.0, 2.0]) / 3.0 * D
    to_cam = eye - Vd
    g = (Vd / np.linalg.norm(Vd, axis=1, keepdims=True) * to_cam).sum(1) / np.linalg.norm(to_cam, axis=1)
    left_out = np.abs(g) < band
    assert left_out.mean() <= 0.25 and (g >= band).sum() > 1000 and (g <= -band).sum() > 1000, (band, left_out.mean())
    tv, tt, cam = torch.from_numpy(V.copy()).to(dev), torch.from_numpy(T.copy()).to(dev), torch.from_numpy(_look_at(eye)).to(dev)[None]
    ov, ot, _, info = meshops.cull_mesh(tv, tt, cam, [VIS_F, VIS_F], VIS_H, VIS_W, visibility=True, depth_tol=tol, library=lib)
    counts = _np(info["counts"])
    assert (counts[:, 0] == 1).all() and (counts[:, 1] == 1).all() and (counts[:, 2] == 1).all()
    assert (counts[g >= band, 3] == 1).all() and (counts[g <= -band, 3] == 0).all()
    # the selection follows the counts: all three corners visible
    want = (counts[:, 3] >= 1)[T].all(1)
    assert np.array_equal(_np(info["keep_face"]), want) and ot.shape[0] == want.sum() and 0 < want.sum() < len(T)
    # the chunked path (two views, one per chunk, and both in one chunk) votes like view_votes on rasterize_mesh's depth maps
    cams = torch.cat([cam, torch.from_numpy(_look_at(-eye)).to(dev)[None]])
    depth = torch.stack([cn.rasterize_mesh(tv, tt, c, torch.tensor([VIS_F, VIS_F], device=dev), VIS_H, VIS_W, library=lib)["depth"] for c in cams])
    ref = meshops.view_votes(tv, cams, [VIS_F, VIS_F], VIS_H, VIS_W, depth=depth, depth_tol=tol, library=lib)
    assert bool(torch.isnan(depth).any())
    for chunk in (1, 8):
        info2 = meshops.cull_mesh(tv, tt, cams, [VIS_F, VIS_F], VIS_H, VIS_W, visibility=True, depth_tol=tol, view_chunk=chunk, library=lib)[3]
        assert torch.equal(info2["counts"], ref)
    # a depth map without a surface anywhere: every seen vertex counts as visible
    nan = torch.full_like(depth, float("nan"))
    c = _np(meshops.view_votes(tv, cams, [VIS_F, VIS_F], VIS_H, VIS_W, depth=nan, depth_tol=tol, library=lib))
    assert np.array_equal(c[:, 3], c[:, 1]) and (c[:, 1] == 2).all()


# ---- NP: selection and compaction ------------------------------------------------------------------------------------------------------------------
def _np_select(tris, V, counts, min_views, max_outside, min_visible, rule):
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    counts = np.asarray(counts, np.int64).reshape(V, 4)
    passes = (counts[:, 1] >= min_views) & (counts[:, 1] - counts[:, 2] <= max_outside) & (counts[:, 3] >= min_visible)
    valid = ((tris >= 0) & (tris < V)).all(1) if len(tris) else np.zeros(0, bool)
    keep_face = np.zeros(len(tris), bool)
    if valid.any():
        pf = passes[tris[valid]]
        keep_face[valid] = pf.any(1) if rule == ANY else pf.all(1)
    keep_vertex = np.zeros(V, bool)
    keep_vertex[tris[keep_face].reshape(-1)] = True
    return {"keep_vertex": keep_vertex.astype(np.uint8), "keep_face": keep_face.astype(np.uint8),
            "vertex_map": np.where(keep_vertex, np.cumsum(keep_vertex) - 1, -1).astype(np.int32),
            "face_map": np.where(keep_face, np.cumsum(keep_face) - 1, -1).astype(np.int32),
            "totals": np.array([keep_vertex.sum(), keep_face.sum()], np.int32), "dropped": np.array([(~valid).sum()], np.int32)}


def _raw_select(lib, dev, tris, V, counts, min_views=1, max_outside=0, min_visible=0, rule=ALL, verts=None, cols=None, fill=0xFF):
    """cnr_mesh_cull_select, then (with verts) cnr_mesh_compact, every buffer exact-size, poisoned and guarded; numpy arrays by name"""
    guard = _guard.Guard(fill)
    t = guard.copy(torch.from_numpy(np.ascontiguousarray(np.asarray(tris, np.int32).reshape(-1, 3))).to(dev))
    c = guard.copy(torch.from_numpy(np.ascontiguousarray(np.asarray(counts, np.int32).reshape(V, 4))).to(dev))
    Fn = t.shape[0]
    i32, u8 = torch.int32, torch.uint8
    o = {"keep_vertex": guard.empty(V, u8, dev), "keep_face": guard.empty(Fn, u8, dev), "vertex_map": guard.empty(V, i32, dev),
         "face_map": guard.empty(Fn, i32, dev), "totals": guard.empty(2, i32, dev), "dropped": guard.empty(1, i32, dev)}
    a, stream = guard.addr, _lib.stream_of(torch.device(dev))
    lib.call("cnr_mesh_cull_select", a(t), Fn, V, a(c), min_views, max_outside, min_visible, rule, a(o["keep_vertex"]), a(o["keep_face"]),
             a(o["vertex_map"]), a(o["face_map"]), a(o["totals"]), a(o["dropped"]), stream)
    if verts is not None:
        nv, nf = (int(x) for x in o["totals"].tolist())
        v = guard.copy(torch.from_numpy(np.asarray(verts, f32).reshape(V, 3)).to(dev))
        cl = guard.copy(torch.from_numpy(np.asarray(cols, f32).reshape(V, 3)).to(dev))
        o["out_vertices"], o["out_colors"], o["out_triangles"] = guard.empty((nv, 3), torch.float32, dev), guard.empty((nv, 3), torch.float32, dev), \
            guard.empty((nf, 3), i32, dev)
        lib.call("cnr_mesh_compact", a(v), a(cl), a(t), Fn, V, a(o["vertex_map"]), a(o["face_map"]), a(o["out_vertices"]), a(o["out_colors"]),
                 a(o["out_triangles"]), stream)
    guard.check()
    return {k: _np(x).copy() for k, x in o.items()}


def _random_counts(g, V, n_views=6):
    seen = g.integers(0, n_views + 1, V)
    inside = (g.random(V) * (seen + 1)).astype(np.int64)
    visible = (g.random(V) * (seen + 1)).astype(np.int64)
    return np.stack([np.full(V, n_views), seen, np.minimum(inside, seen), np.minimum(visible, seen)], 1).astype(np.int32)


def _random_mesh(g, V, Fn):
    """random triangles with repeated corners, duplicates and indices outside [0, V)"""
    t = g.integers(0, V, (Fn, 3)).astype(np.int64)
    k = max(1, Fn // 20)
    t[g.integers(0, Fn, k), g.integers(0, 3, k)] = g.choice([-1, V, V + 5, 2 ** 31 - 1, -2 ** 31], k)
    deg = g.integers(0, Fn, k)
    t[deg, 1] = t[deg, 0]
    dup = g.integers(0, Fn, k)
    t[dup] = t[(dup + 1) % Fn]
    return t.astype(np.int32)


def _check_select(got, want):
    for k in ("keep_vertex", "keep_face", "vertex_map", "face_map", "totals", "dropped"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k


def _check_compact(got, tris, verts, cols, sel):
    kv, kf = sel["keep_vertex"].astype(bool), sel["keep_face"].astype(bool)
    assert np.array_equal(got["out_vertices"].view(np.int32), verts[kv].view(np.int32))
    assert np.array_equal(got["out_colors"].view(np.int32), cols[kv].view(np.int32))
    want = sel["vertex_map"][np.asarray(tris, np.int64)[kf]] if kf.any() else np.zeros((0, 3), np.int32)
    assert np.array_equal(got["out_triangles"], want)
    if len(want):
        assert want.min() >= 0 and want.max() < kv.sum()


@pytest.mark.parametrize("backend", BACKENDS)
def test_selection_and_compaction_on_random_meshes(backend):
    lib, dev = _lib_and_dev(backend)
    g = np.random.default_rng(21)
    hit = set()
    for case, (V, Fn) in enumerate([(40, 300), (97, 257), (300, 500), (5, 64), (1, 3)]):
        tris, counts = _random_mesh(g, V, Fn), _random_counts(g, V)
        verts, cols = g.standard_normal((V, 3)).astype(f32), g.random((V, 3)).astype(f32)
        for mv, mo, mvis, rule in ((1, 0, 0, ALL), (1, 0, 0, ANY), (2, 1, 1, ALL), (0, 6, 0, ALL), (3, 0, 2, ANY), (7, 0, 0, ANY)):
            want = _np_select(tris, V, counts, mv, mo, mvis, rule)
            got = _raw_select(lib, dev, tris, V, counts, mv, mo, mvis, rule, verts, cols, fill=0xFF if case % 2 else 0x00)
            _check_select(got, want)
            _check_compact(got, tris, verts, cols, want)
            assert want["dropped"][0] > 0
            hit.add((int(want["totals"][1]) > 0, rule))
    assert len(hit) == 4


@pytest.mark.parametrize("Fn", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1])
@pytest.mark.parametrize("V", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1])
@pytest.mark.parametrize("backend", BACKENDS)
def test_selection_at_the_scan_chunk(backend, V, Fn):
    lib, dev = _lib_and_dev(backend)
    g = np.random.default_rng(V * 3 + Fn)
    tris = np.stack([np.arange(Fn) % V, (np.arange(Fn) + 1) % V, (np.arange(Fn) + 2) % V], 1).astype(np.int32)      # a strip: every vertex named
    tris[g.integers(0, Fn, 40), 2] = V
    counts = _random_counts(g, V)
    counts[-3:] = [6, 6, 6, 6]                    # the last elements are kept, so the last map entries are the totals - 1
    counts[:3] = [6, 6, 6, 6]
    tris[-1] = [V - 3, V - 2, V - 1]
    verts, cols = g.standard_normal((V, 3)).astype(f32), g.random((V, 3)).astype(f32)
    want = _np_select(tris, V, counts, 2, 1, 0, ALL)
    got = _raw_select(lib, dev, tris, V, counts, 2, 1, 0, ALL, verts, cols)
    _check_select(got, want)
    _check_compact(got, tris, verts, cols, want)
    assert want["keep_face"][-1] and want["face_map"][-1] == want["totals"][1] - 1 and want["vertex_map"][-1] == want["totals"][0] - 1
    assert 100 < want["totals"][1] < Fn - 100


@pytest.mark.parametrize("backend", BACKENDS)
def test_permuting_the_faces_permutes_the_result(backend):
    lib, dev = _lib_and_dev(backend)
    g = np.random.default_rng(8)
    V, Fn = 200, 700
    tris, counts = _random_mesh(g, V, Fn), _random_counts(g, V)
    verts, cols = g.standard_normal((V, 3)).astype(f32), g.random((V, 3)).astype(f32)
    a = _raw_select(lib, dev, tris, V, counts, 1, 1, 0, ALL, verts, cols)
    perm = g.permutation(Fn)
    b = _raw_select(lib, dev, tris[perm], V, counts, 1, 1, 0, ALL, verts, cols)
    assert a["totals"][1] > 20 and np.array_equal(b["keep_face"], a["keep_face"][perm])
    for k in ("keep_vertex", "vertex_map", "totals", "dropped", "out_vertices", "out_colors"):
        assert a[k].tobytes() == b[k].tobytes(), k
    kept = perm[a["keep_face"][perm].astype(bool)]                      # the kept faces in the permuted order
    assert np.array_equal(b["out_triangles"], a["out_triangles"][a["face_map"][kept]])


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_meshes_and_empty_results(backend):
    lib, dev = _lib_and_dev(backend)
    none = np.zeros((0, 3), np.int32)
    got = _raw_select(lib, dev, none, 5, _random_counts(np.random.default_rng(0), 5))
    assert got["totals"].tolist() == [0, 0] and got["dropped"].tolist() == [0] and not got["keep_vertex"].any() and (got["vertex_map"] == -1).all()
    got = _raw_select(lib, dev, none, 0, np.zeros((0, 4), np.int32))
    assert got["totals"].tolist() == [0, 0] and got["dropped"].tolist() == [0]
    got = _raw_select(lib, dev, [(0, 1, 2), (0, 0, 0)], 0, np.zeros((0, 4), np.int32))          # no vertex: every face is invalid
    assert got["totals"].tolist() == [0, 0] and got["dropped"].tolist() == [2] and not got["keep_face"].any()
    # the Python layer: empty tensors out, and no compaction launch
    V, T, bv, bt, c2w = _hull_scene()
    tv, tt, cams = torch.from_numpy(V).to(dev), torch.from_numpy(T).to(dev), torch.from_numpy(c2w).to(dev)
    col = torch.zeros(132, 3, device=dev)
    empty_masks = torch.zeros(6, HULL_H, HULL_W, device=dev)
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        ov, ot, oc, info = meshops.cull_mesh(tv, tt, cams, [HULL_F, HULL_F], HULL_H, HULL_W, masks=empty_masks, colors=col, dilation=3, library=lib)
        names = [r[0] for r in lib.timing_collect()]
    finally:
        lib.timing_enable(False)
    assert "meshcc_compact_kernel" not in names and (backend == "emu" or "cull_votes_kernel" in names)
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and oc.shape == (0, 3) and ot.dtype == torch.int32 and ov.device.type == torch.device(dev).type
    assert info["n_vertices"] == 0 and info["n_faces"] == 0 and not bool(info["keep_vertex"].any()) and (_np(info["counts"])[:, 2] == 0).all()
    ov, ot, oc, info = meshops.cull_mesh(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, dtype=torch.int64, device=dev), cams, [HULL_F, HULL_F],
                                         HULL_H, HULL_W, masks=empty_masks, visibility=True, depth_tol=0.1, library=lib)
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and oc is None and info["counts"].shape == (0, 4)
    ov, ot, _, info = meshops.cull_mesh(tv, torch.zeros(0, 3, dtype=torch.int32, device=dev), cams, [HULL_F, HULL_F], HULL_H, HULL_W,
                                        visibility=True, depth_tol=0.1, library=lib)
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and (_np(info["counts"])[:, 3] == _np(info["counts"])[:, 1]).all()
    assert len(meshops.dilate_masks(torch.zeros(0, 4, 5, device=dev), 1, library=lib)) == 0


# ---- the entries' refusals; binding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_refusals_and_no_ops(backend):
    lib, dev = _lib_and_dev(backend)
    L = lib.lib
    p, null, stream = _lib.ptr, C.c_void_p(0), _lib.stream_of(torch.device(dev))
    odd = lambda t, by=4: C.c_void_p(t.data_ptr() + by)
    big = 2 ** 31
    m = torch.zeros(2, 3, 70, device=dev)
    words = torch.zeros(2 * 3 * 2 + 2, dtype=torch.int64, device=dev)
    words2 = torch.zeros_like(words)
    cases = []
    dil = lambda **kw: (kw.get("m", p(m)), kw.get("n", 2), kw.get("H", 3), kw.get("W", 70), kw.get("r", 1), kw.get("rb", p(words)),
                        kw.get("b", p(words2)), stream)
    for kw, msg in ((dict(m=null), "null argument"), (dict(rb=null), "null argument"), (dict(b=null), "null argument"),
                    (dict(rb=odd(words)), "8-byte aligned"), (dict(b=odd(words2)), "8-byte aligned"), (dict(H=0), "at least 1"),
                    (dict(W=0), "at least 1"), (dict(H=-3), "at least 1"), (dict(W=-1), "at least 1"), (dict(n=-1), "negative"),
                    (dict(r=-1), "radius must lie"), (dict(r=32768), "radius must lie"), (dict(H=2 ** 16, W=2 ** 15), "2\\^31 pixels"),
                    (dict(n=big, H=1, W=1), "2\\^31 words")):
        cases.append(("cnr_mask_dilate", dil(**kw), msg))
    v, cam, foc = torch.zeros(4, 3, device=dev), torch.eye(4, device=dev).repeat(2, 1, 1).contiguous(), torch.ones(2, 2, device=dev)
    counts = torch.zeros(6, 4, dtype=torch.int32, device=dev)
    depth = torch.zeros(2, 3, 70, device=dev)
    vote = lambda **kw: (kw.get("v", p(v)), kw.get("V", 4), kw.get("cam", p(cam)), kw.get("foc", p(foc)), null, 1.0, 1e-3, 0, kw.get("n", 2),
                         kw.get("H", 3), kw.get("W", 70), kw.get("bits", p(words)), kw.get("depth", p(depth)), 0.1, kw.get("counts", p(counts)), stream)
    for kw, msg in ((dict(v=null), "null argument"), (dict(cam=null), "null argument"), (dict(foc=null), "null argument"),
                    (dict(counts=null), "null argument"), (dict(bits=odd(words)), "8-byte aligned"), (dict(counts=odd(counts)), "16-byte aligned"),
                    (dict(counts=odd(counts, 8)), "16-byte aligned"), (dict(V=-1), "n_vertices must lie"), (dict(V=big), "n_vertices must lie"),
                    (dict(n=-1), "negative"), (dict(H=0), "at least 1"), (dict(W=-2), "at least 1"), (dict(H=2 ** 16, W=2 ** 15), "2\\^31 pixels")):
        cases.append(("cnr_mesh_view_votes", vote(**kw), msg))
    t, i4 = torch.zeros(1, 3, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    u8 = torch.zeros(4, dtype=torch.uint8, device=dev)
    sel = lambda **kw: (kw.get("t", p(t)), kw.get("F", 1), kw.get("V", 4), kw.get("counts", p(counts)), kw.get("mv", 1), kw.get("mo", 0),
                        kw.get("mvis", 0), kw.get("rule", 0), kw.get("kv", p(u8)), kw.get("kf", p(u8)), kw.get("vm", p(i4)), kw.get("fm", p(i4)),
                        kw.get("totals", p(i4)), kw.get("dropped", p(i4)), stream)
    for kw, msg in ((dict(F=big), "must not exceed"), (dict(V=big), "must not exceed"), (dict(F=-1), "negative"), (dict(V=-1), "negative"),
                    (dict(rule=2), "face_rule must be"), (dict(rule=-1), "face_rule must be"), (dict(mv=-1), "must not be negative"),
                    (dict(mo=-1), "must not be negative"), (dict(mvis=-1), "must not be negative"), (dict(t=null), "null argument"),
                    (dict(counts=null), "null argument"), (dict(kv=null), "null argument"), (dict(kf=null), "null argument"),
                    (dict(vm=null), "null argument"), (dict(fm=null), "null argument"), (dict(totals=null), "null argument"),
                    (dict(dropped=null), "null argument")):
        cases.append(("cnr_mesh_cull_select", sel(**kw), msg))
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        for name, args, msg in cases:
            assert getattr(L, name)(*args) < 0, (name, msg)
            with pytest.raises(RuntimeError, match=msg) as err:
                lib.call(name, *args)
            assert name in str(err.value)
        # n == 0: successful no-ops, whatever the pointers
        assert L.cnr_mask_dilate(null, 0, 3, 70, 1, null, null, stream) == 0
        assert L.cnr_mesh_view_votes(null, 0, p(cam), p(foc), null, 1.0, 1e-3, 0, 2, 3, 70, null, null, 0.0, null, stream) == 0
        assert L.cnr_mesh_view_votes(p(v), 4, null, null, null, 1.0, 1e-3, 0, 0, 3, 70, null, null, 0.0, p(counts), stream) == 0
        assert lib.timing_collect() == []          # nothing was launched after a refusal or for an empty call
    finally:
        lib.timing_enable(False)
    assert not counts.any() and not words.any() and not words2.any()
    assert L.cnr_abi_version() == _lib.ABI_VERSION == 9


def test_header_binding_and_sources_agree():
    header = open(os.path.join(ROOT, "include", "colorneus_render.h")).read()
    csrc = os.path.join(ROOT, "color-neus_amd", "csrc")
    ops = open(os.path.join(csrc, "cnr_ops.cpp")).read()
    names = ("cnr_mask_dilate", "cnr_mesh_view_votes", "cnr_mesh_cull_select")
    for name, nargs in zip(names, (8, 16, 15)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is C.c_int
        assert header.count("int %s(" % name) == 1 and ops.count("\nint %s(" % name) == 1
    order = list(_lib.SIGNATURES)
    assert [order.index(n) for n in names] == list(range(order.index("cnr_point_mesh_distance") + 1, order.index("cnr_point_mesh_distance") + 4))
    assert not [n for n in _lib.SIGNATURES if n.endswith("_bytes") and ("cull" in n or "dilate" in n or "votes" in n)]
    assert "#define CNR_ABI_VERSION 9\n" in header
    assert "cnr_cull" in open(os.path.join(csrc, "Makefile")).read().split("HIP_UNITS =")[1].split("\n")[0]
    # the carried scan of the keep flags has one definition (one kernel, one emulation loop), which both selections call
    code = {fn: "\n".join(line.split("//")[0] for line in open(os.path.join(csrc, fn)).read().split("\n"))
            for fn in sorted(os.listdir(csrc)) if fn.endswith((".hip", ".h", ".cpp"))}
    assert [fn for fn, text in code.items() if "void meshcc_scan_kernel(" in text] == ["cnr_meshcc.hip"]
    assert sorted(fn for fn, text in code.items() if "void mesh_keep_scan(const MeshKeepScan& p" in text) == ["cnr_kernels_emu.cpp", "cnr_meshcc.h",
                                                                                                                "cnr_meshcc.hip"]
    assert code["cnr_cull.hip"].count("mesh_keep_scan(") == 1 and code["cnr_meshcc.hip"].count("mesh_keep_scan(") == 2
    assert code["cnr_kernels_emu.cpp"].count("mesh_keep_scan(") == 3 and "block_excl_scan" not in code["cnr_cull.hip"]
    assert "totals[0]++" not in code["cnr_kernels_emu.cpp"].split("void be_mesh_cull_select(")[1]
    # the camera and the vertex stage are the rasteriser's functions, not copies
    assert sum("RasterVert raster_project(" in text for text in code.values()) == 1 and "raster_project(" in code["cnr_cull.h"]
    assert sum("RasterCam raster_cam_of(" in text for text in code.values()) == 1 and "raster_cam_of(" in code["cnr_cull.hip"]


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------
def test_python_surface_refuses_bad_arguments():
    lib = cn.load_library(N.EMU_LIB)
    V, T, bv, bt, c2w = _hull_scene()
    tv, tt, cams = torch.from_numpy(V), torch.from_numpy(T), torch.from_numpy(c2w)
    foc, H, W = [HULL_F, HULL_F], HULL_H, HULL_W
    masks = torch.ones(6, H, W)
    with pytest.raises(ValueError, match="expected 3 dimensions"):
        meshops.dilate_masks(torch.ones(H, W), 1, library=lib)
    with pytest.raises(ValueError, match="radius must lie"):
        meshops.dilate_masks(masks, -1, library=lib)
    with pytest.raises(ValueError, match="radius must lie"):
        meshops.dilate_masks(masks, 32768, library=lib)
    vm = meshops.dilate_masks(masks, 1, library=lib)
    assert isinstance(vm, meshops.ViewMasks) and vm.bits.shape == (6, H, 2) and vm.bits.dtype == torch.int64 and (vm.H, vm.W, vm.radius) == (H, W, 1)
    assert bool(vm.to_bool().all()) and vm.to_bool().shape == (6, H, W)
    for bad, msg in ((dict(vertices=torch.zeros(4, 2)), "vertices"), (dict(c2w=cams[0]), "c2w"), (dict(c2w=torch.zeros(6, 3, 4)), "c2w"),
                     (dict(focal=[1.0, 2.0, 3.0]), "focal"), (dict(focal=torch.ones(5, 2)), "focal"), (dict(masks=masks), "expected a ViewMasks"),
                     (dict(masks=meshops.dilate_masks(masks[:5], 0, library=lib)), "expected 6 images"),
                     (dict(masks=meshops.dilate_masks(masks[:, :, :W - 1], 0, library=lib)), "expected 6 images"),
                     (dict(depth=torch.zeros(6, H, W)), "depth requires depth_tol"), (dict(depth=torch.zeros(6, H, W + 1), depth_tol=0.1), "depth: expected"),
                     (dict(counts=torch.zeros(132, 4)), "counts"), (dict(counts=torch.zeros(131, 4, dtype=torch.int32)), "counts"),
                     (dict(H=0), "at least 1"), (dict(radius=2.0), "radius without origin"), (dict(origin=[0.0, 1.0]), "origin")):
        kw = dict(vertices=tv, c2w=cams, focal=foc, H=H, W=W, library=lib)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            meshops.view_votes(**kw)
    for bad, msg in ((dict(visibility=True), "visibility=True requires depth_tol"), (dict(faces="most"), "faces must be 'all' or 'any'"),
                     (dict(dilation=-1), "dilation must lie"), (dict(masks=torch.ones(H, W)), "expected 3 dimensions"),
                     (dict(masks=torch.ones(5, H, W)), "expected 6 images"), (dict(masks=vm, dilation=2), "dilation applies to a raw mask stack"),
                     (dict(min_views=-1), "must not be negative"), (dict(view_chunk=0), "view_chunk"), (dict(triangles=torch.zeros(3, 2, dtype=torch.int64)), "triangles"),
                     (dict(triangles=tt.float()), "integer dtype"), (dict(colors=torch.zeros(5, 3)), "colors")):
        kw = dict(vertices=tv, triangles=tt, c2w=cams, focal=foc, H=H, W=W, library=lib)
        kw.update(bad)
        with pytest.raises(ValueError, match=msg):
            meshops.cull_mesh(**kw)
    with pytest.raises(ValueError, match="visibility=True requires depth_tol"):
        meshops.MeshCuller(cams, foc, H, W, visibility=True, library=lib)
    for call in (lambda: meshops.dilate_masks(masks, 1), lambda: meshops.view_votes(tv, cams, foc, H, W),
                 lambda: meshops.cull_mesh(tv, tt, cams, foc, H, W)):      # CPU tensors only with an explicit emulation library
        with pytest.raises(RuntimeError, match="fallback"):
            call()
    # bool, integer and float64 stacks are the same foreground; a focal of shape [2] is every view's
    want = meshops.dilate_masks(masks, 0, library=lib).bits
    for other in (masks.bool(), masks.to(torch.int32), masks.double() * 1e-300, masks.to(torch.uint8).numpy()):
        assert torch.equal(meshops.dilate_masks(other, 0, library=lib).bits, want)
    a = meshops.view_votes(tv, cams, foc, H, W, library=lib)
    b = meshops.view_votes(tv, cams, torch.tensor(foc).expand(6, 2), H, W, library=lib)
    assert torch.equal(a, b) and a.dtype == torch.int32 and a.shape == (132, 4)
    # counts= accumulates into the caller's tensor
    c = meshops.view_votes(tv, cams[:2], foc, H, W, library=lib)
    assert meshops.view_votes(tv, cams[2:], foc, H, W, counts=c, library=lib) is c and torch.equal(c, a)


def _tiny_renderer(lib, dev):
    fx = G.load("tiny_sharp")
    ocfg, P = G.weights_of("tiny_sharp", fx)
    return N.make_renderer(ocfg, P, lib, dev)


@pytest.mark.parametrize("backend", BACKENDS)
def test_through_the_product(backend):
    """extract_geometry(cull=culler, clean="largest") is extract raw -> cull_mesh -> clean_mesh, bit for bit; render_mesh_view colours only
    what survives; cull=None is the call without the argument."""
    lib, dev = _lib_and_dev(backend)
    r = _tiny_renderer(lib, dev)
    bmin, bmax, res, H, W = [-1.0] * 3, [1.0] * 3, 24, 60, 80
    raw_v, raw_t = r.marching_cubes(r.extract_fields(bmin, bmax, dev, res), bmin, bmax)
    assert raw_t.shape[0] > 300
    cams = torch.from_numpy(np.stack([_look_at(e) for e in ((3, 0, 0), (0, -3, 0), (0, 0, 3), (-2, 2, 1))])).to(dev)
    foc = torch.tensor([70.0, 70.0], device=dev)
    masks = torch.stack([cn.rasterize_mesh(raw_v, raw_t, c, foc, H, W, library=lib)["tri_id"] >= 0 for c in cams]).float()
    masks[0, :, W // 2 + 3:] = 0.0                                 # the first view's mask loses its right part: that side of the mesh goes
    kw = dict(dilation=1, max_outside=0)
    culler = meshops.MeshCuller(cams, foc, H, W, masks=masks, library=lib, **kw)
    cv, ct, _, cinfo = meshops.cull_mesh(raw_v, raw_t, cams, foc, H, W, masks=masks, library=lib, **kw)
    assert 50 < ct.shape[0] < raw_t.shape[0] - 50
    want_v, want_t, _, _ = meshops.clean_mesh(cv, ct, library=lib)
    gv, gt = r.extract_geometry(bmin, bmax, dev, res, clean="largest", cull=culler)
    assert gv.dtype == np.float64 and gt.dtype == np.int64
    assert np.array_equal(gv, _np(want_v).astype(np.float64)) and np.array_equal(gt, _np(want_t).astype(np.int64))
    gv, gt = r.extract_geometry(bmin, bmax, dev, res, cull=culler)
    assert np.array_equal(gv, _np(cv).astype(np.float64)) and np.array_equal(gt, _np(ct).astype(np.int64))
    view = r.render_mesh_view(bmin, bmax, res, cams[3], foc, H, W, clean="largest", cull=culler)
    assert torch.equal(view["triangles"], want_t) and torch.equal(view["vertices"].view(torch.int32), want_v.view(torch.int32))
    assert torch.equal(view["colors"].view(torch.int32), r.vertex_colors(want_v).view(torch.int32))
    # cull=None: the bits of the call without the argument
    pv, pt = r.extract_geometry(bmin, bmax, dev, res)
    nv, nt = r.extract_geometry(bmin, bmax, dev, res, cull=None)
    assert pv.tobytes() == nv.tobytes() and pt.tobytes() == nt.tobytes() and np.array_equal(pt, _np(raw_t).astype(np.int64))
    plain, none = r.render_mesh_view(bmin, bmax, res, cams[3], foc, H, W), r.render_mesh_view(bmin, bmax, res, cams[3], foc, H, W, cull=None)
    assert list(plain) == list(none)
    for k in plain:
        if torch.is_tensor(plain[k]):
            assert _np(plain[k]).tobytes() == _np(none[k]).tobytes() and plain[k].dtype == none[k].dtype, k
        else:
            assert plain[k] == none[k], k


# ---- HIP against the emulation at size -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_against_the_emulation_at_size():
    """about 200 k vertices (two overlapping spheres and a shell beside them on a 304-cell lattice), 8 views of 300 x 400, radius 12,
    visibility: the packed masks, the counts, the maps and the compacted arrays of the two builds are the same bits"""
    assert torch.cuda.is_available(), "needs a GPU"
    hip, emu = cn.load_library(), cn.load_library(N.EMU_LIB)
    dev, res, H, W = torch.device("cuda:0"), 304, 300, 400
    ax = torch.linspace(-1.0, 1.0, res, device=dev)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    u = torch.full_like(x, -1.0)
    for (cx, cy, cz), rad in (((-0.3, 0.0, 0.0), 0.55), ((0.35, 0.1, 0.0), 0.5), ((0.0, 0.0, 0.8), 0.15)):
        u = torch.maximum(u, rad - torch.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2))
    del x, y, z
    r = cn.NeuSRenderer(cn.RenderConfig(type="NeuS"), library=hip)
    verts, tris = r.marching_cubes(u, [-1.0] * 3, [1.0] * 3)
    del u
    assert 150_000 < verts.shape[0] < 260_000, verts.shape
    g = np.random.default_rng(4)
    eyes = g.normal(size=(8, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * 3.0
    cams = torch.from_numpy(np.stack([_look_at(e) for e in eyes]))
    foc = torch.tensor([520.0, 520.0])
    yy, xx = np.mgrid[0:H, 0:W]
    masks = torch.from_numpy(np.stack([((xx - W / 2 - 20 * k + 60) ** 2 + (yy - H / 2) ** 2 < (70 + 5 * k) ** 2) for k in range(8)]).astype(f32))
    kw = dict(dilation=12, visibility=True, depth_tol=0.01, view_chunk=3, min_views=2, max_outside=1)
    a = meshops.cull_mesh(verts, tris, cams.to(dev), foc.to(dev), H, W, masks=masks.to(dev), library=hip, **kw)
    b = meshops.cull_mesh(verts.cpu(), tris.cpu(), cams, foc, H, W, masks=masks, library=emu, **kw)
    pa, pb = meshops.dilate_masks(masks.to(dev), 12, library=hip), meshops.dilate_masks(masks, 12, library=emu)
    assert torch.equal(pa.bits.cpu(), pb.bits) and np.array_equal(_np(pb.to_bool()), _np_dilate(masks.numpy() > 0, 12))
    assert 1000 < a[3]["n_faces"] < tris.shape[0] - 1000 and a[3]["n_faces"] == b[3]["n_faces"] and a[3]["n_vertices"] == b[3]["n_vertices"]
    for k in ("counts", "keep_vertex", "keep_face", "vertex_map", "face_map"):
        assert torch.equal(a[3][k].cpu(), b[3][k]), k
    c = _np(b[3]["counts"])
    assert (c[:, 3] < c[:, 1]).any() and (c[:, 2] < c[:, 1]).any() and (c[:, 1] < 8).any()
    assert torch.equal(a[0].cpu().view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].cpu(), b[1])
