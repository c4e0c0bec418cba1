"""The mesh rasteriser (cnr_mesh_raster; color_neus_amd.imaging.rasterize_mesh / mesh_view_metrics, NeuSRenderer.render_mesh_view).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The yardsticks are written here and
use nothing from the library:

  S32   the specification of include/colorneus_render.h restated in numpy: float32 for the float steps (every numpy operation on float32
        arrays is one IEEE rounding), int64 for the integer steps.  tri_id, depth and rgb must match it BITWISE.
  RC    an independent float64 ray caster: Moeller-Trumbore along the rays of the project's own rays.get_rays_at(normalize=False), whose
        ray parameter of a hit is the camera depth.  Compared away from the projected edges (the rasteriser snaps vertices to 1/256 pixel):
        on the pixels more than 1/64 pixel from every projected edge the triangle must be RC's nearest hit, and
        |1/depth - 1/t| <= (|g_i| + |g_j|) / 256 + 1e-6 / t, g the float64 screen-space gradient of 1/z on that triangle: the snapping error
        of 1/512 pixel per vertex with a factor of two.
"""
import ctypes as C
import functools
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import color_neus_amd as cn
from color_neus_amd import _lib
import _golden as G
import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
f32 = np.float32
H0, W0, F0 = 72, 96, 150.0
SMALL = int(re.search(r"constexpr int CNR_RASTER_SMALL = (\d+);", open(os.path.join(ROOT, "color-neus_amd", "csrc", "cnr_raster.h")).read()).group(1))
NOKEY = np.uint64(2 ** 64 - 1)


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _bits(x):
    x = x.detach().cpu().contiguous().numpy() if torch.is_tensor(x) else np.ascontiguousarray(x)
    return x.view(np.int32)


# ---- inputs (computed once, never modified) ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere():
    """An octahedron subdivided twice onto the sphere of radius 0.5: 66 vertices, 128 triangles; random colours."""
    V = [np.array(v, float) for v in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    Fc = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(2):
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
    V, Fc = (np.array(V) * 0.5).astype(f32), np.array(Fc, dtype=np.int32)
    assert V.shape == (66, 3) and Fc.shape == (128, 3)
    col = np.random.default_rng(99).random((66, 3)).astype(f32)
    for a in (V, Fc, col):
        a.setflags(write=False)
    return V, Fc, col


def _camera(seed, opengl=False, dist=3.0, shift=0.0):
    """c2w (float32 [4, 4]) on the sphere of radius `dist`, looking at the origin, a random orthonormal rotation from a seeded QR; `shift`
    moves the centre along the camera's x axis."""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] *= -1
    c2w = np.eye(4)
    c2w[:3, 3] = -dist * Q[:, 2] + shift * Q[:, 0]
    if opengl:
        Q = Q * np.array([1.0, -1.0, -1.0])
    c2w[:3, :3] = Q
    return c2w.astype(f32)


def _identity_camera():
    return np.eye(4, dtype=f32)


def _pixel_vertex(U, Vp, z=2.0, fx=128.0, W=W0, H=H0):
    """The point that the identity camera with focal 128 projects exactly onto pixel (U, Vp) at depth z = 2 (every step exact in float32)."""
    return [(U - W * 0.5) * z / fx, (Vp - H * 0.5) * z / fx, z]


# ---- S32 -----------------------------------------------------------------------------------------------------------------------------------
def _s32(V, Fc, col, c2w, focal, H, W, opengl=False, origin=None, radius=1.0, z_near=1e-3, background=None):
    V, c2w = np.asarray(V, f32), np.asarray(c2w, f32)
    Fc = np.asarray(Fc, np.int64).reshape(-1, 3)
    R, t = c2w[:3, :3], c2w[:3, 3]
    if origin is not None:
        t = (t - np.asarray(origin, f32)) / f32(radius)
    fx, fy = f32(focal[0]), f32(focal[1])
    with np.errstate(all="ignore"):
        d = V.reshape(-1, 3) - t
        xc, yc, zc = [(R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2] for k in range(3)]
        if opengl:
            yc, zc = -yc, -zc
        u = (fx * xc) / zc + f32(W) * f32(0.5)
        v = (fy * yc) / zc + f32(H) * f32(0.5)
        usable = (zc > f32(z_near)) & (np.abs(u) < f32(2 ** 21)) & (np.abs(v) < f32(2 ** 21))
        X = np.where(usable, np.rint(np.where(usable, u, 0) * f32(256)), 0).astype(np.int64)
        Y = np.where(usable, np.rint(np.where(usable, v, 0) * f32(256)), 0).astype(np.int64)
    key = np.full((H, W), NOKEY)
    jj, ii = np.mgrid[0:H, 0:W]
    px, py = ii.astype(np.int64) * 256, jj.astype(np.int64) * 256
    dropped = [0, 0]
    nv = len(usable)

    def terms(a, b, c):
        A = (X[b] - X[a]) * (Y[c] - Y[a]) - (Y[b] - Y[a]) * (X[c] - X[a])
        if A == 0:
            return None
        if A < 0:
            b, c, A = c, b, -A
        E = lambda p, q: (X[q] - X[p]) * (py - Y[p]) - (Y[q] - Y[p]) * (px - X[p])
        Es = [E(b, c), E(c, a), E(a, b)]
        cov = (Es[0] >= 0) & (Es[1] >= 0) & (Es[2] >= 0)
        with np.errstate(all="ignore"):
            q = [(Ek.astype(f32) / f32(A)) / zc[k] for Ek, k in zip(Es, (a, b, c))]
            s = (q[0] + q[1]) + q[2]
        return (a, b, c), cov, q, s

    depths = []
    for n, (a, b, c) in enumerate(Fc):
        if min(a, b, c) < 0 or max(a, b, c) >= nv:
            dropped[1] += 1
            continue
        if not usable[[a, b, c]].all():
            dropped[0] += 1
            continue
        tm = terms(a, b, c)
        if tm is None:
            continue
        _, cov, q, s = tm
        with np.errstate(all="ignore"):
            dep = (f32(1) / s).astype(f32)
            ok = cov & (dep > 0)
        k = (dep.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(n)
        key = np.where(ok & (k < key), k, key)
        depths.append((ok, dep))
    tid = np.where(key == NOKEY, -1, (key & np.uint64(0xffffffff)).astype(np.int64))
    depth = np.where(tid < 0, f32(np.nan), (key >> np.uint64(32)).astype(np.uint32).view(f32)).astype(f32)
    ties = np.zeros((H, W), int)
    for ok, dep in depths:
        ties += ok & (dep.view(np.uint32) == depth.view(np.uint32))
    out = {"tri_id": tid, "depth": depth, "dropped": tuple(dropped), "tie": ties > 1}
    if col is not None:
        col = np.asarray(col, f32)
        bg = np.zeros(3, f32) if background is None else np.asarray(background, f32)
        rgb = np.broadcast_to(bg, (H, W, 3)).copy()
        for n in np.unique(tid[tid >= 0]):
            (a, b, c), _, q, s = terms(*Fc[n])
            m = tid == n
            w = [qk / s for qk in q]
            for ch in range(3):
                rgb[..., ch][m] = ((w[0] * col[a, ch] + w[1] * col[b, ch]) + w[2] * col[c, ch])[m]
        out["rgb"] = rgb
    return out


# ---- RC ------------------------------------------------------------------------------------------------------------------------------------
def _rc(V, Fc, c2w, focal, H, W, library, opengl=False):
    """float64: per triangle and pixel the ray parameter of the hit (inf: none), the distance of every pixel to the nearest projected edge,
    and per triangle the screen-space gradient of 1/z."""
    o, d = cn.rays.get_rays_at(torch.from_numpy(np.asarray(c2w, f32)), torch.tensor([float(focal[0]), float(focal[1])]), H, W, normalize=False,
                               opengl=opengl, library=library)
    o, d = o.reshape(-1, 3).double().numpy(), d.reshape(-1, 3).double().numpy()
    V = np.asarray(V, float)
    c2w = np.asarray(c2w, float)
    R, t = c2w[:3, :3], c2w[:3, 3]
    Pc = (V - t) @ R
    if opengl:
        Pc = Pc * np.array([1.0, -1.0, -1.0])
    u, v, iz = focal[0] * Pc[:, 0] / Pc[:, 2] + W / 2, focal[1] * Pc[:, 1] / Pc[:, 2] + H / 2, 1.0 / Pc[:, 2]
    jj, ii = np.mgrid[0:H, 0:W]
    px = np.stack([ii.ravel(), jj.ravel()], 1).astype(float)
    tt = np.full((len(Fc), H * W), np.inf)
    mind = np.full(H * W, np.inf)
    grad = np.zeros((len(Fc), 2))
    for n, (a, b, c) in enumerate(Fc):
        e1, e2 = V[b] - V[a], V[c] - V[a]
        h = np.cross(d, e2)
        det = h @ e1
        s = o - V[a]
        with np.errstate(all="ignore"):
            uu = np.einsum("ij,ij->i", h, s) / det
            q = np.cross(s, e1)
            vv = np.einsum("ij,ij->i", d, q) / det
            tv = (q @ e2) / det
        hit = (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tv > 0)
        tt[n] = np.where(hit, tv, np.inf)
        P = np.stack([u[[a, b, c]], v[[a, b, c]]], 1)
        for k in range(3):
            A_, B_ = P[k], P[(k + 1) % 3]
            e = B_ - A_
            w = np.clip(((px - A_) @ e) / (e @ e), 0, 1)
            mind = np.minimum(mind, np.linalg.norm(px - (A_ + w[:, None] * e), axis=1))
        M = np.array([[u[b] - u[a], v[b] - v[a]], [u[c] - u[a], v[c] - v[a]]])
        grad[n] = np.linalg.solve(M, [iz[b] - iz[a], iz[c] - iz[a]])
    return tt, mind.reshape(H, W), grad


def _bound(grad, ids, t):
    return np.abs(grad[ids]).sum(-1) / 256 + 1e-6 / t


@functools.lru_cache(maxsize=None)
def _rc_standard(seed):
    V, Fc, _ = _sphere()
    return _rc(V, Fc, _camera(seed), (F0, F0), H0, W0, N.EMU_LIB)


# ---- the call --------------------------------------------------------------------------------------------------------------------------------
def _raster(backend, V, Fc, col, c2w, focal=(F0, F0), H=H0, W=W0, **kw):
    path, dev = _lib_and_dev(backend)
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)
    return cn.rasterize_mesh(t(V, f32).reshape(-1, 3), t(Fc, np.int64).reshape(-1, 3), t(c2w, f32), t(np.asarray(focal), f32), H, W,
                             colors=t(col, f32) if col is not None else None, library=path, **kw)


def _nan_canon(x):
    """depth bits with every NaN mapped to one pattern"""
    x = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x, f32)
    b = x.view(np.int32).copy()
    b[np.isnan(x)] = 0x7fc00000
    return b


def _same(got, want, rgb=True):
    assert np.array_equal(got["tri_id"].cpu().numpy(), want["tri_id"])
    assert np.array_equal(_nan_canon(got["depth"]), _nan_canon(want["depth"]))
    if rgb:
        assert np.array_equal(_bits(got["rgb"]), _bits(want["rgb"]))
    assert (got["dropped"]["behind_or_far"], got["dropped"]["bad_index"]) == want["dropped"]
    assert np.array_equal(got["mask"].cpu().numpy(), want["tri_id"] >= 0)


# ---- 1. bitwise against S32 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalised", [False, True])
@pytest.mark.parametrize("opengl", [False, True])
@pytest.mark.parametrize("backend", BACKENDS)
def test_bitwise_against_the_specification(backend, opengl, normalised):
    V, Fc, col = _sphere()
    for seed in range(4):
        c2w = _camera(seed, opengl)
        kw = {}
        if normalised:      # the raw camera centre is t * radius + origin; the mesh stays in the normalised frame
            kw = dict(origin=[0.1, -0.2, 0.05], radius=1.5)
            c2w = c2w.copy()
            c2w[:3, 3] = c2w[:3, 3] * f32(1.5) + np.array(kw["origin"], f32)
        want = _s32(V, Fc, col, c2w, (F0, F0), H0, W0, opengl=opengl, **kw)
        assert (want["tri_id"] >= 0).mean() > 0.25 and want["dropped"] == (0, 0)
        _same(_raster(backend, V, Fc, col, c2w, opengl=opengl, **kw), want)


# ---- 2. against RC ---------------------------------------------------------------------------------------------------------------------------
def _check_against_rc(got, tt, mind, grad, standard):
    tid, depth = got["tri_id"].cpu().numpy(), got["depth"].cpu().numpy().astype(float)
    H, W = tid.shape
    far = mind > 1.0 / 64
    best = tt.argmin(0).reshape(H, W)
    tbest = tt.min(0).reshape(H, W)
    rid = np.where(np.isfinite(tbest), best, -1)
    if standard:
        excluded, hits = 1.0 - far.mean(), (rid >= 0).mean()
        print(f"excluded share {excluded:.4f}, hit share {hits:.4f}")
        assert excluded <= 0.02 and hits >= 0.25
        assert np.array_equal(tid[far], rid[far])
        ok = far & (rid >= 0)
    else:
        # several surfaces: the winner c must be RC's nearest hit up to the snapping error of the two triangles involved
        assert np.array_equal((tid >= 0)[far], (rid >= 0)[far])
        ok = far & (rid >= 0)
        tc = tt[tid[ok], np.flatnonzero(ok.ravel())]
        assert np.isfinite(tc).all()
        assert (1.0 / tc >= 1.0 / tbest[ok] - _bound(grad, tid[ok], tc) - _bound(grad, rid[ok], tbest[ok])).all()
        ok = ok & (tid == rid)
    err = np.abs(1.0 / depth[ok] - 1.0 / tbest[ok])
    bound = _bound(grad, rid[ok], tbest[ok])
    print(f"max depth error / bound {np.max(err / bound):.3f} on {ok.sum()} pixels")
    assert ok.sum() > 0.2 * H * W and (err <= bound).all()


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("backend", BACKENDS)
def test_against_the_ray_caster(backend, seed):
    V, Fc, col = _sphere()
    _check_against_rc(_raster(backend, V, Fc, col, _camera(seed)), *_rc_standard(seed), standard=True)


# ---- 3. both paths and the threshold ---------------------------------------------------------------------------------------------------------
QUAD_FOCAL = (128.0, 128.0)


def _flat_depth_ok(depth, z):
    """a plane of constant depth z: the b_k sum to 1 up to the roundings of the pixel stage (int -> float, E / A, the two additions, 1 / s:
    at most 8 half-ulp relative errors in a row)"""
    return bool((np.abs(depth.cpu().numpy().astype(float) - z) <= z * 8 * 2.0 ** -24).all())


def _quad(z=2.0):
    return np.array([_pixel_vertex(-40, -30, z), _pixel_vertex(200, -30, z), _pixel_vertex(200, 150, z), _pixel_vertex(-40, 150, z)], f32)


@pytest.mark.parametrize("order", [((0, 1, 2), (0, 2, 3)), ((0, 2, 3), (0, 1, 2)), ((2, 1, 0), (3, 2, 0))])
@pytest.mark.parametrize("backend", BACKENDS)
def test_full_screen_quad_takes_the_large_path(backend, order):
    V, Fc = _quad(), np.array(order, np.int32)
    col = np.random.default_rng(5).random((4, 3)).astype(f32)
    want = _s32(V, Fc, col, _identity_camera(), QUAD_FOCAL, H0, W0)
    got = _raster(backend, V, Fc, col, _identity_camera(), focal=QUAD_FOCAL)
    _same(got, want)
    tid = got["tri_id"].cpu().numpy()
    assert (tid >= 0).all()                                        # no hole along the shared edge
    jj, ii = np.mgrid[0:H0, 0:W0]
    diag = 3 * (ii + 40) == 4 * (jj + 30)                          # the diagonal corner 0 -> corner 2 passes through these pixel centres
    assert diag.sum() >= 20 and (tid[diag] == 0).all() and want["tie"][diag].all()
    assert set(np.unique(tid)) == {0, 1}
    assert _flat_depth_ok(got["depth"], 2.0)


@pytest.mark.parametrize("n", [SMALL - 1, SMALL, SMALL + 1, SMALL + 2])
@pytest.mark.parametrize("backend", BACKENDS)
def test_right_triangles_at_the_small_box_threshold(backend, n):
    """clipped boxes of exactly n x n pixels, n around CNR_RASTER_SMALL; and the same with the box clipped to n by the screen's corner"""
    V = np.array([_pixel_vertex(10, 20), _pixel_vertex(10 + n - 1, 20), _pixel_vertex(10, 20 + n - 1),
                  _pixel_vertex(W0 - n, H0 - n, 4.0), _pixel_vertex(W0 + 30, H0 - n, 4.0), _pixel_vertex(W0 - n, H0 + 30, 4.0)], f32)
    Fc = np.array([(0, 1, 2), (3, 5, 4)], np.int32)
    col = np.random.default_rng(6).random((6, 3)).astype(f32)
    want = _s32(V, Fc, col, _identity_camera(), QUAD_FOCAL, H0, W0)
    assert (want["tri_id"] == 0).sum() == n * (n + 1) // 2 and (want["tri_id"] == 1).sum() == n * n
    _same(_raster(backend, V, Fc, col, _identity_camera(), focal=QUAD_FOCAL), want)


@pytest.mark.parametrize("backend", BACKENDS)
def test_sphere_with_a_large_quad_through_it(backend):
    V, Fc, col = _sphere()
    c2w = _camera(1)
    Q, t = c2w[:3, :3].astype(float), c2w[:3, 3].astype(float)
    corners = [t + Q @ np.array([x, y, 3.0 + 0.15 * x]) for x, y in ((-2, -2), (2, -2), (2, 2), (-2, 2))]      # tilted: cuts through the sphere
    V2 = np.concatenate([V, np.array(corners, f32)])
    F2 = np.concatenate([Fc, np.array([(66, 67, 68), (66, 68, 69)], np.int32)])
    col2 = np.concatenate([col, np.random.default_rng(7).random((4, 3)).astype(f32)])
    want = _s32(V2, F2, col2, c2w, (F0, F0), H0, W0)
    assert (want["tri_id"] >= 128).mean() > 0.5 and ((want["tri_id"] >= 0) & (want["tri_id"] < 128)).mean() > 0.1
    got = _raster(backend, V2, F2, col2, c2w)
    _same(got, want)
    _check_against_rc(got, *_rc(V2, F2, c2w, (F0, F0), H0, W0, N.EMU_LIB), standard=False)


# ---- 4. ordering -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_order_of_the_triangles_does_not_matter(backend):
    V, Fc, col = _sphere()
    c2w = _camera(2)
    base = _raster(backend, V, Fc, col, c2w)
    again = _raster(backend, V, Fc, col, c2w)
    for k in ("tri_id", "depth", "rgb"):
        assert np.array_equal(_bits(base[k].float()), _bits(again[k].float())), k             # two calls: identical bits
    perm = np.random.default_rng(11).permutation(len(Fc))
    got = _raster(backend, V, Fc[perm], col, c2w)
    assert np.array_equal(_bits(got["depth"]), _bits(base["depth"]))
    tie = _s32(V, Fc, col, c2w, (F0, F0), H0, W0)["tie"]
    tid, tid0 = got["tri_id"].cpu().numpy(), base["tri_id"].cpu().numpy()
    back = np.where(tid >= 0, perm[np.maximum(tid, 0)], -1)
    assert np.array_equal(back[~tie], tid0[~tie]) and tie.mean() < 0.02
    assert np.array_equal(_bits(got["rgb"])[~tie], _bits(base["rgb"])[~tie])


@pytest.mark.parametrize("backend", BACKENDS)
def test_ties_and_nearer_surfaces(backend):
    cam = _identity_camera()
    tri = np.array([_pixel_vertex(5, 5), _pixel_vertex(60, 9), _pixel_vertex(20, 50)], f32)
    col = np.random.default_rng(12).random((6, 3)).astype(f32)
    got = _raster(backend, np.concatenate([tri, tri]), np.array([(3, 4, 5), (0, 1, 2)], np.int32), col, cam, focal=QUAD_FOCAL)
    tid = got["tri_id"].cpu().numpy()
    assert (tid >= 0).sum() > 500 and (tid[tid >= 0] == 0).all()      # coplanar duplicates: the lower index
    V = np.concatenate([_quad(2.0), _quad(4.0)])
    col = np.random.default_rng(13).random((8, 3)).astype(f32)
    near, far = [(0, 1, 2), (0, 2, 3)], [(4, 5, 6), (4, 6, 7)]
    for Fc, want_ids in ((near + far, {0, 1}), (far + near, {2, 3})):
        got = _raster(backend, V, np.array(Fc, np.int32), col, cam, focal=QUAD_FOCAL)
        assert set(np.unique(got["tri_id"].cpu().numpy())) == want_ids
        assert _flat_depth_ok(got["depth"], 2.0)
        _same(got, _s32(V, Fc, col, cam, QUAD_FOCAL, H0, W0))


# ---- 5. edges of the domain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw,shift", [((37, 53), 0.0), ((1, 1), 0.0), ((72, 96), 1.0), ((72, 96), 5.0)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_odd_sizes_and_meshes_off_screen(backend, hw, shift):
    V, Fc, col = _sphere()
    c2w = _camera(3, shift=shift)
    focal = (F0, F0) if hw != (37, 53) else (70.0, 75.0)
    want = _s32(V, Fc, col, c2w, focal, *hw)
    share = (want["tri_id"] >= 0).mean()
    assert {0.0: share > 0.2, 1.0: 0.02 < share < 0.2, 5.0: share == 0}[shift]
    got = _raster(backend, V, Fc, col, c2w, focal=focal, H=hw[0], W=hw[1])
    _same(got, want)
    assert tuple(got["rgb"].shape) == (*hw, 3) and tuple(got["depth"].shape) == hw


@pytest.mark.parametrize("backend", BACKENDS)
def test_dropped_triangles_leave_the_others_alone(backend):
    V, Fc, col = _sphere()
    c2w = _camera(0)
    Q, t = c2w[:3, :3].astype(float), c2w[:3, 3].astype(float)
    base = _s32(V, Fc, col, c2w, (F0, F0), H0, W0)
    extra_col = np.concatenate([col, np.array([[0.5, 0.5, 0.5]], f32)])
    bad_vertices = {"behind": t - Q[:, 2], "nan": [np.nan, 0.0, 0.0], "beyond 2^21": t + Q @ np.array([1000.0, 0.0, 0.01]),
                    "at z_near": t + Q @ np.array([0.0, 0.0, 1e-3 * 0.5])}
    for name, p in bad_vertices.items():
        V2 = np.concatenate([V, np.array([p], f32)])
        F2 = np.concatenate([Fc, np.array([(0, 66, 1)], np.int32)])
        got = _raster(backend, V2, F2, extra_col, c2w)
        _same(got, dict(base, dropped=(1, 0)))
        _same(got, _s32(V2, F2, extra_col, c2w, (F0, F0), H0, W0))
    for bad in (-1, 66):
        F2 = np.concatenate([np.array([(0, bad, 1)], np.int32), Fc])
        got = _raster(backend, V, F2, col, c2w)
        _same(got, dict(base, tri_id=np.where(base["tri_id"] >= 0, base["tri_id"] + 1, -1), dropped=(0, 1)))
    F2 = np.concatenate([Fc, np.array([(0, 0, 1), (5, 5, 5)], np.int32)])      # zero area: skipped silently
    _same(_raster(backend, V, F2, col, c2w), base)


@pytest.mark.parametrize("backend", BACKENDS)
def test_empty_meshes_no_colours_and_the_background(backend):
    V, Fc, col = _sphere()
    c2w = _camera(0)
    bg = [0.25, 0.5, 0.75]
    for Vx, Fx, cx in ((V, np.zeros((0, 3), np.int32), col), (np.zeros((0, 3), f32), np.zeros((0, 3), np.int32), np.zeros((0, 3), f32))):
        got = _raster(backend, Vx, Fx, cx, c2w, background=bg)
        assert (got["tri_id"] == -1).all() and torch.isnan(got["depth"]).all() and not got["mask"].any()
        assert np.array_equal(got["rgb"].cpu().numpy(), np.broadcast_to(np.array(bg, f32), (H0, W0, 3)))
        assert got["dropped"] == {"behind_or_far": 0, "bad_index": 0}
    want = _s32(V, Fc, col, c2w, (F0, F0), H0, W0, background=bg)
    got = _raster(backend, V, Fc, col, c2w, background=bg)
    _same(got, want)
    assert np.array_equal(got["rgb"].cpu().numpy()[want["tri_id"] < 0], np.broadcast_to(np.array(bg, f32), ((want["tri_id"] < 0).sum(), 3)))
    plain = _raster(backend, V, Fc, None, c2w)
    assert "rgb" not in plain and sorted(plain) == ["depth", "dropped", "mask", "tri_id"]
    _same(plain, want, rgb=False)
    # numpy float64 / int64 inputs, as extract_geometry and extract_color return them
    path, dev = _lib_and_dev(backend)
    cam, foc = torch.from_numpy(c2w).to(dev), torch.tensor([F0, F0], device=dev)
    got = cn.rasterize_mesh(V.astype(np.float64), Fc.astype(np.int64), cam, foc, H0, W0, colors=col.astype(np.float64), background=bg, library=path)
    assert got["depth"].device.type == torch.device(dev).type
    _same(got, want)


# ---- 6. ABI ----------------------------------------------------------------------------------------------------------------------------------
def _abi_call(backend):
    """(lib, args: dict of the entry point's arguments in order, keep-alive list) of a valid call on the standard view"""
    path, dev = _lib_and_dev(backend)
    lib = cn.load_library(path)
    V, Fc, col = _sphere()
    t = lambda a: torch.from_numpy(np.array(a)).to(dev)
    v, f, c, cam, foc = t(V), t(Fc), t(col), t(_camera(0)), torch.tensor([F0, F0], dtype=torch.float32, device=dev)
    rgb, depth = torch.empty(H0, W0, 3, device=dev), torch.empty(H0, W0, device=dev)
    tid, dropped = torch.empty(H0, W0, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    nb = lib.lib.cnr_mesh_raster_scratch_bytes(66, 128, H0, W0)
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    args = dict(vertices=p(v), n_vertices=66, triangles=p(f), n_triangles=128, colors=p(c), c2w=p(cam), focal=p(foc), H=H0, W=W0, opengl=0,
                origin=None, radius=1.0, z_near=1e-3, background=None, rgb=p(rgb), depth=p(depth), tri_id=p(tid), dropped=p(dropped),
                scratch=p(scratch), scratch_bytes=nb, stream=_lib.stream_of(v))
    return lib, args, (v, f, c, cam, foc, rgb, depth, tid, dropped, scratch)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_scratch_and_errors(backend):
    lib, args, keep = _abi_call(backend)
    assert lib.lib.cnr_abi_version() == 9
    nb = args["scratch_bytes"]
    assert nb > 0 and nb % 256 == 0
    lib.call("cnr_mesh_raster", *args.values())                      # exactly the queried size
    V, Fc, col = _sphere()
    want = _s32(V, Fc, col, _camera(0), (F0, F0), H0, W0)
    assert np.array_equal(keep[7].cpu().numpy(), want["tri_id"]) and np.array_equal(_bits(keep[5]), _bits(want["rgb"]))
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        with pytest.raises(RuntimeError, match="too small"):
            lib.call("cnr_mesh_raster", *dict(args, scratch_bytes=nb - 256).values())
        assert lib.timing_collect() == []                            # nothing was launched
    finally:
        lib.timing_enable(False)
    null = C.c_void_p(0)
    bad = [dict(H=0), dict(W=0), dict(H=-3), dict(H=65536, W=32768), dict(n_vertices=2 ** 31), dict(n_triangles=2 ** 31), dict(n_vertices=-1),
           dict(vertices=null), dict(triangles=null), dict(c2w=null), dict(focal=null), dict(depth=null), dict(tri_id=null), dict(dropped=null),
           dict(scratch=null), dict(rgb=null), dict(colors=null)]
    for change in bad:
        with pytest.raises(RuntimeError, match=r"cnr_mesh_raster failed: \S") as e:
            lib.call("cnr_mesh_raster", *dict(args, **change).values())
        assert "mesh_raster" in str(e.value), change
    for sizes in ((66, 128, 0, W0), (66, 128, 65536, 32768), (2 ** 31, 128, H0, W0), (66, 2 ** 31, H0, W0)):
        assert lib.lib.cnr_mesh_raster_scratch_bytes(*sizes) == 0
    lib.call("cnr_mesh_raster", *dict(args, rgb=null, colors=null).values())      # both null: depth and tri_id only
    assert np.array_equal(keep[7].cpu().numpy(), want["tri_id"])


def test_cpu_tensors_need_an_explicit_library():
    if not os.path.isfile(cn.library_path()):
        pytest.skip("HIP library not built")
    V, Fc, col = _sphere()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.rasterize_mesh(torch.from_numpy(V.copy()), torch.from_numpy(Fc.copy()), torch.from_numpy(_camera(0)), torch.tensor([F0, F0]), H0, W0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.mesh_view_metrics(V, Fc, col, _camera(0), [F0, F0], np.zeros((H0, W0, 3), f32))


# ---- 7. mesh_view_metrics --------------------------------------------------------------------------------------------------------------------
def _read_png(path):
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, {}
    while at < len(raw):
        (n,) = struct.unpack(">I", raw[at:at + 4])
        tag, data = raw[at + 4:at + 8], raw[at + 8:at + 8 + n]
        assert struct.unpack(">I", raw[at + 8 + n:at + 12 + n])[0] == (zlib.crc32(tag + data) & 0xffffffff)
        chunks[tag] = data
        at += 12 + n
    w, h, depth, ctype = struct.unpack(">IIBB", chunks[b"IHDR"][:10])
    assert (depth, ctype) == (8, 2)
    rows = np.frombuffer(zlib.decompress(chunks[b"IDAT"]), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].reshape(h, w, 3)


@pytest.mark.parametrize("backend", BACKENDS)
def test_mesh_view_metrics(backend, tmp_path):
    path, dev = _lib_and_dev(backend)
    V, Fc, col = _sphere()
    c2w = _camera(1)
    bg = [0.2, 0.3, 0.4]
    view = _raster(backend, V, Fc, col, c2w, background=bg)
    cam, foc = torch.from_numpy(c2w).to(dev), torch.tensor([F0, F0], device=dev)
    png = str(tmp_path / "view.png")
    m = cn.mesh_view_metrics(V.copy(), Fc.copy(), col.copy(), cam, foc, view["rgb"], mask=view["mask"].float(), background=bg, path=png, library=path)
    assert all(type(v) is float for v in m.values()) and sorted(m) == ["iou", "psnr", "ssim"]
    same = cn.image_metrics(view["rgb"], view["rgb"], library=path)
    assert m["psnr"] == float("inf") == float(same["psnr"]) and m["iou"] == 1.0
    # SSIM of identical images: num == den up to the 1e-12 in the denominator, den >= 1e-4 * 9e-4: at most 1.2e-5 below 1
    assert m["ssim"] == float(same["ssim"]) and abs(m["ssim"] - 1.0) <= 2e-5
    pic = _read_png(png)
    assert pic.shape == (H0, 3 * W0, 3)
    assert np.array_equal(pic, cn.panel(view["rgb"], view["rgb"], view["depth"], library=path).cpu().numpy())
    # a perturbed ground truth, and a mask that is not the silhouette
    g = torch.Generator().manual_seed(3)
    gt = (view["rgb"].cpu() + 0.05 * torch.randn(H0, W0, 3, generator=g)).clamp(0.0, 1.0).to(dev)
    m = cn.mesh_view_metrics(V.copy(), Fc.copy(), col.copy(), cam, foc, gt.permute(2, 0, 1), background=bg, library=path)
    ref = cn.image_metrics(view["rgb"], gt, library=path)
    assert sorted(m) == ["psnr", "ssim"] and m["psnr"] == float(ref["psnr"]) and m["ssim"] == float(ref["ssim"]) and 20 < m["psnr"] < 40
    mask = torch.zeros(H0, W0)
    mask[:, : W0 // 2] = 1.0
    m = cn.mesh_view_metrics(V.copy(), Fc.copy(), col.copy(), cam, foc, gt, mask=mask.to(dev), background=bg, library=path)
    rm, mm = view["mask"].cpu().numpy(), mask.numpy() > 0
    assert m["iou"] == (rm & mm).sum() / (rm | mm).sum() and 0.0 < m["iou"] < 1.0
    comp = torch.where(mask.to(dev)[..., None] > 0, gt, torch.tensor(bg, device=dev).expand(H0, W0, 3)).contiguous()
    ref = cn.image_metrics(view["rgb"], comp, library=path)
    assert m["psnr"] == float(ref["psnr"]) and m["ssim"] == float(ref["ssim"])


# ---- 8. render_mesh_view; HIP against the emulation at size ---------------------------------------------------------------------------------
def _tiny_renderer(library, dev):
    fx = G.load("tiny_sharp")
    ocfg, P = G.weights_of("tiny_sharp", fx)
    return N.make_renderer(ocfg, P, library, dev)


VIEW_FOCAL = 250.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_render_mesh_view(backend):
    """lattice -> iso-surface -> vertex colours -> raster without leaving the device; the pieces are the public ones"""
    path, dev = _lib_and_dev(backend)
    r = _tiny_renderer(path, dev)
    cam, foc = torch.from_numpy(_camera(4)).to(dev), torch.tensor([40.0, 40.0], device=dev)
    out = r.render_mesh_view([-1.0] * 3, [1.0] * 3, 16, cam, foc, 36, 48, background=[1.0, 1.0, 1.0])
    verts, tris = r.extract_geometry([-1.0] * 3, [1.0] * 3, dev, 16)
    assert len(tris) > 0 and np.array_equal(out["vertices"].cpu().numpy().astype(np.float64), verts) and out["colors"].device.type == torch.device(dev).type
    assert np.array_equal(out["colors"].cpu().numpy(), r.extract_color(verts, dev))
    want = _s32(verts, tris, out["colors"].cpu().numpy(), _camera(4), (40.0, 40.0), 36, 48, background=[1.0, 1.0, 1.0])
    assert (want["tri_id"] >= 0).mean() > 0.05
    _same(out, want)


@pytest.mark.gpu
def test_hip_against_the_emulation_at_size():
    assert torch.cuda.is_available(), "needs a GPU"
    r = _tiny_renderer(None, "cuda:0")
    c2w = _camera(5)
    cam, foc = torch.from_numpy(c2w).cuda(), torch.tensor([VIEW_FOCAL, VIEW_FOCAL], device="cuda:0")
    out = r.render_mesh_view([-1.0] * 3, [1.0] * 3, 64, cam, foc, 240, 320)
    assert out["triangles"].shape[0] > 1000 and out["mask"].float().mean() > 0.05 and out["dropped"] == {"behind_or_far": 0, "bad_index": 0}
    emu = cn.rasterize_mesh(out["vertices"].cpu(), out["triangles"].cpu(), torch.from_numpy(c2w), foc.cpu(), 240, 320, colors=out["colors"].cpu(),
                            library=N.EMU_LIB)
    assert np.array_equal(out["tri_id"].cpu().numpy(), emu["tri_id"].numpy())
    assert np.array_equal(_nan_canon(out["depth"]), _nan_canon(emu["depth"]))
    assert np.array_equal(_bits(out["rgb"]), _bits(emu["rgb"]))
