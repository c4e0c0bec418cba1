"""ICP registration (cnr_icp), color_neus_amd.registration (icp, Registration, apply_transform) and align= of the metric functions.

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The yardsticks are written here and
use nothing from the library:

  SPEC   the comment block of cnr_icp in include/colorneus_render.h restated in numpy and Python floats: the fp32 move (numpy float32
         arithmetic: one IEEE rounding per operation), the searches' SPEC (the cloud search written here, the mesh search test_surface_metrics'
         restatement of cnr_point_mesh_distance's header), the inlier rule, the 256-chunk tree and the sequential chunk add in numpy float64,
         and the Horn / Jacobi solve in Python floats (IEEE doubles; math.sqrt is correctly rounded).  The library must match it BITWISE:
         idx, dist2, moved, matched, every history row and the 16 doubles of the transform.
  Y64    an independent solve for the inlier pairs of one iteration: Umeyama's method by np.linalg.svd with the determinant fix, in float64,
         on moments summed with math.fsum.  The library's s*R and t must agree with it within 16 x the yardstick's own sensitivity -- the
         largest difference between the yardstick and itself when its moments are summed by plain float64 addition in reversed order --
         with a floor of 2^-40 x the target's extent (16: Horn / Jacobi and an SVD round differently).  Collinear and planar inlier sets
         are compared by the residual sum |s R a + t - b|^2 only: the rotation is not unique there.
  YICP   the yardstick's own ICP (float64 nearest neighbours, the Y64 solve), for the recovery cases.

Launch constants the shapes are built around: the cloud search takes 1024 queries per workgroup and 1024 targets per LDS tile (cnr_nn.hip),
the mesh search 512 queries per workgroup and 256 faces per tile (cnr_surface.hip), the moments 256 points per chunk (cnr_register.h)."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import color_neus_amd as cn
from color_neus_amd import _lib
import _native as N
from test_surface_metrics import _spec_distance as _spec_mesh_search      # the SPEC of cnr_point_mesh_distance (numpy, nothing of the library)

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
CHUNK, TERMS, SWEEPS = 256, 18, 10
f32, f64 = np.float32, np.float64
INF = float("inf")
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], f64)


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- SPEC ------------------------------------------------------------------------------------------------------------------------------------------
def _spec_cloud_search(Q, T):
    """cnr_nn_search's rule: d2 = (dx*dx + dy*dy) + dz*dz in float32, the first strictly smaller d2 from +inf on wins (the lowest index of
    equal minima; a NaN never wins); a query that took nothing takes the first d2 == +inf; else NaN (all bits set) and -1."""
    Q, T = np.asarray(Q, f32), np.asarray(T, f32)
    n = Q.shape[0]
    dist2, idx = np.empty(n, f32), np.empty(n, np.int32)
    step = max(1, 4_000_000 // T.shape[0])
    with np.errstate(all="ignore"):
        for q0 in range(0, n, step):
            q = Q[q0:q0 + step]
            dx, dy, dz = (q[:, None, k] - T[None, :, k] for k in range(3))
            d2 = (dx * dx + dy * dy) + dz * dz
            assert d2.dtype == f32
            finite = d2 < f32(np.inf)
            best = np.where(finite, d2, f32(np.inf)).min(1)
            first = np.argmax(finite & (d2 == best[:, None]), 1)
            first_inf = np.argmax(d2 == f32(np.inf), 1)
            any_fin, any_inf = finite.any(1), (d2 == f32(np.inf)).any(1)
            idx[q0:q0 + step] = np.where(any_fin, first, np.where(any_inf, first_inf, -1))
            dist2[q0:q0 + step] = np.where(any_fin, best, np.where(any_inf, f32(np.inf), np.uint32(0xFFFFFFFF).view(f32)))
    return dist2, idx


def _spec_jacobi(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    den = abs(theta) + math.sqrt(theta * theta + 1.0)
    t = -1.0 / den if theta < 0.0 else 1.0 / den
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[p][p] = A[p][p] - h
    A[q][q] = A[q][q] + h
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r != p and r != q:
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
    for r in range(4):
        vrp, vrq = V[r][p], V[r][q]
        V[r][p] = c * vrp - s * vrq
        V[r][q] = s * vrp + c * vrq


def _spec_solve(S, n_inliers, c_src, c_tgt, with_scale):
    """step 4 of the header in Python floats: (status, the 16 doubles or None)"""
    S = [float(v) for v in S]
    if n_inliers < 3 or not all(math.isfinite(v) for v in S):
        return 1, None
    n = float(n_inliers)
    abar, bbar = [S[k] / n for k in range(3)], [S[3 + k] / n for k in range(3)]
    Cm = [[S[6 + 3 * r + c] - S[3 + r] * abar[c] for c in range(3)] for r in range(3)]
    va = S[15] - ((S[0] * abar[0] + S[1] * abar[1]) + S[2] * abar[2])
    if not va > 0.0:
        return 1, None
    Sxx, Sxy, Sxz, Syx, Syy, Syz, Szx, Szy, Szz = Cm[0][0], Cm[1][0], Cm[2][0], Cm[0][1], Cm[1][1], Cm[2][1], Cm[0][2], Cm[1][2], Cm[2][2]
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0], A[0][1], A[0][2], A[0][3] = (Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx
    A[1][1], A[1][2], A[1][3] = (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz
    A[2][2], A[2][3] = (Syy - Sxx) - Szz, Syz + Szy
    A[3][3] = (Szz - Sxx) - Syy
    for r in range(4):
        for c in range(r):
            A[r][c] = A[c][r]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                _spec_jacobi(A, V, p, q)
    best = 0
    for j in range(1, 4):
        if A[j][j] > A[best][best]:
            best = j
    w, x, y, z = (V[r][best] for r in range(4))
    nrm = math.sqrt(((w * w + x * x) + y * y) + z * z)
    w, x, y, z = w / nrm, x / nrm, y / nrm, z / nrm
    if w < 0.0:
        w, x, y, z = -w, -x, -y, -z
    R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
         2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
         2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]
    s = 1.0
    if with_scale:
        tr = R[0] * Cm[0][0]
        for j in range(1, 9):
            tr = tr + R[j] * Cm[j // 3][j % 3]
        s = tr / va
    p = [abar[k] + float(c_src[k]) for k in range(3)]
    t = [(bbar[r] + float(c_tgt[r])) - s * ((R[3 * r] * p[0] + R[3 * r + 1] * p[1]) + R[3 * r + 2] * p[2]) for r in range(3)]
    if not (math.isfinite(s) and s > 0.0 and all(math.isfinite(v) for v in R + t)):
        return 1, None
    return 0, np.array(R + t + [s, 0.0, 0.0, 0.0], f64)


def _spec_icp(src, tgt, tri, pivots, with_scale, max_dist2, iterations, T0, prev_idx=None, stop_at_fixed_point=False):
    """cnr_icp restated: dict(T, history [K, 4], idx, dist2, moved, matched) after `iterations` iterations from the transform T0.  prev_idx: the
    previous call's idx (resume != 0) or None.  stop_at_fixed_point: return early behind an iteration that changed neither a correspondence
    nor the transform's bits against an ungated cloud (every later iteration then repeats it bit for bit; the caller checks that)."""
    src, tgt = np.asarray(src, f32), np.asarray(tgt, f32)
    n = src.shape[0]
    c_src, c_tgt = np.asarray(pivots[:3], f64), np.asarray(pivots[3:], f64)
    T = np.array(T0, f64)
    hist = np.zeros((iterations, 4), f64)
    out = None
    nchunks = (n + CHUNK - 1) // CHUNK
    for k in range(iterations):
        m = [f32(float(T[12]) * float(T[j])) for j in range(9)]
        tf = [f32(T[9 + r]) for r in range(3)]
        x, y, z = src[:, 0], src[:, 1], src[:, 2]
        with np.errstate(all="ignore"):
            moved = np.stack([((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + tf[r] for r in range(3)], 1)
        assert moved.dtype == f32
        if tri is None:
            dist2, idx = _spec_cloud_search(moved, tgt)
            matched = np.where((idx >= 0)[:, None], tgt[np.maximum(idx, 0)], f32(np.nan))
        else:
            dist2, face, matched, _ = _spec_mesh_search(moved, tgt, tri)
            idx = face.astype(np.int32)
        with np.errstate(invalid="ignore"):
            inl = (idx >= 0) & (dist2 <= f32(max_dist2))
        n_changed = n if prev_idx is None else int((idx != prev_idx).sum())
        a = src.astype(f64) - c_src[None]
        b = np.where(inl[:, None], matched, f32(0)).astype(f64) - c_tgt[None]
        terms = np.zeros((nchunks * CHUNK, TERMS), f64)
        rows = np.concatenate([a, b, (b[:, :, None] * a[:, None, :]).reshape(n, 9),
                               ((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])[:, None],
                               ((b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2])[:, None],
                               np.where(inl, dist2, f32(0)).astype(f64)[:, None]], 1)
        terms[:n] = np.where(inl[:, None], rows, 0.0)
        part = terms.reshape(nchunks, CHUNK, TERMS).copy()
        h = CHUNK // 2
        while h >= 1:
            part[:, :h] = part[:, :h] + part[:, h:2 * h]
            h //= 2
        S = np.zeros(TERMS, f64)
        for c in range(nchunks):
            S = S + part[c, 0]
        status, Tn = _spec_solve(S, int(inl.sum()), c_src, c_tgt, with_scale)
        hist[k] = (float(inl.sum()), float(n_changed), S[17], float(status))
        fixed = n_changed == 0 and (Tn is None or _same_bits(Tn, T))
        if Tn is not None:
            T = Tn
        prev_idx = idx
        out = dict(T=T.copy(), history=hist, idx=idx, dist2=dist2, moved=moved, matched=matched.astype(f32), rows_done=k + 1)
        if stop_at_fixed_point and fixed and tri is None and max_dist2 == INF:
            break
    return out


# ---- the library ---------------------------------------------------------------------------------------------------------------------------------
def _abi_icp(path, dev, src, tgt, tri, pivots, with_scale, max_dist2, iterations, T0, resume=0, state=None, fill=0x5A):
    """One cnr_icp call on fresh buffers of `fill` bytes (or on `state`, the buffers of an earlier call: resume): dict like _spec_icp's plus
    the buffers themselves."""
    lib = _lib.resolve_library(path)
    n = src.shape[0]
    p = _lib.ptr
    if state is None:
        mk = lambda shape, dt: torch.full(shape, fill, dtype=torch.uint8, device=dev).view(dt) if int(np.prod(shape)) else torch.empty(0, dtype=dt, device=dev)
        state = dict(moved=mk((n, 12), torch.float32).view(n, 3), matched=mk((n, 12), torch.float32).view(n, 3), dist2=mk((n * 4,), torch.float32),
                     idx=mk((n * 4,), torch.int32), keys=mk((n * 8,), torch.int64), partials=mk(((n + CHUNK - 1) // CHUNK, TERMS * 8), torch.float64),
                     T=_t(np.array(T0, f64), dev))
    hist = torch.full((max(iterations, 1), 32), fill, dtype=torch.uint8, device=dev).view(torch.float64)
    s, t = _t(np.asarray(src, f32), dev), _t(np.asarray(tgt, f32), dev)
    tr = _t(np.asarray(tri, np.int32), dev) if tri is not None else None
    piv = torch.from_numpy(np.ascontiguousarray(np.asarray(pivots, f64)))
    lib.call("cnr_icp", p(s), n, p(t), t.shape[0], p(tr), 0 if tr is None else tr.shape[0], p(piv), int(with_scale), float(max_dist2), iterations, resume,
             p(state["T"]), p(hist), p(state["moved"]), p(state["matched"]), p(state["dist2"]), p(state["idx"]), p(state["keys"]), p(state["partials"]),
             _lib.stream_of(torch.device(dev)))
    if dev != "cpu":
        torch.cuda.synchronize()
    g = lambda x: x.detach().cpu().numpy().copy()
    return dict(T=g(state["T"]), history=g(hist)[:iterations], idx=g(state["idx"]), dist2=g(state["dist2"]), moved=g(state["moved"]),
                matched=g(state["matched"]), state=state)


def _assert_same(got, want, what=("T", "history", "idx", "dist2", "moved", "matched")):
    for k in what:
        a, b = got[k], want[k]
        if k == "history":
            b = b[:a.shape[0]]
        assert _same_bits(a, b), (k, a.ravel()[:8], b.ravel()[:8])


def _pivots(src, tgt):
    return np.concatenate([np.asarray(src, f64).mean(0), np.asarray(tgt, f64).mean(0)])


def _rot(axis, deg):
    axis = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    a = math.radians(deg)
    return np.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _T16(R, t, s):
    return np.concatenate([np.asarray(R, f64).reshape(9), np.asarray(t, f64), [s, 0.0, 0.0, 0.0]])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def _shape(n, seed):
    """the recovery cases' closed surface: an ellipsoid with one bump, float32"""
    d = np.random.default_rng(seed).normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * np.array([0.5, 0.35, 0.2]) + 0.15 * np.exp(-8 * ((d - np.array([0.6, 0.64, 0.48])) ** 2).sum(1))[:, None] * d
    return p.astype(f32)


@functools.lru_cache(maxsize=None)
def _cloud_case(n_source, n_target):
    """n_target random target points in a box; the source: target points (cycled) pushed through a moderate similarity plus noise"""
    rng = np.random.default_rng(1000 * n_source + n_target)
    tgt = (rng.uniform(-1, 1, (n_target, 3)) * np.array([0.6, 0.4, 0.3])).astype(f32)
    pick = tgt[np.arange(n_source) % n_target].astype(f64) + rng.normal(0, 0.01, (n_source, 3))
    R, s, t = _rot((1, 2, 3), 6.0), 1.05, np.array([0.02, -0.01, 0.03])
    src = ((pick - t) @ R / s).astype(f32)
    return src, tgt


@functools.lru_cache(maxsize=None)
def _bump_mesh():
    """a 24 x 24 vertex grid over [-0.5, 0.5]^2 with an off-centre bump and a slope: 23 * 23 * 2 = 1058 faces"""
    k = 24
    gx, gy = np.meshgrid(np.linspace(-0.5, 0.5, k), np.linspace(-0.5, 0.5, k), indexing="ij")
    gz = 0.25 * np.exp(-12 * ((gx - 0.13) ** 2 + (gy + 0.08) ** 2)) + 0.1 * gx * gy + 0.12 * np.exp(-30 * ((gx + 0.3) ** 2 + (gy - 0.25) ** 2))
    V = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1).astype(f32)
    at = lambda i, j: i * k + j
    tris = []
    for i in range(k - 1):
        for j in range(k - 1):
            tris += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    T = np.asarray(tris, np.int32)
    assert T.shape[0] == 1058
    return V, T


@functools.lru_cache(maxsize=None)
def _closed_mesh():
    """the recovery cases' bumped ellipsoid as a closed mesh: a 14 x 24 latitude / longitude grid and two poles, 672 faces.  Unlike the nearly
    flat bump patch it cannot slide along itself, so a point-to-surface ICP settles in a few iterations."""
    nu, nv = 14, 24
    th = np.linspace(0, np.pi, nu + 2)[1:-1]
    ph = np.arange(nv) * (2 * np.pi / nv)
    d = np.stack([np.outer(np.sin(th), np.cos(ph)).ravel(), np.outer(np.sin(th), np.sin(ph)).ravel(), np.outer(np.cos(th), np.ones(nv)).ravel()], 1)
    d = np.concatenate([d, [[0, 0, 1.0], [0, 0, -1.0]]])
    V = (d * np.array([0.5, 0.35, 0.2]) + 0.15 * np.exp(-8 * ((d - np.array([0.6, 0.64, 0.48])) ** 2).sum(1))[:, None] * d).astype(f32)
    at = lambda i, j: i * nv + (j % nv)
    top, bottom = nu * nv, nu * nv + 1
    tris = []
    for j in range(nv):
        tris.append([top, at(0, j), at(0, j + 1)])
        tris.append([bottom, at(nu - 1, j + 1), at(nu - 1, j)])
        for i in range(nu - 1):
            tris += [[at(i, j), at(i + 1, j), at(i + 1, j + 1)], [at(i, j), at(i + 1, j + 1), at(i, j + 1)]]
    return V, np.asarray(tris, np.int32)


def _mesh_samples(n, seed, mesh=None):
    """n points on the bump mesh, or on `mesh` (uniform barycentric draws on random faces: good enough as query points), float64"""
    V, T = mesh or _bump_mesh()
    rng = np.random.default_rng(seed)
    f = rng.integers(0, T.shape[0], n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    a, b, c = (V[T[f, k]].astype(f64) for k in range(3))
    return a + u[:, None] * (b - a) + v[:, None] * (c - a)


# ---- SPEC: bitwise -----------------------------------------------------------------------------------------------------------------------------------
N_SOURCE = [1, 3, 255, 256, 257, 1023, 1025, 2051]
N_TARGET = [1, 1023, 1025, 3000]


@pytest.mark.parametrize("n_target", N_TARGET)
@pytest.mark.parametrize("n_source", N_SOURCE)
@pytest.mark.parametrize("backend", BACKENDS)
def test_cloud_target_restates_the_header_bitwise(backend, n_source, n_target):
    """S1.  Rigid and with scale, three iterations from the identity, around every launch constant: 256 points per moment chunk, 1024 queries
    per workgroup, 1024 targets per tile (3000: three tiles, a split candidate range).  One target point (or fewer than three source points)
    is the degenerate solve: status 1, the transform untouched -- the SPEC says so too."""
    path, dev = _lib_and_dev(backend)
    src, tgt = _cloud_case(n_source, n_target)
    piv = _pivots(src, tgt)
    for with_scale in (0, 1):
        want = _spec_icp(src, tgt, None, piv, with_scale, INF, 3, IDENTITY)
        got = _abi_icp(path, dev, src, tgt, None, piv, with_scale, INF, 3, IDENTITY)
        _assert_same(got, want)
        assert got["history"][0, 1] == n_source and (got["history"][:, 0] == n_source).all()
        if n_source < 3 or (n_target == 1 and with_scale):
            assert (got["history"][:, 3] == 1).all() and _same_bits(got["T"], IDENTITY)
        elif n_target > 1:
            assert (got["history"][:, 3] == 0).all() and not _same_bits(got["T"], IDENTITY)
            assert got["history"][1, 2] < got["history"][0, 2]


@pytest.mark.parametrize("n_source", [1, 3, 255, 256, 257, 511, 512, 513, 1023, 1025, 2051])
@pytest.mark.parametrize("backend", BACKENDS)
def test_mesh_target_restates_the_header_bitwise(backend, n_source):
    """S2.  The mesh target (1058 faces: five tiles of 256), rigid and with scale, from a transform that is not the identity; matched is the
    closest point on the matched face.  The sizes of the cloud case (the 256-point moment chunk, 1023 / 1025, 2051) and the boundary of the
    surface search's 512 queries per workgroup (511, 512, 513).  One source point is the degenerate solve."""
    path, dev = _lib_and_dev(backend)
    V, T = _bump_mesh()
    R, s, t = _rot((2, -1, 1), 5.0), 1.04, np.array([0.02, 0.01, -0.015])
    src = ((_mesh_samples(n_source, 7) - t) @ R / s).astype(f32)
    piv = _pivots(src, V)
    T0 = _T16(_rot((0, 0, 1), 1.0), (0.001, 0.0, 0.002), 1.01)
    for with_scale in (0, 1):
        want = _spec_icp(src, V, T, piv, with_scale, INF, 3, T0)
        got = _abi_icp(path, dev, src, V, T, piv, with_scale, INF, 3, T0)
        _assert_same(got, want)
        assert (got["history"][:, 3] == (1 if n_source < 3 else 0)).all() and (got["idx"] >= 0).all() and (got["idx"] < 1058).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_mesh_target_sum_of_squares_does_not_increase(backend):
    """S3.  Samples of the bump mesh under a 5 degree / 0.02 map, registered back to the mesh.  With exact closest points every iteration can only
    lower the sum of squared distances: the solve minimises it for the current closest points, and the next closest points are no farther.  The
    test's own float64 closest-point ICP shows it on these inputs first (so bad inputs are told apart from a bad library); the library must then
    equal SPEC bitwise and its fp32 sums must not increase either.  Twelve iterations: the yardstick's sum falls from 2.6e-1 to 1.4e-2, by 9 % or
    more per iteration (the patch is nearly flat and slides slowly), far above the fp32 rounding of the distances (1e-7 relative): an increase
    would not be rounding."""
    path, dev = _lib_and_dev(backend)
    V, T = _bump_mesh()
    R, t = _rot((1, 2, 3), 5.0), np.array([0.02, -0.012, 0.016])
    src = ((_mesh_samples(600, 11) - t) @ R).astype(f32)
    piv = _pivots(src, V)
    iters = 12
    sums, Ty = _yard_mesh_icp(src.astype(f64), V, T, iters)
    print("yardstick sums:", " ".join(f"{v:.3e}" for v in sums))
    assert all(sums[k + 1] < sums[k] for k in range(iters - 1))
    want = _spec_icp(src, V, T, piv, 0, INF, iters, IDENTITY)
    got = _abi_icp(path, dev, src, V, T, piv, 0, INF, iters, IDENTITY)
    _assert_same(got, want)
    h = got["history"]
    print("library sums:  ", " ".join(f"{v:.3e}" for v in h[:, 2]))
    assert (h[:, 3] == 0).all() and all(h[k + 1, 2] <= h[k, 2] for k in range(iters - 1))


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_gate(backend):
    """S4.  max_dist2 finite: some points gated out, all of them, all but two (fewer than three inliers: status 1, transform untouched)."""
    path, dev = _lib_and_dev(backend)
    src, tgt = _cloud_case(1025, 1023)
    piv = _pivots(src, tgt)
    d2 = np.sort(_spec_icp(src, tgt, None, piv, 0, INF, 1, IDENTITY)["dist2"])
    assert d2[0] > 0 and d2[1] < d2[2] and d2[511] < d2[512]
    for gate, inliers, status in ((float(d2[511]), 512, 0), (float(d2[0]) * 0.5, 0, 1), (float(d2[1]), 2, 1), (float(d2[-1]), 1025, 0), (0.0, 0, 1)):
        want = _spec_icp(src, tgt, None, piv, 1, gate, 2, IDENTITY)
        got = _abi_icp(path, dev, src, tgt, None, piv, 1, gate, 2, IDENTITY)
        _assert_same(got, want)
        assert got["history"][0].tolist()[:2] == [inliers, 1025] and got["history"][0, 3] == status, (gate, got["history"])
        assert _same_bits(got["T"], IDENTITY) == bool(status)
        if status:
            assert got["history"][1].tolist() == [inliers, 0.0, got["history"][0, 2], 1.0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_nan_points_and_equal_points(backend):
    """S5.  A source point with a NaN coordinate has no candidate: idx -1, NaN dist2 / moved / matched, never an inlier.  All source points equal:
    no extent (va = 0), status 1 and the transform exactly as it was, identity or not."""
    path, dev = _lib_and_dev(backend)
    src, tgt = _cloud_case(257, 1025)
    src = src.copy()
    src[5, 1] = np.nan
    src[256] = np.nan
    piv = _pivots(np.nan_to_num(src), tgt)
    for tri, target in ((None, tgt), (_bump_mesh()[1], _bump_mesh()[0])):
        want = _spec_icp(src, target, tri, piv, 1, INF, 2, IDENTITY)
        got = _abi_icp(path, dev, src, target, tri, piv, 1, INF, 2, IDENTITY)
        _assert_same(got, want)
        assert got["idx"][5] == -1 and got["idx"][256] == -1 and np.isnan(got["matched"][5]).all() and np.isnan(got["dist2"][256])
        assert got["history"][:, 0].tolist() == [255, 255] and (got["history"][:, 3] == 0).all()
    same = np.tile(np.array([[0.1, -0.2, 0.05]], f32), (300, 1))
    for T0 in (IDENTITY, _T16(_rot((1, 0, 1), 20.0), (0.1, 0.2, 0.3), 0.9)):
        piv = _pivots(same, tgt)
        want = _spec_icp(same, tgt, None, piv, 0, INF, 2, T0)
        got = _abi_icp(path, dev, same, tgt, None, piv, 0, INF, 2, T0)
        _assert_same(got, want)
        assert got["history"].tolist() == [[300.0, 300.0, got["history"][0, 2], 1.0], [300.0, 0.0, got["history"][0, 2], 1.0]]
        assert _same_bits(got["T"], np.array(T0, f64))


@pytest.mark.parametrize("target_kind", ["cloud", "mesh"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_resume_repeat_and_buffer_contents(backend, target_kind):
    """S6.  Seven iterations in one call = three, then four with resume; the same call twice; output buffers that start as 0xFF bytes or as
    0x00 bytes: the same bits everywhere."""
    path, dev = _lib_and_dev(backend)
    if target_kind == "cloud":
        src, tgt = _cloud_case(1025, 3000)
        tri = None
    else:
        tgt, tri = _bump_mesh()
        src = ((_mesh_samples(777, 3) - 0.02) @ _rot((1, 1, 0), 4.0)).astype(f32)
    piv = _pivots(src, tgt)
    gate = 0.05
    one = _abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 7, IDENTITY)
    a = _abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 3, IDENTITY)
    b = _abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 4, None, resume=1, state=a["state"])
    _assert_same(b, one, ("T", "idx", "dist2", "moved", "matched"))
    assert _same_bits(np.concatenate([a["history"], b["history"]]), one["history"])
    assert one["history"][1:, 1].max() < src.shape[0]              # n_changed of the resumed call's first iteration is a count, not n
    _assert_same(_abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 7, IDENTITY), one)
    _assert_same(_abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 3, IDENTITY, fill=0xFF), a)
    _assert_same(_abi_icp(path, dev, src, tgt, tri, piv, 1, gate, 3, IDENTITY, fill=0x00), a)
    _assert_same(a, _spec_icp(src, tgt, tri, piv, 1, gate, 3, IDENTITY))


@pytest.mark.gpu
def test_hip_matches_the_emulation_bitwise():
    """S7.  The two builds against each other, cloud and mesh, more chunks than the other cases (20 000 points: 79 rows of partials)."""
    tgt = _shape(4000, 3)
    src = (_shape(20000, 4).astype(f64) @ _rot((1, 2, 3), 8.0) * 0.95 + 0.01).astype(f32)
    V, T = _bump_mesh()
    msrc = ((_mesh_samples(20000, 9) - 0.01) @ _rot((0, 1, 1), 3.0)).astype(f32)
    for s, t, tri, gate in ((src, tgt, None, 0.01), (msrc, V, T, INF)):
        piv = _pivots(s, t)
        emu = _abi_icp(N.EMU_LIB, "cpu", s, t, tri, piv, 1, gate, 4, IDENTITY)
        hip = _abi_icp(None, "cuda:0", s, t, tri, piv, 1, gate, 4, IDENTITY)
        _assert_same(hip, emu)
        assert (emu["history"][:, 3] == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_argument_checks(backend):
    """S8.  Every refusal with its message; nothing is launched after a refusal or for an empty call, and transform stays untouched."""
    path, dev = _lib_and_dev(backend)
    lib = _lib.resolve_library(path)
    L = lib.lib
    assert L.cnr_abi_version() == _lib.ABI_VERSION == 9
    p, null, stream = _lib.ptr, C.c_void_p(0), _lib.stream_of(torch.device(dev))
    n = 4
    src, tgt = torch.rand(n, 3, device=dev), torch.rand(5, 3, device=dev)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    piv = torch.zeros(6, dtype=torch.float64)
    T = _t(IDENTITY.copy(), dev)
    hist, part = torch.zeros(3, 4, dtype=torch.float64, device=dev), torch.zeros(2, TERMS, dtype=torch.float64, device=dev)
    moved, matched = torch.zeros(n, 3, device=dev), torch.zeros(n, 3, device=dev)
    d2, idx, keys = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n + 1, dtype=torch.int64, device=dev)
    odd = lambda x: C.c_void_p(x.data_ptr() + 4)
    big = 2 ** 31
    call = lambda **kw: (kw.get("src", p(src)), kw.get("n", n), kw.get("tgt", p(tgt)), kw.get("m", 5), kw.get("tri", null), kw.get("F", 0),
                         kw.get("piv", p(piv)), 0, kw.get("gate", INF), kw.get("iters", 2), 0, kw.get("T", p(T)), kw.get("hist", p(hist)),
                         kw.get("moved", p(moved)), kw.get("matched", p(matched)), kw.get("d2", p(d2)), kw.get("idx", p(idx)), kw.get("keys", p(keys)),
                         kw.get("part", p(part)), stream)
    cases = [(dict(n=-1), "n_source must be in"), (dict(n=big), "n_source must be in"), (dict(m=0), "n_target must be in"),
             (dict(m=-3), "n_target must be in"), (dict(m=big), "n_target must be in"), (dict(tri=p(tri), F=-1), "n_triangles must be in"),
             (dict(tri=p(tri), F=big), "n_triangles must be in"), (dict(F=1), "triangles must be null exactly when"),
             (dict(tri=p(tri), F=0), "triangles must be null exactly when"), (dict(iters=-1), "iterations < 0"),
             (dict(gate=float("nan")), "max_dist2 must not be NaN or negative"), (dict(gate=-1.0), "max_dist2 must not be NaN or negative"),
             (dict(T=odd(T)), "8-byte aligned"), (dict(hist=odd(hist)), "8-byte aligned"), (dict(keys=odd(keys)), "8-byte aligned"),
             (dict(part=odd(part)), "8-byte aligned")]
    cases += [({k: null}, "null argument") for k in ("src", "tgt", "piv", "T", "hist", "moved", "matched", "d2", "idx", "keys", "part")]
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        for kw, msg in cases:
            assert L.cnr_icp(*call(**kw)) < 0, kw
            with pytest.raises(RuntimeError, match=msg):
                lib.call("cnr_icp", *call(**kw))
        # no source points, or no iterations: a successful no-op, whatever the other pointers
        assert L.cnr_icp(null, 0, p(tgt), 5, null, 0, null, 0, INF, 2, 0, null, null, null, null, null, null, null, null, stream) == 0
        assert L.cnr_icp(*call(iters=0, hist=null)) == 0
        assert lib.timing_collect() == []
    finally:
        lib.timing_enable(False)
    if dev != "cpu":
        torch.cuda.synchronize()
    assert _same_bits(T.cpu().numpy(), IDENTITY)
    lib.call("cnr_icp", *call())
    lib.call("cnr_icp", *call(tri=p(tri), F=1))
    if dev != "cpu":
        torch.cuda.synchronize()
    assert hist[:2, 0].tolist() == [4.0, 4.0]


def test_header_binding_and_sources_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "colorneus_render.h")).read()
    csrc = os.path.join(root, "color-neus_amd", "csrc")
    assert len(_lib.SIGNATURES["cnr_icp"][1]) == 20 and _lib.SIGNATURES["cnr_icp"][0] is C.c_int
    assert header.count("int cnr_icp(") == 1 and open(os.path.join(csrc, "cnr_ops.cpp")).read().count("\nint cnr_icp(") == 1
    assert not [s for s in _lib.SIGNATURES if s.endswith("_bytes") and "icp" in s]
    reg = open(os.path.join(csrc, "cnr_register.h")).read()
    assert f"constexpr int kIcpChunk = {CHUNK};" in reg and f"constexpr int kIcpTerms = {TERMS};" in reg and f"constexpr int kIcpSweeps = {SWEEPS};" in reg
    assert "cnr_register" in open(os.path.join(csrc, "Makefile")).read().split("HIP_UNITS =")[1].split("\n")[0]


# ---- Y64: an independent solve -------------------------------------------------------------------------------------------------------------------
def _umeyama(a, b, with_scale, exact_sums=True):
    """Umeyama (1991) for b ~ s R a + t: float64, np.linalg.svd, the determinant fix.  exact_sums: the moments by math.fsum; else by plain float64
    addition in REVERSED order (the sensitivity probe).  Returns (s*R, t, R)."""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    n = a.shape[0]
    if exact_sums:
        tot = lambda v: math.fsum(v.tolist())
    else:
        def tot(v):
            s = 0.0
            for x in v.tolist()[::-1]:
                s = s + x
            return s
    abar, bbar = np.array([tot(a[:, k]) / n for k in range(3)]), np.array([tot(b[:, k]) / n for k in range(3)])
    da, db = a - abar, b - bbar
    Sig = np.array([[tot(db[:, r] * da[:, c]) / n for c in range(3)] for r in range(3)])
    var = tot((da * da).sum(1)) / n
    U, D, Vt = np.linalg.svd(Sig)
    fix = np.array([1.0, 1.0, 1.0 if np.linalg.det(U) * np.linalg.det(Vt) > 0 else -1.0])
    R = U @ np.diag(fix) @ Vt
    s = float((D * fix).sum() / var) if with_scale else 1.0
    return s * R, bbar - s * R @ abar, R


def _residual(sR, t, a, b):
    return float((((np.asarray(a, f64) @ sR.T + t) - np.asarray(b, f64)) ** 2).sum())


def _y64_check(T16, a, b, with_scale, extent, unique=True):
    """the library's transform against Y64 on the pairs (a, b); returns the observed difference and the tolerance"""
    sR_y, t_y, _ = _umeyama(a, b, with_scale)
    sR_p, t_p, _ = _umeyama(a, b, with_scale, exact_sums=False)
    sens = max(np.abs(sR_y - sR_p).max(), np.abs(t_y - t_p).max())
    tol = max(16.0 * sens, 2.0 ** -40 * extent)
    R = T16[:9].reshape(3, 3)
    sR, t = T16[12] * R, T16[9:12]
    assert abs(np.linalg.det(R) - 1.0) < 1e-14 and np.abs(R @ R.T - np.eye(3)).max() < 1e-14
    diff = max(np.abs(sR - sR_y).max(), np.abs(t - t_y).max())
    # the residual is stationary at the optimum: a map within tol of it changes the residual in second order only; what remains is the
    # rounding of evaluating a sum of n squares of numbers of size `extent`: n * 2^-52 * extent^2, times 64 for the intermediate sums
    r_lib, r_y = _residual(sR, t, a, b), _residual(sR_y, t_y, a, b)
    r_tol = 64.0 * len(a) * 2.0 ** -52 * extent * extent + 4.0 * len(a) * tol * tol
    assert abs(r_lib - r_y) <= r_tol, (r_lib, r_y, r_tol)
    if unique:
        assert diff <= tol, (diff, tol, sens)
    return diff, tol, sens


def _inlier_pairs(out, src, gate=INF):
    with np.errstate(invalid="ignore"):
        inl = (out["idx"] >= 0) & (out["dist2"] <= f32(gate))
    return src[inl].astype(f64), out["matched"][inl].astype(f64)


@pytest.mark.parametrize("kind", ["cloud", "cloud_gate", "mesh", "mirror", "planar", "collinear"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_solve_against_umeyama_by_svd(backend, kind):
    """Y1.  ONE iteration; the pairs are the library's own correspondence (bitwise SPEC's), the solve is checked against Y64 -- rigid and with
    scale.  `mirror`: the target is the source mirrored in x, the best PROPER rotation is wanted: det R = +1 (checked for every kind) and the
    yardstick's residual.  `planar` / `collinear`: all pairs in a plane / on a line, the residual only.
    Observed |difference| / tolerance (emulation = HIP, the bits are equal): cloud 2.1e-15 / 9.1e-13, cloud_gate 1.9e-15 / 9.1e-13,
    mesh 1.1e-15 / 9.1e-13, mirror 1.6e-15 / 9.1e-13 -- the 2^-40 floor everywhere; the yardstick's own sensitivity is below 1e-15."""
    path, dev = _lib_and_dev(backend)
    tri, gate, unique = None, INF, True
    if kind in ("cloud", "cloud_gate"):
        src, tgt = _cloud_case(1025, 3000)
        gate = 0.002 if kind == "cloud_gate" else INF
    elif kind == "mesh":
        tgt, tri = _bump_mesh()
        src = ((_mesh_samples(700, 21) - 0.015) @ _rot((3, 1, 2), 6.0) / 1.03).astype(f32)
    elif kind == "mirror":
        src = _shape(600, 8)
        tgt = (src * np.array([-1, 1, 1], f32)).astype(f32)
    elif kind == "planar":
        rng = np.random.default_rng(3)
        src = np.concatenate([rng.uniform(-0.5, 0.5, (400, 2)), np.zeros((400, 1))], 1).astype(f32)
        tgt, unique = (src[::2] + np.array([0.01, 0.02, 0.0], f32)).astype(f32), False
    else:
        u = np.linspace(-0.5, 0.5, 300)
        src = np.stack([u, np.zeros_like(u), np.zeros_like(u)], 1).astype(f32)
        tgt, unique = (src[::3] + np.array([0.004, 0.0, 0.0], f32)).astype(f32), False
    piv = _pivots(src, tgt)
    extent = float(np.abs(tgt).max())
    for with_scale in (0, 1):
        got = _abi_icp(path, dev, src, tgt, tri, piv, with_scale, gate, 1, IDENTITY)
        _assert_same(got, _spec_icp(src, tgt, tri, piv, with_scale, gate, 1, IDENTITY))
        assert got["history"][0, 3] == 0
        a, b = _inlier_pairs(got, src, gate)
        assert len(a) == got["history"][0, 0] >= 100
        diff, tol, sens = _y64_check(got["T"], a, b, with_scale, extent, unique)
        print(f"{kind} with_scale={with_scale}: |lib - Y64| = {diff:.2e}, tolerance {tol:.2e} (sensitivity {sens:.2e}), {len(a)} pairs")


# ---- recovery -----------------------------------------------------------------------------------------------------------------------------------------
def _yard_nn(q, t):
    d2 = ((q[:, None, :] - t[None, :, :]) ** 2).sum(2)
    return d2.argmin(1)


def _yard_icp(src, tgt, with_scale, iterations):
    """YICP: float64 nearest neighbours and the Y64 solve, from the identity; (the iteration with no changed correspondence or None, sR, t)"""
    src, tgt = src.astype(f64), tgt.astype(f64)
    sR, t, prev = np.eye(3), np.zeros(3), None
    for k in range(iterations):
        idx = _yard_nn(src @ sR.T + t, tgt)
        if prev is not None and (idx == prev).all():
            return k, sR, t
        sR, t, _ = _umeyama(src, tgt[idx], with_scale)
        prev = idx
    return None, sR, t


def _yard_mesh_closest(q, V, T):
    """the test's own closest points on a mesh in float64 (NOT Ericson's regions): the plane projection where it falls inside the triangle, else the
    nearest point of the three edges; all (point, face) pairs at once"""
    a, b, c = (V[T[:, k]].astype(f64)[None] for k in range(3))           # [1, F, 3]
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
    Q = q[:, None, :]                                                      # [n, 1, 3]
    proj = Q - ((Q - a) * nrm).sum(2, keepdims=True) * nrm
    inside = np.ones(proj.shape[:2], bool)
    cand = [proj]
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        inside &= (np.cross(e, proj - u) * nrm).sum(2) >= 0
        s = np.clip(((Q - u) * e).sum(2) / (e * e).sum(2), 0.0, 1.0)
        cand.append(u + s[:, :, None] * e)
    d = np.stack([((Q - p) ** 2).sum(2) for p in cand], 2)                # [n, F, 4]
    d[:, :, 0] = np.where(inside, d[:, :, 0], np.inf)
    flat = d.reshape(len(q), -1).argmin(1)
    f, j = flat // 4, flat % 4
    rows = np.arange(len(q))
    return d[rows, f, j], np.stack(cand, 2)[rows, f, j]


def _yard_mesh_icp(src, V, T, iterations):
    """rigid float64 ICP to the mesh surface; (the sum of squared distances each iteration STARTED with, the final map)"""
    sR, t, sums = np.eye(3), np.zeros(3), []
    for _ in range(iterations):
        d2, cp = _yard_mesh_closest(src @ sR.T + t, V, T)
        sums.append(float(d2.sum()))
        sR, t, _ = _umeyama(src, cp, False)
    return sums, (sR, t)


@pytest.mark.parametrize("deg,s0", [(10.0, 1.0), (10.0, 1.1), (20.0, 1.0), (20.0, 1.15)])
@pytest.mark.parametrize("backend", BACKENDS)
def test_recovery_of_a_known_map(backend, deg, s0):
    """R1.  Target: 2000 points of the bumped ellipsoid.  Source: every second target point, the first 900, taken through the inverse of the true
    map (rotation about (1, 2, 3), t0 = (0.03, -0.02, 0.04), scale s0), so that the true correspondence exists.  From the identity, at most 60
    iterations.  YICP converges on these inputs first (an iteration without a changed correspondence: measured at 20 / 22 / 36 / 40); then the
    library's trajectory is SPEC's bitwise, it reaches n_changed == 0 as well, every later iteration repeats that one bit for bit, and the
    recovered map is YICP's within the Y64 tolerance -- and the true one within 1e-6 (float32 source coordinates)."""
    path, dev = _lib_and_dev(backend)
    with_scale = int(s0 != 1.0)
    tgt = _shape(2000, 1)
    R0, t0 = _rot((1, 2, 3), deg), np.array([0.03, -0.02, 0.04])
    src = ((tgt[::2][:900].astype(f64) - t0) @ R0 / s0).astype(f32)
    at, sR_y, t_y = _yard_icp(src, tgt, with_scale, 60)
    print(f"{deg} deg, s0 = {s0}: YICP has no changed correspondence at iteration {at}")
    assert at is not None
    piv = _pivots(src, tgt)
    got = _abi_icp(path, dev, src, tgt, None, piv, with_scale, INF, 60, IDENTITY)
    want = _spec_icp(src, tgt, None, piv, with_scale, INF, 60, IDENTITY, stop_at_fixed_point=True)
    k = want["rows_done"]
    h = got["history"]
    print(f"  the library: n_changed == 0 first at iteration {int(np.argmax(h[:, 1] == 0))}, SPEC fixed point after {k} iterations")
    assert k < 60 and _same_bits(h[:k], want["history"][:k]) and (h[:, 3] == 0).all()
    assert all(_same_bits(h[j], h[k - 1]) for j in range(k, 60))
    _assert_same(got, want, ("T", "idx", "dist2", "moved", "matched"))
    assert (got["idx"] == 2 * np.arange(900)).all()
    a, b = src.astype(f64), tgt[got["idx"]].astype(f64)
    diff, tol, _ = _y64_check(got["T"], a, b, with_scale, float(np.abs(tgt).max()))
    sR, t = got["T"][12] * got["T"][:9].reshape(3, 3), got["T"][9:12]
    d_y = max(np.abs(sR - sR_y).max(), np.abs(t - t_y).max())
    d_true = max(np.abs(sR - s0 * R0).max(), np.abs(t - t0).max())
    print(f"  |lib - Y64| = {diff:.2e}, |lib - YICP| = {d_y:.2e} (tolerance {tol:.2e}), |lib - true| = {d_true:.2e}")
    assert d_y <= tol and d_true < 1e-6


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------------------
def _reg_equal(a, b):
    return (torch.equal(a.matrix, b.matrix) and torch.equal(a.history, b.history) and a.converged == b.converged and a.scale == b.scale
            and torch.equal(a.rotation, b.rotation) and torch.equal(a.translation, b.translation))


@pytest.mark.parametrize("backend", BACKENDS)
def test_icp_init_modes(backend):
    """P1.  Every init mode against a torch restatement of the starting transform (iterations=0 returns it), and one iteration from it against
    SPEC; a mesh source is sample_surface's points under the seed."""
    path, dev = _lib_and_dev(backend)
    src, tgt = _cloud_case(1025, 1023)
    s, t = _t(src, dev), _t(tgt, dev)
    cs, ct = s.double().mean(0).cpu(), t.double().mean(0).cpu()
    ms = (s.double().cpu() - cs).norm(dim=1).max().item()
    mt = (t.double().cpu() - ct).norm(dim=1).max().item()
    M = torch.eye(4, dtype=torch.float64)
    M[:3, :3] = torch.from_numpy(1.2 * _rot((0, 1, 0), 30.0))
    M[:3, 3] = torch.tensor([0.1, 0.2, -0.3], dtype=torch.float64)
    want = {None: torch.eye(4, dtype=torch.float64), "centroid": torch.eye(4, dtype=torch.float64), "normalize": torch.eye(4, dtype=torch.float64) * (mt / ms), "matrix": M}
    want["centroid"][:3, 3] = ct - cs
    want["normalize"][3, 3] = 1.0
    want["normalize"][:3, 3] = ct - (mt / ms) * cs
    piv = np.concatenate([cs.numpy(), ct.numpy()])
    for mode in (None, "centroid", "normalize", "matrix"):
        init = M if mode == "matrix" else mode
        r0 = cn.registration.icp(s, t, init=init, iterations=0, library=path)
        assert r0.matrix.dtype == torch.float64 and r0.matrix.device.type == "cpu" and r0.history.shape == (0, 4) and not r0.converged
        assert torch.allclose(r0.matrix, want[mode], rtol=0, atol=1e-15), (mode, r0.matrix, want[mode])
        assert math.isnan(r0.rms)
        r1 = cn.registration.icp(s, t, init=init, iterations=1, with_scale=True, library=path)
        T0 = _T16(r0.rotation.numpy(), r0.translation.numpy(), r0.scale)
        spec = _spec_icp(src, tgt, None, piv, 1, INF, 1, T0)
        assert _same_bits(r1.history.numpy(), spec["history"])
        assert _same_bits(_T16(r1.rotation.numpy(), r1.translation.numpy(), r1.scale), spec["T"])
        assert r1.rms == math.sqrt(spec["history"][0, 2] / spec["history"][0, 0])
        assert torch.equal(r1.matrix[:3, :3], r1.scale * r1.rotation) and torch.equal(r1.matrix[:3, 3], r1.translation) and r1.matrix[3].tolist() == [0, 0, 0, 1]
    V, T = _bump_mesh()
    rm = cn.icp((_t(V, dev), _t(T, dev)), (_t(V, dev), _t(T, dev)), n_samples=500, seed=3, iterations=2, library=path)
    pts = cn.sample_surface(_t(V, dev), _t(T, dev), 500, seed=3, library=path)[0]
    rp = cn.icp(pts, (_t(V, dev), _t(T, dev)), iterations=2, library=path)
    assert _reg_equal(rm, rp) and rm.history[0, 0] == 500 and rm.rms < 1e-6
    mirror, shear, row = M.clone(), M.clone(), M.clone()
    mirror[:3, 0] = -mirror[:3, 0]
    shear[0, 1] += 0.1
    row[3, 0] = 0.5
    for bad in (dict(init="nearest"), dict(iterations=-1), dict(check_every=0), dict(max_dist=-1.0), dict(init=mirror), dict(init=shear), dict(init=row),
                dict(init=torch.zeros(4, 4)), dict(init=torch.eye(3))):
        with pytest.raises(ValueError):
            cn.icp(s, t, library=path, **bad)
    assert cn.icp is cn.registration.icp and cn.Registration is cn.registration.Registration and cn.apply_transform is cn.registration.apply_transform


@pytest.mark.parametrize("backend", BACKENDS)
def test_icp_batching_and_apply(backend):
    """P2.  check_every batches give the Registration of one unbatched call (an ungated cloud target: the iterations behind the fixed point
    repeat it); the history ends with the first row without a changed correspondence; apply is float64 matmul in the input's dtype."""
    path, dev = _lib_and_dev(backend)
    tgt = _shape(2000, 1)
    src = ((tgt[::2][:900].astype(f64) - np.array([0.03, -0.02, 0.04])) @ _rot((1, 2, 3), 10.0)).astype(f32)
    s, t = _t(src, dev), _t(tgt, dev)
    whole = cn.icp(s, t, iterations=40, check_every=None, library=path)
    assert whole.converged and whole.history[-1, 1] == 0 and (whole.history[:-1, 1] > 0).all() and whole.history.shape[0] < 40
    for every in (1, 7, 10, 40):
        assert _reg_equal(cn.icp(s, t, iterations=40, check_every=every, library=path), whole), every
    short = cn.icp(s, t, iterations=5, library=path)
    assert not short.converged and short.history.shape == (5, 4) and torch.equal(short.history, whole.history[:5])
    gated = cn.icp(s, t, iterations=3, max_dist=0.05, library=path)
    d = np.float32(0.05)
    assert _same_bits(gated.history.numpy(), _spec_icp(src, tgt, None, _pivots(src, tgt), 0, float(d * d), 3, IDENTITY)["history"])
    assert 0 < gated.history[0, 0] < 900
    for dt in (torch.float32, torch.float64):
        x = s.to(dt)
        y = whole.apply(x)
        # three products and three additions of numbers below 1 in float64, fused or not (a device matmul may fuse): below 4 * 2^-53; a float32
        # result adds its own rounding, 2^-25 below 1
        ref = x.double().cpu() @ whole.matrix[:3, :3].T + whole.matrix[:3, 3]
        assert float(ref.abs().max()) < 1.0
        assert y.dtype == dt and y.device == x.device and float((y.double().cpu() - ref).abs().max()) <= (2.0 ** -51 if dt == torch.float64 else 2.0 ** -25 + 2.0 ** -51)
        assert torch.equal(cn.apply_transform(x, whole.matrix), y) and torch.equal(cn.apply_transform(x, whole.matrix.tolist()), y)
    assert float((whole.apply(s).cpu() - t.cpu()[::2][:900]).abs().max()) < 1e-6


@pytest.mark.parametrize("backend", BACKENDS)
def test_icp_result_is_one_state_for_every_batching(backend):
    """P2b.  Against a mesh, or with a gate, an iteration without a changed correspondence is not a fixed point, and the rest of its batch
    refines the transform.  Whatever check_every is, the Registration is ONE state: its history is that of a single cnr_icp call of as many
    iterations as it has rows, and its matrix the transform behind them, bit for bit; check_every=1 ends at the stopping row itself."""
    path, dev = _lib_and_dev(backend)
    V, T = _closed_mesh()
    tgt = _shape(400, 6)
    msrc = ((_mesh_samples(300, 5, (V, T)) - 0.002) @ _rot((1, 2, 3), 0.5)).astype(f32)      # small maps: both settle within the 30 iterations
    csrc = ((tgt[::2].astype(f64) - 0.004) @ _rot((1, 2, 3), 2.0)).astype(f32)
    for src, target, tri, gate in ((msrc, (_t(V, dev), _t(T, dev)), T, None), (csrc, _t(tgt, dev), None, 0.05)):
        tv = V if tri is not None else tgt
        d = np.float32(gate) if gate is not None else None
        piv = np.concatenate([_t(src, dev).double().mean(0).cpu().numpy(), _t(tv, dev).double().mean(0).cpu().numpy()])     # icp's own pivots
        rows = {}
        for every in (1, 4, None):
            r = cn.icp(_t(src, dev), target, iterations=30, check_every=every, max_dist=gate, library=path)
            k = r.history.shape[0]
            raw = _abi_icp(path, dev, src, tv, tri, piv, 0, INF if d is None else float(d * d), k, IDENTITY)
            assert _same_bits(r.history.numpy(), raw["history"]), every
            assert _same_bits(_T16(r.rotation.numpy(), r.translation.numpy(), r.scale), raw["T"]), every
            stops = np.nonzero((raw["history"][:, 1] == 0) | (raw["history"][:, 3] != 0))[0]
            assert r.converged == bool(len(stops) and raw["history"][stops[0], 3] == 0)
            rows[every] = k
            if every == 1:
                assert k == (stops[0] + 1 if len(stops) else 30)
            elif every == 4:
                assert k == (min(30, 4 * (stops[0] // 4 + 1)) if len(stops) else 30)
            else:
                assert k == 30
        print("mesh" if tri is not None else "gated cloud", "rows per check_every:", rows)
        assert rows[1] < 30, "the inputs must reach an iteration without a changed correspondence"


@pytest.mark.parametrize("backend", BACKENDS)
def test_metrics_without_align_are_unchanged(backend):
    """P3.  align=None: every metric function returns what it returned before the argument existed -- the same keys, and the values of the
    same composition of searches -- on the inputs tests/test_nn_metrics.py and tests/test_surface_metrics.py use."""
    import test_nn_metrics as tn
    import test_surface_metrics as ts
    path, dev = _lib_and_dev(backend)
    x, y = (c.to(dev) for c in tn._case1())
    m = cn.metrics.mesh_metrics(x, y, library=path)
    assert m == cn.metrics.mesh_metrics(x, y, library=path, align=None)
    d_xy = cn.metrics.nearest_neighbors(x, y, library=path)[0].double()
    d_yx = cn.metrics.nearest_neighbors(y, x, library=path)[0].double()
    assert set(m) == {"accuracy", "completeness", "chamfer_l1", "chamfer_l2"} | {f"{k}@{t}" for k in ("precision", "recall", "fscore") for t in ("0.01", "0.02", "0.05")}
    assert m["accuracy"] == d_xy.sqrt().mean().item() and m["completeness"] == d_yx.sqrt().mean().item()
    cd = cn.metrics.chamfer_distance(x, y, library=path, align=None)
    assert cd.item() == (d_xy.mean() + d_yx.mean()).item() == m["chamfer_l2"] == cn.metrics.chamfer_distance(x, y, library=path).item()
    pred, gt = ts._square(0.0, dev), ts._square(np.float32(0.1), dev, flip=True)
    sm = cn.metrics.surface_metrics(pred, gt, n_samples=4000, seed=5, library=path)
    assert sm == cn.metrics.surface_metrics(pred, gt, n_samples=4000, seed=5, library=path, align=None) and "transform" not in sm
    ps = cn.sample_surface(*pred, 4000, seed=5, library=path)[0]
    gs = cn.sample_surface(*gt, 4000, seed=6, library=path)[0]
    assert sm["accuracy"] == cn.metrics.point_mesh_distance(ps, *gt, library=path)[0].double().sqrt().mean().item()
    assert sm["completeness"] == cn.metrics.point_mesh_distance(gs, *pred, library=path)[0].double().sqrt().mean().item()


@pytest.mark.parametrize("backend", BACKENDS)
def test_metrics_with_align(backend, tmp_path):
    """P4.  surface_metrics of a mesh against a rotated, scaled and shifted copy of itself: an F-score of 1 at the 0.01 threshold with
    align="similarity", not without it; the dict carries the transform and its rms; a Registration or a matrix is applied as given; the cloud
    functions and the PLY helpers take the argument too."""
    path, dev = _lib_and_dev(backend)
    V, T = _closed_mesh()
    R, s0, t0 = _rot((1, 2, 3), 8.0), 1.1, np.array([0.05, -0.03, 0.04])
    G = (V.astype(f64) @ (s0 * R).T + t0).astype(f32)                 # gt = the map of pred
    pred, gt = (_t(V, dev), _t(T, dev)), (_t(G, dev), _t(T, dev))
    kw = dict(n_samples=3000, seed=2, library=path)
    plain = cn.surface_metrics(pred, gt, **kw)
    assert plain["fscore@0.01"] < 0.9 and "transform" not in plain and "align_rms" not in plain
    m = cn.surface_metrics(pred, gt, align="similarity", **kw)
    M = np.array(m["transform"])
    print("fscore@0.01", plain["fscore@0.01"], "->", m["fscore@0.01"], "align_rms", m["align_rms"], "|M - true|", np.abs(M[:3, :3] - s0 * R).max(), np.abs(M[:3, 3] - t0).max())
    assert m["fscore@0.01"] == 1.0 and m["precision@0.01"] == 1.0 and m["recall@0.01"] == 1.0
    assert M.shape == (4, 4) and type(m["transform"]) is list and type(m["align_rms"]) is float and m["align_rms"] < 0.003
    assert set(m) == set(plain) | {"transform", "align_rms"}
    reg = cn.icp(pred, gt, with_scale=True, init="normalize", library=path)
    assert reg.matrix.tolist() == m["transform"] and reg.rms == m["align_rms"]
    assert cn.surface_metrics(pred, gt, align=reg, **kw) == m
    by_matrix = cn.surface_metrics(pred, gt, align=reg.matrix, **kw)
    assert by_matrix["align_rms"] is None and {k: v for k, v in by_matrix.items() if k != "align_rms"} == {k: v for k, v in m.items() if k != "align_rms"}
    moved = (cn.apply_transform(pred[0], reg.matrix), pred[1])
    assert {k: v for k, v in m.items() if k not in ("transform", "align_rms")} == cn.surface_metrics(moved, gt, **kw)
    with pytest.raises(ValueError, match="align"):
        cn.surface_metrics(pred, gt, align="affine", **kw)
    # clouds: a rigid copy
    x = _t(_shape(1500, 2), dev)
    y = _t((_shape(1500, 2).astype(f64) @ _rot((1, 2, 3), 6.0).T + np.array([0.02, 0.01, -0.02])).astype(f32), dev)
    mm = cn.mesh_metrics(x, y, align="rigid", library=path)
    assert mm["fscore@0.01"] == 1.0 and cn.mesh_metrics(x, y, library=path)["fscore@0.01"] < 1.0 and mm["accuracy"] < 1e-6
    assert cn.chamfer_distance(x, y, align="rigid", library=path).item() == mm["chamfer_l2"] < 1e-12
    # PLY files
    cn.write_ply(str(tmp_path / "pred.ply"), V, T)
    cn.write_ply(str(tmp_path / "gt.ply"), G, T)
    fm = cn.compute_surface_metrics(str(tmp_path / "pred.ply"), str(tmp_path / "gt.ply"), device=dev, align="similarity", **kw)
    assert fm == m
    cdf = cn.compute_chamfer_distance(str(tmp_path / "pred.ply"), str(tmp_path / "gt.ply"), device=dev, align="similarity", library=path)
    assert cdf.item() < 1e-3 * cn.compute_chamfer_distance(str(tmp_path / "pred.ply"), str(tmp_path / "gt.ply"), device=dev, library=path).item()
