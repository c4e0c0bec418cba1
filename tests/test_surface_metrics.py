"""Mesh surface sampling (cnr_mesh_area_cdf, cnr_mesh_sample), exact point-to-mesh distance (cnr_point_mesh_distance) and the surface metrics on
top of them (meshops.sample_surface, metrics.point_mesh_distance / surface_metrics / compute_surface_metrics, meshio.read_ply_mesh).

Every case runs on the CPU-emulation library (device cpu) and, marked gpu, on the HIP library (cuda:0).  The yardsticks are written here and
use nothing from the library:

  SPEC   the comment block of include/colorneus_render.h restated in numpy float32 / integer arithmetic (every numpy operation on float32
         arrays is one IEEE rounding, the selects are np.where from the last region to the first, the candidates are folded with the same
         64-bit key): the library must match it BITWISE -- dist2, face and closest; weights, cdf, summary, faces, bary and points.  The sampler's
         Philox4x32-10 is written again here.
  Y64    a closest-point yardstick that is NOT Ericson's method: the distance to the plane where the projection falls inside the triangle,
         otherwise the minimum of the three segment distances, in float64 on the float32 inputs.  The tolerance on d = sqrt(d2) is 8 x the
         largest difference between Y64 and the same yardstick evaluated in float32 (Y32): the yardstick's own fp32 error, a factor 8 because
         the two algorithms round differently.

Launch constants the shapes below are built around (color-neus_amd/csrc/cnr_surface.hip): kSurfThreads = 256 threads x kSurfQ = 2 queries per
lane = 512 queries per workgroup; kSurfTile = 256 faces per LDS tile; the single-workgroup scan of cnr_mesh_area_cdf takes 8192 faces per trip
(kMeshScanChunk, cnr_meshcc.h)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import color_neus_amd as cn
from color_neus_amd import _lib
import _guard
import _native as N

BACKENDS = ["emu", pytest.param("hip", marks=pytest.mark.gpu)]
QUERIES_PER_WORKGROUP, FACES_PER_TILE, SCAN_CHUNK = 512, 256, 8192
f32 = np.float32


def _lib_and_dev(backend):
    if backend == "emu":
        assert os.path.isfile(N.EMU_LIB), "emulation library not built"
        return N.EMU_LIB, "cpu"
    assert torch.cuda.is_available(), "needs a GPU"
    return None, "cuda:0"


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _np(x):
    return x.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- SPEC: the distance ------------------------------------------------------------------------------------------------------------------------
def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _spec_records(V, T):
    """per face: valid, a, ab, ac (each [F, 3]) and abab, abac, acac, in float32"""
    V, T = np.asarray(V, f32), np.asarray(T, np.int64)
    valid = ((T >= 0) & (T < V.shape[0])).all(1)
    Ts = np.where(valid[:, None], T, 0)
    Vp = V if V.shape[0] else np.zeros((1, 3), f32)
    a, b, c = Vp[Ts[:, 0]], Vp[Ts[:, 1]], Vp[Ts[:, 2]]
    ab, ac = b - a, c - a
    return {"valid": valid, "a": a, "ab": ab, "ac": ac, "abab": _dot(*ab.T, *ab.T), "abac": _dot(*ab.T, *ac.T), "acac": _dot(*ac.T, *ac.T)}


def _spec_closest(q, r):
    """q [n, 3] against the records r (F faces): closest [n, F, 3] and d2 [n, F], float32, the header's order of operations"""
    zero, one = f32(0), f32(1)
    with np.errstate(all="ignore"):
        ax, ay, az = (r["a"][None, :, k] for k in range(3))
        abx, aby, abz = (r["ab"][None, :, k] for k in range(3))
        acx, acy, acz = (r["ac"][None, :, k] for k in range(3))
        qx, qy, qz = (q[:, None, k] for k in range(3))
        apx, apy, apz = qx - ax, qy - ay, qz - az
        d1, d2 = _dot(abx, aby, abz, apx, apy, apz), _dot(acx, acy, acz, apx, apy, apz)
        d3, d4, d5, d6 = d1 - r["abab"][None], d2 - r["abac"][None], d1 - r["abac"][None], d2 - r["acac"][None]
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        n1, n2, den = vb, vc, (va + vb) + vc
        for cond, m1, m2, mden in (((va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56),
                                   ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                   ((d6 >= 0) & (d5 <= d6), zero, one, one),
                                   ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                   ((d3 >= 0) & (d4 <= d3), one, zero, one),
                                   ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
            n1, n2, den = np.where(cond, m1, n1), np.where(cond, m2, n2), np.where(cond, mden, den)
        inv = one / den
        v, w = n1 * inv, n2 * inv
        cx, cy, cz = (ax + v * abx) + w * acx, (ay + v * aby) + w * acy, (az + v * abz) + w * acz
        dx, dy, dz = qx - cx, qy - cy, qz - cz
        dist2 = (dx * dx + dy * dy) + dz * dz
    assert dist2.dtype == f32
    return np.stack([cx, cy, cz], -1), dist2


def _spec_distance(Q, V, T):
    """(dist2 float32 [n], face int64 [n], closest float32 [n, 3], ties int [n]: the number of faces at the minimal d2 -- counted only when the
    faces fit one chunk, else None)"""
    Q = np.asarray(Q, f32)
    rec = _spec_records(V, T)
    n, F = Q.shape[0], rec["valid"].shape[0]
    nokey = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full(n, nokey, np.uint64)
    ties = np.zeros(n, np.int64) if F <= 16384 else None
    fchunk = min(F, 16384)
    qchunk = max(1, 2_000_000 // fchunk)
    for q0 in range(0, n, qchunk):
        q = Q[q0:q0 + qchunk]
        for f0 in range(0, F, fchunk):
            r = {k: x[f0:f0 + fchunk] for k, x in rec.items()}
            _, d2 = _spec_closest(q, r)
            ok = np.isfinite(d2) & r["valid"][None]
            key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.arange(f0, f0 + d2.shape[1], dtype=np.uint64)[None])
            key = np.where(ok, key, nokey)
            kmin = key.min(1)
            if ties is not None:
                ties[q0:q0 + qchunk] = (((key >> np.uint64(32)) == (kmin >> np.uint64(32))[:, None]) & ok).sum(1)
            keys[q0:q0 + qchunk] = np.minimum(keys[q0:q0 + qchunk], kmin)
    dist2 = (keys >> np.uint64(32)).astype(np.uint32).view(f32)
    face = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).astype(np.int64)
    closest = np.full((n, 3), np.nan, f32)
    got = face >= 0
    if got.any():
        one = {k: x[face[got]] for k, x in rec.items()}
        idx = np.nonzero(got)[0]                            # (one pair per query: the diagonal of a small product, chunked to stay small)
        for s in range(0, idx.size, 1024):
            sel = idx[s:s + 1024]
            c, _ = _spec_closest(Q[sel], {k: x[s:s + 1024] for k, x in one.items()})
            closest[sel] = c[np.arange(sel.size), np.arange(sel.size)]
    return dist2, face, closest, ties


def _run_distance(lib, dev, Q, V, T):
    d2, face, closest = cn.metrics.point_mesh_distance(_t(np.asarray(Q, f32), dev), _t(np.asarray(V, f32), dev), _t(np.asarray(T, np.int32), dev),
                                                       return_closest=True, library=lib)
    assert d2.dtype == torch.float32 and face.dtype == torch.int64 and closest.dtype == torch.float32
    assert d2.shape == (len(Q),) and face.shape == (len(Q),) and closest.shape == (len(Q), 3) and d2.device.type == torch.device(dev).type
    return _np(d2), _np(face), _np(closest)


def _assert_spec(got, spec):
    d2, face, closest = got
    assert _same_bits(d2, spec[0]), int((d2.view(np.int32) != spec[0].view(np.int32)).sum())
    assert np.array_equal(face, spec[1]), int((face != spec[1]).sum())
    assert _same_bits(closest, spec[2]), int((closest.view(np.int32) != spec[2].view(np.int32)).any(1).sum())


# ---- Y64 / Y32: the independent yardstick -----------------------------------------------------------------------------------------------------------
def _cross(u, v):
    return np.stack([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])


def _seg(p, a, b):
    ab = b - a
    t = np.clip(((p - a) * ab).sum(0) / np.maximum((ab * ab).sum(0), 1e-300), 0, 1)
    return ((p - (a + t * ab)) ** 2).sum(0)


def _yard(q, a, b, c, dt, pairwise=False):
    """squared distance of every query [n, 3] to every triangle (a, b, c: [F, 3]) in the dtype dt: [n, F], and whether the projection is inside;
    pairwise: query i against triangle i only, [n].  (Components first: the arrays are [3, n, F] or [3, n].)"""
    p, a, b, c = (x.astype(dt).T for x in (q, a, b, c))
    if not pairwise:
        p, a, b, c = p[:, :, None], a[:, None, :], b[:, None, :], c[:, None, :]
    n = _cross(b - a, c - a)
    nn = (n * n).sum(0)
    dist = ((p - a) * n).sum(0)
    pr = p - (dist / nn) * n

    def side(u, v):
        return (_cross(v - u, pr - u) * n).sum(0) >= 0

    inside = side(a, b) & side(b, c) & side(c, a)
    e = np.minimum(np.minimum(_seg(p, a, b), _seg(p, b, c)), _seg(p, c, a))
    return np.where(inside, dist * dist / nn, e), inside


def _region64(q, a, b, c):
    """float64 region of the closest point of triangle (a, b, c) [n, 3] for the queries q [n, 3], pairwise: 0 1 2 = vertex a b c, 3 4 5 = edge
    ab ac bc, 6 = interior (by the segment parameters of the yardstick, not by Ericson's tests)"""
    q, a, b, c = (x.astype(np.float64) for x in (q, a, b, c))
    _, inside = _yard(q, a, b, c, np.float64, pairwise=True)
    best, region = np.full(len(q), np.inf), np.full(len(q), 6)
    for code, u, v, cu, cv in ((3, a, b, 0, 1), (5, b, c, 1, 2), (4, a, c, 0, 2)):
        uv = v - u
        t = np.clip(((q - u) * uv).sum(-1) / (uv * uv).sum(-1), 0.0, 1.0)
        dd = ((q - (u + t[:, None] * uv)) ** 2).sum(-1)
        reg = np.where(t == 0.0, cu, np.where(t == 1.0, cv, code))
        region = np.where(dd < best, reg, region)
        best = np.minimum(best, dd)
    return np.where(inside, 6, region)


# ---- D1: random soup against Y64 -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _soup():
    rng = np.random.default_rng(0)
    F, n = 1500, 3000
    c = rng.uniform(-1, 1, (F, 3))
    a, b, cc = (c + rng.uniform(-.15, .15, (F, 3)) for _ in range(3))
    q = rng.uniform(-1, 1, (n, 3))
    a, b, cc, q = (x.astype(f32) for x in (a, b, cc, q))
    V = np.concatenate([a, b, cc])
    T = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], -1).astype(np.int32)
    y64 = np.concatenate([_yard(q[s:s + 100], a, b, cc, np.float64)[0] for s in range(0, n, 100)])       # (by chunks that stay in the cache)
    y32 = np.concatenate([_yard(q[s:s + 100], a, b, cc, f32)[0] for s in range(0, n, 100)])
    d64, d32 = np.sqrt(y64.min(1)), np.sqrt(y32.min(1).astype(np.float64))
    tol = 8.0 * np.abs(d64 - d32).max()
    j64 = y64.argmin(1)
    shares = np.bincount(_region64(q, a[j64], b[j64], cc[j64]), minlength=7) / n
    return q, (a, b, cc), V, T, y64, d64, tol, _spec_distance(q, V, T), shares


@pytest.mark.parametrize("backend", BACKENDS)
def test_random_soup_against_the_float64_yardstick(backend):
    """D1.  3000 queries x 1500 triangles.  |d - d64| <= tol, the returned face is within tol of the nearest one, closest lies on that face at
    distance d, tol = 8 x max |Y32 - Y64| (printed); each of the seven regions wins at least 3 % of the queries.  And SPEC, bitwise."""
    lib, dev = _lib_and_dev(backend)
    q, (a, b, c), V, T, y64, d64, tol, spec, shares = _soup()
    d2, face, closest = _run_distance(lib, dev, q, V, T)
    d = np.sqrt(d2.astype(np.float64))
    print("regions (a b c ab ac bc interior):", np.round(shares, 3))
    assert shares.min() >= 0.03, shares
    rows = np.arange(len(q))
    on_face = np.sqrt(_yard(closest, a[face], b[face], c[face], np.float64, pairwise=True)[0])
    at_d = np.sqrt(((q.astype(np.float64) - closest.astype(np.float64)) ** 2).sum(1))
    print(f"tol {tol:.3e} (Y32 against Y64: {tol / 8:.3e}); max |d - d64| {np.abs(d - d64).max():.3e}; returned-face excess "
          f"{(np.sqrt(y64[rows, face]) - d64).max():.3e}; closest off its face {on_face.max():.3e}; | |q - closest| - d | {np.abs(at_d - d).max():.3e}")
    assert (face >= 0).all() and (face < 1500).all()
    assert (np.abs(d - d64) <= tol).all()
    assert (np.sqrt(y64[rows, face]) <= d64 + tol).all()
    assert (on_face <= tol).all() and (np.abs(at_d - d) <= tol).all()
    _assert_spec((d2, face, closest), spec[:3])


# ---- D2: an exact case ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dyadic_case():
    """axis-aligned right isosceles triangles, legs L in {1/2, 1, 2}, corners on multiples of 1/4; queries on multiples of 1/8: every product is a
    short dyadic number and every quotient has the denominator |ab|^2 = L^2, |bc|^2 = 2 L^2 or |n|^2 = L^4, a power of two"""
    rng = np.random.default_rng(1)
    F, n = 300, 1500
    a = rng.integers(-12, 13, (F, 3)) / 4.0
    L = 2.0 ** rng.integers(-1, 2, F)
    ax1 = rng.integers(0, 3, F)
    ax2 = (ax1 + rng.integers(1, 3, F)) % 3
    b, c = a.copy(), a.copy()
    b[np.arange(F), ax1] += L * rng.choice([-1.0, 1.0], F)
    c[np.arange(F), ax2] += L * rng.choice([-1.0, 1.0], F)
    q = rng.integers(-32, 33, (n, 3)) / 8.0
    a, b, c, q = (x.astype(f32) for x in (a, b, c, q))
    V = np.concatenate([a, b, c])
    T = np.stack([np.arange(F), np.arange(F) + F, np.arange(F) + 2 * F], -1).astype(np.int32)
    return q, (a, b, c), V, T


@pytest.mark.parametrize("backend", BACKENDS)
def test_dyadic_inputs_are_exact(backend):
    """D2.  dist2 equals the float64 yardstick bit for bit (as float64 numbers), and the face is its first minimum."""
    lib, dev = _lib_and_dev(backend)
    q, (a, b, c), V, T = _dyadic_case()
    y64, _ = _yard(q, a, b, c, np.float64)
    d2, face, closest = _run_distance(lib, dev, q, V, T)
    assert np.array_equal(d2.astype(np.float64), y64.min(1)), int((d2.astype(np.float64) != y64.min(1)).sum())
    assert np.array_equal(face, y64.argmin(1))
    assert np.array_equal(((q.astype(np.float64) - closest.astype(np.float64)) ** 2).sum(1), y64.min(1))


# ---- D3: ties ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tie_case():
    rng = np.random.default_rng(2)
    q0, (a, b, c), V0, T0 = _dyadic_case()
    T = [T0[:120]]
    V = [V0]
    nv = V0.shape[0]
    hubs = rng.integers(-16, 17, (40, 3)) / 8.0               # fans: 40 hubs, 5 triangles each around the hub, the hub in every corner role
    queries = [q0[:200]]
    for h in hubs:
        rim = h + np.concatenate([rng.integers(1, 5, (10, 1)), rng.integers(-4, 5, (10, 2))], 1) / 4.0      # all on the hub's +x side
        V.append(np.concatenate([h[None], rim]).astype(f32))
        for k in range(5):
            tri = np.roll([nv, nv + 1 + 2 * k, nv + 2 + 2 * k], k % 3)
            T.append(np.asarray(tri, np.int32)[None])
        nv += 11
        queries.append((h - np.arange(12)[:, None] * np.array([[1.0, 0, 0]]) / 64.0).astype(f32))      # on its -x side: nearest the hub
    T = np.concatenate(T)
    T = np.concatenate([T, T[rng.permutation(T.shape[0])]])                        # every face again, shuffled, at higher indices
    V, Q = np.concatenate(V), np.concatenate(queries)
    return Q, V, T, _spec_distance(Q, V, T)


@pytest.mark.parametrize("backend", BACKENDS)
def test_ties_go_to_the_lowest_face_index(backend):
    """D3.  Every triangle duplicated at a higher index, and fans around a shared vertex with queries nearest that vertex (two faces at the
    minimum from the duplicates alone, more where the hub is the closest point of several fan triangles): the lowest index is returned."""
    lib, dev = _lib_and_dev(backend)
    Q, V, T, spec = _tie_case()
    tied = int((spec[3] > 1).sum())
    print(f"{tied} of {len(Q)} queries have more than one face at the minimal d2")
    assert 2 * tied >= len(Q), (tied, len(Q))
    fans = int((spec[3] >= 10).sum())           # a hub that is the closest point of its five triangles and of their duplicates
    print(f"{fans} of them tie over the five distinct triangles of a fan")
    assert 4 * fans >= len(Q), fans
    _assert_spec(_run_distance(lib, dev, Q, V, T), spec[:3])


# ---- D4: shapes ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shape_case(n, F):
    rng = np.random.default_rng(1000 * n + F)
    if F > 1000:        # a strip along a random walk: small faces spread over the unit box, every vertex shared by three of them
        V = np.cumsum(rng.uniform(-0.005, 0.005, (F + 2, 3)), 0).astype(f32)
        T = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], -1).astype(np.int32)
    else:
        nv = max(3, min(3 * F, 3000))
        V = rng.uniform(-1, 1, (nv, 3)).astype(f32)
        T = rng.integers(0, nv, (F, 3)).astype(np.int32)
    Q = rng.uniform(-1, 1, (n, 3)).astype(f32)
    return Q, V, T, _spec_distance(Q, V, T)


# 37 x 200 003: the face range is split over many workgroups; 5000 x 1; query counts at one workgroup's load (512) and that +- 1; face counts
# at one LDS tile (256) and that +- 1
SHAPES = [(37, 200003), (5000, 1), (QUERIES_PER_WORKGROUP - 1, 300), (QUERIES_PER_WORKGROUP, 300), (QUERIES_PER_WORKGROUP + 1, 300),
          (100, FACES_PER_TILE - 1), (100, FACES_PER_TILE), (100, FACES_PER_TILE + 1)]


@pytest.mark.parametrize("n,F", SHAPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_launch_shapes(backend, n, F):
    """D4.  SPEC, bitwise."""
    lib, dev = _lib_and_dev(backend)
    Q, V, T, spec = _shape_case(n, F)
    _assert_spec(_run_distance(lib, dev, Q, V, T), spec[:3])


# ---- D5: edges -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_distance_edges(backend):
    lib, dev = _lib_and_dev(backend)
    pmd = cn.metrics.point_mesh_distance
    q, _, V, T = _soup()[:4]
    q, V, T = _t(q[:300], dev), _t(V, dev), _t(T[:400], dev)
    # n = 0 / F = 0
    d2, face, closest = pmd(q[:0], V, T, return_closest=True, library=lib)
    assert d2.shape == (0,) and face.shape == (0,) and closest.shape == (0, 3)
    assert d2.dtype == torch.float32 and face.dtype == torch.int64 and closest.dtype == torch.float32
    assert len(pmd(q[:0], V, T, library=lib)) == 2
    with pytest.raises(ValueError):
        pmd(q, V, T[:0], library=lib)
    base = pmd(q, V, T, return_closest=True, library=lib)
    same = lambda got: all(_same_bits(_np(x), _np(y)) for x, y in zip(got, base))
    assert (base[1] >= 0).all()
    # an all-NaN triangle and a triangle with an index outside [0, V) change nothing
    nan = float("nan")
    V_nan = torch.cat([V, torch.full((3, 3), nan, device=dev)])
    T_nan = torch.cat([T, torch.tensor([[V.shape[0], V.shape[0] + 1, V.shape[0] + 2]], dtype=torch.int32, device=dev)])
    assert same(pmd(q, V_nan, T_nan, return_closest=True, library=lib))
    for bad in ([0, 1, V.shape[0]], [-1, 1, 2], [0, 2 ** 31 - 1, 2]):
        T_bad = torch.cat([T, torch.tensor([bad], dtype=torch.int32, device=dev)])
        assert same(pmd(q, V, T_bad, return_closest=True, library=lib))
    T_front = torch.cat([torch.tensor([[0, 1, V.shape[0]]], dtype=torch.int32, device=dev), T])
    d2, face, closest = pmd(q, V, T_front, return_closest=True, library=lib)
    assert _same_bits(_np(d2), _np(base[0])) and torch.equal(face, base[1] + 1) and _same_bits(_np(closest), _np(base[2]))
    # only invalid faces: no candidate
    d2, face, closest = pmd(q[:5], V, torch.tensor([[0, 1, -1]], dtype=torch.int32, device=dev), return_closest=True, library=lib)
    assert torch.isnan(d2).all() and (face == -1).all() and torch.isnan(closest).all()
    # a triangle collapsed to one point behaves as that point (the header: "vertex a" for every query)
    p = torch.tensor([[0.25, -0.5, 0.125]], device=dev)
    d2, face, closest = pmd(q, p, torch.zeros(1, 3, dtype=torch.int32, device=dev), return_closest=True, library=lib)
    d2_nn, _ = cn.metrics.nearest_neighbors(q, p, library=lib)
    assert _same_bits(_np(d2), _np(d2_nn)) and (face == 0).all() and torch.equal(closest, p.expand(300, 3))
    # a NaN query: {NaN, -1}, NaN in closest; the other queries keep their bits
    q_nan = q.clone()
    q_nan[7, 1] = nan
    d2, face, closest = pmd(q_nan, V, T, return_closest=True, library=lib)
    assert face[7].item() == -1 and torch.isnan(d2[7]).item() and torch.isnan(closest[7]).all()
    keep = torch.arange(300, device=dev) != 7
    assert _same_bits(_np(d2[keep]), _np(base[0][keep])) and torch.equal(face[keep], base[1][keep]) and _same_bits(_np(closest[keep]), _np(base[2][keep]))
    # float64, non-contiguous and requires_grad inputs: the bits of their contiguous float32 copies, no graph
    q_nc = torch.zeros(300, 6, device=dev)[:, ::2]
    q_nc.copy_(q)
    V_t = V.t().contiguous().t()
    T_nc = torch.zeros(400, 6, dtype=torch.int64, device=dev)[:, ::2]
    T_nc.copy_(T)
    assert not q_nc.is_contiguous() and not V_t.is_contiguous() and not T_nc.is_contiguous()
    for qq, vv, tt in ((q.double(), V.double(), T.long()), (q_nc, V_t, T_nc), (q.clone().requires_grad_(True), V.clone().requires_grad_(True), T)):
        got = pmd(qq, vv, tt, return_closest=True, library=lib)
        assert same(got)
        assert all(x.grad_fn is None and not x.requires_grad for x in got)


def test_cpu_points_need_an_emulation_library():
    """No CPU fallback: CPU tensors with the HIP library (the default) are an error, not a torch computation."""
    if not os.path.isfile(cn.library_path()):
        pytest.skip("HIP library not built")
    q, _, V, T = _soup()[:4]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.metrics.point_mesh_distance(torch.from_numpy(q), torch.from_numpy(V), torch.from_numpy(T))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cn.meshops.sample_surface(torch.from_numpy(V), torch.from_numpy(T), 10)


# ---- D6: HIP against the emulation ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_distance_matches_the_emulation_bitwise_at_2_14():
    """2^14 queries x (2^14 + 3) triangles of seeded normal inputs: dist2, face and closest bitwise; again on a side stream."""
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator().manual_seed(14)
    F = (1 << 14) + 3
    q = torch.randn(1 << 14, 3, generator=g)
    centre = torch.randn(F, 1, 3, generator=g)
    V = (centre + 0.3 * torch.randn(F, 3, 3, generator=g)).reshape(-1, 3).contiguous()
    T = torch.arange(3 * F, dtype=torch.int32).reshape(F, 3)
    emu = cn.metrics.point_mesh_distance(q, V, T, return_closest=True, library=N.EMU_LIB)
    qd, Vd, Td = q.cuda(), V.cuda(), T.cuda()
    hip = cn.metrics.point_mesh_distance(qd, Vd, Td, return_closest=True)
    for name, x, y in zip(("dist2", "face", "closest"), hip, emu):
        assert _same_bits(_np(x), _np(y)), (name, int((x.cpu() != y).sum()))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = cn.metrics.point_mesh_distance(qd, Vd, Td, return_closest=True)
    side.synchronize()
    for x, y in zip(again, emu):
        assert _same_bits(_np(x), _np(y))


# ---- D7 / S5: guarded outputs ----------------------------------------------------------------------------------------------------------------------
def _abi_distance(lib, dev, Q, V, T, guard=None, want_closest=True):
    Q, V, T = _t(np.asarray(Q, f32), dev), _t(np.asarray(V, f32), dev), _t(np.asarray(T, np.int32), dev)
    n = Q.shape[0]
    if guard is None:
        empty, addr, inp = (lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)), _lib.ptr, (lambda t: t)
    else:
        empty, addr, inp = (lambda shape, dt: guard.empty(shape, dt, dev)), guard.addr, guard.copy
    Q, V, T = inp(Q), inp(V), inp(T)
    o = {"dist2": empty(n, torch.float32), "face": empty(n, torch.int32), "closest": empty((n, 3), torch.float32), "keys": empty(n, torch.int64)}
    lib.call("cnr_point_mesh_distance", addr(Q), n, addr(V), V.shape[0], addr(T), T.shape[0], addr(o["dist2"]), addr(o["face"]),
             addr(o["closest"]) if want_closest else C.c_void_p(0), addr(o["keys"]), _lib.stream_of(torch.device(dev)))
    if guard is not None:
        guard.check()
    return {k: _np(x).copy() for k, x in o.items()}


@pytest.mark.parametrize("fill", [0xFF, 0x00])
@pytest.mark.parametrize("backend", BACKENDS)
def test_guarded_distance_buffers(backend, fill):
    """D7.  dist2, face, closest and keys as exact-size poisoned payloads between guard bytes, the inputs between NaN guards: the bits of a plain
    run, no guard byte touched.  513 queries x 257 faces: one query past a workgroup's load, one face past a tile."""
    path, dev = _lib_and_dev(backend)
    lib = _lib.resolve_library(path)
    Q, V, T, spec = _shape_case(QUERIES_PER_WORKGROUP + 1, 300)
    T = T[:FACES_PER_TILE + 1]
    plain = _abi_distance(lib, dev, Q, V, T)
    guard = _guard.Guard(fill)
    got = _abi_distance(lib, dev, Q, V, T, guard)
    assert len(guard.regions) == 7
    for k in ("dist2", "face", "closest"):
        assert _same_bits(got[k], plain[k]), k
    guard = _guard.Guard(fill)
    got = _abi_distance(lib, dev, Q, V, T, guard, want_closest=False)           # closest = NULL: nothing written there
    assert _same_bits(got["dist2"], plain["dist2"]) and _same_bits(got["face"], plain["face"])
    assert (got["closest"].view(np.uint8) == fill).all()


# ---- SPEC: the sampler ---------------------------------------------------------------------------------------------------------------------------
M32 = np.uint64(0xFFFFFFFF)


def _philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint64 arrays that hold 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def test_the_philox_restatement_matches_the_published_vectors():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors): counter and key all zero, all ones, and the digits of pi"""
    for ctr, key, out in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                          ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        got = _philox(*[np.array([c]) for c in ctr], *key)
        assert tuple(int(x[0]) for x in got) == out


def _spec_cdf(V, T):
    """(weights uint64 [F], cdf uint64 [F], summary int64 [4])"""
    V, T = np.asarray(V, f32), np.asarray(T, np.int64)
    valid = ((T >= 0) & (T < V.shape[0])).all(1)
    Ts = np.where(valid[:, None], T, 0)
    Vp = V if V.shape[0] else np.zeros((1, 3), f32)
    a, b, c = Vp[Ts[:, 0]], Vp[Ts[:, 1]], Vp[Ts[:, 2]]
    with np.errstate(all="ignore"):
        e1, e2 = b - a, c - a
        nx = (e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1])
        ny = (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2])
        nz = (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])
        A = np.sqrt((nx * nx + ny * ny) + nz * nz)
        assert A.dtype == f32
        valid = valid & np.isfinite(A)
        amax = A[valid].max() if valid.any() else f32(0)
        w = np.zeros(len(T), np.uint64)
        if amax > 0:
            w[valid] = ((A[valid] / amax) * f32(4294967296.0)).astype(np.uint64)
    cdf = np.cumsum(w, dtype=np.uint64)
    summary = np.array([int(cdf[-1]), int((w == 0).sum()), int((~valid).sum()), int(np.asarray(amax, f32).view(np.uint32))], np.int64)
    return w, cdf, summary


def _spec_sample(V, T, cdf, n, seed):
    """(faces int64 [n], uv float32 [n, 2], points float32 [n, 3]) for a total > 0"""
    V, T = np.asarray(V, f32), np.asarray(T, np.int64)
    i = np.arange(n, dtype=np.uint64)
    s = seed & (2 ** 64 - 1)
    w0, w1, w2, w3 = _philox(i & M32, i >> np.uint64(32), np.zeros(n, np.uint64), np.zeros(n, np.uint64), s & 0xFFFFFFFF, s >> 32)
    total = int(cdf[-1])
    r = np.array([((int(x) << 32 | int(y)) * total) >> 64 for x, y in zip(w0, w1)], np.uint64)
    faces = np.searchsorted(cdf, r, side="right").astype(np.int64)          # the first f with cdf[f] > r
    iu, iv = (w2 >> np.uint64(8)).astype(np.int64), (w3 >> np.uint64(8)).astype(np.int64)
    fold = iu + iv > 2 ** 24
    iu, iv = np.where(fold, 2 ** 24 - iu, iu), np.where(fold, 2 ** 24 - iv, iv)
    u, v = iu.astype(f32) * f32(2.0 ** -24), iv.astype(f32) * f32(2.0 ** -24)
    a, b, c = V[T[faces, 0]], V[T[faces, 1]], V[T[faces, 2]]
    points = (a + u[:, None] * (b - a)) + v[:, None] * (c - a)
    assert points.dtype == f32
    return faces, np.stack([u, v], -1), points


def _abi_sample(lib, dev, V, T, n, seed, guard=None):
    V, T = _t(np.asarray(V, f32), dev), _t(np.asarray(T, np.int32), dev)
    F = T.shape[0]
    if guard is None:
        empty, addr, inp = (lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)), _lib.ptr, (lambda t: t)
    else:
        empty, addr, inp = (lambda shape, dt: guard.empty(shape, dt, dev)), guard.addr, guard.copy
    V, T = inp(V), inp(T)
    o = {"cdf": empty(F, torch.int64), "summary": empty(4, torch.int64), "points": empty((n, 3), torch.float32), "faces": empty(n, torch.int32),
         "bary": empty((n, 2), torch.float32)}
    stream = _lib.stream_of(torch.device(dev))
    lib.call("cnr_mesh_area_cdf", addr(V), V.shape[0], addr(T), F, addr(o["cdf"]), addr(o["summary"]), stream)
    lib.call("cnr_mesh_sample", addr(V), V.shape[0], addr(T), F, addr(o["cdf"]), n, seed, addr(o["points"]), addr(o["faces"]), addr(o["bary"]), stream)
    if guard is not None:
        guard.check()
    return {k: _np(x).copy() for k, x in o.items()}


@functools.lru_cache(maxsize=None)
def _wide_mesh():
    """9000 triangles (the scan crosses a chunk boundary) whose sizes span three decades, so their areas six; a few faces of weight 0"""
    rng = np.random.default_rng(3)
    F = 9000
    centre = rng.uniform(-1, 1, (F, 1, 3))
    size = 10.0 ** rng.uniform(-3, 0, (F, 1, 1))
    V = (centre + size * rng.uniform(-0.5, 0.5, (F, 3, 3))).reshape(-1, 3).astype(f32)
    T = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    T[17] = (5, 5, 6)                       # zero area
    T[8191] = (0, 1, 3 * F)                 # invalid
    T[8192] = (-1, 1, 2)
    return V, T


@pytest.mark.parametrize("backend", BACKENDS)
def test_sampler_restates_the_header_bitwise(backend):
    """S1.  weights (through cdf), cdf, summary, faces, bary and points against SPEC, all bitwise; two seeds, one with all 64 bits in use."""
    path, dev = _lib_and_dev(backend)
    lib = _lib.resolve_library(path)
    V, T = _wide_mesh()
    w, cdf, summary = _spec_cdf(V, T)
    areas = w[w > 0].astype(np.float64)
    assert areas.max() / areas.min() > 1e6 and summary[1] == 3 and summary[2] == 2
    for seed in (0, -0x123456789ABCDEF):
        got = _abi_sample(lib, dev, V, T, 4099, seed)
        assert np.array_equal(got["cdf"].view(np.uint64), cdf) and np.array_equal(got["summary"], summary)
        faces, uv, points = _spec_sample(V, T, cdf, 4099, seed)
        assert np.array_equal(got["faces"], faces)
        assert _same_bits(got["bary"], uv) and _same_bits(got["points"], points)
    # and through the Python layer: int64 faces, barycentric triples, colours interpolated with them
    col = np.random.default_rng(4).uniform(0, 1, V.shape).astype(f32)
    pts, fc, bary, c = cn.meshops.sample_surface(_t(V, dev), _t(T, dev), 4099, seed=-0x123456789ABCDEF, colors=_t(col, dev), library=path)
    assert fc.dtype == torch.int64 and np.array_equal(_np(fc), faces) and _same_bits(_np(pts), points)
    assert _same_bits(_np(bary[:, 1:]), uv) and _same_bits(_np(bary[:, 0]), (f32(1) - uv[:, 0]) - uv[:, 1])
    ref = (col[T[faces]].astype(np.float64) * _np(bary).astype(np.float64)[:, :, None]).sum(1)
    assert np.abs(_np(c) - ref).max() <= 4 * 2.0 ** -24          # three products and two additions of numbers in [0, 1]
    assert len(cn.meshops.sample_surface(_t(V, dev), _t(T, dev), 5, library=path)) == 3
    assert cn.sample_surface is cn.meshops.sample_surface


@pytest.mark.parametrize("backend", BACKENDS)
def test_sample_distribution(backend):
    """S2.  A fixed seed makes the test deterministic; the bounds are 5 sigma of the binomial.  (The integer weights put p within 2^-31 of its
    value: 1e-4 of a sample.)"""
    lib, dev = _lib_and_dev(backend)
    n = 200000
    bound = lambda p: 5.0 * np.sqrt(n * p * (1 - p))
    # two triangles of area 1 : 3
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 0, 0], [8, 0, 0], [5, 1, 0]], f32)
    T = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    pts, faces, bary = cn.meshops.sample_surface(_t(V, dev), _t(T, dev), n, seed=11, library=lib)
    first = int((faces == 0).sum())
    print(f"face 0 drew {first} of {n}: expected {n / 4:.0f} +- {bound(0.25):.0f}")
    assert abs(first - n / 4) <= bound(0.25)
    assert bool(((bary >= 0) & (bary <= 1)).all())
    assert bool(((pts[:, 0] < 2) == (faces == 0)).all())
    # one triangle: its four midpoint sub-triangles hold a quarter each
    pts, faces, bary = cn.meshops.sample_surface(_t(V[:3], dev), _t(T[:1], dev), n, seed=12, library=lib)
    b = _np(bary)
    assert (faces == 0).all() and (b >= 0).all() and (b <= 1).all() and np.array_equal((b[:, 0] + b[:, 1]) + b[:, 2], np.ones(n, f32))
    corner = [int((b[:, k] > 0.5).sum()) for k in range(3)]
    counts = corner + [n - sum(corner)]
    print(f"sub-triangles drew {counts}: expected {n / 4:.0f} +- {bound(0.25):.0f}")
    assert all(abs(k - n / 4) <= bound(0.25) for k in counts), counts
    assert np.abs(_np(pts) - (b[:, 1:2] * V[1] + b[:, 2:3] * V[2])).max() <= 2.0 ** -23


@pytest.mark.parametrize("backend", BACKENDS)
def test_weights_and_summary(backend):
    """S3.  Faces of weight 0 (zero area, below 2^-32 of the largest) and invalid faces (an index out of range, a NaN corner) are never drawn
    and summary counts them; a mesh of only such faces raises ValueError."""
    path, dev = _lib_and_dev(backend)
    lib = _lib.resolve_library(path)
    nan = float("nan")
    V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1e-6, 0, 1], [0, 1e-6, 1], [nan, 0, 0], [2, 2, 2], [3, 2, 2], [2, 3, 2]], f32)
    T = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 6], [0, 1, 10], [1, 1, 2], [7, 8, 9], [0, -1, 2]], np.int32)
    #             area 1     1e-12      NaN        index      zero      area 1     index
    got = _abi_sample(lib, dev, V, T, 20000, 5)
    w, cdf, summary = _spec_cdf(V, T)
    assert w.tolist() == [2 ** 32, 0, 0, 0, 0, 2 ** 32, 0] and summary.tolist() == [2 ** 33, 5, 3, int(np.float32(1).view(np.uint32))]
    assert np.array_equal(got["summary"], summary) and np.array_equal(got["cdf"].view(np.uint64), cdf)
    assert set(np.unique(got["faces"]).tolist()) == {0, 5}
    with pytest.raises(ValueError, match="no face can be drawn"):
        cn.meshops.sample_surface(_t(V, dev), _t(T[2:5], dev), 10, library=path)
    with pytest.raises(ValueError, match="no faces"):
        cn.meshops.sample_surface(_t(V, dev), _t(T[:0], dev), 10, library=path)
    # total == 0 at the ABI: face -1, NaN points and bary
    got = _abi_sample(lib, dev, V, T[2:5], 7, 0)
    assert got["summary"].tolist() == [0, 3, 2, 0] and (got["faces"] == -1).all() and np.isnan(got["points"]).all() and np.isnan(got["bary"]).all()
    # n = 0: empty tensors of the right dtypes
    pts, faces, bary = cn.meshops.sample_surface(_t(V, dev), _t(T, dev), 0, library=path)
    assert pts.shape == (0, 3) and faces.shape == (0,) and bary.shape == (0, 3) and faces.dtype == torch.int64 and pts.dtype == torch.float32


@pytest.mark.parametrize("backend", BACKENDS)
def test_seeds_and_prefixes(backend):
    """S4."""
    lib, dev = _lib_and_dev(backend)
    V, T = _wide_mesh()
    V, T = _t(V, dev), _t(T, dev)
    a = cn.meshops.sample_surface(V, T, 3000, seed=7, library=lib)
    b = cn.meshops.sample_surface(V, T, 3000, seed=7, library=lib)
    c = cn.meshops.sample_surface(V, T, 3000, seed=8, library=lib)
    short = cn.meshops.sample_surface(V, T, 1237, seed=7, library=lib)
    for x, y, z, s in zip(a, b, c, short):
        assert _same_bits(_np(x), _np(y)) and not _same_bits(_np(x), _np(z)) and _same_bits(_np(x[:1237]), _np(s))
    assert int((a[1] != c[1]).sum()) > 2900
    assert all(x.grad_fn is None and not x.requires_grad for x in cn.meshops.sample_surface(V.clone().requires_grad_(True), T, 10, library=lib))


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_hip_sampler_matches_the_emulation_bitwise(fill):
    """S5.  F = 100 003 (the scan crosses its chunk boundaries), n = 10 007 (no multiple of the block): bitwise; the outputs under guards."""
    assert torch.cuda.is_available(), "needs a GPU"
    rng = np.random.default_rng(5)
    F, n = 100003, 10007
    V = rng.normal(size=(40000, 3)).astype(f32)
    T = rng.integers(0, 40000, (F, 3)).astype(np.int32)
    T[rng.integers(0, F, 50)] = -1
    emu = _abi_sample(cn.load_library(N.EMU_LIB), "cpu", V, T, n, 99)
    guard = _guard.Guard(fill)
    hip = _abi_sample(cn.load_library(), "cuda:0", V, T, n, 99, guard)
    assert len(guard.regions) == 7
    for k in emu:
        assert _same_bits(hip[k], emu[k]), k


# ---- metrics -------------------------------------------------------------------------------------------------------------------------------------
def _square(z, dev, flip=False):
    V = torch.tensor([[0, 0, z], [1, 0, z], [1, 1, z], [0, 1, z]], dtype=torch.float32, device=dev)
    T = torch.tensor([[0, 1, 3], [1, 2, 3]] if flip else [[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)
    return V, T


@pytest.mark.parametrize("backend", BACKENDS)
def test_parallel_squares(backend):
    """M1.  Two unit squares at distance h.  A sample of one lies exactly in its plane (z is a + u*0 + v*0), the closest point exactly in the other
    plane, so dz = h exactly and dx, dy are rounding residues below 4 ulp of 1: (dx*dx + dy*dy) < 1.2e-13 = 1.2e-11 h^2.  d2 = (..) + dz*dz has
    two roundings (the product, the sum): a relative error below 2 * 2^-24 + 1.2e-11, half of it on d = sqrt(d2) in float64.  Bounds: 1.01 * 2^-24
    relative on accuracy, completeness and chamfer_l1, 2.02 * 2^-24 on chamfer_l2 = 2 h^2."""
    lib, dev = _lib_and_dev(backend)
    h = float(np.float32(0.1))
    m = cn.metrics.surface_metrics(_square(0.0, dev), _square(np.float32(0.1), dev, flip=True), n_samples=20000, seed=1, thresholds=(0.05, 0.2),
                                   library=lib)
    assert all(type(v) is float for v in m.values())
    assert set(m) == {"accuracy", "completeness", "chamfer_l1", "chamfer_l2"} | {f"{k}@{t}" for k in ("precision", "recall", "fscore") for t in ("0.05", "0.2")}
    eps = 2.0 ** -24
    for k in ("accuracy", "completeness", "chamfer_l1"):
        print(k, m[k], abs(m[k] - h) / h / eps, "x 2^-24")
        assert abs(m[k] - h) <= 1.01 * eps * h, (k, m[k])
    assert abs(m["chamfer_l2"] - 2 * h * h) <= 2.02 * eps * 2 * h * h, m["chamfer_l2"]
    assert m["precision@0.05"] == 0.0 and m["recall@0.05"] == 0.0 and m["fscore@0.05"] == 0.0
    assert m["precision@0.2"] == 1.0 and m["recall@0.2"] == 1.0 and m["fscore@0.2"] == 1.0
    assert cn.surface_metrics is cn.metrics.surface_metrics and cn.point_mesh_distance is cn.metrics.point_mesh_distance


def _two_tessellations(dev):
    """the unit square as 2 triangles, and with the half x >= 1/2 as 2 * 64^2 triangles (the half x <= 1/2 as 2)"""
    coarse = _square(0.0, dev)
    k = 64
    gx, gy = np.meshgrid(0.5 + 0.5 * np.arange(k + 1) / k, np.arange(k + 1) / k, indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel(), np.zeros((k + 1) ** 2)], -1)
    idx = lambda i, j: 4 + i * (k + 1) + j
    tris = [[0, 1, 2], [0, 2, 3]]
    for i in range(k):
        for j in range(k):
            tris += [[idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)], [idx(i, j), idx(i + 1, j + 1), idx(i, j + 1)]]
    V = np.concatenate([np.array([[0, 0, 0], [0.5, 0, 0], [0.5, 1, 0], [0, 1, 0]]), grid]).astype(f32)
    return coarse, (_t(V, dev), _t(np.asarray(tris, np.int32), dev))


@pytest.mark.parametrize("backend", BACKENDS)
def test_surface_metrics_do_not_move_with_the_tessellation(backend):
    """M2.  The reason for the feature: the same surface tessellated two ways has a vertex-cloud completeness above 0.1 and surface figures that
    are rounding residues (both meshes lie in the plane z = 0)."""
    lib, dev = _lib_and_dev(backend)
    coarse, fine = _two_tessellations(dev)
    assert fine[1].shape[0] == 2 + 2 * 64 * 64
    cloud = cn.metrics.mesh_metrics(coarse[0], fine[0], library=lib)
    surf = cn.metrics.surface_metrics(coarse, fine, n_samples=20000, seed=2, exact=True, library=lib)
    print("vertex clouds:", cloud["accuracy"], cloud["completeness"], " surfaces:", surf["accuracy"], surf["completeness"])
    assert cloud["completeness"] > 0.1
    assert 0.0 <= surf["accuracy"] < 1e-6 and 0.0 <= surf["completeness"] < 1e-6
    assert surf["fscore@0.01"] == 1.0


@pytest.mark.parametrize("backend", BACKENDS)
def test_surface_metric_variants(backend):
    """M3.  gt as a bare cloud; exact=False is mesh_metrics of the two sample sets; max_dist clamps."""
    lib, dev = _lib_and_dev(backend)
    n = 4000
    pred, gt = _square(0.0, dev), _square(np.float32(0.1), dev, flip=True)
    ps = cn.meshops.sample_surface(*pred, n, seed=5, library=lib)[0]
    gs = cn.meshops.sample_surface(*gt, n, seed=6, library=lib)[0]
    assert cn.metrics.surface_metrics(pred, gt, n_samples=n, seed=5, exact=False, library=lib) == cn.metrics.mesh_metrics(ps, gs, library=lib)
    # a cloud: accuracy is samples -> cloud, completeness cloud -> pred surface
    cloud = gs[:777]
    m = cn.metrics.surface_metrics(pred, cloud, n_samples=n, seed=5, library=lib)
    acc = cn.metrics.nearest_neighbors(ps, cloud, library=lib)[0].double().sqrt().mean().item()
    comp = cn.metrics.point_mesh_distance(cloud, *pred, library=lib)[0].double().sqrt().mean().item()
    assert m["accuracy"] == acc and m["completeness"] == comp and acc > comp > 0.0999
    m = cn.metrics.surface_metrics(pred, cloud, n_samples=n, seed=5, exact=False, library=lib)
    assert m == cn.metrics.mesh_metrics(ps, cloud, library=lib)
    # max_dist
    m = cn.metrics.surface_metrics(pred, gt, n_samples=n, seed=5, max_dist=0.05, thresholds=(0.06,), library=lib)
    for k, want in (("accuracy", 0.05), ("completeness", 0.05), ("chamfer_l1", 0.05), ("chamfer_l2", 2 * 0.05 * 0.05)):
        assert m[k] == pytest.approx(want, rel=1e-12), (k, m[k])       # (every distance is the clamp itself: only the float64 sums round)
    assert m["precision@0.06"] == 1.0
    for bad in (dict(n_samples=0), dict(max_dist=0.0)):
        with pytest.raises(ValueError):
            cn.metrics.surface_metrics(pred, gt, library=lib, **bad)
    with pytest.raises(ValueError):
        cn.metrics.surface_metrics((pred[0], pred[1][:0]), gt, library=lib)


@pytest.mark.parametrize("backend", BACKENDS)
def test_surface_metrics_on_ply_files(backend, tmp_path):
    """M4."""
    lib, dev = _lib_and_dev(backend)
    rng = np.random.default_rng(6)
    va, vb = (rng.uniform(-1, 1, (n, 3)).astype(f32) for n in (200, 150))
    ta, tb = rng.integers(0, 200, (90, 3)).astype(np.int32), rng.integers(0, 150, (70, 3)).astype(np.int32)
    pa, pb, pc, pd, pq = (str(tmp_path / f"{n}.ply") for n in "abcdq")
    cn.write_ply(pa, va, ta, colors=rng.uniform(0, 1, (200, 3)))
    cn.write_ply(pb, vb, tb)
    with open(pc, "w") as fh:       # ASCII, normals behind the positions, a quality in front of the index list, vertex_index
        fh.write("ply\nformat ascii 1.0\ncomment hand written\nelement vertex 150\nproperty float x\nproperty float y\nproperty float z\n"
                 "property float nx\nproperty float ny\nproperty float nz\nelement face 70\nproperty uchar quality\n"
                 "property list uchar int vertex_index\nend_header\n")
        for v in vb:
            fh.write(" ".join(repr(float(c)) for c in v) + " 0 0 1\n")
        for t in tb:
            fh.write("9 3 %d %d %d\n" % tuple(t))
    for path, v, t in ((pa, va, ta), (pb, vb, tb), (pc, vb, tb)):
        gv, gt = cn.meshio.read_ply_mesh(path)
        assert gv.dtype == f32 and gt.dtype == np.int32 and np.array_equal(gv, v) and np.array_equal(gt, t), path
    kw = dict(n_samples=3000, seed=3, thresholds=(0.05, 0.2), library=lib)
    on_arrays = cn.metrics.surface_metrics((_t(va, dev), _t(ta, dev)), (_t(vb, dev), _t(tb, dev)), **kw)
    assert on_arrays["accuracy"] > 0
    for gt_path in (pb, pc):
        assert cn.metrics.compute_surface_metrics(pa, gt_path, device=dev, **kw) == on_arrays
    assert cn.compute_surface_metrics is cn.metrics.compute_surface_metrics
    # a file without faces is a cloud
    with open(pd, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 150\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
        for v in vb:
            fh.write(" ".join(repr(float(c)) for c in v) + "\n")
    assert cn.meshio.read_ply_mesh(pd)[1] is None
    assert cn.metrics.compute_surface_metrics(pa, pd, device=dev, **kw) == cn.metrics.surface_metrics((_t(va, dev), _t(ta, dev)), _t(vb, dev), **kw)
    with pytest.raises(ValueError):
        cn.metrics.compute_surface_metrics(pd, pa, device=dev, **kw)
    # a quad face, in ASCII and in binary
    with open(pq, "w") as fh:
        fh.write("ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                 "property list uchar int vertex_indices\nend_header\n0 0 0\n1 0 0\n1 1 0\n0 1 0\n4 0 1 2 3\n")
    with pytest.raises(ValueError, match="not a triangle"):
        cn.meshio.read_ply_mesh(pq)
    with open(pq, "wb") as fh:
        fh.write(b"ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                 b"property list uchar int vertex_indices\nend_header\n")
        fh.write(np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], "<f4").tobytes() + bytes([4]) + np.array([0, 1, 2, 3], "<i4").tobytes())
    with pytest.raises(ValueError, match="not a triangle"):
        cn.meshio.read_ply_mesh(pq)
    with open(pq, "w") as fh:       # a face element without an index list
        fh.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nproperty float z\nelement face 1\n"
                 "property int flags\nend_header\n0 0 0\n1\n")
    with pytest.raises(ValueError, match="vertex_indices"):
        cn.meshio.read_ply_mesh(pq)


# ---- ABI -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_argument_checks(backend):
    path, dev = _lib_and_dev(backend)
    lib = _lib.resolve_library(path)
    L = lib.lib
    assert L.cnr_abi_version() == _lib.ABI_VERSION == 9
    p, null, stream = _lib.ptr, C.c_void_p(0), _lib.stream_of(torch.device(dev))
    v, q = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], device=dev), torch.zeros(4, 3, device=dev)
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    cdf, summary, keys = (torch.zeros(k, dtype=torch.int64, device=dev) for k in (2, 5, 5))
    pts, faces, bary = torch.zeros(4, 3, device=dev), torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(4, 2, device=dev)
    d2 = torch.zeros(4, device=dev)
    big = 2 ** 31
    odd = lambda x: C.c_void_p(x.data_ptr() + 4)
    cases = []
    area = lambda **kw: (kw.get("v", p(v)), kw.get("V", 4), kw.get("t", p(t)), kw.get("F", 1), kw.get("cdf", p(cdf)), kw.get("summary", p(summary)), stream)
    for kw, msg in ((dict(F=0), "no faces"), (dict(F=-1), "no faces"), (dict(F=big), "below 2\\^31"), (dict(V=-1), "negative"), (dict(V=big), "below 2\\^31"),
                    (dict(v=null), "null argument"), (dict(t=null), "null argument"), (dict(cdf=null), "null argument"), (dict(summary=null), "null argument"),
                    (dict(cdf=odd(cdf)), "8-byte aligned"), (dict(summary=odd(summary)), "8-byte aligned")):
        cases.append(("cnr_mesh_area_cdf", area(**kw), msg))
    samp = lambda **kw: (kw.get("v", p(v)), kw.get("V", 4), kw.get("t", p(t)), kw.get("F", 1), kw.get("cdf", p(cdf)), kw.get("n", 4), 0,
                         kw.get("pts", p(pts)), kw.get("faces", p(faces)), kw.get("bary", p(bary)), stream)
    for kw, msg in ((dict(F=0), "no faces"), (dict(F=-1), "no faces"), (dict(F=big), "below 2\\^31"), (dict(V=-1), "negative"), (dict(V=big), "below 2\\^31"),
                    (dict(n=-1), "n_samples < 0"), (dict(v=null), "null argument"), (dict(t=null), "null argument"), (dict(cdf=null), "null argument"),
                    (dict(pts=null), "null argument"), (dict(faces=null), "null argument"), (dict(cdf=odd(cdf)), "8-byte aligned")):
        cases.append(("cnr_mesh_sample", samp(**kw), msg))
    dist = lambda **kw: (kw.get("q", p(q)), kw.get("n", 4), kw.get("v", p(v)), kw.get("V", 4), kw.get("t", p(t)), kw.get("F", 1), kw.get("d2", p(d2)),
                         kw.get("face", p(faces)), kw.get("closest", p(pts)), kw.get("keys", p(keys)), stream)
    for kw, msg in ((dict(F=0), "no faces"), (dict(F=-1), "no faces"), (dict(F=big), "below 2\\^31"), (dict(V=-1), "negative"), (dict(V=big), "below 2\\^31"),
                    (dict(n=-1), "n_query < 0"), (dict(q=null), "null argument"), (dict(v=null), "null argument"), (dict(t=null), "null argument"),
                    (dict(d2=null), "null argument"), (dict(face=null), "null argument"), (dict(keys=null), "null argument"),
                    (dict(keys=odd(keys)), "8-byte aligned")):
        cases.append(("cnr_point_mesh_distance", dist(**kw), msg))
    lib.timing_enable(True)
    try:
        lib.timing_collect()
        for name, args, msg in cases:
            assert getattr(L, name)(*args) < 0, (name, msg)
            with pytest.raises(RuntimeError, match=msg):
                lib.call(name, *args)
        # n == 0: a successful no-op, whatever the other pointers
        assert L.cnr_mesh_sample(p(v), 4, p(t), 1, p(cdf), 0, 0, null, null, null, stream) == 0
        assert L.cnr_point_mesh_distance(null, 0, p(v), 4, p(t), 1, null, null, null, null, stream) == 0
        assert lib.timing_collect() == []          # nothing was launched after a refusal or for an empty call
    finally:
        lib.timing_enable(False)
    # bary = NULL and closest = NULL are legal
    lib.call("cnr_mesh_area_cdf", *area())
    lib.call("cnr_mesh_sample", *samp(bary=null))
    lib.call("cnr_point_mesh_distance", *dist(closest=null))
    if dev != "cpu":
        torch.cuda.synchronize()
    assert faces.tolist() == [0, 0, 0, 0] and not torch.isnan(d2).any()


def test_header_binding_and_sources_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "colorneus_render.h")).read()
    csrc = os.path.join(root, "color-neus_amd", "csrc")
    ops = open(os.path.join(csrc, "cnr_ops.cpp")).read()
    names = ("cnr_mesh_area_cdf", "cnr_mesh_sample", "cnr_point_mesh_distance")
    for name, nargs in zip(names, (7, 11, 11)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and _lib.SIGNATURES[name][0] is C.c_int
        assert header.count("int %s(" % name) == 1 and ops.count("\nint %s(" % name) == 1
    order = list(_lib.SIGNATURES)
    assert [order.index(n) for n in names] == list(range(order.index("cnr_mesh_compact") + 1, order.index("cnr_mesh_compact") + 4))
    assert not [n for n in _lib.SIGNATURES if n.endswith("_bytes") and ("surface" in n or "sample" in n or "area" in n or "point_mesh" in n)]
    hip = open(os.path.join(csrc, "cnr_surface.hip")).read()
    assert "constexpr int kSurfThreads = 256;" in hip and "constexpr int kSurfQ = 2;" in hip and "constexpr int kSurfTile = 256;" in hip
    assert QUERIES_PER_WORKGROUP == 256 * 2 and FACES_PER_TILE == 256
    assert "constexpr int kMeshScanThreads = 1024, kMeshScanPer = 8;" in open(os.path.join(csrc, "cnr_meshcc.h")).read() and SCAN_CHUNK == 1024 * 8
    assert "cnr_surface" in open(os.path.join(csrc, "Makefile")).read().split("HIP_UNITS =")[1].split("\n")[0]
    # the Philox and multiply-high helpers have one definition, shared by the pixel choice and the sampler
    for fn, want in (("cnr_philox.h", 1), ("cnr_pixels.h", 0), ("cnr_surface.h", 0)):
        text = open(os.path.join(csrc, fn)).read()
        assert text.count("CNR_HD void pix_philox(") == want and text.count("CNR_HD unsigned long long pix_mulhi64(") == want, fn
