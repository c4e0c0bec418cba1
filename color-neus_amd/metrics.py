"""Geometry metrics of the evaluation path on the device library: nearest neighbours, Chamfer distance, accuracy / completeness / F-score.

The reference scores an extracted mesh with ``compute_chamfer_distance`` (lib/utils/mesh_tools.py:59-70): the vertices of two mesh files,
optionally normalised (``normalize_point_cloud``, :43-56), handed to ``pytorch3d.loss.chamfer_distance``.  Here the all-pairs search behind
it is one exact brute-force kernel (``cnr_nn_search``, include/colorneus_render.h); the reductions on its per-point results are a few torch
calls in float64.  That is the vertex-cloud parity route.  Vertex density is not surface density -- two tessellations of one surface have a
non-zero vertex Chamfer -- so ``surface_metrics`` measures the same figures between surfaces: points drawn uniformly by area
(``meshops.sample_surface``) and the exact closest triangle of a mesh for every point (``point_mesh_distance``, ``cnr_point_mesh_distance``).

Every function takes ``(N, 3)`` tensors of any float dtype and any strides, converts them to contiguous float32 on their own device and runs on
the current stream.  CUDA tensors go through the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no
CPU fallback).  NOTHING HERE IS DIFFERENTIABLE: inputs are detached and results carry no graph."""
import torch

from . import _lib, meshio, meshops, registration
from ._lib import points3, ptr, stream_of

__all__ = ["nearest_neighbors", "normalize_point_cloud", "chamfer_distance", "mesh_metrics", "compute_chamfer_distance", "point_mesh_distance",
           "surface_metrics", "compute_surface_metrics"]


def _library(library, dev):
    return _lib.library_for(library, dev, ("points", "searched"))


def _search(q, t, lib):
    """q (n,3), t (m,3): contiguous float32 on one device -> dist2 float32 (n,), idx int32 (n,)."""
    n, m = q.shape[0], t.shape[0]
    if m == 0:
        raise ValueError("nearest_neighbors: the target cloud is empty")
    dist2 = torch.empty(n, dtype=torch.float32, device=q.device)
    idx = torch.empty(n, dtype=torch.int32, device=q.device)
    if n == 0:
        return dist2, idx
    scratch, nb = lib.scratch("cnr_nn_scratch_bytes", q.device, n, m)
    lib.call("cnr_nn_search", ptr(q), n, ptr(t), m, ptr(dist2), ptr(idx), ptr(scratch), nb, stream_of(q))
    return dist2, idx


def _pair(x, y, names, library):
    x, y = points3(x, names[0]), points3(y, names[1])
    if x.device != y.device:
        raise ValueError(f"{names[0]} is on {x.device}, {names[1]} on {y.device}")
    return x, y, _library(library, x.device)


def nearest_neighbors(query, target, library=None):
    """For every query point the squared distance to its nearest target point and that point's index: ``(dist2 float32 (N,), idx int64 (N,))``.

    Exact brute force in float32: ``d2 = (dx*dx + dy*dy) + dz*dz`` with every operation rounded separately; of several targets at the minimal
    distance the one with the LOWEST index is returned; a NaN distance never wins, and a query with a NaN coordinate gets ``idx = -1`` and a NaN
    distance.  An empty target raises ValueError; an empty query returns empty tensors.  Not differentiable."""
    q, t, lib = _pair(query, target, ("query", "target"), library)
    dist2, idx = _search(q, t, lib)
    return dist2, idx.to(torch.int64)


def normalize_point_cloud(pc):
    """The reference's normalisation (mesh_tools.py:43-56) in float32: subtract the centroid, divide by the largest distance from it.
    Returns ``(pc_normalized, centroid, m)``."""
    centroid = torch.mean(pc, dim=0)
    pc = pc - centroid
    m = torch.max(torch.sqrt(torch.sum(pc ** 2, dim=1)))
    return pc / m, centroid, m


def _aligned(pred, gt, align, library, name):
    """``align=`` of the metric functions: ``pred`` (a cloud, or a ``(vertices, triangles)`` mesh) moved onto ``gt`` before anything is sampled or
    searched.  ``"rigid"`` / ``"similarity"`` run ``registration.icp(pred -> gt)`` from ``init="normalize"``; a ``Registration`` or a 4x4 matrix
    is applied as given.  The registration runs with ``icp``'s own defaults -- a mesh ``pred`` is sampled with 20 000 points under seed 0, 50
    iterations -- whatever ``n_samples`` / ``seed`` the metric itself uses; pass a ``Registration`` made with other settings to change that.  Returns ``(pred', {"transform": nested lists, "align_rms": the registration's rms, None for a bare matrix})``."""
    if isinstance(align, str):
        if align not in ("rigid", "similarity"):
            raise ValueError(f"{name}: align must be None, 'rigid', 'similarity', a Registration or a 4x4 matrix (got {align!r})")
        align = registration.icp(pred, gt, with_scale=align == "similarity", init="normalize", library=library)
    matrix, rms = (align.matrix, align.rms) if isinstance(align, registration.Registration) else (registration.as_matrix(align), None)
    info = {"transform": matrix.tolist(), "align_rms": rms}
    if isinstance(pred, (tuple, list)):
        return (registration.apply_transform(pred[0], matrix), pred[1]), info
    return registration.apply_transform(pred, matrix), info


def chamfer_distance(x, y, norm=False, library=None, align=None):
    """``mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2`` as a 0-dim float64 tensor on the inputs' device: squared distances, the mean
    over the points of each direction, the two directions added.

    This is what ``pytorch3d.loss.chamfer_distance(x[None], y[None])`` returns with the defaults the reference calls it with (one batch element,
    ``point_reduction="mean"``, ``norm=2``; mesh_tools.py:68).  pytorch3d is not a dependency of this package, so that equivalence is stated from
    its documentation and not checked by the tests.  ``norm=True`` first applies ``normalize_point_cloud`` to each cloud separately, as the
    reference does.  The nearest-neighbour distances are float32 (``nearest_neighbors``); the two means are float64 sums of them.
    ``align`` (None: off) first moves ``x`` onto ``y``: ``"rigid"`` / ``"similarity"`` by ``registration.icp``, or a given ``Registration`` /
    4x4 matrix.  Not differentiable."""
    x, y, lib = _pair(x, y, ("x", "y"), library)
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError("chamfer_distance: empty point cloud")
    if align is not None:
        x = _aligned(x, y, align, lib, "chamfer_distance")[0].contiguous()
    if norm:
        x, y = normalize_point_cloud(x)[0].contiguous(), normalize_point_cloud(y)[0].contiguous()
    dxy, _ = _search(x, y, lib)
    dyx, _ = _search(y, x, lib)
    return dxy.to(torch.float64).mean() + dyx.to(torch.float64).mean()


def mesh_metrics(pred, gt, thresholds=(0.01, 0.02, 0.05), library=None, align=None):
    """The usual surface-reconstruction figures from ONE pair of searches (pred -> gt and gt -> pred), as a dict of Python floats:

    ``accuracy`` mean distance pred -> gt, ``completeness`` mean distance gt -> pred, ``chamfer_l1`` their mean, ``chamfer_l2`` the value of
    ``chamfer_distance(pred, gt)``, and per threshold t the keys ``"precision@t"``, ``"recall@t"``, ``"fscore@t"`` (t formatted with ``%g``,
    e.g. ``"fscore@0.02"``): the share of pred points / of gt points whose distance is < t, and 2PR / (P + R) (0 when P + R = 0).  Distances are sqrt of the float32 squared distances,
    taken and averaged in float64.  ``align`` (None: off; ``"rigid"``, ``"similarity"``, a ``Registration`` or a 4x4 matrix) first moves ``pred``
    onto ``gt`` (``registration.icp`` from ``init="normalize"``); the dict then also carries ``"transform"`` (the 4x4 matrix as nested lists) and
    ``"align_rms"``.  Not differentiable."""
    p, g, lib = _pair(pred, gt, ("pred", "gt"), library)
    if p.shape[0] == 0 or g.shape[0] == 0:
        raise ValueError("mesh_metrics: empty point cloud")
    info = {}
    if align is not None:
        p, info = _aligned(p, g, align, lib, "mesh_metrics")
        p = p.contiguous()
    d2_pg, _ = _search(p, g, lib)
    d2_gp, _ = _search(g, p, lib)
    return {**_figures(d2_pg, d2_gp, thresholds, None), **info}


def _mesh(mesh, name, dev=None):
    """``(vertices, triangles)`` -> contiguous float32 (V, 3) and int32 (F, 3) on the vertices' device; F == 0 raises ValueError."""
    if not isinstance(mesh, (tuple, list)) or len(mesh) != 2:
        raise ValueError(f"{name}: expected a (vertices, triangles) pair")
    v = points3(mesh[0], f"{name} vertices", dev)
    t = meshops._triangles(mesh[1], v.device)
    if t.shape[0] == 0:
        raise ValueError(f"{name}: the mesh has no faces")
    return v, t


def _closest_face(q, v, t, lib, want_closest=False):
    """q (n,3), v (V,3) float32, t (F,3) int32, contiguous on one device, F > 0 -> dist2 float32 (n,), face int32 (n,), closest (n,3) or None."""
    n, dev = q.shape[0], q.device
    dist2 = torch.empty(n, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev)
    closest = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_closest else None
    if n > 0:
        keys, _ = lib.scratch("cnr_point_mesh_distance", dev, nbytes=8 * n)      # the library's uint64 candidate keys, one per query
        lib.call("cnr_point_mesh_distance", ptr(q), n, ptr(v), v.shape[0], ptr(t), t.shape[0], ptr(dist2), ptr(face), ptr(closest), ptr(keys),
                 stream_of(dev))
    return dist2, face, closest


def point_mesh_distance(points, vertices, triangles, return_closest=False, library=None):
    """For every point the squared distance to the mesh SURFACE and the face that attains it (``cnr_point_mesh_distance``):
    ``(dist2 float32 (N,), face int64 (N,))``, with ``return_closest=True`` also the closest point on that face, float32 (N, 3).

    Exact brute force over all point / triangle pairs in float32, the closest point of each closed triangle by Ericson's region classification
    (include/colorneus_render.h writes the order of operations down); of several faces at the minimal distance the one with the LOWEST index is
    returned.  A face with an index outside ``[0, V)`` or a non-finite distance never wins; a point with a NaN coordinate gets ``face = -1`` and
    NaN.  A mesh without faces raises ValueError; no points gives empty tensors.  Not differentiable."""
    q = points3(points, "points")
    v, t = _mesh((vertices, triangles), "mesh", q.device)
    lib = _lib.library_for(library, q.device, ("points", "measured"))
    dist2, face, closest = _closest_face(q, v, t, lib, return_closest)
    return (dist2, face.to(torch.int64), closest) if return_closest else (dist2, face.to(torch.int64))


def _figures(d2_pg, d2_gp, thresholds, max_dist):
    """mesh_metrics' dict from the two directions' float32 squared distances (float64 reductions; ``max_dist`` clamps the distances)."""
    d2_pg, d2_gp = d2_pg.to(torch.float64), d2_gp.to(torch.float64)
    d_pg, d_gp = d2_pg.sqrt(), d2_gp.sqrt()
    if max_dist is not None:
        m = float(max_dist)
        d_pg, d_gp, d2_pg, d2_gp = d_pg.clamp(max=m), d_gp.clamp(max=m), d2_pg.clamp(max=m * m), d2_gp.clamp(max=m * m)
    acc, comp = d_pg.mean(), d_gp.mean()
    out = {"accuracy": float(acc), "completeness": float(comp), "chamfer_l1": float((acc + comp) * 0.5), "chamfer_l2": float(d2_pg.mean() + d2_gp.mean())}
    for t in thresholds:
        prec = float((d_pg < float(t)).sum()) / d_pg.shape[0]
        rec = float((d_gp < float(t)).sum()) / d_gp.shape[0]
        out[f"precision@{t:g}"], out[f"recall@{t:g}"] = prec, rec
        out[f"fscore@{t:g}"] = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return out


def surface_metrics(pred, gt, n_samples=100000, seed=0, thresholds=(0.01, 0.02, 0.05), exact=True, max_dist=None, library=None, align=None):
    """The figures of ``mesh_metrics`` -- same keys, same definitions, float64 reductions -- measured between SURFACES instead of vertex clouds,
    so that they do not move with the tessellation.  ``pred`` is ``(vertices, triangles)``; ``gt`` is ``(vertices, triangles)`` or a bare
    ``(N, 3)`` cloud (a scanned ground truth, as DTU's).

    Each mesh is sampled by area (``meshops.sample_surface``: ``n_samples`` points, pred under ``seed``, gt under ``seed + 1``).  Accuracy is
    measured from the pred samples, completeness from the gt samples (or the gt cloud).  ``exact=True``: each point to the other SURFACE
    (``point_mesh_distance``; to the gt cloud's nearest point when gt is a cloud).  ``exact=False``: point to the other side's SAMPLES through
    ``cnr_nn_search`` -- ``mesh_metrics`` of the two sample sets.  ``max_dist`` clamps every distance before the means and thresholds (the DTU
    protocol's outlier cap); ``chamfer_l2`` then clamps the squared distances at ``max_dist ** 2``.  ``align`` (None: off; ``"rigid"``,
    ``"similarity"``, a ``Registration`` or a 4x4 matrix) first moves the pred mesh onto ``gt`` -- ``registration.icp`` of its samples to the gt
    surface (or cloud) from ``init="normalize"``, with ``icp``'s own ``n_samples=20000, seed=0`` and not this call's -- before anything is sampled
    or measured; the dict then also carries ``"transform"`` and
    ``"align_rms"``.  Not differentiable."""
    n_samples = int(n_samples)
    if n_samples <= 0:
        raise ValueError(f"surface_metrics: n_samples must be positive (got {n_samples})")
    if max_dist is not None and not float(max_dist) > 0.0:
        raise ValueError(f"surface_metrics: max_dist must be positive (got {max_dist})")
    pv, pt = _mesh(pred, "pred")
    dev = pv.device
    lib = _lib.library_for(library, dev, ("meshes", "compared"))
    info = {}
    if align is not None:
        (pv, pt), info = _aligned((pv, pt), gt, align, lib, "surface_metrics")
        pv = pv.contiguous()
    ps = meshops.sample_surface(pv, pt, n_samples, seed=seed, library=lib)[0]
    if isinstance(gt, (tuple, list)):
        gv, gtri = _mesh(gt, "gt", dev)
        gs = meshops.sample_surface(gv, gtri, n_samples, seed=int(seed) + 1, library=lib)[0]
        d2_pg = _closest_face(ps, gv, gtri, lib)[0] if exact else _search(ps, gs, lib)[0]
    else:
        gs = points3(gt, "gt", dev)
        if gs.shape[0] == 0:
            raise ValueError("surface_metrics: the gt cloud is empty")
        d2_pg = _search(ps, gs, lib)[0]
    d2_gp = _closest_face(gs, pv, pt, lib)[0] if exact else _search(gs, ps, lib)[0]
    return {**_figures(d2_pg, d2_gp, thresholds, max_dist), **info}


def compute_surface_metrics(path_pred, path_gt, device="cuda", n_samples=100000, seed=0, thresholds=(0.01, 0.02, 0.05), exact=True, max_dist=None,
                            library=None, align=None):
    """``surface_metrics`` on two PLY files (``meshio.read_ply_mesh``): ``path_pred`` must hold triangles; a ``path_gt`` without a face element
    (or with an empty one) is taken as a cloud.  ``align``: as in ``surface_metrics``."""
    pv, pt = meshio.read_ply_mesh(path_pred)
    gv, gt = meshio.read_ply_mesh(path_gt)
    if pt is None:
        raise ValueError(f"{path_pred}: the predicted mesh has no face element")
    pred = (torch.from_numpy(pv).to(device), torch.from_numpy(pt).to(device))
    gt = (torch.from_numpy(gv).to(device), torch.from_numpy(gt).to(device)) if gt is not None and gt.shape[0] else torch.from_numpy(gv).to(device)
    return surface_metrics(pred, gt, n_samples=n_samples, seed=seed, thresholds=thresholds, exact=exact, max_dist=max_dist, library=library,
                           align=align)


def compute_chamfer_distance(path_source, path_target, device="cuda", norm=False, library=None, align=None):
    """The reference helper (mesh_tools.py:59-70; its ``deivce`` argument spelled ``device``) on the vertices of two PLY files:
    ``chamfer_distance`` of the two vertex clouds on ``device`` (``align``: as there).  Not differentiable."""
    src = torch.from_numpy(meshio.read_ply_vertices(path_source)).to(device)
    tgt = torch.from_numpy(meshio.read_ply_vertices(path_target)).to(device)
    return chamfer_distance(src, tgt, norm=norm, library=library, align=align)
