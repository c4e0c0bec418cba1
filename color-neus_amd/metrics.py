"""Geometry metrics of the evaluation path on the device library: nearest neighbours, Chamfer distance, accuracy / completeness / F-score.

The reference scores an extracted mesh with ``compute_chamfer_distance`` (lib/utils/mesh_tools.py:59-70): the vertices of two mesh files,
optionally normalised (``normalize_point_cloud``, :43-56), handed to ``pytorch3d.loss.chamfer_distance``.  Here the all-pairs search behind
it is one exact brute-force kernel (``cnr_nn_search``, include/colorneus_render.h); the reductions on its per-point results are a few torch
calls in float64.

Every function takes ``(N, 3)`` tensors of any float dtype and any strides, converts them to contiguous float32 on their own device and runs on
the current stream.  CUDA tensors go through the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no
CPU fallback).  NOTHING HERE IS DIFFERENTIABLE: inputs are detached and results carry no graph."""
import torch

from . import _lib, meshio
from ._lib import ptr, stream_of

__all__ = ["nearest_neighbors", "normalize_point_cloud", "chamfer_distance", "mesh_metrics", "compute_chamfer_distance"]


def _library(library, dev):
    return _lib.library_for(library, dev, ("points", "searched"))


def _points(x, name):
    if not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dim() != 2 or x.shape[1] != 3 or not x.is_floating_point():
        raise ValueError(f"{name}: expected a floating-point (N, 3) tensor, got {tuple(x.shape)} {x.dtype}")
    return x.detach().to(torch.float32).contiguous()


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
    x, y = _points(x, names[0]), _points(y, names[1])
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


def _mean64(d):
    return d.to(torch.float64).mean()


def chamfer_distance(x, y, norm=False, library=None):
    """``mean_i min_j |x_i - y_j|^2 + mean_j min_i |x_i - y_j|^2`` as a 0-dim float64 tensor on the inputs' device: squared distances, the mean
    over the points of each direction, the two directions added.

    This is what ``pytorch3d.loss.chamfer_distance(x[None], y[None])`` returns with the defaults the reference calls it with (one batch element,
    ``point_reduction="mean"``, ``norm=2``; mesh_tools.py:68).  pytorch3d is not a dependency of this package, so that equivalence is stated from
    its documentation and not checked by the tests.  ``norm=True`` first applies ``normalize_point_cloud`` to each cloud separately, as the
    reference does.  The nearest-neighbour distances are float32 (``nearest_neighbors``); the two means are float64 sums of them.
    Not differentiable."""
    x, y, lib = _pair(x, y, ("x", "y"), library)
    if x.shape[0] == 0 or y.shape[0] == 0:
        raise ValueError("chamfer_distance: empty point cloud")
    if norm:
        x, y = normalize_point_cloud(x)[0].contiguous(), normalize_point_cloud(y)[0].contiguous()
    dxy, _ = _search(x, y, lib)
    dyx, _ = _search(y, x, lib)
    return _mean64(dxy) + _mean64(dyx)


def mesh_metrics(pred, gt, thresholds=(0.01, 0.02, 0.05), library=None):
    """The usual surface-reconstruction figures from ONE pair of searches (pred -> gt and gt -> pred), as a dict of Python floats:

    ``accuracy`` mean distance pred -> gt, ``completeness`` mean distance gt -> pred, ``chamfer_l1`` their mean, ``chamfer_l2`` the value of
    ``chamfer_distance(pred, gt)``, and per threshold t the keys ``"precision@t"``, ``"recall@t"``, ``"fscore@t"`` (t formatted with ``%g``,
    e.g. ``"fscore@0.02"``): the share of pred points / of gt points whose distance is < t, and 2PR / (P + R) (0 when P + R = 0).  Distances are sqrt of the float32 squared distances,
    taken and averaged in float64.  Not differentiable."""
    p, g, lib = _pair(pred, gt, ("pred", "gt"), library)
    if p.shape[0] == 0 or g.shape[0] == 0:
        raise ValueError("mesh_metrics: empty point cloud")
    d2_pg, _ = _search(p, g, lib)
    d2_gp, _ = _search(g, p, lib)
    d_pg, d_gp = d2_pg.to(torch.float64).sqrt(), d2_gp.to(torch.float64).sqrt()
    acc, comp = d_pg.mean(), d_gp.mean()
    out = {"accuracy": float(acc), "completeness": float(comp), "chamfer_l1": float((acc + comp) * 0.5),
           "chamfer_l2": float(_mean64(d2_pg) + _mean64(d2_gp))}
    for t in thresholds:
        prec = float((d_pg < float(t)).sum()) / p.shape[0]
        rec = float((d_gp < float(t)).sum()) / g.shape[0]
        out[f"precision@{t:g}"], out[f"recall@{t:g}"] = prec, rec
        out[f"fscore@{t:g}"] = 2.0 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return out


def compute_chamfer_distance(path_source, path_target, device="cuda", norm=False, library=None):
    """The reference helper (mesh_tools.py:59-70; its ``deivce`` argument spelled ``device``) on the vertices of two PLY files:
    ``chamfer_distance`` of the two vertex clouds on ``device``.  Not differentiable."""
    src = torch.from_numpy(meshio.read_ply_vertices(path_source)).to(device)
    tgt = torch.from_numpy(meshio.read_ply_vertices(path_target)).to(device)
    return chamfer_distance(src, tgt, norm=norm, library=library)
