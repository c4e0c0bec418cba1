"""ICP registration on the device library: the rigid or similarity map that takes a reconstruction onto its ground truth.

With learnable cameras (``cameras.PoseNet`` / ``FocalNet``; ``LEARN_R`` / ``LEARN_T`` / ``LEARN_FOCAL`` in the reference configurations) a
reconstruction drifts by a similarity transform against the scan, and every distance of ``metrics`` then measures that drift.  The reference's
answer, ``compute_chamfer_distance(norm=True)``, moves each cloud to its centroid and divides by its largest radius: it does not rotate, and one
floater moves both.  ``icp`` registers instead: iterated closest points, to a cloud (point to point) or to a mesh (point to the exact closest
surface point), rigid or with scale.  An iteration is the existing exact search plus a reduction and a closed-form solve (``cnr_icp``,
include/colorneus_render.h writes every operation down); the loop stays on the device and gives the same bits on every run and build.

CUDA tensors go through the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no CPU fallback).
NOTHING HERE IS DIFFERENTIABLE."""
import math

import numpy as np
import torch

from . import _lib, meshops
from ._lib import points3, ptr, stream_of

__all__ = ["icp", "Registration", "apply_transform", "as_matrix"]

_CHUNK, _TERMS = 256, 18     # cnr_icp's moment chunk and terms per chunk row


def as_matrix(matrix, dev=None):
    """Anything 4x4 (a tensor, nested lists, a numpy array) -> a detached float64 (4, 4) tensor (on ``dev`` when given)."""
    m = matrix if torch.is_tensor(matrix) else torch.as_tensor(np.asarray(matrix, dtype=np.float64))
    if tuple(m.shape) != (4, 4):
        raise ValueError(f"expected a 4x4 matrix, got {tuple(m.shape)}")
    return m.detach().to(device=dev, dtype=torch.float64)


def apply_transform(points, matrix):
    """``points @ M[:3, :3].T + M[:3, 3]`` in float64, returned in the dtype (and on the device) of ``points``.  ``matrix``: 4x4."""
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.asarray(points))
    m = as_matrix(matrix, points.device)
    out = points.detach().to(torch.float64) @ m[:3, :3].T + m[:3, 3]
    return out.to(points.dtype)


class Registration:
    """The result of ``icp``: ``matrix`` (4x4 float64, on the CPU) = ``[[s*R, t], [0, 1]]``, its parts ``scale`` (float), ``rotation``
    (3x3 float64) and ``translation`` (3, float64), ``history`` ((K, 4) float64: per iteration the inliers, the correspondences that changed,
    the sum of the inliers' squared distances and the solve's status, all under the transform the iteration STARTED with), ``converged`` (an
    iteration changed no correspondence and its solve was accepted) and ``rms`` (the last row's ``sqrt(sum_d2 / n_inliers)``, NaN without
    inliers).  ``matrix`` is always the transform behind the LAST row of ``history``; ``rms`` is measured in front of that row's solve.  At a
    fixed point (``converged`` against a cloud without a gate) the two transforms are the same bits, so ``rms`` is the residual of ``matrix``
    itself; otherwise ``matrix`` is one solve ahead of ``rms``, which is then an upper figure for a mesh target (every solve lowers it)."""

    def __init__(self, rotation, translation, scale, history, converged):
        self.rotation = rotation.to(torch.float64)
        self.translation = translation.to(torch.float64)
        self.scale = float(scale)
        self.history = history
        self.converged = bool(converged)
        self.matrix = torch.eye(4, dtype=torch.float64)
        self.matrix[:3, :3] = self.scale * self.rotation
        self.matrix[:3, 3] = self.translation

    @property
    def rms(self):
        if self.history.shape[0] == 0 or float(self.history[-1, 0]) <= 0:
            return float("nan")
        return math.sqrt(float(self.history[-1, 2]) / float(self.history[-1, 0]))

    def apply(self, points):
        return apply_transform(points, self.matrix)

    def __repr__(self):
        return f"Registration(scale={self.scale:.6g}, iterations={self.history.shape[0]}, converged={self.converged}, rms={self.rms:.6g})"


def _initial(init, src, tgt_pts, c_src, c_tgt):
    """The starting transform as cnr_icp's 16 doubles (on the CPU) from ``init``; c_src / c_tgt: the float64 means (CPU tensors)."""
    T = torch.zeros(16, dtype=torch.float64)
    R, t, s = torch.eye(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64), 1.0
    if init is None:
        pass
    elif isinstance(init, str):
        if init == "centroid":
            t = c_tgt - c_src
        elif init == "normalize":
            # normalize_point_cloud of each side: (x - c) / m with m the largest distance from the centroid; matching the two normalised
            # clouds is x' = (m_tgt / m_src) * (x - c_src) + c_tgt
            m_src = float((src.to(torch.float64).cpu() - c_src).norm(dim=1).max())
            m_tgt = float((tgt_pts.to(torch.float64).cpu() - c_tgt).norm(dim=1).max())
            if not (m_src > 0.0 and m_tgt > 0.0):
                raise ValueError("icp: init='normalize' needs clouds with an extent")
            s = m_tgt / m_src
            t = c_tgt - s * c_src
        else:
            raise ValueError(f"icp: unknown init {init!r} (None, 'centroid', 'normalize' or a 4x4 matrix)")
    else:
        m = as_matrix(init).cpu()
        A = m[:3, :3]
        det = float(torch.linalg.det(A))
        if not det > 0.0:
            raise ValueError(f"icp: the init matrix must be [[s*R, t], [0, 1]] with s > 0 and a proper rotation R (its determinant is {det:g}: "
                             "singular, or a reflection)")
        s = det ** (1.0 / 3.0)
        R, t = A / s, m[:3, 3].clone()
        # float64 round-off of a composed similarity is below 1e-12; 1e-6 also takes a matrix that went through float32
        if float((R @ R.T - torch.eye(3, dtype=torch.float64)).abs().max()) > 1e-6 or m[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
            raise ValueError("icp: the init matrix must be [[s*R, t], [0, 1]]: its upper block is not a scaled rotation (shear or unequal scales), "
                             "or its last row is not (0, 0, 0, 1)")
    T[:9], T[9:12], T[12] = R.reshape(9), t, s
    return T


def _stops(history):
    """Per history row: nothing changed (a fixed point) or the solve was refused (status 1)."""
    return (history[:, 1] == 0) | (history[:, 3] != 0)


def icp(source, target, *, with_scale=False, init=None, iterations=50, check_every=10, max_dist=None, n_samples=20000, seed=0, library=None):
    """Register ``source`` to ``target`` by iterated closest points (``cnr_icp``) and return a ``Registration``.

    ``source``: an ``(N, 3)`` cloud, or a ``(vertices, triangles)`` mesh, which is sampled by area (``meshops.sample_surface``: ``n_samples``
    points under ``seed``).  ``target``: a cloud (point to point) or a mesh (point to the exact closest surface point).  ``with_scale``: solve a
    similarity instead of a rigid map.  ``init``: None (the identity), ``"centroid"`` (the translation between the float64 means),
    ``"normalize"`` (the similarity ``metrics.normalize_point_cloud`` implies: centroids matched, ``s = m_tgt / m_src`` -- the reference's
    ``norm=True`` as a starting point; a mesh target's vertices stand for it) or a 4x4 matrix ``[[s*R, t], [0, 1]]`` with ``s > 0`` and a proper
    rotation (a reflection, a shear or unequal scales raise ValueError: the solve keeps none of them).  ``max_dist``: pairs
    farther apart are left out of the solve (squared in float32 for the gate); None: no gate.

    The loop issues ``check_every`` iterations at a time, reads their history rows and issues no further batch once one of them has no changed
    correspondence (``converged``) or status 1 (a degenerate solve: fewer than three inliers, no extent).  ``check_every=None`` runs all
    ``iterations`` without a synchronisation.  What the batch ran behind the stopping row:

    * status 1, or no changed correspondence against a CLOUD WITHOUT A GATE: the pairs, hence the solve, hence every later iteration repeat
      that row bit for bit.  The history is cut behind the stopping row and the result does not depend on ``check_every``.
    * no changed correspondence against a MESH (the closest points still move on their faces) or WITH A GATE (the inlier set may still change):
      the later iterations of the batch have refined the transform.  All their rows are kept, so ``matrix`` is the transform behind the last
      row, and the number of rows depends on ``check_every`` (``check_every=1`` stops at the stopping row itself).

    The moments are taken about the two clouds' float64 means, computed once (the one set-up
    synchronisation).  Not differentiable."""
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"icp: iterations must not be negative (got {iterations})")
    if check_every is not None and int(check_every) <= 0:
        raise ValueError(f"icp: check_every must be positive or None (got {check_every})")
    if isinstance(source, (tuple, list)):
        sv = points3(source[0], "source vertices")
        dev = sv.device
        lib = _lib.library_for(library, dev, ("points", "registered"))
        src = meshops.sample_surface(sv, source[1], int(n_samples), seed=seed, library=lib)[0]
    else:
        src = points3(source, "source")
        dev = src.device
        lib = _lib.library_for(library, dev, ("points", "registered"))
    if isinstance(target, (tuple, list)):
        tgt = points3(target[0], "target vertices", dev)
        tri = meshops._triangles(target[1], dev)
        if tri.shape[0] == 0:
            raise ValueError("icp: the target mesh has no faces")
    else:
        tgt, tri = points3(target, "target", dev), None
    n, m = src.shape[0], tgt.shape[0]
    if n == 0 or m == 0:
        raise ValueError("icp: empty point cloud")
    if max_dist is None:
        max_dist2 = float("inf")
    else:
        if not float(max_dist) >= 0.0:
            raise ValueError(f"icp: max_dist must not be negative (got {max_dist})")
        d = np.float32(max_dist)
        max_dist2 = float(d * d)
    c_src, c_tgt = src.to(torch.float64).mean(dim=0).cpu(), tgt.to(torch.float64).mean(dim=0).cpu()
    pivots = torch.cat([c_src, c_tgt]).contiguous()                      # host
    transform = _initial(init, src, tgt, c_src, c_tgt).to(dev)
    history = torch.empty(max(iterations, 1), 4, dtype=torch.float64, device=dev)
    moved, matched = torch.empty(n, 3, dtype=torch.float32, device=dev), torch.empty(n, 3, dtype=torch.float32, device=dev)
    dist2, idx = torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    partials = torch.empty((n + _CHUNK - 1) // _CHUNK, _TERMS, dtype=torch.float64, device=dev)
    step = iterations if check_every is None else int(check_every)
    done = 0
    while done < iterations:
        k = min(step, iterations - done)
        lib.call("cnr_icp", ptr(src), n, ptr(tgt), m, ptr(tri), 0 if tri is None else tri.shape[0], ptr(pivots), 1 if with_scale else 0, max_dist2,
                 k, 1 if done else 0, ptr(transform), ptr(history[done:]), ptr(moved), ptr(matched), ptr(dist2), ptr(idx), ptr(keys), ptr(partials),
                 stream_of(dev))
        done += k
        if check_every is not None and bool(_stops(history[done - k:done].cpu()).any()):
            break
    # matrix = the transform behind the last row kept: the rows behind a stopping row are dropped only where they provably repeat it (see above)
    hist = history[:done].cpu().clone()
    stop = _stops(hist).nonzero()
    converged = False
    if stop.numel():
        first = int(stop[0, 0])
        converged = bool(hist[first, 3] == 0)
        if not converged or (tri is None and max_dist is None):
            hist = hist[:first + 1]
    T = transform.cpu()
    return Registration(T[:9].reshape(3, 3).clone(), T[9:12].clone(), float(T[12]), hist, converged)
