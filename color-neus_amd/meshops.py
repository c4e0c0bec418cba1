"""Mesh clean-up on the device library: connected components of an indexed triangle mesh and removal of the small ones ("floaters").

The iso-surface of a NeuS-style SDF almost always carries small closed shells away from the object and fragments near the bounding box;
evaluation scripts remove them before scoring (``trimesh.split`` and "keep the largest" in the reference's environment).  Here that is
three entry points of the C ABI (include/colorneus_render.h, where the definitions are): ``cnr_mesh_components`` labels the components with a
lock-free union-find, ``cnr_mesh_select`` marks what to keep and scans the marks into index maps, ``cnr_mesh_compact`` writes the kept
vertices, colours and triangles in their original order.  Everything is integer work: the results are exact and the same bits on every run.
``sample_surface`` draws points uniformly by area on a mesh (``cnr_mesh_area_cdf``, ``cnr_mesh_sample``): the input of the surface metrics.

``triangles`` may be a tensor or a numpy array of any integer dtype and any strides, ``vertices`` / ``colors`` of any float dtype; they are
converted to contiguous int32 / float32 on the device of ``vertices`` (``connected_components``: of ``triangles``).  CUDA tensors go through
the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no CPU fallback).  NOTHING HERE IS
DIFFERENTIABLE: inputs are detached and results carry no graph."""
import numpy as np
import torch

from . import _lib
from ._lib import points3, ptr, stream_of

__all__ = ["connected_components", "clean_mesh", "sample_surface"]

_MODES = {"largest": 0, "threshold": 1}


def _triangles(t, dev=None):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise ValueError(f"triangles: expected an integer dtype, got {t.dtype}")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"triangles: expected an (F, 3) tensor, got {tuple(t.shape)}")
    t = t.detach()
    if t.numel() and t.dtype == torch.int64:
        # an index that does not fit int32 is outside [0, V) for every V the library takes: it stays invalid (-1) instead of wrapping
        t = torch.where((t < 0) | (t > 2 ** 31 - 1), torch.full_like(t, -1), t)
    return t.to(device=dev if dev is not None else t.device, dtype=torch.int32).contiguous()


def _components(t, n_vertices, lib):
    """t: contiguous int32 (F, 3) -> (labels, face_count, vertex_count, summary [4], dropped [1]), all device int32, nothing read back."""
    dev, V = t.device, int(n_vertices)
    labels, face_count, vertex_count = (torch.empty(V, dtype=torch.int32, device=dev) for _ in range(3))
    summary = torch.empty(4, dtype=torch.int32, device=dev)
    dropped = torch.empty(1, dtype=torch.int32, device=dev)
    lib.call("cnr_mesh_components", ptr(t), t.shape[0], V, ptr(labels), ptr(face_count), ptr(vertex_count), ptr(summary), ptr(dropped),
             stream_of(dev))
    return labels, face_count, vertex_count, summary, dropped


def connected_components(triangles, n_vertices, library=None):
    """The connected components of the mesh ``triangles`` [F, 3] over ``n_vertices`` vertices (``cnr_mesh_components``).

    Returns a dict: device int32 tensors ``labels`` [V] (the smallest vertex index of each vertex's component), ``face_count`` [V] and
    ``vertex_count`` [V] (a component's totals at its root ``r``, where ``labels[r] == r``; 0 elsewhere), and Python ints ``n_components``,
    ``n_components_with_faces``, ``largest_label`` (most faces, ties to the lowest label; -1 without a valid triangle),
    ``largest_face_count`` and ``dropped`` (triangles with an index outside ``[0, n_vertices)``: they connect nothing).  A vertex no valid
    triangle names is a component of its own with zero faces.  Reading the five ints is the call's one host synchronisation."""
    n_vertices = int(n_vertices)
    if n_vertices < 0:
        raise ValueError(f"connected_components: n_vertices must not be negative (got {n_vertices})")
    t = _triangles(triangles)
    lib = _lib.library_for(library, t.device, ("a mesh", "labelled"))
    labels, face_count, vertex_count, summary, dropped = _components(t, n_vertices, lib)
    s = torch.cat([summary, dropped]).tolist()
    return {"labels": labels, "face_count": face_count, "vertex_count": vertex_count, "n_components": s[0], "n_components_with_faces": s[1],
            "largest_label": s[2], "largest_face_count": s[3], "dropped": s[4]}


def clean_mesh(vertices, triangles, colors=None, keep="largest", min_faces=0, min_ratio=0.0, library=None):
    """Remove components from a mesh: ``(vertices', triangles', colors' or None, info)``, device tensors (float32 [V', 3], int32 [F', 3],
    float32 [V', 3]) in the ORIGINAL order of the kept vertices and faces, the indices of ``triangles'`` renumbered.

    ``keep="largest"`` keeps the component with the most faces (ties: the one with the lowest vertex index) and takes no thresholds;
    ``keep="threshold"`` keeps every component with at least ``max(min_faces, ceil(min_ratio * largest_face_count))`` faces (the product and
    the ceiling in float32).  Triangles with an index outside ``[0, V)`` and vertices that no kept triangle's component holds -- unreferenced
    vertices included -- are removed.  ``info``: the ints of ``connected_components`` plus ``n_vertices`` / ``n_faces`` (of the result) and the
    device tensors ``labels``, ``face_count``, ``vertex_count``, ``keep_vertex`` / ``keep_face`` (bool) and ``vertex_map`` [V] / ``face_map`` [F]
    (int32: the new index, -1 for what was removed).  One host read (the summary and the two totals) sizes the outputs, as in
    ``marching_cubes``.  Not differentiable."""
    if keep not in _MODES:
        raise ValueError(f"clean_mesh: keep must be 'largest' or 'threshold', got {keep!r}")
    min_faces, min_ratio = int(min_faces), float(min_ratio)
    if min_faces < 0 or not min_ratio >= 0.0:
        raise ValueError(f"clean_mesh: min_faces and min_ratio must not be negative (got {min_faces}, {min_ratio})")
    if keep == "largest" and (min_faces or min_ratio):
        raise ValueError("clean_mesh: keep='largest' takes no min_faces / min_ratio (use keep='threshold')")
    dev = vertices.device if torch.is_tensor(vertices) else (triangles.device if torch.is_tensor(triangles) else torch.device("cpu"))
    lib = _lib.library_for(library, dev, ("a mesh", "cleaned"))
    v = points3(vertices, "vertices", dev)
    t = _triangles(triangles, dev)
    col = points3(colors, "colors", dev, v.shape[0]) if colors is not None else None
    V, F = v.shape[0], t.shape[0]
    labels, face_count, vertex_count, summary, dropped = _components(t, V, lib)
    keep_vertex, keep_face = torch.empty(V, dtype=torch.uint8, device=dev), torch.empty(F, dtype=torch.uint8, device=dev)
    vertex_map, face_map = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int32, device=dev)
    lib.call("cnr_mesh_select", ptr(t), F, V, ptr(labels), ptr(face_count), ptr(summary), _MODES[keep], min_faces, min_ratio, ptr(keep_vertex),
             ptr(keep_face), ptr(vertex_map), ptr(face_map), ptr(totals), stream_of(dev))
    s = torch.cat([summary, dropped, totals]).tolist()      # the one host round trip: the caller owns the output buffers
    nv, nf = s[5], s[6]
    out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
    out_t = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    out_c = torch.empty(nv, 3, dtype=torch.float32, device=dev) if col is not None else None
    if nv > 0:      # (a kept vertex has a kept face and the other way round: both are empty together, and empty tensors have no address)
        lib.call("cnr_mesh_compact", ptr(v), ptr(col), ptr(t), F, V, ptr(vertex_map), ptr(face_map), ptr(out_v), ptr(out_c), ptr(out_t),
                 stream_of(dev))
    info = {"n_components": s[0], "n_components_with_faces": s[1], "largest_label": s[2], "largest_face_count": s[3], "dropped": s[4],
            "n_vertices": nv, "n_faces": nf, "labels": labels, "face_count": face_count, "vertex_count": vertex_count,
            "keep_vertex": keep_vertex.bool(), "keep_face": keep_face.bool(), "vertex_map": vertex_map, "face_map": face_map}
    return out_v, out_t, out_c, info


def _area_cdf(v, t, lib):
    """v: contiguous float32 (V, 3), t: contiguous int32 (F, 3), F > 0 -> (cdf uint64-as-int64 [F], summary int64 [4]), device tensors."""
    cdf = torch.empty(t.shape[0], dtype=torch.int64, device=v.device)       # (the library's uint64 prefix sums: below 2^63, so int64 reads them)
    summary = torch.empty(4, dtype=torch.int64, device=v.device)
    lib.call("cnr_mesh_area_cdf", ptr(v), v.shape[0], ptr(t), t.shape[0], ptr(cdf), ptr(summary), stream_of(v.device))
    return cdf, summary


def _sample(v, t, cdf, n, seed, lib):
    """n samples of the mesh (v, t) with the prefix sums cdf -> (points float32 [n, 3], faces int32 [n], bary float32 [n, 2])."""
    dev = v.device
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 2, dtype=torch.float32, device=dev)
    if n > 0:
        lib.call("cnr_mesh_sample", ptr(v), v.shape[0], ptr(t), t.shape[0], ptr(cdf), n, seed, ptr(points), ptr(faces), ptr(bary), stream_of(dev))
    return points, faces, bary


def sample_surface(vertices, triangles, n_samples, seed=0, colors=None, library=None):
    """``n_samples`` points drawn uniformly by area on the mesh (``cnr_mesh_area_cdf`` + ``cnr_mesh_sample``): ``(points, faces, bary)``, device
    tensors float32 [n, 3], int64 [n] (the face each point lies on) and float32 [n, 3] (the barycentric weights of the face's three corners, in
    [0, 1], the first one ``1 - u - v``); with ``colors`` [V, 3] a fourth result, the colours interpolated with those weights (float32 [n, 3]).

    The draw is counter based (Philox under ``seed``, a 64-bit integer): the same seed gives the same bits on every run and build, and the
    first k samples of a longer draw are the k samples of a shorter one.  Faces are weighted by integer weights of 32 bits relative to the largest
    face: a face below 2^-32 of the largest area, a face with an index outside ``[0, V)`` and one with a non-finite area are never drawn.  A
    mesh on which nothing can be drawn (no faces, or no face of positive weight) raises ValueError; reading that total is the call's one host
    synchronisation.  Not differentiable."""
    n, seed = int(n_samples), int(seed)
    if n < 0:
        raise ValueError(f"sample_surface: n_samples must not be negative (got {n})")
    if not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError(f"sample_surface: seed must fit 64 bits (got {seed})")
    seed = seed - 2 ** 64 if seed >= 2 ** 63 else seed
    dev = vertices.device if torch.is_tensor(vertices) else (triangles.device if torch.is_tensor(triangles) else torch.device("cpu"))
    lib = _lib.library_for(library, dev, ("a mesh", "sampled"))
    v = points3(vertices, "vertices", dev)
    t = _triangles(triangles, dev)
    col = points3(colors, "colors", dev, v.shape[0]) if colors is not None else None
    if t.shape[0] == 0:
        raise ValueError("sample_surface: the mesh has no faces")
    cdf, summary = _area_cdf(v, t, lib)
    total, zero, invalid, _ = summary.tolist()
    if total <= 0:
        raise ValueError(f"sample_surface: no face can be drawn ({t.shape[0]} faces, {zero} of weight 0, {invalid} of them invalid)")
    points, faces, uv = _sample(v, t, cdf, n, seed, lib)
    faces = faces.to(torch.int64)
    bary = torch.cat([(1.0 - uv[:, :1]) - uv[:, 1:], uv], dim=1)      # exact: u, v and u + v are multiples of 2^-24 in [0, 1]
    if col is None:
        return points, faces, bary
    corners = col[t.to(torch.int64)[faces]]                            # [n, 3 corners, 3 channels]
    return points, faces, bary, (corners * bary[:, :, None]).sum(dim=1)
