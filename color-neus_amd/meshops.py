"""Mesh clean-up on the device library: connected components of an indexed triangle mesh and removal of the small ones ("floaters").

The iso-surface of a NeuS-style SDF almost always carries small closed shells away from the object and fragments near the bounding box;
evaluation scripts remove them before scoring (``trimesh.split`` and "keep the largest" in the reference's environment).  Here that is
three entry points of the C ABI (include/colorneus_render.h, where the definitions are): ``cnr_mesh_components`` labels the components with a
lock-free union-find, ``cnr_mesh_select`` marks what to keep and scans the marks into index maps, ``cnr_mesh_compact`` writes the kept
vertices, colours and triangles in their original order.  Everything is integer work: the results are exact and the same bits on every run.
``sample_surface`` draws points uniformly by area on a mesh (``cnr_mesh_area_cdf``, ``cnr_mesh_sample``): the input of the surface metrics.
``dilate_masks`` / ``view_votes`` / ``cull_mesh`` / ``MeshCuller`` remove what the cameras never constrained (``cnr_mask_dilate``,
``cnr_mesh_view_votes``, ``cnr_mesh_cull_select``): the visual hull of the dilated masks and, optionally, a depth test against the mesh's own
z-buffers.

``triangles`` may be a tensor or a numpy array of any integer dtype and any strides, ``vertices`` / ``colors`` of any float dtype; they are
converted to contiguous int32 / float32 on the device of ``vertices`` (``connected_components``: of ``triangles``).  CUDA tensors go through
the HIP library; CPU tensors only with an explicitly passed emulation ``library=`` (there is no CPU fallback).  NOTHING HERE IS
DIFFERENTIABLE: inputs are detached and results carry no graph."""
import numpy as np
import torch

from . import _lib
from ._lib import points3, ptr, stream_of

__all__ = ["connected_components", "clean_mesh", "sample_surface", "ViewMasks", "dilate_masks", "view_votes", "cull_mesh", "MeshCuller"]

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


# ---- culling against the views ------------------------------------------------------------------------------------------------------------------
_FACE_RULES = {"all": 0, "any": 1}
_MAX_DILATION = 32767


def _tensor(x, name, dim):
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    if x.dim() != dim:
        raise ValueError(f"{name}: expected {dim} dimensions, got shape {tuple(x.shape)}")
    return x.detach()


class ViewMasks:
    """A mask stack packed one bit per pixel (``cnr_mask_dilate``'s output): ``bits`` int64 [N, H, Wq], ``Wq = ceil(W / 64)``; bit ``b`` of
    word ``k`` of a row is pixel ``64 k + b`` and the bits at columns ``>= W`` are zero.  ``radius`` is the dilation it was built with."""

    def __init__(self, bits, H, W, radius):
        self.bits, self.H, self.W, self.radius = bits, int(H), int(W), int(radius)

    def __len__(self):
        return self.bits.shape[0]

    def to_bool(self):
        """The stack as a bool tensor [N, H, W] (torch ops on the bits' device)."""
        shifts = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        b = (self.bits[..., None] >> shifts) & 1
        return b.reshape(self.bits.shape[0], self.H, -1)[:, :, :self.W] != 0


def dilate_masks(masks, radius, library=None):
    """Pack a mask stack ``masks`` [N, H, W] (bool, integer or float; foreground is ``> 0``, NaN is background) to one bit per pixel and
    dilate every image with a ``(2 radius + 1)^2`` box of ones (``cnr_mask_dilate``; ``cv2.dilate`` with that kernel, pixels outside the
    image being background).  ``radius == 0`` packs only.  Returns a ``ViewMasks``.  A float32 stack -- the ``PixelSampler``'s resident
    one -- is read as it is.  CUDA tensors use the HIP library; CPU tensors need an explicit emulation ``library=``.  Not differentiable."""
    m = _tensor(masks, "masks", 3)
    if m.is_complex():
        raise ValueError(f"masks: expected a bool, integer or float dtype, got {m.dtype}")
    radius = int(radius)
    if radius < 0 or radius > _MAX_DILATION:
        raise ValueError(f"dilate_masks: the dilation radius must lie in [0, {_MAX_DILATION}] (got {radius})")
    N, H, W = m.shape
    if H < 1 or W < 1:
        raise ValueError(f"masks: H and W must be at least 1 (got {H} x {W})")
    lib = _lib.library_for(library, m.device, ("masks", "dilated"))
    m = m.contiguous() if m.dtype == torch.float32 else (m > 0).to(torch.float32).contiguous()
    Wq = (W + 63) // 64
    bits = torch.empty(N, H, Wq, dtype=torch.int64, device=m.device)
    if N > 0:
        row_bits = torch.empty_like(bits)
        lib.call("cnr_mask_dilate", ptr(m), N, H, W, radius, ptr(row_bits), ptr(bits), stream_of(m.device))
    return ViewMasks(bits, H, W, radius)


def _cameras(c2w, focal, dev):
    """c2w [N, 4, 4] and focal ([2], broadcast, or [N, 2]) as contiguous float32 tensors on ``dev``."""
    cam = _tensor(c2w, "c2w", 3)
    if tuple(cam.shape[1:]) != (4, 4) or not cam.is_floating_point():
        raise ValueError(f"c2w: expected a floating-point (N, 4, 4) tensor, got {tuple(cam.shape)} {cam.dtype}")
    cam = cam.to(device=dev, dtype=torch.float32).contiguous()
    foc = focal if torch.is_tensor(focal) else torch.as_tensor(np.asarray(focal))
    foc = foc.detach().to(device=dev, dtype=torch.float32)
    if tuple(foc.shape) == (2,):
        foc = foc.expand(cam.shape[0], 2)
    if tuple(foc.shape) != (cam.shape[0], 2):
        raise ValueError(f"focal: expected shape (2,) or ({cam.shape[0]}, 2), got {tuple(foc.shape)}")
    return cam, foc.contiguous()


def _origin(origin, radius, dev, who):
    if origin is None:
        if float(radius) != 1.0:
            raise ValueError(f"{who}: radius without origin (pass origin=[0, 0, 0] to scale only)")
        return None
    org = _tensor(origin, "origin", 1).to(device=dev, dtype=torch.float32).contiguous()
    if org.shape[0] != 3:
        raise ValueError(f"origin: expected 3 values, got {org.shape[0]}")
    return org


def _votes(lib, v, cam, foc, org, radius, z_near, opengl, H, W, bits, depth, depth_tol, counts):
    """one cnr_mesh_view_votes call on prepared tensors (bits: int64 [n, H, Wq] or None; depth: float32 [n, H, W] or None)"""
    if v.shape[0] and cam.shape[0]:
        lib.call("cnr_mesh_view_votes", ptr(v), v.shape[0], ptr(cam), ptr(foc), ptr(org), float(radius), float(z_near), int(bool(opengl)),
                 cam.shape[0], H, W, ptr(bits), ptr(depth), float(depth_tol), ptr(counts), stream_of(v.device))


def view_votes(vertices, c2w, focal, H, W, masks=None, depth=None, depth_tol=None, opengl=False, origin=None, radius=1.0, z_near=1e-3,
               counts=None, library=None):
    """Per-vertex counts over the views (``cnr_mesh_view_votes``): int32 [V, 4] = (views, views that SEE the vertex -- it projects in front
    of the camera and inside the image --, of those the views whose mask holds its pixel, of those the views whose depth map does not hide
    it).  The camera model and the projection are ``rasterize_mesh``'s; the pixel is the nearest pixel centre.

    ``c2w`` [N, 4, 4]; ``focal`` [2] (all views) or [N, 2]; ``masks``: a ``ViewMasks`` of N images of H x W, or None (column 2 = column 1);
    ``depth``: float [N, H, W] camera depths with NaN where nothing is covered (``rasterize_mesh``'s), or None (column 3 = column 1) -- it
    requires ``depth_tol``: a vertex is hidden when its depth exceeds the map's by more than the factor ``1 + depth_tol``; a NaN pixel hides
    nothing.  ``counts``: an int32 [V, 4] tensor to ADD to (views in chunks); None starts from zero.  Not differentiable."""
    dev = vertices.device if torch.is_tensor(vertices) else (c2w.device if torch.is_tensor(c2w) else torch.device("cpu"))
    lib = _lib.library_for(library, dev, ("a mesh", "voted on"))
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"view_votes: H and W must be at least 1 (got {H} x {W})")
    v = points3(vertices, "vertices", dev)
    cam, foc = _cameras(c2w, focal, dev)
    org = _origin(origin, radius, dev, "view_votes")
    bits = _mask_bits(masks, cam.shape[0], H, W, dev)
    if depth is not None:
        if depth_tol is None:
            raise ValueError("view_votes: depth requires depth_tol (the relative depth excess that still counts as visible)")
        depth = _tensor(depth, "depth", 3)
        if tuple(depth.shape) != (cam.shape[0], H, W):
            raise ValueError(f"depth: expected shape ({cam.shape[0]}, {H}, {W}), got {tuple(depth.shape)}")
        depth = depth.to(device=dev, dtype=torch.float32).contiguous()
    if counts is None:
        counts = torch.zeros(v.shape[0], 4, dtype=torch.int32, device=dev)
    elif not (torch.is_tensor(counts) and counts.dtype == torch.int32 and tuple(counts.shape) == (v.shape[0], 4) and counts.is_contiguous()
              and counts.device == v.device):
        raise ValueError(f"counts: expected a contiguous int32 ({v.shape[0]}, 4) tensor on {v.device}")
    _votes(lib, v, cam, foc, org, radius, z_near, opengl, H, W, bits, depth, 0.0 if depth_tol is None else depth_tol, counts)
    return counts


def _mask_bits(masks, n, H, W, dev):
    if masks is None:
        return None
    if not isinstance(masks, ViewMasks):
        raise ValueError("masks: expected a ViewMasks (dilate_masks packs a raw stack)")
    if (len(masks), masks.H, masks.W) != (n, H, W):
        raise ValueError(f"masks: expected {n} images of {H} x {W}, got {len(masks)} of {masks.H} x {masks.W}")
    if masks.bits.device != dev:
        raise ValueError(f"masks: packed on {masks.bits.device}, the mesh is on {dev}")
    return masks.bits


class MeshCuller:
    """``cull_mesh`` with its views prepared once: the cameras on the device and the packed, dilated masks stay resident between meshes.
    ``MeshCuller(c2w, focal, H, W, masks=None, **cull_mesh's keywords)``; ``culler(vertices, triangles, colors=None)`` returns what
    ``cull_mesh`` returns.  ``NeuSRenderer.extract_geometry`` / ``render_mesh_view`` take one as ``cull=``."""

    def __init__(self, c2w, focal, H, W, masks=None, dilation=0, min_views=1, max_outside=0, visibility=False, depth_tol=None, min_visible=1,
                 faces="all", view_chunk=8, opengl=False, origin=None, radius=1.0, z_near=1e-3, library=None):
        if faces not in _FACE_RULES:
            raise ValueError(f"cull_mesh: faces must be 'all' or 'any', got {faces!r}")
        dilation = int(dilation)
        if dilation < 0 or dilation > _MAX_DILATION:
            raise ValueError(f"cull_mesh: dilation must lie in [0, {_MAX_DILATION}] (got {dilation})")
        if visibility and depth_tol is None:
            raise ValueError("cull_mesh: visibility=True requires depth_tol: there is no default, the right value is the pixel footprint over "
                             "the scene's depth times the surface slope it should forgive")
        self.min_views, self.max_outside, self.min_visible, self.view_chunk = int(min_views), int(max_outside), int(min_visible), int(view_chunk)
        if self.min_views < 0 or self.max_outside < 0 or self.min_visible < 0:
            raise ValueError(f"cull_mesh: min_views, max_outside and min_visible must not be negative (got {min_views}, {max_outside}, {min_visible})")
        if self.view_chunk < 1:
            raise ValueError(f"cull_mesh: view_chunk must be at least 1 (got {view_chunk})")
        self.H, self.W = int(H), int(W)
        if self.H < 1 or self.W < 1:
            raise ValueError(f"cull_mesh: H and W must be at least 1 (got {H} x {W})")
        if isinstance(masks, ViewMasks):
            dev = masks.bits.device
        elif torch.is_tensor(c2w):
            dev = c2w.device
        else:
            dev = masks.device if torch.is_tensor(masks) else torch.device("cpu")
        self.device, self.library = dev, library
        self.c2w, self.focal = _cameras(c2w, focal, dev)
        self.origin = _origin(origin, radius, dev, "cull_mesh")
        self.radius, self.z_near, self.opengl = float(radius), float(z_near), bool(opengl)
        self.visibility, self.depth_tol, self.faces = bool(visibility), (None if depth_tol is None else float(depth_tol)), faces
        if masks is not None and not isinstance(masks, ViewMasks):
            m = _tensor(masks, "masks", 3)
            masks = dilate_masks(m.to(dev), dilation, library=library)
        elif masks is not None and dilation != 0:
            raise ValueError("cull_mesh: dilation applies to a raw mask stack; a ViewMasks is used as it was built")
        self.masks = masks
        _mask_bits(masks, self.c2w.shape[0], self.H, self.W, dev)

    def _visible_votes(self, lib, v, t, counts):
        """the views ``view_chunk`` at a time: the chunk's depth maps (cnr_mesh_raster without colours, one scratch for all), then its votes"""
        dev, H, W, n, V, F = self.device, self.H, self.W, self.c2w.shape[0], v.shape[0], t.shape[0]
        chunk = min(self.view_chunk, n)
        depth = torch.empty(chunk, H, W, dtype=torch.float32, device=dev)
        tri_id = torch.empty(H, W, dtype=torch.int32, device=dev)
        raster_dropped = torch.empty(2, dtype=torch.int32, device=dev)
        scratch, nb = lib.scratch("cnr_mesh_raster_scratch_bytes", dev, V, F, H, W, at_least=1)
        bits = self.masks.bits if self.masks is not None else None
        for n0 in range(0, n, chunk):
            n1 = min(n0 + chunk, n)
            for k in range(n0, n1):
                lib.call("cnr_mesh_raster", ptr(v), V, ptr(t if F else None), F, None, ptr(self.c2w[k]), ptr(self.focal[k]), H, W, int(self.opengl),
                         ptr(self.origin), self.radius, self.z_near, None, None, ptr(depth[k - n0]), ptr(tri_id), ptr(raster_dropped), ptr(scratch),
                         nb, stream_of(dev))
            _votes(lib, v, self.c2w[n0:n1], self.focal[n0:n1], self.origin, self.radius, self.z_near, self.opengl, H, W,
                   bits[n0:n1] if bits is not None else None, depth[:n1 - n0], self.depth_tol, counts)

    def __call__(self, vertices, triangles, colors=None):
        dev = self.device
        lib = _lib.library_for(self.library, dev, ("a mesh", "culled"))
        v = points3(vertices, "vertices", dev)
        t = _triangles(triangles, dev)
        col = points3(colors, "colors", dev, v.shape[0]) if colors is not None else None
        V, F = v.shape[0], t.shape[0]
        counts = torch.zeros(V, 4, dtype=torch.int32, device=dev)
        if V > 0 and self.visibility:
            self._visible_votes(lib, v, t, counts)
        elif V > 0:
            _votes(lib, v, self.c2w, self.focal, self.origin, self.radius, self.z_near, self.opengl, self.H, self.W,
                   self.masks.bits if self.masks is not None else None, None, 0.0, counts)
        keep_vertex, keep_face = torch.empty(V, dtype=torch.uint8, device=dev), torch.empty(F, dtype=torch.uint8, device=dev)
        vertex_map, face_map = torch.empty(V, dtype=torch.int32, device=dev), torch.empty(F, dtype=torch.int32, device=dev)
        totals, dropped = torch.empty(2, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        # (without the depth test column 3 equals column 1: min_visible would only repeat min_views)
        lib.call("cnr_mesh_cull_select", ptr(t), F, V, ptr(counts), self.min_views, self.max_outside, self.min_visible if self.visibility else 0,
                 _FACE_RULES[self.faces], ptr(keep_vertex), ptr(keep_face), ptr(vertex_map), ptr(face_map), ptr(totals), ptr(dropped), stream_of(dev))
        nv, nf, n_dropped = torch.cat([totals, dropped]).tolist()      # the one host round trip: the caller owns the output buffers
        out_v = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        out_t = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        out_c = torch.empty(nv, 3, dtype=torch.float32, device=dev) if col is not None else None
        if nv > 0:      # (a kept vertex has a kept face and the other way round: both are empty together)
            lib.call("cnr_mesh_compact", ptr(v), ptr(col), ptr(t), F, V, ptr(vertex_map), ptr(face_map), ptr(out_v), ptr(out_c), ptr(out_t),
                     stream_of(dev))
        info = {"n_vertices": nv, "n_faces": nf, "dropped": n_dropped, "n_views": self.c2w.shape[0], "counts": counts,
                "keep_vertex": keep_vertex.bool(), "keep_face": keep_face.bool(), "vertex_map": vertex_map, "face_map": face_map}
        return out_v, out_t, out_c, info


def cull_mesh(vertices, triangles, c2w, focal, H, W, masks=None, colors=None, dilation=0, min_views=1, max_outside=0, visibility=False,
              depth_tol=None, min_visible=1, faces="all", view_chunk=8, opengl=False, origin=None, radius=1.0, z_near=1e-3, library=None):
    """Remove from a mesh what the views never constrained: ``(vertices', triangles', colors' or None, info)``, device tensors in the ORIGINAL
    order of the kept vertices and faces, the indices renumbered (``cnr_mesh_view_votes`` -> ``cnr_mesh_cull_select`` -> ``cnr_mesh_compact``).

    An SDF trained with masks is supervised only inside the union of the view cones through the masks; outside it the iso-surface grows
    sheets, caps and skirts that are attached to the object, so ``clean_mesh`` keeps them.  Per vertex, over the N views ``c2w`` [N, 4, 4] /
    ``focal`` ([2] or [N, 2]) of ``H`` x ``W`` pixels (``rasterize_mesh``'s camera model, ``opengl`` / ``origin`` / ``radius`` / ``z_near``
    included): ``seen`` = the views in which it projects inside the image, ``inside`` = of those the views whose mask holds its pixel,
    ``visible`` = of those the views whose z-buffer of THIS mesh does not hide it.  A vertex passes iff ``seen >= min_views`` and
    ``seen - inside <= max_outside`` (and, with ``visibility``, ``visible >= min_visible``); the defaults are the visual hull: seen at least
    once and outside no mask.  A face stays when all (``faces="all"``) or any (``"any"``) of its vertices pass; a vertex stays iff a face
    that stays names it.

    ``masks``: a raw stack [N, H, W] (foreground ``> 0``), packed and dilated here by ``dilation`` pixels (``dilate_masks``), a ready
    ``ViewMasks``, or None (image bounds only).  ``visibility=True`` rasterises the mesh into the views, ``view_chunk`` depth maps at a time
    (``cnr_mesh_raster`` without colours, one scratch), and votes each chunk against its maps; it REQUIRES ``depth_tol``: a vertex is hidden
    when its camera depth exceeds the map's by more than the factor ``1 + depth_tol``.  The project ships no default, because the right value
    is the pixel footprint over the scene's depth times the surface slope it should forgive: a vertex is tested against the depth at the
    nearest pixel CENTRE, up to half a pixel away, and on a surface seen at a grazing angle that half pixel is a real depth difference.

    ``info``: ``n_vertices`` / ``n_faces`` (of the result), ``dropped`` (faces with an index outside ``[0, V)``), ``n_views`` and the device
    tensors ``counts`` (int32 [V, 4] = views, seen, inside, visible), ``keep_vertex`` / ``keep_face`` (bool), ``vertex_map`` / ``face_map``
    (int32: the new index, -1 for what was removed).  One host read (the totals and ``dropped``) sizes the outputs, as in ``clean_mesh``.
    For several meshes against the same views build a ``MeshCuller`` once.  Not differentiable."""
    dev = vertices.device if torch.is_tensor(vertices) else (triangles.device if torch.is_tensor(triangles) else torch.device("cpu"))
    if isinstance(masks, ViewMasks):
        dev = masks.bits.device
    to_dev = lambda x: x.to(dev) if torch.is_tensor(x) else torch.as_tensor(np.asarray(x)).to(dev)
    culler = MeshCuller(to_dev(c2w), focal, H, W, masks=masks if masks is None or isinstance(masks, ViewMasks) else to_dev(masks),
                        dilation=dilation, min_views=min_views, max_outside=max_outside, visibility=visibility, depth_tol=depth_tol,
                        min_visible=min_visible, faces=faces, view_chunk=view_chunk, opengl=opengl, origin=origin, radius=radius, z_near=z_near,
                        library=library)
    return culler(vertices, triangles, colors)
