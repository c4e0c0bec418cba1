"""Mesh culling benchmark: cnr_mask_dilate / cnr_mesh_view_votes / cnr_mesh_cull_select and meshops.cull_mesh on the iso-surface of a 512-cell
lattice (tools/bench_mesh_clean.py's: two overlapping spheres and seeded debris) against 64 views of 1200 x 1600 and their mask stack.
Prints one JSON line.

python tools/bench_mesh_cull.py [--res 512] [--views 64] [--height 1200] [--width 1600] [--radius 12] [--reps 7] [--out profiles/mesh_cull_bench.txt]

The cameras sit on a seeded sphere of radius 3 around the origin and look at it; the masks are discs (the silhouette of a ball slightly smaller
than the scene, so that the hull really cuts).  Reported: the device time of every launch of the three entries from the library's timing
records (events around each launch; median, min and max over the repeats after one warm-up call) with the algorithmic bytes each record
carries and the rate they give; each entry by device events around a window of calls; meshops.cull_mesh with and without visibility as a
caller sees it (host clock around a call that ends in a synchronise: its one host read and its allocations included; the masks are
prepared once, as a MeshCuller keeps them); and the composition a user would write today on the same device with torch alone --
F.max_pool2d for the dilation, a matmul projection per view, a gather of the mask, boolean indexing and a cumsum for the re-indexing --
whose kept faces must equal the library's.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import color_neus_amd as cn  # noqa: E402
from color_neus_amd import meshops  # noqa: E402
from color_neus_amd._lib import ptr, stream_of  # noqa: E402
from bench_mesh_clean import BOUND, lattice  # noqa: E402


def look_at(eye):
    eye = np.asarray(eye, float)
    fwd = -eye / np.linalg.norm(eye)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, np.cross(fwd, right), fwd, eye
    return c2w.astype(np.float32)


def torch_dilate(masks, r, chunk=8):
    """the dilation a user writes today: max_pool2d with a (2 r + 1)^2 window, stride 1, padding r, a few images at a time"""
    out = torch.empty(masks.shape, dtype=torch.bool, device=masks.device)
    for n0 in range(0, masks.shape[0], chunk):
        out[n0:n0 + chunk] = F.max_pool2d((masks[n0:n0 + chunk] > 0).float()[:, None], 2 * r + 1, 1, r)[:, 0] > 0
    return out


def torch_hull(verts, tris, c2w, focal, H, W, dil):
    """project every vertex into every view, look its nearest pixel up in the dilated masks, keep the faces whose corners are seen at least
    once and outside no mask, and re-index: (vertices', triangles', keep_face)"""
    seen = torch.zeros(verts.shape[0], dtype=torch.int32, device=verts.device)
    inside = torch.zeros_like(seen)
    for n in range(c2w.shape[0]):
        pc = (verts - c2w[n, :3, 3]) @ c2w[n, :3, :3]
        z = pc[:, 2]
        i = torch.floor(focal[0] * pc[:, 0] / z + W * 0.5 + 0.5).long()
        j = torch.floor(focal[1] * pc[:, 1] / z + H * 0.5 + 0.5).long()
        s = (z > 1e-3) & (i >= 0) & (i < W) & (j >= 0) & (j < H)
        seen += s
        inside += s & dil[n, j.clamp(0, H - 1), i.clamp(0, W - 1)]
    passes = (seen >= 1) & (seen == inside)
    keep_face = passes[tris.long()].all(1)
    kept = tris[keep_face].long()
    keep_vertex = torch.zeros(verts.shape[0], dtype=torch.bool, device=verts.device)
    keep_vertex[kept.reshape(-1)] = True
    vertex_map = torch.cumsum(keep_vertex, 0) - 1
    return verts[keep_vertex], vertex_map[kept].int(), keep_face


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--debris", type=int, default=200)
    ap.add_argument("--views", type=int, default=64)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--radius", type=int, default=12)
    ap.add_argument("--depth-tol", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--library", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_cull_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_cull.py needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library(a.library)
    r = cn.NeuSRenderer(cn.RenderConfig(type="NeuS"), library=lib)
    u = lattice(a.res, a.debris, dev)
    verts, tris = r.marching_cubes(u, [-BOUND] * 3, [BOUND] * 3, 0.0)
    del u
    verts, tris = verts.contiguous(), tris.contiguous()
    V, Fn, N, H, W = verts.shape[0], tris.shape[0], a.views, a.height, a.width
    g = np.random.default_rng(0)
    eyes = g.normal(size=(N, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * 3.0
    c2w = torch.from_numpy(np.stack([look_at(e) for e in eyes])).to(dev)
    fpx = 0.55 * H                                             # the unit ball fills most of the image's height
    focal = torch.tensor([fpx, fpx], device=dev).expand(N, 2).contiguous()
    jj, ii = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    disc = (((ii - W / 2) ** 2 + (jj - H / 2) ** 2) < (fpx * 0.75 / 3.0) ** 2).float()      # a ball of radius 0.75 at distance 3
    masks = disc[None].repeat(N, 1, 1).contiguous()
    Wq = (W + 63) // 64
    row_bits, bits = (torch.empty(N, H, Wq, dtype=torch.int64, device=dev) for _ in range(2))
    counts = torch.zeros(V, 4, dtype=torch.int32, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
    keep_vertex, keep_face, vertex_map, face_map, totals, dropped = u8(V), u8(Fn), i32(V), i32(Fn), i32(2), i32(1)
    s = stream_of(dev)
    chunk = min(8, N)
    depth = torch.empty(chunk, H, W, device=dev)
    culler = meshops.MeshCuller(c2w, focal, H, W, masks=masks, dilation=a.radius, library=lib)
    depth_culler = meshops.MeshCuller(c2w, focal, H, W, masks=culler.masks, visibility=True, depth_tol=a.depth_tol, library=lib)
    for k in range(chunk):      # the depth maps of the first chunk, for the votes with both tests
        depth[k] = cn.rasterize_mesh(verts, tris, c2w[k], focal[k], H, W, library=lib)["depth"]

    def dilate():
        lib.call("cnr_mask_dilate", ptr(masks), N, H, W, a.radius, ptr(row_bits), ptr(bits), s)

    def votes():
        lib.call("cnr_mesh_view_votes", ptr(verts), V, ptr(c2w), ptr(focal), None, 1.0, 1e-3, 0, N, H, W, ptr(bits), None, 0.0, ptr(counts), s)

    def votes_depth():
        lib.call("cnr_mesh_view_votes", ptr(verts), V, ptr(c2w), ptr(focal), None, 1.0, 1e-3, 0, chunk, H, W, ptr(bits), ptr(depth), a.depth_tol,
                 ptr(counts), s)

    def select():
        lib.call("cnr_mesh_cull_select", ptr(tris), Fn, V, ptr(counts), 1, 0, 0, 0, ptr(keep_vertex), ptr(keep_face), ptr(vertex_map), ptr(face_map),
                 ptr(totals), ptr(dropped), s)

    entries = (("cnr_mask_dilate", dilate), ("cnr_mesh_view_votes", votes), ("cnr_mesh_view_votes_chunk_depth", votes_depth),
               ("cnr_mesh_cull_select", select))
    dilate()
    assert torch.equal(bits, culler.masks.bits)
    counts.zero_()
    votes()
    select()
    torch.cuda.synchronize()
    nv, nf = totals.tolist()
    per_launch, launch_bytes = {}, {}
    for _ in range(a.reps):
        for name, fn in entries:
            counts.zero_()
            if name == "cnr_mesh_cull_select":
                votes()
            torch.cuda.synchronize()
            lib.timing_enable(True)
            fn()
            recs = lib.timing_collect()
            lib.timing_enable(False)
            for x in recs:
                key = x[0] if name != "cnr_mesh_view_votes_chunk_depth" else x[0] + "[%d views, depth]" % chunk
                per_launch.setdefault(key, []).append(x[7])
                launch_bytes[key] = x[8]
    windows = {}
    for name, fn in entries:
        inner = 3 if name == "cnr_mesh_view_votes" else 10
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / inner)
        windows[name] = ms
    wall = {}
    for name, fn in (("cull_mesh", culler), ("cull_mesh_visibility", depth_culler)):
        fn(verts, tris)      # warm-up
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(verts, tris)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        wall[name] = (ts, out)
    hull_v, hull_t, _, hull_info = wall["cull_mesh"][1]
    vis_info = wall["cull_mesh_visibility"][1][3]
    assert hull_info["n_faces"] == nf and hull_info["n_vertices"] == nv

    # the torch composition on the same device
    tw = {"torch_max_pool2d_dilate": [], "torch_project_gather_reindex": []}
    dil = torch_dilate(masks, a.radius)
    tv, tt, tkeep = torch_hull(verts, tris, c2w, focal[0], H, W, dil)      # warm-up
    for _ in range(max(3, a.reps // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dil = torch_dilate(masks, a.radius)
        torch.cuda.synchronize()
        tw["torch_max_pool2d_dilate"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        tv, tt, tkeep = torch_hull(verts, tris, c2w, focal[0], H, W, dil)
        torch.cuda.synchronize()
        tw["torch_project_gather_reindex"].append((time.perf_counter() - t0) * 1e3)
    same_masks = bool(torch.equal(dil, culler.masks.to_bool()))
    # (torch rounds the projection differently in the last bit: a vertex whose pixel coordinate sits on a rounding boundary may differ)
    face_diff = int((tkeep != hull_info["keep_face"]).sum())

    med = lambda v: round(statistics.median(v), 4)
    span = lambda v: [round(min(v), 4), round(max(v), 4)]
    out = {"bench": "mesh_cull", "device": torch.cuda.get_device_name(0), "library": os.path.basename(lib.path), "lattice": a.res, "V": V, "F": Fn,
           "views": N, "H": H, "W": W, "radius": a.radius, "depth_tol": a.depth_tol, "kept_V": nv, "kept_F": nf,
           "visibility_kept_V": vis_info["n_vertices"], "visibility_kept_F": vis_info["n_faces"],
           "launch_ms": {k: med(v) for k, v in per_launch.items()}, "launch_ms_min_max": {k: span(v) for k, v in per_launch.items()},
           "launch_algorithmic_MB": {k: round(v / 1e6, 3) for k, v in launch_bytes.items()},
           "launch_GBps": {k: round(launch_bytes[k] / 1e6 / statistics.median(v), 1) for k, v in per_launch.items() if statistics.median(v) > 0},
           "call_ms": {k: med(v) for k, v in windows.items()}, "call_ms_min_max": {k: span(v) for k, v in windows.items()},
           "wall_ms": {k: med(v[0]) for k, v in wall.items()}, "wall_ms_min_max": {k: span(v[0]) for k, v in wall.items()},
           "torch_wall_ms": {k: med(v) for k, v in tw.items()}, "torch_wall_ms_min_max": {k: span(v) for k, v in tw.items()},
           "torch_masks_equal": same_masks, "torch_keep_face_differences": face_diff, "reps": a.reps}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
