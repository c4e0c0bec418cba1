"""Mesh clean-up benchmark: cnr_mesh_components / cnr_mesh_select / cnr_mesh_compact on the iso-surface of a 512-cell lattice with two
large spheres that overlap (one component) and seeded debris: small closed shells away from them.  Prints one JSON line.

python tools/bench_mesh_clean.py [--res 512] [--debris 200] [--reps 9] [--library PATH] [--no-host] [--out profiles/mesh_clean_bench.txt]

The lattice is analytic (u = max over the spheres of r - |x - c|, written block by block on the device); the mesh is the library's marching
cubes of it.  Reported: V, F, the component count, what "largest" keeps; the device time of every launch of the three entries from the
library's timing records (events around each launch; median, min and max over the repeats after one warm-up call); each entry and the three
in a row by device events around windows of 20 calls; the time of meshops.clean_mesh as a caller sees it (with its one host read and its
allocations); and, unless --no-host, a sequential union-find over the same triangles in numpy / Python on the host, whose labels must equal
the device's.  --library times another build of the library (the A/B of the counting launch).  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402
from color_neus_amd import meshops  # noqa: E402
from color_neus_amd._lib import ptr, stream_of  # noqa: E402

INNER = 20
BOUND = 1.01


def lattice(res, n_debris, dev, seed=0):
    """u[x][y][z] on linspace(-BOUND, BOUND, res)^3: two spheres of radius 0.42 around (+-0.4, 0, 0) and n_debris shells of radius 3 .. 8 cells
    at least 0.12 outside them (and, by rejection, clear of each other)."""
    ax = torch.linspace(-BOUND, BOUND, res, device=dev)
    cell = 2.0 * BOUND / (res - 1)
    u = torch.empty(res, res, res, device=dev)
    big = [((-0.4, 0.0, 0.0), 0.42), ((0.4, 0.0, 0.0), 0.42)]
    for x0 in range(0, res, 64):      # slabs: no lattice-sized temporaries
        x, y, z = torch.meshgrid(ax[x0:x0 + 64], ax, ax, indexing="ij")
        u[x0:x0 + 64] = torch.maximum(*[r - torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) for c, r in big])
    g = np.random.default_rng(seed)
    placed = []
    while len(placed) < n_debris:
        c, r = g.uniform(-0.9, 0.9, 3), g.uniform(3.0, 8.0) * cell
        if any(np.linalg.norm(c - np.array(b)) < rb + r + 0.12 for b, rb in big):
            continue
        if any(np.linalg.norm(c - pc) < pr + r + 4 * cell for pc, pr in placed):
            continue
        placed.append((c, r))
        lo = [max(0, int((ci - r + BOUND) / cell) - 2) for ci in c]
        hi = [min(res, int((ci + r + BOUND) / cell) + 4) for ci in c]
        x, y, z = torch.meshgrid(ax[lo[0]:hi[0]], ax[lo[1]:hi[1]], ax[lo[2]:hi[2]], indexing="ij")
        blk = u[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        blk.copy_(torch.maximum(blk, float(r) - torch.sqrt((x - float(c[0])) ** 2 + (y - float(c[1])) ** 2 + (z - float(c[2])) ** 2)))
    return u


def host_union_find(tris, V):
    """sequential union-find with path halving and min-index roots over int32 [F][3] (all indices valid); returns labels"""
    parent = list(range(V))
    for a, b, c in tris.tolist():
        for x in (b, c):
            ra = a
            while parent[ra] != ra:
                parent[ra] = parent[parent[ra]]
                ra = parent[ra]
            rx = x
            while parent[rx] != rx:
                parent[rx] = parent[parent[rx]]
                rx = parent[rx]
            if ra != rx:
                if ra < rx:
                    parent[rx] = ra
                else:
                    parent[ra] = rx
    p = np.array(parent, np.int64)
    while True:
        q = p[p]
        if np.array_equal(q, p):
            return p.astype(np.int32)
        p = q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--debris", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--library", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_clean_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh_clean.py needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library(a.library)
    r = cn.NeuSRenderer(cn.RenderConfig(type="NeuS"), library=lib)
    u = lattice(a.res, a.debris, dev)
    verts, tris = r.marching_cubes(u, [-BOUND] * 3, [BOUND] * 3, 0.0)
    del u
    verts, tris = verts.contiguous(), tris.contiguous()
    V, F = verts.shape[0], tris.shape[0]
    colors = torch.rand(V, 3, device=dev)
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    u8 = lambda n: torch.empty(n, dtype=torch.uint8, device=dev)
    labels, face_count, vertex_count, summary, dropped = i32(V), i32(V), i32(V), i32(4), i32(1)
    keep_vertex, keep_face, vertex_map, face_map, totals = u8(V), u8(F), i32(V), i32(F), i32(2)
    s = stream_of(dev)

    def components():
        lib.call("cnr_mesh_components", ptr(tris), F, V, ptr(labels), ptr(face_count), ptr(vertex_count), ptr(summary), ptr(dropped), s)

    def select():
        lib.call("cnr_mesh_select", ptr(tris), F, V, ptr(labels), ptr(face_count), ptr(summary), 0, 0, 0.0, ptr(keep_vertex), ptr(keep_face),
                 ptr(vertex_map), ptr(face_map), ptr(totals), s)

    components()
    select()
    nv, nf = totals.tolist()
    out_v, out_c, out_t = torch.empty(nv, 3, device=dev), torch.empty(nv, 3, device=dev), torch.empty(nf, 3, dtype=torch.int32, device=dev)

    def compact():
        lib.call("cnr_mesh_compact", ptr(verts), ptr(colors), ptr(tris), F, V, ptr(vertex_map), ptr(face_map), ptr(out_v), ptr(out_c), ptr(out_t), s)

    def three():
        components()
        select()
        compact()

    three()      # warm-up
    torch.cuda.synchronize()
    summ = summary.tolist()
    per_launch, order = {}, []
    for _ in range(a.reps):
        lib.timing_enable(True)
        three()
        recs = lib.timing_collect()
        lib.timing_enable(False)
        order = [x[0] for x in recs]
        for x in recs:
            per_launch.setdefault(x[0], []).append(x[7])
    windows = {}
    for name, fn in (("cnr_mesh_components", components), ("cnr_mesh_select", select), ("cnr_mesh_compact", compact), ("three_entries", three)):
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / INNER)
        windows[name] = ms
    wall = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cv, ct, cc, info = meshops.clean_mesh(verts, tris, colors=colors, library=lib)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    assert torch.equal(cv, out_v) and torch.equal(ct, out_t) and torch.equal(cc, out_c) and info["n_faces"] == nf
    labels_first = labels.clone()
    components()
    assert torch.equal(labels, labels_first)
    med = lambda v: round(statistics.median(v), 4)
    out = {"bench": "mesh_clean", "device": torch.cuda.get_device_name(0), "library": os.path.basename(lib.path), "lattice": a.res, "debris": a.debris,
           "V": V, "F": F, "n_components": summ[0], "n_components_with_faces": summ[1], "largest_face_count": summ[3], "dropped": dropped.tolist()[0],
           "kept_V": nv, "kept_F": nf, "launch_order": order, "launch_ms": {k: med(v) for k, v in per_launch.items()},
           "launch_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in per_launch.items()},
           "launch_sum_ms": round(sum(statistics.median(v) for v in per_launch.values()), 4),
           "call_ms": {k: med(v) for k, v in windows.items()}, "call_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in windows.items()},
           "clean_mesh_wall_ms": med(wall), "clean_mesh_wall_ms_min_max": [round(min(wall), 4), round(max(wall), 4)], "reps": a.reps}
    if not a.no_host:
        th = tris.cpu().numpy()
        t0 = time.perf_counter()
        host_labels = host_union_find(th, V)
        out["host_union_find_s"] = round(time.perf_counter() - t0, 3)
        assert np.array_equal(host_labels, labels.cpu().numpy())
        out["host_labels_equal"] = True
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
