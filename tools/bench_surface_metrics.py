"""Surface-metric benchmark: cnr_mesh_area_cdf, cnr_mesh_sample and cnr_point_mesh_distance on the iso-surface of the 512-cell synthetic lattice
of tools/bench_mesh_clean.py (two overlapping spheres and debris, about 1.07 M triangles), with cnr_nn_search at the same size beside them.

python tools/bench_surface_metrics.py [--res 512] [--samples 1048576] [--reps 3] [--out profiles/surface_metrics_bench.txt]

Timed: the launches of cnr_mesh_area_cdf and of cnr_mesh_sample for --samples samples; cnr_point_mesh_distance for the --samples samples of the mesh,
moved off the surface by seeded normal noise (sigma 0.01), against the mesh; cnr_nn_search for the same queries against --samples other samples
of the mesh.  Device events around every call after one warm-up call of each, the two searches alternating; median, min and max over the repeats;
the launches of one more call from the library's timing records.

There is no earlier implementation of the distance, so its yardstick is the sibling kernel: the time per pair, the ratio to cnr_nn_search's time per
pair, the ratio of the fp32 operations per pair (56 against 8: ap 3, d1 d2 10, d3..d6 4, va vb vc 9, e43 e56 2, the four candidate denominators 5, the
division 1, v w 2, the point 12, the distance 8; compares and selects are not counted on either side), and the share of the fp32 vector peak the
time corresponds to (157.3 TFLOP/s, which counts a fused multiply-add as two operations: a kernel that may not fuse cannot pass 50 %).  Needs a GPU:
there is no fallback."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402
from color_neus_amd._lib import ptr, stream_of  # noqa: E402
from bench_mesh_clean import lattice, BOUND  # noqa: E402

FP32_VECTOR_PEAK = 157.3e12
OPS_DIST, OPS_NN = 56, 8


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--debris", type=int, default=200)
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_metrics_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_surface_metrics.py needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    r = cn.NeuSRenderer(cn.RenderConfig(type="NeuS"), library=lib)
    u = lattice(a.res, a.debris, dev)
    verts, tris = r.marching_cubes(u, [-BOUND] * 3, [BOUND] * 3, 0.0)
    del u
    verts, tris = verts.contiguous(), tris.contiguous()
    V, F, n = verts.shape[0], tris.shape[0], a.samples
    s = stream_of(dev)
    cdf, summary = torch.empty(F, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
    points, faces, bary = torch.empty(n, 3, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, 2, device=dev)
    dist2, face, idx = torch.empty(n, device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    nn_bytes = lib.lib.cnr_nn_scratch_bytes(n, n)
    keys = torch.empty(max(nn_bytes, 8 * n), dtype=torch.uint8, device=dev)       # both searches' candidate keys

    def area_cdf():
        lib.call("cnr_mesh_area_cdf", ptr(verts), V, ptr(tris), F, ptr(cdf), ptr(summary), s)

    def sample(seed=0):
        lib.call("cnr_mesh_sample", ptr(verts), V, ptr(tris), F, ptr(cdf), n, seed, ptr(points), ptr(faces), ptr(bary), s)

    area_cdf()
    sample(1)
    targets = points.clone()
    sample(0)
    query = (points + 0.01 * torch.randn(n, 3, device=dev, generator=torch.Generator(device=dev).manual_seed(0))).contiguous()
    total, zero, invalid, _ = summary.tolist()

    def distance():
        lib.call("cnr_point_mesh_distance", ptr(query), n, ptr(verts), V, ptr(tris), F, ptr(dist2), ptr(face), None, ptr(keys), s)

    def nn():
        lib.call("cnr_nn_search", ptr(query), n, ptr(targets), n, ptr(dist2), ptr(idx), ptr(keys), nn_bytes, s)

    sides = {"cnr_mesh_area_cdf": area_cdf, "cnr_mesh_sample": sample, "cnr_point_mesh_distance": distance, "cnr_nn_search": nn}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, fn in sides.items():
            ms[k].append(timed(fn))
    lib.timing_enable(True)
    for fn in sides.values():
        fn()
    launches = lib.timing_collect()
    lib.timing_enable(False)
    on_surface = float(dist2.double().sqrt().mean())      # (dist2 holds the last nn run: queries to samples)
    distance()
    to_surface = float(dist2.double().sqrt().mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    pairs_d, pairs_n = float(n) * float(F), float(n) * float(n)
    per_d, per_n = med["cnr_point_mesh_distance"] * 1e-3 / pairs_d, med["cnr_nn_search"] * 1e-3 / pairs_n
    lines = [f"device {torch.cuda.get_device_name(0)}, library {lib.backend}, lattice {a.res}: V {V}, F {F}; {n} samples / queries, {a.reps} alternating "
             f"repeats after one warm-up call of each",
             f"weights: total {total}, {zero} faces of weight 0, {invalid} of them invalid"]
    for k in sides:
        lines.append(f"{k}: median {med[k]:.3f} ms (min {min(ms[k]):.3f}, max {max(ms[k]):.3f})")
    lines.append("launches of one more call of each: " + ", ".join(f"{x[0]} {x[7]:.3f} ms" for x in launches))
    lines.append(f"cnr_point_mesh_distance: {n} x {F} pairs, {per_d * 1e12:.4f} ps per pair = {1.0 / per_d:.3e} pairs/s; {OPS_DIST} fp32 ops/pair = "
                 f"{OPS_DIST / per_d / 1e12:.1f} TFLOP/s = {100.0 * OPS_DIST / per_d / FP32_VECTOR_PEAK:.1f} % of the fp32 vector peak")
    lines.append(f"cnr_nn_search: {n} x {n} pairs, {per_n * 1e12:.4f} ps per pair = {1.0 / per_n:.3e} pairs/s; {OPS_NN} fp32 ops/pair = "
                 f"{OPS_NN / per_n / 1e12:.1f} TFLOP/s = {100.0 * OPS_NN / per_n / FP32_VECTOR_PEAK:.1f} % of the fp32 vector peak")
    lines.append(f"time per pair, distance / nn: {per_d / per_n:.2f}; fp32 operations per pair, distance / nn: {OPS_DIST / OPS_NN:.2f}")
    lines.append(f"mean distance of the queries: to the surface {to_surface:.6f}, to the nearest of {n} surface samples {on_surface:.6f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
