"""Registration benchmark: cnr_icp against a cloud and against a mesh, with a torch composition of the same loop beside it.

python tools/bench_registration.py [--res 512] [--samples 20000] [--cloud 1048576] [--iterations 50] [--reps 5] [--out profiles/registration_bench.txt]

The mesh is the iso-surface of the 512-cell synthetic lattice of tools/bench_mesh_clean.py (two overlapping spheres and debris, about 1.07 M
triangles); the cloud target is --cloud area-uniform samples of it; the source is --samples other samples taken through the inverse of a
5 degree / 1.02 / (0.01, -0.02, 0.015) similarity, so that the loop has something to do.  Timed, after one warm-up call of each:

  one iteration     cnr_icp(iterations=1) per target kind, --reps repeats: the launches from the library's timing records (median and range per
                    kernel), the share of the existing search in the iteration, the new kernels as the remainder
  a registration    cnr_icp(iterations=--iterations) in ONE call, no host synchronisation inside: device events around it, median and range
  torch             the same loop in torch on the same GPU against the cloud: fp32 map, chunked cdist / argmin, float64 moments, torch.linalg.svd
                    with the determinant fix, and the `(idx != previous).any()` read a convergence test needs -- one host synchronisation
                    per iteration, against one per check_every iterations (or none) here

Needs a GPU unless an emulation --library is given (a dry run of the script at small sizes; its times mean nothing)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402
from color_neus_amd._lib import ptr, stream_of  # noqa: E402
from bench_mesh_clean import lattice, BOUND  # noqa: E402

SEARCH_KERNELS = ("nn_search_kernel", "nn_unpack_kernel", "surf_dist_kernel", "surf_finish_kernel")


def timed(fn, dev):
    if dev.type != "cuda":
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f})"


def torch_icp(src, tgt, iterations, with_scale, chunk):
    """the loop a user composes from torch: returns (4x4 float64, host synchronisations)"""
    dev = src.device
    A, t = torch.eye(3, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)
    a64 = src.double()
    prev, syncs = None, 0
    for _ in range(iterations):
        moved = src @ A.float().T + t.float()
        idx = torch.cat([torch.cdist(moved[i:i + chunk], tgt).argmin(1) for i in range(0, moved.shape[0], chunk)])
        if prev is not None:
            unchanged = not bool((idx != prev).any())          # the convergence test: a host read
            syncs += 1
            if unchanged:
                break
        prev = idx
        b64 = tgt[idx].double()
        ca, cb = a64.mean(0), b64.mean(0)
        da, db = a64 - ca, b64 - cb
        U, D, Vt = torch.linalg.svd(db.T @ da)
        fix = torch.ones(3, dtype=torch.float64, device=dev)
        fix[2] = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
        R = U @ torch.diag(fix) @ Vt
        s = (D * fix).sum() / (da * da).sum() if with_scale else torch.ones((), dtype=torch.float64, device=dev)
        A, t = s * R, cb - s * R @ ca
    M = torch.eye(4, dtype=torch.float64, device=dev)
    M[:3, :3], M[:3, 3] = A, t
    return M, syncs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--debris", type=int, default=200)
    ap.add_argument("--samples", type=int, default=20000)
    ap.add_argument("--cloud", type=int, default=1 << 20)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-chunk", type=int, default=512)
    ap.add_argument("--library", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "registration_bench.txt"))
    a = ap.parse_args()
    lib = cn.load_library(a.library)
    on_gpu = lib.backend.startswith("hip")
    if on_gpu and not torch.cuda.is_available():
        sys.exit("bench_registration.py needs a GPU (no fallback)")
    dev = torch.device("cuda:0" if on_gpu else "cpu")
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    r = cn.NeuSRenderer(cn.RenderConfig(type="NeuS"), library=lib)
    u = lattice(a.res, a.debris, dev)
    verts, tris = r.marching_cubes(u, [-BOUND] * 3, [BOUND] * 3, 0.0)
    del u
    verts, tris = verts.contiguous(), tris.contiguous()
    V, F, n = verts.shape[0], tris.shape[0], a.samples
    cloud = cn.sample_surface(verts, tris, a.cloud, seed=1, library=lib)[0].contiguous()
    true = torch.eye(4, dtype=torch.float64)
    ang = torch.tensor(5.0).deg2rad().double()
    true[:3, :3] = 1.02 * torch.tensor([[torch.cos(ang), -torch.sin(ang), 0], [torch.sin(ang), torch.cos(ang), 0], [0, 0, 1]], dtype=torch.float64)
    true[:3, 3] = torch.tensor([0.01, -0.02, 0.015], dtype=torch.float64)
    src = cn.apply_transform(cn.sample_surface(verts, tris, n, seed=0, library=lib)[0], torch.linalg.inv(true)).contiguous()
    s = stream_of(dev)
    chunks = (n + 255) // 256
    buf = dict(T=torch.empty(16, dtype=torch.float64, device=dev), hist=torch.empty(max(a.iterations, 1), 4, dtype=torch.float64, device=dev),
               moved=torch.empty(n, 3, device=dev), matched=torch.empty(n, 3, device=dev), d2=torch.empty(n, device=dev),
               idx=torch.empty(n, dtype=torch.int32, device=dev), keys=torch.empty(n, dtype=torch.int64, device=dev),
               part=torch.empty(chunks, 18, dtype=torch.float64, device=dev))
    identity = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=dev)
    targets = {"cloud": (cloud, None), "mesh": (verts, tris)}
    pivots = {k: torch.cat([src.double().mean(0), t[0].double().mean(0)]).cpu().contiguous() for k, t in targets.items()}

    def icp(kind, iterations):
        tgt, tri = targets[kind]
        buf["T"].copy_(identity)
        lib.call("cnr_icp", ptr(src), n, ptr(tgt), tgt.shape[0], ptr(tri), 0 if tri is None else tri.shape[0], ptr(pivots[kind]), 1, float("inf"),
                 iterations, 0, ptr(buf["T"]), ptr(buf["hist"]), ptr(buf["moved"]), ptr(buf["matched"]), ptr(buf["d2"]), ptr(buf["idx"]),
                 ptr(buf["keys"]), ptr(buf["part"]), s)

    lines = [f"device {torch.cuda.get_device_name(0) if on_gpu else 'cpu'}, library {lib.backend}, lattice {a.res}: V {V}, F {F}; {n} source samples, "
             f"cloud target {a.cloud} points; {a.reps} repeats after one warm-up call of each; with scale, no gate, from the identity"]
    for kind in targets:
        icp(kind, 1)
        sync()
        per = {}
        for _ in range(a.reps):
            lib.timing_enable(True)
            lib.timing_collect()
            icp(kind, 1)
            recs = lib.timing_collect()
            lib.timing_enable(False)
            for x in recs:
                per.setdefault(x[0], []).append(x[7])
        total = sum(statistics.median(v) for v in per.values()) or float("nan")      # (the emulation keeps no launch records)
        search = sum(statistics.median(v) for k, v in per.items() if k in SEARCH_KERNELS)
        lines.append(f"{kind}: one iteration, launches: " + "; ".join(f"{k} {spread(v)}" for k, v in per.items()))
        lines.append(f"{kind}: one iteration {total:.3f} ms of launches, the existing search {search:.3f} ms = {100.0 * search / total:.1f} %, "
                     f"move + moments + solve {total - search:.3f} ms = {100.0 * (total - search) / total:.1f} %")
        icp(kind, a.iterations)
        sync()
        ms = [timed(lambda: icp(kind, a.iterations), dev) for _ in range(a.reps)]
        sync()
        hist = buf["hist"][:a.iterations].cpu()
        M = torch.eye(4, dtype=torch.float64)
        T = buf["T"].cpu()
        M[:3, :3], M[:3, 3] = T[12] * T[:9].reshape(3, 3), T[9:12]
        stop = ((hist[:, 1] == 0) | (hist[:, 3] != 0)).nonzero()
        lines.append(f"{kind}: {a.iterations} iterations in one call (0 host synchronisations), {spread(ms)} = {statistics.median(ms) / a.iterations:.3f} ms "
                     f"per iteration; rms {float((hist[0, 2] / hist[0, 0]).sqrt()):.3e} -> {float((hist[-1, 2] / hist[-1, 0]).sqrt()):.3e}, "
                     f"changed correspondences {int(hist[1, 1]) if a.iterations > 1 else n} -> {int(hist[-1, 1])}, first stopping row "
                     f"{int(stop[0, 0]) if stop.numel() else None}, |M - true| {float((M - true).abs().max()):.2e}")
    # the torch composition, against the cloud
    M_t, syncs = torch_icp(src, cloud, 2, True, a.torch_chunk)
    sync()
    ms_t, done = [], 0
    for _ in range(a.reps):
        t0 = time.perf_counter()
        M_t, syncs = torch_icp(src, cloud, a.iterations, True, a.torch_chunk)
        sync()
        ms_t.append((time.perf_counter() - t0) * 1e3)
        done = syncs + 1
    lines.append(f"torch composition against the cloud (cdist in chunks of {a.torch_chunk} queries, argmin, float64 moments, torch.linalg.svd): "
                 f"{done} iterations, {spread(ms_t)} wall = {statistics.median(ms_t) / done:.3f} ms per iteration, {syncs} host synchronisations "
                 f"(1 per iteration; cnr_icp: 0 in a call, registration.icp 1 per check_every iterations), |M - true| {float((M_t.cpu() - true).abs().max()):.2e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
