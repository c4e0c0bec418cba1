"""Mesh-rasteriser benchmark: cnr_mesh_raster on the mesh of a lattice extraction of the benchmark's synthetic scene (the trained-like sphere
of radius 0.5, tools/bench_eval.py), seen by the synthetic camera.  Prints one JSON line.

python tools/bench_raster.py [--res 512] [--height 1200] [--width 1600] [--focal 2200] [--reps 9] [--out profiles/mesh_raster_bench.txt]

The default focal length shows the sphere about 800 pixels across (the triangles of a 512-cell lattice then have boxes of 2-3 pixels).  Reported:
V, F, the share of triangles that took the large-triangle launch (the length of the list the small-triangle launch leaves in scratch), the
time of the small-triangle launch with the mesh beside the screen (gather, setup and clip only: what it lacks is the box walk and the atomics), the
device time of each of the four launches from the library's timing records (events around each launch; median over the repeats after one
warm-up call), the whole call by device events around windows of 200 calls, and the launches' sum against the streaming floor of the bytes the
call must move: 12 V read + 12 V written (projection), 12 F of indices + 36 F of gathered projected vertices, 8 HW of key initialisation +
8 HW of key reads + 20 HW of outputs, at the chip's 8 TB/s.  The projected vertices and the keys of one view fit in the 256 MB last-level
cache, so part of those bytes need not come from HBM: the floor is a yardstick for the launches' sum, not a bound on each launch.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import color_neus_amd as cn  # noqa: E402
from color_neus_amd import synthetic  # noqa: E402
from color_neus_amd._lib import ptr, stream_of  # noqa: E402

HBM_PEAK = 8.0e12
INNER = 200
LAUNCHES = ["raster_project_kernel", "raster_small_kernel", "raster_large_kernel", "raster_resolve_kernel"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--focal", type=float, default=2200.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_raster_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_raster.py needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    cfg = cn.RenderConfig(type="Color_NeuS", col_mode="no_view_dir", col_d_in=6, col_multires_view=0)
    torch.manual_seed(0)
    r = synthetic.make_trained_like_(cn.ColorNeuSRenderer(cfg)).to(dev)
    bmin, bmax = [-1.01] * 3, [1.01] * 3
    u = r.extract_fields(bmin, bmax, dev, a.res)
    verts, tris = r.marching_cubes(u, bmin, bmax, 0.0)
    del u
    colors = r.vertex_colors(verts)
    c2w, focal, _, _ = synthetic.synthetic_camera(8, 8, a.focal, device=dev)
    c2w = c2w[0].contiguous()
    H, W, V, F = a.height, a.width, verts.shape[0], tris.shape[0]
    rgb, depth = torch.empty(H, W, 3, device=dev), torch.empty(H, W, device=dev)
    tri_id, dropped = torch.empty(H, W, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    scratch, nb = lib.scratch("cnr_mesh_raster_scratch_bytes", dev, V, F, H, W)

    # the same camera turned 60 degrees about its y axis: every vertex stays in front of it and projects beside the screen
    turn = torch.tensor([[0.5, 0.0, 0.8660254], [0.0, 1.0, 0.0], [-0.8660254, 0.0, 0.5]], device=dev)
    c2w_away = c2w.clone()
    c2w_away[:3, :3] = c2w[:3, :3] @ turn

    def call(cam=c2w):
        lib.call("cnr_mesh_raster", ptr(verts), V, ptr(tris), F, ptr(colors), ptr(cam), ptr(focal), H, W, 0, None, 1.0, 1e-3, None, ptr(rgb),
                 ptr(depth), ptr(tri_id), ptr(dropped), ptr(scratch), nb, stream_of(dev))

    call()      # warm-up
    torch.cuda.synchronize()
    n_large = int(scratch[nb - 256:nb - 252].view(torch.int32).item())      # the layout's last part: the length of the large-triangle list
    covered = float((tri_id >= 0).float().mean())
    n_dropped = dropped.tolist()
    per_launch = {k: [] for k in LAUNCHES}
    whole = []
    for _ in range(a.reps):
        lib.timing_enable(True)
        call()
        recs = lib.timing_collect()
        lib.timing_enable(False)
        assert [x[0] for x in recs] == LAUNCHES, recs
        for x in recs:
            per_launch[x[0]].append(x[7])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            call()
        e1.record()
        e1.synchronize()
        whole.append(e0.elapsed_time(e1) / INNER)
    # the small-triangle launch with the whole mesh beside the screen: index reads, the gather, the setup and the box clip alone, no box walk
    # and no atomic -- the difference to the launch above is the walk and the 64-bit atomic min
    away = []
    for _ in range(a.reps):
        lib.timing_enable(True)
        call(c2w_away)
        away.append(dict((x[0], x[7]) for x in lib.timing_collect())["raster_small_kernel"])
        lib.timing_enable(False)
    torch.cuda.synchronize()
    assert not bool((tri_id >= 0).any()) and dropped.tolist() == [0, 0]
    call()
    torch.cuda.synchronize()
    again = tri_id.clone()
    call()
    torch.cuda.synchronize()
    assert torch.equal(again, tri_id)
    hw = H * W
    floor_bytes = 24.0 * V + 48.0 * F + 36.0 * hw
    med = {k: statistics.median(v) for k, v in per_launch.items()}
    total = sum(med.values())
    out = {"bench": "mesh_raster", "device": torch.cuda.get_device_name(0), "lattice": a.res, "H": H, "W": W, "focal": a.focal, "V": V, "F": F,
           "large_share": n_large / max(F, 1), "n_large": n_large, "covered_share": round(covered, 4), "dropped": n_dropped,
           "launch_ms": {k: round(v, 4) for k, v in med.items()},
           "launch_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in per_launch.items()},
           "launch_sum_ms": round(total, 4), "call_ms": round(statistics.median(whole), 4), "call_ms_min_max": [round(min(whole), 4), round(max(whole), 4)],
           "floor_bytes": floor_bytes, "floor_ms_at_8TBps": round(floor_bytes / HBM_PEAK * 1e3, 4),
           "launch_sum_over_floor": round(total / (floor_bytes / HBM_PEAK * 1e3), 2),
           "small_launch_Mtri_per_s": round(F / (med["raster_small_kernel"] * 1e-3) / 1e6, 1), "small_launch_mesh_off_screen_ms": round(statistics.median(away), 4), "reps": a.reps}
    text = json.dumps(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
