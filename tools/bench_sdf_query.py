"""SDF point-query micro-benchmark (DTU-size network): forward + backward of
  (i)  sdf_network.sdf(x) with a d_sdf cotangent (loss = sum sdf), and
  (ii) sdf_network.gradient(x) with the eikonal cotangent (loss = sum (|g| - 1)^2),
every parameter and the points requiring grad, against the oracle's float32 torch-autograd version of the same call on the same GPU.
python tools/bench_sdf_query.py [n ...]   (one JSON line per case, then the library's per-kernel times of one call)"""
import json, os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _native as N
from oracle import colorneus_oracle as O

ocfg = O.dtu_config()
P = O.init_params(ocfg, seed=0, dtype=torch.float32, trained_like=True)
r = N.make_renderer(ocfg, P, None, "cuda:0")
Pt = {k: v.to("cuda:0").requires_grad_(k.startswith("sdf_network.")) for k, v in P.items()}
sizes = [int(a) for a in sys.argv[1:]] or [1 << 16, 1 << 19, 1 << 20]


def native(x, case):
    if case == "sdf":
        loss = r.sdf_network.sdf(x).sum()
    else:
        loss = ((r.sdf_network.gradient(x)[:, 0].norm(dim=-1) - 1.0) ** 2).sum()
    loss.backward()


def torch_ref(x, case):
    sdf, _, g = O.sdf_forward(Pt, ocfg.sdf, x, want_grad=case == "eik")
    loss = sdf.sum() if case == "sdf" else ((g.norm(dim=-1) - 1.0) ** 2).sum()
    loss.backward()


def timed(fn, x0, reps):
    def once():
        x = x0.clone().requires_grad_(True)
        fn(x, case)
    for _ in range(2):
        once()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


for n in sizes:
    x0 = (torch.rand(n, 3, generator=torch.Generator().manual_seed(n)) * 2 - 1).to("cuda:0")
    for case in ("sdf", "eik"):
        reps = 10 if n <= (1 << 19) else 5
        t_nat = timed(native, x0, reps)
        t_ref = timed(torch_ref, x0, max(2, reps // 2))
        lib = r._lib
        torch.cuda.synchronize()
        lib.timing_enable(True)
        lib.timing_collect()
        x = x0.clone().requires_grad_(True)
        native(x, case)
        torch.cuda.synchronize()
        agg = {}
        for name, kind, nt, Pn, Nn, K, pairs, ms, nbytes in lib.timing_collect():
            a = agg.setdefault(name, [0.0, 0]); a[0] += ms; a[1] += 1
        lib.timing_enable(False)
        print(json.dumps(dict(case=case, n=n, native_ms=round(t_nat * 1e3, 3), torch_fp32_ms=round(t_ref * 1e3, 3),
                              speedup=round(t_ref / t_nat, 2), kernel_ms=round(sum(v[0] for v in agg.values()), 3))))
        print("   per call:", ", ".join("%s %.3f ms x%d" % (k, v[0], v[1]) for k, v in sorted(agg.items(), key=lambda kv: -kv[1][0])))
        sys.stdout.flush()
