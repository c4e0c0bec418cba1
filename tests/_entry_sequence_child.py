"""Child process of tests/test_width_lattice.py::test_entry_point_launch_sequences: the ordered per-launch records of the entry points of the HIP
library that no other sequence test pins, under the default environment.  Background forward and backward (16 rays: the 12 of the
tiny_outside fixture and its first 4 again); a forward-only render with prune_eps > 0 on 16 rays of tiny_sharp (64 wide: compact copies, the
per-layer chains) and of dtu_sharp (256 wide: the chain-fused launch reading through the index list); extract_color on 37 vertices,
extract_fields at resolution 8 and a point-query forward and backward with want_grad at 37 points, all three on tiny_sharp.  Writes
{case: [[name, kind, nt, P, N, K, pairs], ...]} as JSON to argv[1]."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import color_neus_amd as cn
    from color_neus_amd import background as B
    import _golden as G
    import _native as N
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    res = {}

    def records(call):
        """the records of call() alone: whatever ran before is collected and dropped first"""
        torch.cuda.synchronize()
        lib.timing_collect()
        out = call()
        torch.cuda.synchronize()
        return out, [list(rec[:7]) for rec in lib.timing_collect()]

    def fixture(name, n=16):
        fx = G.load(name)
        ocfg, P = G.weights_of(name, fx)
        rays = [torch.from_numpy(fx[k]).to(dev) for k in ("rays_o", "rays_d", "jit:near", "jit:far")]
        return N.make_renderer(ocfg, P, lib, dev), [torch.cat([t, t])[:n].contiguous() for t in rays]

    lib.timing_enable(True)
    try:
        r, (o, d, near, far) = fixture("tiny_outside")
        n_feed = r.rcfg.n_total + r.n_outside
        z_feed = torch.sort(torch.rand(16, n_feed, generator=torch.Generator().manual_seed(4)) * 3.0 + 0.5, dim=-1).values.to(dev)
        params = [p.detach().requires_grad_(True) for p in r.nerf.ordered_params(lib)]
        (alpha, color), res["background_forward"] = records(lambda: B.Background.apply(lib, r.nerf.config(), 2.0 / r.n_samples, o, d, z_feed, *params))
        _, res["background_backward"] = records(lambda: torch.autograd.backward([alpha, color], [torch.ones_like(alpha), torch.ones_like(color)]))
        for name in ("tiny_sharp", "dtu_sharp"):
            r, rays = fixture(name)
            with torch.no_grad():
                _, res["forward_only_prune_" + name] = records(lambda: r(*rays, perturb_overwrite=0, prune_eps=1e-3))
        r, _ = fixture("tiny_sharp")
        x = torch.rand(37, 3, generator=torch.Generator().manual_seed(3)) - 0.5
        _, res["extract_color"] = records(lambda: r.extract_color(x.numpy(), dev))
        _, res["extract_fields"] = records(lambda: r.extract_fields([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0], dev, 8))
        g, res["query_forward"] = records(lambda: r.sdf_network.gradient(x.to(dev).requires_grad_(True)))
        _, res["query_backward"] = records(lambda: (g.norm(dim=-1) - 1.0).pow(2).mean().backward())
    finally:
        lib.timing_enable(False)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
