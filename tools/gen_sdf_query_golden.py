#!/usr/bin/env python3
"""Capture the reference SDFNetwork's own point-query values and gradients (THIS CONTAINER ONLY).

    python tools/gen_sdf_query_golden.py     # writes tests/golden/sdf_query.npz

For each network (tiny, mid, tiny_nown_skip2, tiny_twoskip, DTU widths) the unmodified reference (imported through tools/ref_import.py)
evaluates SDFNetwork.forward and SDFNetwork.gradient (fields.py:81-115) at 64 seeded points, some outside the unit sphere, and
differentiates one fixed loss that uses all three cotangents,

    L = sum a * sdf + sum B * feat + sum c * g + sum (|g| - 1)^2,    g = gradient(x) (create_graph=True: the double backward),

with seeded a, B, c, in float32 and in float64.  Stored: the weight recipe (seed + checksum of oracle.init_params, trained-like), the points,
a / B / c, the float32 forward / gradient values, the loss, and the gradients of every sdf_network parameter and of the points in both
precisions.  Parameter gradients with more than STRIDE_LIMIT entries keep every `stride`-th entry of the flattened tensor (stored as
`<tag>:stride`); the file stays well under 1 MB.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
warnings.filterwarnings("ignore")

import ref_import  # noqa: E402
from gen_golden import node_from_config  # noqa: E402
from oracle import colorneus_oracle as O  # noqa: E402  (config dataclasses + weight recipe)
import _golden as G  # noqa: E402  (the test configurations)

OUT = os.path.join(ROOT, "tests", "golden", "sdf_query.npz")
N_PTS = 64
STRIDE_LIMIT = 1024

NETS = {   # tag -> (config, weight seed, gradient stride)
    "tiny": (O.tiny_config, 3, 5),
    "mid": (G.mid_config, 4, 7),
    "tiny_nown_skip2": (G.CONFIGS["tiny_nown_skip2"], 5, 7),
    "tiny_twoskip": (G.CONFIGS["tiny_twoskip"], 6, 7),
    "dtu": (O.dtu_config, 0, 197),
}


def points(n, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    return d * torch.rand(n, 1, generator=g, dtype=torch.float64) ** (1.0 / 3.0) * 1.3


def run(ref_net, x, a, B, c, dtype):
    net = ref_net.to(dtype)
    for p in net.parameters():
        p.grad = None
    x = x.to(dtype).clone().requires_grad_(True)   # before the forward: d L / d x takes the value path too
    out = net(x)
    g = net.gradient(x)[:, 0]
    loss = (a.to(dtype) * out[:, 0]).sum() + (B.to(dtype) * out[:, 1:]).sum() + (c.to(dtype) * g).sum() + ((g.norm(dim=-1) - 1.0) ** 2).sum()
    loss.backward()
    grads = {"sdf_network." + k: p.grad.detach().clone() for k, p in net.named_parameters()}
    return out.detach(), g.detach(), loss.detach(), grads, x.grad.detach().clone()


def main():
    torch.set_num_threads(8)
    Color_NeuS, NeuS, CN, mods = ref_import.import_reference()
    fx = {}
    for i, (tag, (mk, seed, stride)) in enumerate(NETS.items()):
        cfg = mk()
        P = O.init_params(cfg, seed=seed, dtype=torch.float32, trained_like=True)
        cls = Color_NeuS if cfg.type == "Color_NeuS" else NeuS
        r = cls(node_from_config(cfg, CN))
        r.load_state_dict(P)
        x = points(N_PTS, 100 + i).float()
        g = torch.Generator().manual_seed(200 + i)
        a = torch.randn(N_PTS, generator=g)
        B = torch.randn(N_PTS, cfg.sdf.d_out - 1, generator=g) * 0.1
        c = torch.randn(N_PTS, 3, generator=g)
        fx.update({f"{tag}:weight_seed": np.int64(seed), f"{tag}:weight_checksum": np.float64(O.params_checksum(P)),
                   f"{tag}:stride": np.int64(stride), f"{tag}:x": x.numpy(), f"{tag}:a": a.numpy(), f"{tag}:B": B.numpy(), f"{tag}:c": c.numpy()})
        for dt, name in ((torch.float32, "f32"), (torch.float64, "f64")):
            out, gr, loss, grads, xg = run(r.sdf_network, x, a, B, c, dt)
            if dt == torch.float32:
                fx[f"{tag}:forward"], fx[f"{tag}:gradient"] = out.numpy(), gr.numpy()
            fx[f"{tag}:{name}:loss"] = loss.numpy()
            fx[f"{tag}:{name}:x_grad"] = xg.numpy()
            for k, v in grads.items():
                v = v.reshape(-1)
                fx[f"{tag}:{name}:{k}"] = (v if v.numel() <= STRIDE_LIMIT else v[::stride]).numpy()
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
