#!/usr/bin/env python3
"""Capture the drop-in fixture from the imported upstream reference (where a reference checkout is present).

    python tools/gen_dropin_golden.py     # writes tests/golden/reference_dropin.npz

What tests/test_reference_dropin.py needs, as data only:
  cfg:<yml>      the MODEL.RENDERER node of the reference's config/<yml> (JSON: settings only)
  sd:<yml>       name and shape of every entry of the reference renderer's state_dict built from that node (JSON)
  params:<yml>   the names of its named_parameters (JSON)
  fwd:*          the Color_NeuS_dtu renderer at torch.manual_seed(0): 6 seeded rays, the reference's near / far for them, the reference
                 module's outputs with perturbation off, the names of its outputs, and per-tensor sums of its state_dict (float64) so
                 that the test can tell that the native module's seeded init produced the same weights.
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
warnings.filterwarnings("ignore")

import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "reference_dropin.npz")
YMLS = ["Color_NeuS_dtu.yml", "NeuS_dtu.yml", "Color_NeuS_iho.yml", "Color_NeuS_bmvs.yml"]
FWD_KEYS = ("color_fine", "depth", "weight_sum", "gradient_error", "global_color")


def plain(x):
    return {k: plain(v) for k, v in x.items()} if isinstance(x, dict) else x


def main():
    import yaml
    Color_NeuS, NeuS, CN, mods = ref_import.import_reference()
    from lib.utils import builder
    fx = {}
    for yml in YMLS:
        with open(os.path.join(ref_import.REFERENCE_ROOT, "config", yml)) as f:
            raw = yaml.safe_load(f)["MODEL"]["RENDERER"]
        ref_r = builder.build_from_cfg(CN(raw), builder.RENDERER)
        fx["cfg:" + yml] = np.array(json.dumps(plain(raw)))
        fx["sd:" + yml] = np.array(json.dumps([[k, list(v.shape)] for k, v in ref_r.state_dict().items()]))
        fx["params:" + yml] = np.array(json.dumps([k for k, _ in ref_r.named_parameters()]))
    with open(os.path.join(ref_import.REFERENCE_ROOT, "config", "Color_NeuS_dtu.yml")) as f:
        node = CN(yaml.safe_load(f))["MODEL"]["RENDERER"]
    torch.manual_seed(0)
    ref_r = Color_NeuS(node)
    g = torch.Generator().manual_seed(1)
    o = torch.nn.functional.normalize(torch.randn(6, 3, generator=g), dim=-1) * 2.7
    d = torch.nn.functional.normalize(torch.randn(6, 3, generator=g) * 0.3 - o, dim=-1)
    near, far = mods["ray_utils"].near_far_from_sphere(o, d)
    a = ref_r(o, d, near.squeeze(), far.squeeze(), perturb_overwrite=0)
    fx.update({"fwd:rays_o": o.numpy(), "fwd:rays_d": d.numpy(), "fwd:near": near.squeeze().numpy(), "fwd:far": far.squeeze().numpy(),
               "fwd:keys": np.array(json.dumps(sorted(a.keys())))})
    for k in FWD_KEYS:
        fx["fwd:out_" + k] = a[k].detach().numpy()
    for k, v in ref_r.state_dict().items():
        fx["fwd:wsum:" + k] = np.array([float(v.double().sum()), float(v.double().abs().sum())])
    np.savez_compressed(OUT, **fx)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
