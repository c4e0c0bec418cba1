"""The drop-in claim against the reference, from what the reference itself recorded (tests/golden/reference_dropin.npz, written by
tools/gen_dropin_golden.py from the reference's own config files, classes and registry builder).

The native classes are registered into a registry of the reference's form (register_module(name=, force=, module=)), built from the
MODEL.RENDERER nodes of the reference's config/*.yml, and must take a state_dict with exactly the names and shapes of the reference
renderer's (strict=True); a forward on the CPU-emulation build is compared with the reference module's outputs on the same rays, with the
same weights (the native module's seeded init reproduces the reference's: checked against the recorded per-tensor sums)."""
import json
import os

import numpy as np
import pytest
import torch

import _golden as G
import _native as N
import color_neus_amd as cn

FIXTURE = os.path.join(G.GOLDEN, "reference_dropin.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(FIXTURE)


class _Node(dict):
    __getattr__ = dict.__getitem__


def _wrap(d):
    return _Node({k: _wrap(v) if isinstance(v, dict) else v for k, v in d.items()})


def _node(fx, yml):
    return _wrap(json.loads(str(fx["cfg:" + yml])))


class _Registry:
    """a registry of the reference's form: register_module(name=, force=, module=), looked up by the node's TYPE"""

    def __init__(self):
        self._module_dict = {}

    def register_module(self, name=None, force=False, module=None):
        assert name not in self._module_dict or force
        self._module_dict[name] = module
        return module

    def build(self, node):
        return self._module_dict[node["TYPE"]](node)


@pytest.mark.parametrize("yml,cls_name", [("Color_NeuS_dtu.yml", "ColorNeuSRenderer"), ("NeuS_dtu.yml", "NeuSRenderer"),
                                          ("Color_NeuS_iho.yml", "ColorNeuSRenderer"), ("Color_NeuS_bmvs.yml", "ColorNeuSRenderer")])
def test_register_build_and_strict_load(fx, yml, cls_name):
    node = _node(fx, yml)
    reg = _Registry()
    cn.register_into(reg)                                              # one line in a user's train.py
    ours = reg.build(node)
    assert type(ours).__name__ == cls_name and isinstance(ours, cn.NeuSRenderer)
    ref_sd = json.loads(str(fx["sd:" + yml]))
    sd = {k: torch.zeros(shape) for k, shape in ref_sd}               # the reference renderer's state_dict: names and shapes
    missing, unexpected = ours.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    ref_params = json.loads(str(fx["params:" + yml]))
    assert [k for k, _ in ours.named_parameters()] and set(dict(ours.named_parameters())) == set(ref_params)
    shapes = dict((k, shape) for k, shape in ref_sd)
    for k, p in ours.named_parameters():
        assert list(p.shape) == shapes[k], k


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_forward_matches_live_reference_on_same_rays(fx):
    """Same cfg node, same weights, same rays through both modules (perturb off): per-ray outputs to 1e-4 (init regime, G3)."""
    node = _node(fx, "Color_NeuS_dtu.yml")
    torch.manual_seed(0)
    ours = cn.ColorNeuSRenderer(node, library=N.EMU_LIB)
    for k, v in ours.state_dict().items():                            # the reference's weights at the same seed
        s = np.array([float(v.double().sum()), float(v.double().abs().sum())])
        assert np.allclose(s, fx["fwd:wsum:" + k], rtol=1e-9, atol=0), (k, s, fx["fwd:wsum:" + k])
    o, d = torch.from_numpy(fx["fwd:rays_o"]), torch.from_numpy(fx["fwd:rays_d"])
    near, far = torch.from_numpy(fx["fwd:near"]), torch.from_numpy(fx["fwd:far"])
    b = ours(o, d, near, far, perturb_overwrite=0)
    assert float((b["z_vals"] - b["z_vals"].sort(-1).values).abs().max()) == 0.0
    for k in ("color_fine", "depth", "weight_sum", "gradient_error", "global_color"):
        ra = torch.from_numpy(fx["fwd:out_" + k]).reshape(-1)
        err = float((b[k].detach().reshape(-1) - ra).abs().max()) / max(float(ra.abs().max()), 1e-30)
        assert err < 1e-4, (k, err)
    assert set(json.loads(str(fx["fwd:keys"]))) <= set(b.keys())
