"""Child process of tests/test_width_lattice.py::test_backward_launch_sequence_per_switch: the ordered per-launch records of the backward
calls of the HIP library under the CNR_* switches of the environment it was started with (the library reads them once per process).  DTU-width
Color-NeuS configuration: one training step with d_rays requested at each of the two batch shapes of the width lattice, and one point-query
backward of 64 points without and with the gradient (want_grad 0 / 1).  Writes {case: [[name, kind, nt, P, N, K, pairs], ...]} as JSON to
argv[1]."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import color_neus_amd as cn
    import _native as N
    import test_width_lattice as T
    from oracle import colorneus_oracle as O      # inputs only (weights, rays)
    dev = torch.device("cuda:0")
    lib = cn.load_library()
    res = {}

    def backward_records(loss):
        """the records of loss.backward() alone: whatever the forward launched is collected and dropped first"""
        torch.cuda.synchronize()
        lib.timing_collect()
        loss.backward()
        torch.cuda.synchronize()
        return [list(rec[:7]) for rec in lib.timing_collect()]

    lib.timing_enable(True)
    try:
        for shape, (R, ns, ni, steps) in T.SHAPES.items():
            ocfg = O.dtu_config(ns, ni)
            ocfg.up_sample_steps = steps
            r = N.make_renderer(ocfg, O.init_params(ocfg, seed=5, trained_like=True), None, dev)
            o, d, near, far, t_rand, gt, mask = [t.to(dev) for t in T._batch(R, 7)]
            out = r(o.requires_grad_(True), d.requires_grad_(True), near, far)
            loss, _ = cn.compute_loss(out, gt, mask)
            res["step_" + shape] = backward_records(loss)
        x = (torch.rand(64, 3, generator=torch.Generator().manual_seed(17)) * 2.0 - 1.0).to(dev)
        res["query_want_grad_0"] = backward_records(r.sdf_network.sdf(x.clone().requires_grad_(True)).sum())
        res["query_want_grad_1"] = backward_records((r.sdf_network.gradient(x.clone()).norm(dim=-1) - 1.0).pow(2).mean())
    finally:
        lib.timing_enable(False)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    main()
