#!/usr/bin/env python3
"""Bit-identity of the Python binding layer between two checkouts: makes every kind of library call the package offers on the CPU-emulation
library, at the tiny configuration with 5 rays, and writes each output and gradient to OUT/NNN_name.npy.  Run it in a fresh process on each
checkout (it imports the package it lies next to) and compare the two directories file by file:

    python tools/binding_ab.py OUT            # on each checkout
    python tools/binding_ab.py --compare A B  # prints the number of arrays compared and the names that differ; exit status 1 if any does

Calls: a training step (render, fused loss, backward, ClipAdam) with the full dict and with training_outputs="loss_only"; a forward-only call
without and with prune_eps; sdf, extract_fields / _slab at resolution 8, marching_cubes, extract_color; sample_pdf and up_sample; a point query
forward and backward with want_grad; the N_OUTSIDE path forward and backward; get_rays_at and rays_for_training backward; the camera forward
and backward; image_metrics and panel; nearest_neighbors; one plain layer (37 x 43 -> 33) forward and backward; every *_bytes query of a
caller-provided buffer at 5 and 4096 rays / points."""
import ctypes as C
import filecmp
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def compare(a, b):
    fa, fb = sorted(os.listdir(a)), sorted(os.listdir(b))
    if fa != fb:
        print("file lists differ:", sorted(set(fa) ^ set(fb)))
        return 1
    bad = [f for f in fa if not filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False)]
    print(f"{len(fa)} arrays compared, {len(bad)} differ", *bad)
    return 1 if bad else 0


def main(out_dir):
    import numpy as np
    import torch
    import color_neus_amd as cn
    from color_neus_amd import rays, synthetic
    import _golden as G
    import _native as N

    os.makedirs(out_dir, exist_ok=True)
    lib = cn.load_library(N.EMU_LIB)
    count = [0]

    def save(name, t):
        np.save(os.path.join(out_dir, "%03d_%s.npy" % (count[0], name)), t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
        count[0] += 1

    def save_dict(tag, d):
        for k, v in d.items():
            if v is not None:
                save(f"{tag}.{k}", v)

    def renderer(name, n=5):
        fx = G.load(name)
        ocfg, P = G.weights_of(name, fx)
        r = N.make_renderer(ocfg, P, lib, "cpu")
        t = lambda k: torch.from_numpy(fx[k][:n].copy())
        return r, t("rays_o"), t("rays_d"), t("jit:near"), t("jit:far"), t("rgb_gt"), t("mask")

    # -- training steps: render, fused loss, backward, ClipAdam -------------------------------------------------------------------------
    r, o, d, near, far, rgb, mask = renderer("tiny_sharp")
    opt = cn.ClipAdam(r._ordered_params(), lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=1.0, library=lib)
    for step, mode in enumerate(("dict", "loss_only", "dict")):
        torch.manual_seed(step)
        oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        out = r(oo, dd, near, far, training_outputs=mode, cos_anneal_ratio=0.25 * step)
        loss, ld = cn.compute_loss_fused(out, rgb, mask, library=lib)
        for p in r.parameters():
            p.grad = None
        loss.backward()
        save_dict(f"train{step}.out", out)
        save_dict(f"train{step}.loss", ld)
        save_dict(f"train{step}.grad", {k: p.grad for k, p in r.named_parameters()})
        save(f"train{step}.d_rays_o", oo.grad)
        save(f"train{step}.d_rays_d", dd.grad)
        opt.step()
        save_dict(f"train{step}.param", dict(r.named_parameters()))
    # the sampler without importance sampling: near / far take gradients
    r0, o0, d0, near0, far0, rgb0, mask0 = renderer("tiny_noimp_sharp")
    nr, fr = near0.clone().requires_grad_(True), far0.clone().requires_grad_(True)
    out = r0(o0, d0, nr, fr, perturb_overwrite=0, background_rgb=[0.2, 0.4, 0.6])
    cn.compute_loss(out, rgb0, mask0)[0].backward()
    save_dict("noimp.out", out)
    save("noimp.d_near", nr.grad)
    save("noimp.d_far", fr.grad)

    # -- forward only, without and with pruning -----------------------------------------------------------------------------------------
    with torch.no_grad():
        save_dict("infer.out", r(o, d, near, far, perturb_overwrite=0))
        save_dict("infer_prune.out", r(o, d, near, far, perturb_overwrite=0, prune_eps=1e-3))
        save_dict("empty.out", r(o[:0], d[:0], near[:0], far[:0]))

    # -- evaluation paths ---------------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(3)
    pts = torch.rand(7, 3, generator=g) - 0.5
    save("sdf", r.sdf(pts))
    bmin, bmax = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    u = r.extract_fields(bmin, bmax, "cpu", 8)
    save("extract_fields", u)
    save("extract_fields_slab", r.extract_fields_slab(bmin, bmax, "cpu", 8, 2, 5))
    verts, tris = r.marching_cubes(u, bmin, bmax, float(u.median()))
    save("mc.verts", verts)
    save("mc.tris", tris)
    save("extract_color", r.extract_color(verts.numpy(), "cpu"))
    z = torch.sort(torch.rand(5, 9, generator=g), dim=-1).values
    w = torch.rand(5, 8, generator=g)
    save("sample_pdf.det", cn.renderer.sample_pdf(z, w, 6, det=True, library=lib))
    torch.manual_seed(5)
    save("sample_pdf.rand", cn.renderer.sample_pdf(z, w, 6, det=False, library=lib))
    save("up_sample", r.up_sample(o, d, z + 2.0, torch.rand(5, 9, generator=g) - 0.5, 4, 64.0))

    # -- point query forward and backward with want_grad --------------------------------------------------------------------------------
    for p in r.parameters():
        p.grad = None
    x = pts.clone()
    grad = r.sdf_network.gradient(x)
    both = r.sdf_network(x)
    save("query.gradient", grad)
    save("query.forward", both)
    save("query.sdf", r.sdf_network.sdf(x))
    ((grad.norm(dim=-1) - 1.0).pow(2).mean() + (both * torch.rand(both.shape, generator=g)).sum()).backward()
    save("query.d_x", x.grad)
    save_dict("query.grad", {k: p.grad for k, p in r.sdf_network.named_parameters()})

    # -- N_OUTSIDE > 0 ------------------------------------------------------------------------------------------------------------------
    rb, o, d, near, far, rgb, mask = renderer("tiny_outside")
    torch.manual_seed(2)
    oo, dd = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    out = rb(oo, dd, near, far)
    cn.compute_loss(out, rgb, mask)[0].backward()
    save_dict("outside.out", out)
    save_dict("outside.grad", {k: p.grad for k, p in rb.named_parameters()})
    save("outside.d_rays_o", oo.grad)
    save("outside.d_rays_d", dd.grad)

    # -- rays ---------------------------------------------------------------------------------------------------------------------------
    H, W = 6, 5
    c2w, focal, image, msk = synthetic.synthetic_camera(height=H, width=W, focal=7.0, seed=1)
    ro, rd = rays.get_rays_at(c2w[0], focal, H, W, normalize=True, library=lib)
    save("get_rays_at.o", ro)
    save("get_rays_at.d", rd)
    c2w_g, focal_g = c2w.clone().requires_grad_(True), focal.clone().requires_grad_(True)
    torch.manual_seed(4)
    res = rays.rays_for_training(c2w_g, focal_g, image, 5, [0.1, 0.0, -0.1], 1.5, normalize=True, mask=msk, return_mask=True, library=lib)
    for k, t in zip(("o", "d", "near", "far", "rgb", "mask"), res):
        save(f"rays_for_training.{k}", t)
    wts = [torch.rand(t.shape, generator=g) for t in res[:4]]
    sum((t * w_).sum() for t, w_ in zip(res[:4], wts)).backward()
    save("rays_for_training.d_c2w", c2w_g.grad)
    save("rays_for_training.d_focal", focal_g.grad)

    # -- cameras ------------------------------------------------------------------------------------------------------------------------
    init = torch.eye(4).repeat(3, 1, 1) + 0.1 * torch.rand(3, 4, 4, generator=g)
    for mode in ("3d", "6d"):
        cams = cn.cameras.Cameras(cn.cameras.FocalNet(H, W, True, False, init_focal=7.0, library=lib),
                                  cn.cameras.PoseNet(3, True, True, pose_mode=mode, init_c2w=init, library=lib), library=lib)
        with torch.no_grad():
            cams.pose_net.r.add_(0.1 * torch.rand(cams.pose_net.r.shape, generator=g))
            cams.pose_net.t.add_(0.1 * torch.rand(3, 3, generator=g))
        cw, fc = cams([0, 2, 2])
        save(f"cameras{mode}.c2w", cw)
        save(f"cameras{mode}.focal", fc)
        ((cw * torch.rand(cw.shape, generator=g)).sum() + (fc * torch.rand(2, generator=g)).sum()).backward()
        save_dict(f"cameras{mode}.grad", {k: p.grad for k, p in cams.named_parameters()})

    # -- image metrics, nearest neighbours ----------------------------------------------------------------------------------------------
    a, b = torch.rand(H, W, 3, generator=g), torch.rand(H, W, 3, generator=g)
    save_dict("image_metrics", cn.image_metrics(a, b, return_map=True, library=lib))
    save("panel", cn.imaging.panel(a, b, torch.rand(H, W, generator=g), library=lib))
    d2, idx = cn.metrics.nearest_neighbors(torch.rand(9, 3, generator=g), torch.rand(11, 3, generator=g), library=lib)
    save("nn.dist2", d2)
    save("nn.idx", idx)

    # -- one plain layer: ragged in all three dimensions, with ReLU and without, with db and without ----------------------------------------
    n, k, n_out = 37, 43, 33
    L, ptr, null = lib.lib, cn._lib.ptr, cn._lib.ptr(None)
    xl, wl, bl, dyl = (torch.randn(*shape, generator=g) for shape in ((n, k), (n_out, k), (n_out,), (n, n_out)))
    for relu in (0, 1):
        y = torch.empty(n, n_out)
        buf, nb = lib.scratch("cnr_linear_scratch_bytes", "cpu", n, k, n_out, 0)
        lib.call("cnr_linear_forward", ptr(xl), n, k, ptr(wl), ptr(bl), n_out, relu, ptr(y), ptr(buf), nb, null)
        save(f"linear.relu{relu}.y", y)
        for with_db in (0, 1):
            dx, dW, db = torch.empty(n, k), torch.empty(n_out, k), torch.empty(n_out) if with_db else None
            buf, nb = lib.scratch("cnr_linear_scratch_bytes", "cpu", n, k, n_out, 1)
            lib.call("cnr_linear_backward", ptr(xl), ptr(y), ptr(dyl), n, k, ptr(wl), n_out, relu, ptr(dx), ptr(dW), ptr(db), ptr(buf), nb, null)
            save_dict(f"linear.relu{relu}.db{with_db}", dict(dx=dx, dW=dW, db=db))

    # -- every *_bytes query of the caller-provided buffers, at the configurations built above ------------------------------------------------
    sizes = []
    for n in (5, 4096):
        for ren in (r, r0, rb):
            c = C.byref(ren._ccfg)
            sizes += [L.cnr_ctx_bytes(c, n), L.cnr_bwd_scratch_bytes(c, n), L.cnr_infer_scratch_bytes(c, n), L.cnr_vertex_color_scratch_bytes(c, n)]
            sizes += [fn(c, n, wg) for wg in (0, 1) for fn in (L.cnr_sdf_query_ctx_bytes, L.cnr_sdf_query_bwd_scratch_bytes)]
        ncfg, n_feed = rb.nerf.config(), rb.rcfg.n_total + rb.n_outside
        sizes += [L.cnr_background_ctx_bytes(C.byref(ncfg), n, n_feed), L.cnr_background_bwd_scratch_bytes(C.byref(ncfg), n, n_feed)]
        sizes += [L.cnr_linear_scratch_bytes(n, k, n_out, backward) for backward in (0, 1)]
    save("scratch_bytes", np.asarray(sizes, dtype=np.int64))
    print(f"{count[0]} arrays written to {out_dir}")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
