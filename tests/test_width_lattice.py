"""The lattice of network widths build_model accepts, beyond the two points every other test uses (the 64-wide tiny network and the 256-wide
DTU one): SDF d_hidden any multiple of 16 in [48, 256], colour / relight d_hidden any multiple of 16 in [16, 256], d_feature 1..256 (top SDF
layer 2..257 wide), skip layers of width d_hidden - embedding.  All fused fast paths are gated on 256; every other width goes through the
general layer / weight-gradient kernels in instantiations no other GPU test launches (weight-stationary kernel with 96..224 weight rows or an
odd number of k16 blocks, the 3-tile general kernel, tail fill behind a 9- or 89-wide skip layer, partial weight-gradient tiles and their row
tails).  Eight configurations x two batch shapes through the product route against the float64 oracle run live, under the project's own
gates (tests/_golden.py: nothing new); CPU: emulation build (loose rule, as everywhere), GPU (-m gpu): HIP build (strict rule).  A ninth
configuration, `deep`, adds depth instead of a width: 29 linear layers, more than one batch of the batched weight launches holds; shape B only.

Batch shapes: (A) 64 rays x (16 + 16) samples, 4 up-sampling steps: 2048 points, all tiles full; (B) 67 rays x (12 + 9), 3 steps: 1407
points, P % 32 = 31, a ragged last tile in every kernel.

Seeds: rays / jitter / targets / mask of a case come from one torch.Generator (the recipe of test_edge_batches._batch).  A case's seed is
the first one >= 7 at which the float32 ORACLE ITSELF passes the strict gradient gate against its float64 run on every tensor (asserted in
every test as a precondition, never skipped) and, at shape A, at most 8 of the 64 rays are sensitive ones of the sampler -- so that no tensor
needs to be excluded from any case."""
import functools
import os

import pytest
import torch

import _golden as G
import _native as N

DEV = "cuda:0"
SHAPES = {"A": (64, 16, 16, 4), "B": (67, 12, 9, 3)}     # rays, N_SAMPLES, N_IMPORTANCE, UP_SAMPLE_STEPS


def _cfg(kind, sdf, d_feature, color, relight, multires=6):
    from oracle import colorneus_oracle as O
    h, n, skip = sdf
    if color[0] == "idr":
        col = O.ColorConfig(d_feature=d_feature, mode="idr", d_in=9, multires_view=color[1], d_hidden=color[2], n_layers=color[3])
    else:
        col = O.ColorConfig(d_feature=d_feature, mode="no_view_dir", d_in=6, multires_view=0, d_hidden=color[2], n_layers=color[3])
    rel = O.RelightConfig(d_hidden=relight[0], n_layers=relight[1], y_in_layer=relight[2]) if relight else None
    return O.RenderConfig(type=kind, sdf=O.SDFConfig(d_out=d_feature + 1, d_hidden=h, n_layers=n, skip_in=list(skip), multires=multires), color=col, relight=rel)


# name -> configuration.  (SDF d_hidden, layers, skip), d_feature, (colour mode, multires_view, hidden, layers), (relight hidden, layers, y_in_layer)
CONFIGS = {
    # ws kernel at 128 rows and 8 k-blocks; 89-wide skip layer: 3-tile general kernel + tail fill; 128 x 128 weight-gradient tiles
    "w128": lambda: _cfg("Color_NeuS", (128, 4, [2]), 128, ("no_view_dir", 0, 128, 2), (128, 3, 2)),
    # lower end of every range: 9-wide skip layer, 1- and 2-tile general kernel, weight-gradient row tails <= 32, skinny strips
    "w48": lambda: _cfg("Color_NeuS", (48, 3, [2]), 20, ("no_view_dir", 0, 16, 1), (32, 2, 1)),
    # ws kernel at 96 and at 128 rows with 101 live; 7 k-blocks (K = 112); K = 240, the boundary of the stream form
    "mixed": lambda: _cfg("Color_NeuS", (96, 3, [1]), 100, ("no_view_dir", 0, 112, 2), (240, 2, 2)),
    # a 256-wide colour stack beside a 208-wide SDF net (K = 208, just outside the fused weight-gradient shapes); 169-wide skip layer
    "w208": lambda: _cfg("Color_NeuS", (208, 3, [2]), 256, ("no_view_dir", 0, 256, 2), (144, 2, 1)),
    # 80-wide colour stack (3-tile general kernel); the idr view branch at a new width
    "neus176": lambda: _cfg("NeuS", (176, 2, []), 192, ("idr", 4, 80, 2), None),
    # fused hidden layers under a top layer EXACTLY 256 wide: no narrow remainder launch, so the fused top layer is off
    "f255": lambda: _cfg("Color_NeuS", (256, 3, [2]), 255, ("no_view_dir", 0, 256, 2), (256, 3, 2)),
    # the 96-column threshold of the ws kernel from both sides (95 + 1 = 96-wide top layer, 96-wide colour stack); 27-column embedding
    "thresh": lambda: _cfg("Color_NeuS", (160, 3, [2]), 95, ("no_view_dir", 0, 96, 2), (192, 2, 1), multires=4),
    # top layer exactly one 32-column tile (the boundary of the weight-gradient row tails)
    "f31": lambda: _cfg("NeuS", (64, 2, []), 31, ("idr", 2, 48, 1), None),
    # 13 + 9 + 7 = 29 linear layers: more than the 24 jobs of one batched weight-preparation / weight-gradient finish launch, so both take a second
    # batch (shape B only: the depth, not the widths, is what this row adds)
    "deep": lambda: _cfg("Color_NeuS", (48, 12, [4]), 20, ("no_view_dir", 0, 16, 8), (16, 6, 1)),
}
ONLY_SHAPE = {"deep": "B"}        # configurations that run at one batch shape

# Seeds (see the module docstring): 7 wherever the float32 oracle passes the strict gate at 7.  Rejected: f255 / A at 7 and w208 / B at 7
# and 8 -- on those draws only deviation_network.variance fails, the one-entry cancelling sum (tests/_golden.py scalar_tolerance), where the
# float32 oracle itself sits beyond 5e-4 of the float64 value.
CASES = [(name, shape) for name in CONFIGS for shape in SHAPES if ONLY_SHAPE.get(name, shape) == shape]
SEEDS = {case: 7 for case in CASES}
SEEDS["f255", "A"] = 8
SEEDS["w208", "B"] = 9
MAX_SENSITIVE_RAYS = 8


def _batch(R, seed):
    from oracle import colorneus_oracle as O
    g = torch.Generator().manual_seed(seed)
    o = torch.randn(R, 3, generator=g)
    o = o / o.norm(dim=-1, keepdim=True).clamp_min(1e-6) * 2.7
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g) * 0.3 - o, dim=-1)
    near, far = O.near_far_from_sphere(o, d)
    t_rand = torch.rand(R, 1, generator=g)
    gt = torch.rand(R, 3, generator=g)
    mask = (torch.rand(R, generator=g) > 0.3).float()
    return o, d, near, far, t_rand, gt, mask


def _oracle_run(O, ocfg, P, o, d, near, far, z, gt, mask, dt):
    Pd = {k: v.to(dt).clone().requires_grad_(True) for k, v in P.items()}
    od, dd = o.to(dt).clone().requires_grad_(True), d.to(dt).clone().requires_grad_(True)
    out = O.render(Pd, ocfg, od, dd, near.to(dt), far.to(dt), z_vals=z.to(dt))
    loss, _ = O.compute_loss(out, gt.to(dt), mask.to(dt))
    loss.backward()
    g = {k: v.grad for k, v in Pd.items()}
    g["rays_o"], g["rays_d"] = od.grad, dd.grad
    return {k: v.detach() for k, v in out.items() if torch.is_tensor(v)}, loss.detach(), g


@functools.lru_cache(maxsize=None)
def _reference(name, shape, seed=None):
    """The oracle's side of one case, computed once and shared by every test that needs it (never modified): configuration, weights, batch,
    the float32 sampler's z (the positions every render below uses), the float64 sampler's z, and the float64 / float32 renders + gradients."""
    from oracle import colorneus_oracle as O
    R, ns, ni, steps = SHAPES[shape]
    ocfg = CONFIGS[name]()
    ocfg.n_samples, ocfg.n_importance, ocfg.up_sample_steps = ns, ni, steps
    P = O.init_params(ocfg, seed=5, trained_like=True)
    o, d, near, far, t_rand, gt, mask = _batch(R, SEEDS[name, shape] if seed is None else seed)
    z32 = O.sample_z(P, ocfg, o, d, near, far, t_rand)
    z64 = O.sample_z({k: v.double() for k, v in P.items()}, ocfg, o.double(), d.double(), near.double(), far.double(), t_rand.double())
    out64, l64, g64 = _oracle_run(O, ocfg, P, o, d, near, far, z32, gt, mask, torch.float64)
    out32, l32, g32 = _oracle_run(O, ocfg, P, o, d, near, far, z32, gt, mask, torch.float32)
    return dict(O=O, ocfg=ocfg, P=P, batch=(o, d, near, far, t_rand, gt, mask), z32=z32, z64=z64, out64=out64, l64=l64, g64=g64, out32=out32, l32=l32, g32=g32)


def _live(ref):
    """(g64, g32) restricted to the tensors the oracle gives a gradient that is not identically zero, and the names of the others"""
    dead = [k for k, v in ref["g64"].items() if v is None or float(v.abs().max()) == 0.0]
    g64 = {k: v for k, v in ref["g64"].items() if k not in dead}
    return g64, {k: ref["g32"][k] for k in g64}, dead


def _preconditions(name, shape, ref):
    """What the seeds were chosen for; asserted, never skipped: the float32 oracle's own gradients pass the strict rule against its float64
    run on every tensor, and at shape A at most MAX_SENSITIVE_RAYS rays are ones whose samples the oracle's own two precisions place apart."""
    g64, g32, _ = _live(ref)
    bad = G.check_grads_full(g64, g32, g32, strict=True)
    assert not bad, ("float32 oracle outside the strict gate: choose another seed", name, shape, bad)
    if shape == "A":
        n = int(((ref["z32"].double() - ref["z64"]).abs().amax(dim=1) > 2e-4).sum())
        assert n <= MAX_SENSITIVE_RAYS, ("too many sensitive rays: choose another seed", name, shape, n)


def _grad_rows(g64, g32, got, strict):
    """format_grad_table rows of one case (sum columns as in the fixtures' table, over all entries)"""
    rows = []
    cap = G._gate(strict)[2]
    for k, r64 in g64.items():
        r64 = r64.detach().double().reshape(-1)
        full = got[k].detach().cpu().double().reshape(-1)
        den = max(float(r64.abs().max()), 1e-300)
        e = (full - r64).abs() / den
        r32 = g32[k].detach().double().reshape(-1)
        spread = float((r32 - r64).abs().max()) / den
        lim = min(cap, G.grad_tolerance(spread, strict) if e.numel() > 1 else G.scalar_tolerance(spread))
        allowed = G._allowed(e.numel(), strict)
        bulk = float(torch.sort(e).values[-(allowed + 1)]) if e.numel() > allowed else 0.0
        gabs = max(float(r64.abs().sum()), 1e-300)
        rows.append((k, e.numel(), float(e.max()), float((full - r32).abs().max()) / den, lim, abs(float(full.sum() - r64.sum())) / gabs,
                     abs(float(full.abs().sum()) - float(r64.abs().sum())) / gabs, int((e > lim).sum()), bulk))
    return rows


_RESULTS = {}     # (name, shape, build) -> format_grad_table rows, filled by _check: the error-table test reuses what the case tests computed


def _check(name, shape, library, device, strict):
    import color_neus_amd as cn
    ref = _reference(name, shape)
    _preconditions(name, shape, ref)
    O, ocfg, P = ref["O"], ref["ocfg"], ref["P"]
    o, d, near, far, t_rand, gt, mask = ref["batch"]
    R, M = o.shape[0], ocfg.n_samples + ocfg.n_importance
    r = N.make_renderer(ocfg, P, library, device)
    dv = lambda t: t.to(device)
    # (clone: on the CPU .to() returns the shared reference's own tensor, whose .grad a second _check of the case would add to)
    og, dg = dv(o).clone().requires_grad_(True), dv(d).clone().requires_grad_(True)
    out = r(og, dg, dv(near), dv(far), z_vals=dv(ref["z32"]))
    loss, _ = cn.compute_loss(out, dv(gt), dv(mask))
    loss.backward()
    bad = []
    # -- outputs: against float64 within max(1e-4, 1.5 x the float32 oracle's own distance) (check_outputs' rule for float64 fixtures)
    lims = {}
    out64, out32 = ref["out64"], ref["out32"]
    assert out["gradients"].shape == (R, M, 3)
    for k in G.OUTPUT_KEYS:
        if k not in out64:
            assert k in ("global_color", "delta_relight") and ocfg.type == "NeuS", k
            continue
        e = G.relerr(out[k].detach().cpu().reshape(out64[k].shape), out64[k])
        lims[k] = lim = max(1e-4, 1.5 * G.relerr(out32[k], out64[k]))
        if k == "weight_max":
            lim = max(lim, lims["weights"])
        print("%s/%s out %-16s err %.2e lim %.2e" % (name, shape, k, e, lim))
        if not e < lim:
            bad.append((k, e, lim))
    l64 = float(ref["l64"])
    el = abs(float(loss.detach()) - l64) / abs(l64)
    print("%s/%s loss err %.2e" % (name, shape, el))
    if not el < 1e-4:
        bad.append(("loss", el, 1e-4))
    # -- gradients: every entry of every parameter gradient + d rays under check_grads_full; exactly zero where the oracle has none
    got = {(k[len("renderer."):] if k.startswith("renderer.") else k): p.grad for k, p in r.named_parameters()}
    got["rays_o"], got["rays_d"] = og.grad, dg.grad
    assert set(got) == set(ref["g64"]), set(got) ^ set(ref["g64"])
    g64, g32, dead = _live(ref)
    for k in dead:
        assert got[k] is None or float(got[k].abs().max()) == 0.0, (k, "the oracle's gradient is zero")
    rows = _grad_rows(g64, g32, got, strict)
    _RESULTS[name, shape, "hip" if library is None else "emu"] = rows
    print(G.format_grad_table("%s / %s" % (name, shape), rows))
    bad += G.check_grads_full(g64, g32, got, strict=strict)
    assert not bad, (name, shape, bad)
    return r, out


def _check_sampler(name, r, ref, device):
    """The library's own sampler (z_vals=None, the case's jitter draw fed through the module's CPU-generator call) against the float64
    sampler, second rule of check_g1: rays on which the oracle's own float32 and float64 samplers differ by more than 2e-4 may sit up to
    half a coarse section away, every other ray within 1e-3."""
    ocfg = ref["ocfg"]
    o, d, near, far, t_rand = [t.to(device) for t in ref["batch"][:4]] + [ref["batch"][4]]
    orig = torch.rand
    try:
        torch.rand = lambda *a, **k: t_rand.clone()
        with torch.no_grad():
            z = r(o, d, near, far)["z_vals"].cpu()
    finally:
        torch.rand = orig
    assert bool((z[:, 1:] >= z[:, :-1]).all()), "z_vals must be sorted"
    df = (z.double() - ref["z64"]).abs().amax(dim=1)
    sensitive = (ref["z32"].double() - ref["z64"]).abs().amax(dim=1) > 2e-4
    stray = int(((df > 1e-3) & ~sensitive).sum())
    print("%s/A sampler: max |dz| %.2e, %d sensitive ray(s), %d stray" % (name, float(df.max()), int(sensitive.sum()), stray))
    assert float(df.max()) < 1.0 / (2 * ocfg.n_samples) and stray == 0, (name, float(df.max()), stray, int(sensitive.sum()))


_FWD_KEYS = ["color_fine", "s_val", "cdf_fine", "weight_sum", "weight_max", "gradients", "weights", "gradient_error", "inside_sphere", "depth",
             "global_color", "delta_relight", "z_vals", "eik_sums"]      # tests/test_forward_only.py KEYS


def _check_eval(name, r, out, ref, device):
    """sdf() on 3000 points of [-1, 1]^3 against the float64 oracle at 2e-5 of the output's scale (the bound of
    test_fused_sdf_chain_matches_per_layer_kernels), and the forward-only entry point (the same render under torch.no_grad()) against the
    training forward: bit-identical in every output (the rule of tests/test_forward_only.py)."""
    O, ocfg = ref["O"], ref["ocfg"]
    pts = torch.rand(3000, 3, generator=torch.Generator().manual_seed(17)) * 2.0 - 1.0
    want = O.sdf_value({k: v.double() for k, v in ref["P"].items()}, ocfg.sdf, pts.double()).reshape(-1)
    got = r.sdf(pts.to(device)).cpu().double().reshape(-1)
    e = float((got - want).abs().max()) / float(want.abs().max())
    print("%s sdf() err %.2e" % (name, e))
    assert e < 2e-5, (name, "sdf", e)
    o, d, near, far = [t.to(device) for t in ref["batch"][:4]]
    with torch.no_grad():
        fwd = r(o, d, near, far, z_vals=ref["z32"].to(device))
        fwd2 = r(o, d, near, far, z_vals=ref["z32"].to(device), forward_only=True)
    for k in _FWD_KEYS:
        if k in out:
            assert torch.equal(out[k].detach(), fwd[k]), (name, k, float((out[k].detach() - fwd[k]).abs().max()))
            assert torch.equal(fwd[k], fwd2[k]), (name, k)
    assert set(fwd) == set(out)


def _case(name, shape, library, device, strict):
    r, out = _check(name, shape, library, device, strict)
    if shape == "A":
        ref = _reference(name, shape)
        _check_sampler(name, r, ref, device)
        _check_eval(name, r, out, ref, device)


@pytest.mark.parametrize("name,shape", CASES)
def test_width_lattice_emu(name, shape):
    """CPU emulation build: shares the host units (cnr_plan.h), none of the HIP kernels; loose gradient rule as everywhere."""
    _case(name, shape, N.EMU_LIB, torch.device("cpu"), strict=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name,shape", CASES)
def test_width_lattice_hip(name, shape):
    _case(name, shape, None, torch.device(DEV), strict=True)


@pytest.mark.gpu
def test_width_lattice_error_table():
    """The per-tensor error table of the HIP build on all 17 cases (what the gate above condenses: error against float64, bulk error, distance
    from the float32 oracle, tolerance), written to profiles/width_lattice_error_table.txt: the measured numbers live there, not in the gates."""
    lines = []
    for name, shape in CASES:
        if (name, shape, "hip") not in _RESULTS:
            _check(name, shape, None, torch.device(DEV), strict=True)
        rows = _RESULTS[name, shape, "hip"]
        R, ns, ni, steps = SHAPES[shape]
        lines.append(G.format_grad_table("%s / %s (%d rays x (%d + %d) samples, seed %d): HIP gradients vs the float64 oracle (own scale per tensor; "
                                         "err_vs_f32: against the float32 oracle)" % (name, shape, R, ns, ni, SEEDS[name, shape]), rows))
        lines.append("")
        assert max(r[2] for r in rows) <= G.STRICT_TOL_CAP
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        with open(os.path.join(root, "profiles", "width_lattice_error_table.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass


# The launches this file exists for, as (record name, nt, N, K) of the library's per-launch records: pinned from a run on the MI355X.  A later
# change of dispatch that routes these shapes elsewhere fails here instead of silently shrinking what the cases above cover.
CENSUS = [
    ('dw_gemm', 1811, 9, 48), ('dw_gemm', 1811, 16, 26), ('dw_gemm', 1811, 21, 48), ('dw_gemm', 1811, 32, 33), ('dw_gemm', 1811, 32, 35),
    ('dw_gemm', 1811, 32, 64), ('dw_gemm', 8112, 48, 39), ('dw_gemm', 8112, 48, 48), ('dw_gemm', 8112, 48, 52), ('dw_gemm', 8112, 57, 39),
    ('dw_gemm', 8112, 64, 39), ('dw_gemm', 8112, 64, 64), ('dw_gemm', 8112, 128, 33), ('dw_gemm', 8112, 128, 39), ('dw_gemm', 8112, 144, 33),
    ('dw_gemm', 8112, 160, 27), ('dw_gemm', 8112, 176, 39), ('dw_gemm', 8112, 192, 33), ('dw_gemm', 8112, 208, 39), ('dw_gemm', 8112, 240, 33),
    ('dw_gemm_bx', 4224, 96, 160), ('dw_gemm_bx', 4224, 101, 96), ('dw_gemm_bx', 4224, 129, 128), ('dw_gemm_bx', 4224, 193, 176), ('dw_gemm_bx', 4224, 256, 256),
    ('dw_gemm_hx', 4224, 80, 80), ('dw_gemm_hx', 4224, 80, 225), ('dw_gemm_hx', 4224, 89, 128), ('dw_gemm_hx', 4224, 96, 96), ('dw_gemm_hx', 4224, 96, 101),
    ('dw_gemm_hx', 4224, 112, 106), ('dw_gemm_hx', 4224, 112, 112), ('dw_gemm_hx', 4224, 128, 128), ('dw_gemm_hx', 4224, 128, 131), ('dw_gemm_hx', 4224, 128, 134),
    ('dw_gemm_hx', 4224, 133, 160), ('dw_gemm_hx', 4224, 144, 147), ('dw_gemm_hx', 4224, 160, 160), ('dw_gemm_hx', 4224, 169, 208), ('dw_gemm_hx', 4224, 176, 176),
    ('dw_gemm_hx', 4224, 192, 195), ('dw_gemm_hx', 4224, 208, 208), ('dw_gemm_hx', 4224, 240, 240), ('dw_gemm_hx', 4224, 256, 208), ('dw_gemm_hx', 4224, 256, 256),
    ('dw_skinny', 1, 1, 208), ('dw_skinny', 1, 3, 16), ('dw_skinny', 1, 3, 32), ('dw_skinny', 1, 3, 48), ('dw_skinny', 1, 3, 80),
    ('dw_skinny', 1, 3, 96), ('dw_skinny', 1, 3, 112), ('dw_skinny', 1, 3, 128), ('dw_skinny', 1, 3, 144), ('dw_skinny', 1, 3, 192),
    ('dw_skinny', 1, 3, 243), ('dw_skinny', 2, 256, 5),
    ('layer_gemm', 1, 1, 48), ('layer_gemm', 1, 1, 64), ('layer_gemm', 1, 1, 160), ('layer_gemm', 1, 3, 16), ('layer_gemm', 1, 3, 32),
    ('layer_gemm', 1, 3, 48), ('layer_gemm', 1, 3, 80), ('layer_gemm', 1, 3, 96), ('layer_gemm', 1, 3, 112), ('layer_gemm', 1, 3, 128),
    ('layer_gemm', 1, 3, 144), ('layer_gemm', 1, 3, 192), ('layer_gemm', 1, 3, 243), ('layer_gemm', 1, 5, 256), ('layer_gemm', 1, 16, 3),
    ('layer_gemm', 1, 16, 26), ('layer_gemm', 1, 20, 48), ('layer_gemm', 1, 26, 16), ('layer_gemm', 1, 27, 160), ('layer_gemm', 1, 31, 64),
    ('layer_gemm', 1, 32, 3), ('layer_gemm', 1, 32, 33), ('layer_gemm', 1, 32, 35), ('layer_gemm', 2, 33, 32), ('layer_gemm', 2, 33, 128),
    ('layer_gemm', 2, 33, 144), ('layer_gemm', 2, 33, 192), ('layer_gemm', 2, 33, 240), ('layer_gemm', 2, 35, 32), ('layer_gemm', 2, 39, 48),
    ('layer_gemm', 2, 39, 57), ('layer_gemm', 2, 39, 64), ('layer_gemm', 2, 39, 128), ('layer_gemm', 2, 39, 176), ('layer_gemm', 2, 39, 208),
    ('layer_gemm', 2, 48, 3), ('layer_gemm', 2, 48, 9), ('layer_gemm', 2, 48, 21), ('layer_gemm', 2, 48, 39), ('layer_gemm', 2, 48, 48),
    ('layer_gemm', 2, 48, 52), ('layer_gemm', 2, 52, 48), ('layer_gemm', 2, 64, 32), ('layer_gemm', 2, 64, 39), ('layer_gemm', 2, 64, 64),
    ('layer_gemm', 3, 80, 3), ('layer_gemm', 3, 80, 80), ('layer_gemm', 3, 80, 225), ('layer_gemm', 3, 95, 160),
    ('layer_gemm_ws', 103, 96, 3), ('layer_gemm_ws', 103, 96, 39), ('layer_gemm_ws', 103, 96, 96), ('layer_gemm_ws', 103, 96, 101), ('layer_gemm_ws', 104, 100, 96),
    ('layer_gemm_ws', 104, 101, 96), ('layer_gemm_ws', 104, 106, 112), ('layer_gemm_ws', 104, 112, 3), ('layer_gemm_ws', 104, 112, 106), ('layer_gemm_ws', 104, 112, 112),
    ('layer_gemm_ws', 104, 128, 3), ('layer_gemm_ws', 104, 128, 33), ('layer_gemm_ws', 104, 128, 39), ('layer_gemm_ws', 104, 128, 89), ('layer_gemm_ws', 104, 128, 128),
    ('layer_gemm_ws', 104, 128, 129), ('layer_gemm_ws', 104, 128, 131), ('layer_gemm_ws', 104, 128, 134), ('layer_gemm_ws', 105, 131, 128), ('layer_gemm_ws', 105, 134, 128),
    ('layer_gemm_ws', 105, 144, 3), ('layer_gemm_ws', 105, 144, 33), ('layer_gemm_ws', 105, 144, 147), ('layer_gemm_ws', 105, 147, 144), ('layer_gemm_ws', 105, 160, 27),
    ('layer_gemm_ws', 105, 160, 96), ('layer_gemm_ws', 105, 160, 133), ('layer_gemm_ws', 105, 160, 160), ('layer_gemm_ws', 106, 176, 39), ('layer_gemm_ws', 106, 176, 176),
    ('layer_gemm_ws', 106, 176, 193), ('layer_gemm_ws', 106, 192, 3), ('layer_gemm_ws', 106, 192, 33), ('layer_gemm_ws', 106, 192, 176), ('layer_gemm_ws', 106, 192, 195),
    ('layer_gemm_ws', 107, 195, 192), ('layer_gemm_ws', 107, 208, 39), ('layer_gemm_ws', 107, 208, 169), ('layer_gemm_ws', 107, 208, 208), ('layer_gemm_ws', 107, 208, 257),
    ('layer_gemm_ws', 108, 225, 80), ('layer_gemm_ws', 108, 240, 33), ('layer_gemm_ws', 108, 240, 240), ('layer_gemm_ws', 108, 243, 3), ('layer_gemm_ws', 108, 255, 256),
    ('layer_gemm_ws', 108, 256, 33), ('layer_gemm_ws', 108, 256, 39), ('layer_gemm_ws', 108, 256, 208), ('layer_gemm_ws', 108, 256, 217), ('layer_gemm_ws', 108, 256, 256),
    ('layer_gemm_ws', 108, 256, 259), ('layer_gemm_ws', 108, 256, 261), ('layer_gemm_ws', 108, 256, 262),
]


@pytest.mark.gpu
def test_width_lattice_launch_census():
    """Shape A of the eight width configurations and shape B of `deep` (forward + backward) under the library's per-launch records: the union of
    launches contains the general-kernel instantiations named in the module docstring, and `deep`, with its 29 layers, takes a second batch of the
    batched row-job launches (24 jobs each: prep_weight, finish_weight; split_planes holds 48, W and Wt of a layer, and splits with prep_weight)."""
    import color_neus_amd as cn
    lib = cn.load_library()
    dev = torch.device(DEV)
    seen, batches = set(), {}
    for name in CONFIGS:
        ref = _reference(name, ONLY_SHAPE.get(name, "A"))
        o, d, near, far, t_rand, gt, mask = [t.to(dev) for t in ref["batch"]]
        r = N.make_renderer(ref["ocfg"], ref["P"], None, dev)
        lib.timing_enable(True)
        try:
            lib.timing_collect()
            out = r(o, d, near, far, z_vals=ref["z32"].to(dev))
            loss, _ = cn.compute_loss(out, gt, mask)
            loss.backward()
            torch.cuda.synchronize()
            recs = lib.timing_collect()
        finally:
            lib.timing_enable(False)
        seen |= {(rec[0], rec[2], rec[4], rec[5]) for rec in recs if rec[0].startswith(("layer_gemm", "dw_"))}
        batches[name] = {k: [rec[3] for rec in recs if rec[0] == k] for k in ("prep_weight", "finish_weight")}      # rows of each launch
        print("%s batched row-job launches (rows): %r" % (name, batches[name]))
    for k in ("prep_weight", "finish_weight"):      # every step of <= 24 layers launches each once per pass that needs it, `deep` twice
        assert len(batches["w48"][k]) > 0 and len(batches["deep"][k]) == 2 * len(batches["w48"][k]) and min(batches["deep"][k]) > 0, (k, batches)
    print("width lattice launch census:")
    for rec in sorted(seen):
        print("    %r," % (rec,))
    ws = [rec for rec in seen if rec[0] == "layer_gemm_ws"]
    assert {96, 128} <= {n for _, _, n, _ in ws}, sorted(ws)
    assert {112, 128, 240} <= {k for _, _, _, k in ws}, sorted(ws)
    assert any(n == 256 and k <= 240 for _, _, n, k in ws), sorted(ws)
    assert any(rec[0] == "layer_gemm" and rec[1] == 3 for rec in seen)
    assert any(rec[0] == "dw_gemm_hx" and (rec[2] < 256 or rec[3] < 256) for rec in seen)      # a partial tile on the split-f16 path
    assert any(rec[0] == "dw_skinny" for rec in seen)
    missing = [rec for rec in CENSUS if rec not in seen]
    assert CENSUS and not missing, missing


# The backward pass's launches under each switch that changes what the host plan fuses, as the ordered (name, kind, nt, P, N, K, pairs) of the
# library's per-launch records, by case of tests/_bwd_sequence_child.py: [(the settings that give this list, the list)].  The CPU emulation never
# takes the sweep0 / narrow_bwd / head / strip forms (its be_*_ok return false), so these states of the plan exist only on the device.
# Recorded on the MI355X from the commit BEFORE the plan (sdf_backward / stack_layer_bwd deciding inline), see profiles/bwd_plan_refactor_ab.txt:
# a later change of the plan that moves, drops or adds a launch fails here.
BWD_SWITCHES = ["default", "CNR_NO_FDW", "CNR_FDW_SPLIT", "CNR_NO_TOP_FUSE", "CNR_NO_SWEEP0", "CNR_NO_NARROW_BWD", "CNR_NO_HEAD_BWD", "CNR_NO_STRIP_BWD"]
BWD_SEQUENCES = {
    'step_A': [
        (('default',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('strip_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 33, 2), ('coltop_bwd', 2, 0, 2048, 0, 0, 0),
            ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 201, 2048, 256, 256, 2), ('strip_bwd', 2, 6, 2048, 256, 6, 1),
            ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('sweep0_dw', 0, 300, 2048, 256, 39, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 217, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 39, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_FDW',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('strip_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm', 0, 2, 2048, 33, 256, 1), ('dw_gemm', 1, 8112, 2048, 256, 33, 1),
            ('coltop_bwd', 2, 0, 2048, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('strip_bwd', 2, 6, 2048, 256, 6, 1), ('gbar_finish', 2, 0, 2048, 0, 0, 0),
            ('layer_gemm_ws', 0, 108, 2048, 256, 39, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 257, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 217, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm', 0, 2, 2048, 39, 256, 1), ('dw_gemm', 1, 8112, 2048, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 2048, 217, 256, 2),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('dw_skinny', 1, 1, 2048, 1, 256, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_FDW_SPLIT',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('strip_bwd', 2, 3, 2048, 256, 3, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('narrow_bwd', 0, 301, 2048, 256, 33, 2), ('coltop_bwd', 2, 0, 2048, 0, 0, 0),
            ('head_bwd', 2, 3, 2048, 256, 3, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('strip_bwd', 2, 6, 2048, 256, 6, 1), ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('sweep0_dw', 0, 300, 2048, 256, 39, 2),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 217, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 257, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 2048, 217, 256, 1),
            ('layer_gemm_ws', 0, 108, 2048, 256, 217, 1), ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('narrow_bwd', 0, 301, 2048, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('dw_skinny', 1, 1, 2048, 1, 256, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0),
            ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_TOP_FUSE',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('strip_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 33, 2), ('coltop_bwd', 2, 0, 2048, 0, 0, 0),
            ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 201, 2048, 256, 256, 2), ('strip_bwd', 2, 6, 2048, 256, 6, 1),
            ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('sweep0_dw', 0, 300, 2048, 256, 39, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_gemm_ws', 0, 108, 2048, 256, 257, 1), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 217, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('dw_skinny', 1, 1, 2048, 1, 256, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0),
            ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_SWEEP0',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('strip_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 33, 2), ('coltop_bwd', 2, 0, 2048, 0, 0, 0),
            ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 201, 2048, 256, 256, 2), ('strip_bwd', 2, 6, 2048, 256, 6, 1),
            ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('layer_gemm_ws', 0, 108, 2048, 256, 39, 1), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 217, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_gemm', 0, 2, 2048, 39, 256, 1),
            ('dw_gemm', 1, 8112, 2048, 256, 39, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 2048, 0, 0, 0),
            ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_NARROW_BWD',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('strip_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_gemm', 0, 2, 2048, 33, 256, 1), ('dw_gemm', 1, 8112, 2048, 256, 33, 1),
            ('coltop_bwd', 2, 0, 2048, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 201, 2048, 256, 256, 2),
            ('strip_bwd', 2, 6, 2048, 256, 6, 1), ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('sweep0_dw', 0, 300, 2048, 256, 39, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 217, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_gemm', 0, 2, 2048, 39, 256, 1), ('dw_gemm', 1, 8112, 2048, 256, 39, 1), ('finish_weight', 2, 0, 4320, 0, 0, 0),
            ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_HEAD_BWD',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('layer_gemm_ws', 0, 108, 2048, 256, 3, 1),
            ('dw_skinny', 1, 1, 2048, 3, 256, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('strip_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 33, 2),
            ('coltop_bwd', 2, 0, 2048, 0, 0, 0), ('layer_gemm_ws', 0, 108, 2048, 256, 3, 1), ('dw_skinny', 1, 1, 2048, 3, 256, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 201, 2048, 256, 256, 2), ('strip_bwd', 2, 6, 2048, 256, 6, 1), ('gbar_finish', 2, 0, 2048, 0, 0, 0),
            ('sweep0_dw', 0, 300, 2048, 256, 39, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 217, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 39, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0),
            ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
        (('CNR_NO_STRIP_BWD',), [
            ('composite_bwd', 2, 0, 64, 0, 0, 0), ('variance_finish', 2, 0, 64, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_gemm', 0, 1, 2048, 3, 256, 1), ('dw_skinny', 1, 2, 2048, 256, 3, 1),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 33, 2),
            ('coltop_bwd', 2, 0, 2048, 0, 0, 0), ('head_bwd', 2, 3, 2048, 256, 3, 1), ('layer_dw', 0, 209, 2048, 256, 256, 2),
            ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_dw', 0, 209, 2048, 256, 256, 2), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
            ('layer_gemm', 0, 1, 2048, 6, 256, 1), ('dw_gemm_hx', 1, 4224, 2048, 256, 256, 1), ('dw_skinny', 1, 2, 2048, 256, 6, 1),
            ('gbar_finish', 2, 0, 2048, 0, 0, 0), ('sweep0_dw', 0, 300, 2048, 256, 39, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2), ('layer_dw', 0, 207, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 217, 2),
            ('layer_dw', 0, 208, 2048, 256, 256, 2), ('layer_dw', 0, 208, 2048, 256, 256, 2), ('narrow_bwd', 0, 301, 2048, 256, 39, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 2048, 0, 0, 0), ('rays_grad_finish', 2, 0, 64, 0, 0, 0),
        ]),
    ],
    'step_B': [
        (('default', 'CNR_FDW_SPLIT', 'CNR_NO_TOP_FUSE'), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 33, 2), ('coltop_bwd', 2, 0, 1407, 0, 0, 0),
            ('head_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('strip_bwd', 2, 6, 1407, 256, 6, 1), ('gbar_finish', 2, 0, 1407, 0, 0, 0), ('sweep0_dw', 0, 300, 1407, 256, 39, 2),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('narrow_bwd', 0, 301, 1407, 256, 39, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('dw_skinny', 1, 1, 1407, 1, 256, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 1407, 0, 0, 0),
            ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
        (('CNR_NO_FDW',), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm', 0, 2, 1407, 33, 256, 1), ('dw_gemm', 1, 8112, 1407, 256, 33, 1),
            ('coltop_bwd', 2, 0, 1407, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 6, 1407, 256, 6, 1), ('gbar_finish', 2, 0, 1407, 0, 0, 0),
            ('layer_gemm_ws', 0, 108, 1407, 256, 39, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm', 0, 2, 1407, 39, 256, 1), ('dw_gemm', 1, 8112, 1407, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 1, 1407, 1, 256, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 1407, 0, 0, 0), ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
        (('CNR_NO_SWEEP0',), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 33, 2), ('coltop_bwd', 2, 0, 1407, 0, 0, 0),
            ('head_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('strip_bwd', 2, 6, 1407, 256, 6, 1), ('gbar_finish', 2, 0, 1407, 0, 0, 0), ('layer_gemm_ws', 0, 108, 1407, 256, 39, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm', 0, 2, 1407, 39, 256, 1), ('dw_gemm', 1, 8112, 1407, 256, 39, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 1, 1407, 1, 256, 2), ('finish_weight', 2, 0, 4320, 0, 0, 0),
            ('pbar_finish', 2, 0, 1407, 0, 0, 0), ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
        (('CNR_NO_NARROW_BWD',), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm', 0, 2, 1407, 33, 256, 1), ('dw_gemm', 1, 8112, 1407, 256, 33, 1),
            ('coltop_bwd', 2, 0, 1407, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 6, 1407, 256, 6, 1), ('gbar_finish', 2, 0, 1407, 0, 0, 0),
            ('sweep0_dw', 0, 300, 1407, 256, 39, 2), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm', 0, 2, 1407, 39, 256, 1), ('dw_gemm', 1, 8112, 1407, 256, 39, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 1, 1407, 1, 256, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 1407, 0, 0, 0), ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
        (('CNR_NO_HEAD_BWD',), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('layer_gemm_ws', 0, 108, 1407, 256, 3, 1),
            ('dw_skinny', 1, 1, 1407, 3, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('strip_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 33, 2),
            ('coltop_bwd', 2, 0, 1407, 0, 0, 0), ('layer_gemm_ws', 0, 108, 1407, 256, 3, 1), ('dw_skinny', 1, 1, 1407, 3, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('strip_bwd', 2, 6, 1407, 256, 6, 1),
            ('gbar_finish', 2, 0, 1407, 0, 0, 0), ('sweep0_dw', 0, 300, 1407, 256, 39, 2), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 1, 1407, 1, 256, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 1407, 0, 0, 0), ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
        (('CNR_NO_STRIP_BWD',), [
            ('composite_bwd', 2, 0, 67, 0, 0, 0), ('variance_finish', 2, 0, 67, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm', 0, 1, 1407, 3, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('dw_skinny', 1, 2, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 33, 2),
            ('coltop_bwd', 2, 0, 1407, 0, 0, 0), ('head_bwd', 2, 3, 1407, 256, 3, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm', 0, 1, 1407, 6, 256, 1), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 2, 1407, 256, 6, 1),
            ('gbar_finish', 2, 0, 1407, 0, 0, 0), ('sweep0_dw', 0, 300, 1407, 256, 39, 2), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 257, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 217, 1),
            ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('layer_gemm_ws', 0, 108, 1407, 256, 256, 1), ('narrow_bwd', 0, 301, 1407, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 217, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 1407, 256, 256, 1), ('dw_skinny', 1, 1, 1407, 1, 256, 2),
            ('finish_weight', 2, 0, 4320, 0, 0, 0), ('pbar_finish', 2, 0, 1407, 0, 0, 0), ('rays_grad_finish', 2, 0, 67, 0, 0, 0),
        ]),
    ],
    'query_want_grad_0': [
        (('default', 'CNR_NO_TOP_FUSE', 'CNR_NO_SWEEP0', 'CNR_NO_NARROW_BWD', 'CNR_NO_HEAD_BWD', 'CNR_NO_STRIP_BWD'), [
            ('query_seed', 2, 0, 8704, 0, 0, 0), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 217, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 1), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1),
            ('dw_skinny', 1, 1, 128, 1, 256, 1), ('finish_weight', 2, 0, 2266, 0, 0, 0), ('pbar_finish', 2, 0, 128, 0, 0, 0),
            ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_NO_FDW',), [
            ('query_seed', 2, 0, 8704, 0, 0, 0), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 217, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 1), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 128, 217, 256, 1), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_skinny', 1, 1, 128, 1, 256, 1), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_FDW_SPLIT',), [
            ('query_seed', 2, 0, 8704, 0, 0, 0), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 217, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 217, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 1),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_skinny', 1, 1, 128, 1, 256, 1), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
    ],
    'query_want_grad_1': [
        (('default', 'CNR_NO_HEAD_BWD', 'CNR_NO_STRIP_BWD'), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('sweep0_dw', 0, 300, 128, 256, 39, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 217, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('narrow_bwd', 0, 301, 128, 256, 39, 2), ('finish_weight', 2, 0, 2266, 0, 0, 0), ('pbar_finish', 2, 0, 128, 0, 0, 0),
            ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_NO_FDW',), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('layer_gemm_ws', 0, 108, 128, 256, 39, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 217, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 2), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 128, 217, 256, 2), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 2),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_skinny', 1, 1, 128, 1, 256, 2), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_FDW_SPLIT',), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('sweep0_dw', 0, 300, 128, 256, 39, 2),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 217, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 128, 217, 256, 1),
            ('layer_gemm_ws', 0, 108, 128, 256, 217, 1), ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1),
            ('dw_gemm_bx', 1, 4224, 128, 256, 256, 1), ('layer_gemm_ws', 0, 108, 128, 256, 256, 1), ('narrow_bwd', 0, 301, 128, 256, 39, 2),
            ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_skinny', 1, 1, 128, 1, 256, 2), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_NO_TOP_FUSE',), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('sweep0_dw', 0, 300, 128, 256, 39, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_gemm_ws', 0, 108, 128, 256, 257, 1), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 217, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('narrow_bwd', 0, 301, 128, 256, 39, 2), ('dw_gemm_hx', 1, 4224, 128, 256, 256, 1), ('dw_skinny', 1, 1, 128, 1, 256, 2),
            ('finish_weight', 2, 0, 2266, 0, 0, 0), ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_NO_SWEEP0',), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('layer_gemm_ws', 0, 108, 128, 256, 39, 1),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 217, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 2), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
        (('CNR_NO_NARROW_BWD',), [
            ('query_seed', 2, 0, 8832, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('sweep0_dw', 0, 300, 128, 256, 39, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 207, 128, 256, 256, 2),
            ('layer_dw', 0, 207, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_dw', 0, 208, 128, 256, 217, 2), ('layer_dw', 0, 208, 128, 256, 256, 2), ('layer_dw', 0, 208, 128, 256, 256, 2),
            ('layer_gemm', 0, 2, 128, 39, 256, 1), ('dw_gemm', 1, 8112, 128, 256, 39, 1), ('finish_weight', 2, 0, 2266, 0, 0, 0),
            ('pbar_finish', 2, 0, 128, 0, 0, 0), ('query_out', 2, 0, 192, 0, 0, 0),
        ]),
    ],
}


_CHILD_DIED = []     # the setting whose child died with a signal or ran into its time limit: no further child is started on the device


@pytest.mark.gpu
@pytest.mark.parametrize("setting", BWD_SWITCHES)
def test_backward_launch_sequence_per_switch(setting, tmp_path):
    """One training step of the DTU-width Color-NeuS configuration with d_rays requested at shape A (2048 points, full tiles: every fused
    form) and shape B (1407 points, P % 32 = 31: every fallback), and one point-query backward of 64 points with want_grad 0 and 1, in one
    child process per switch setting (the library reads the switches once per process), one at a time: the whole ordered list of backward
    launch records equals the recorded one.  After a child that died with a signal or ran into its time limit the remaining settings fail
    without starting theirs."""
    import json
    import subprocess
    import sys
    assert not _CHILD_DIED, ("no child started: the child of an earlier setting died or hung", _CHILD_DIED)
    assert sorted(s for groups in BWD_SEQUENCES.values() for names, _ in groups for s in names) == sorted(BWD_SWITCHES * len(BWD_SEQUENCES))
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_bwd_sequence_child.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CNR_")}
    if setting != "default":
        env[setting] = "1"
    out = os.path.join(str(tmp_path), setting + ".json")
    try:
        r = subprocess.run([sys.executable, child, out], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append(setting)
        raise
    if r.returncode < 0:
        _CHILD_DIED.append(setting)
    assert r.returncode == 0, (setting, r.returncode, r.stdout[-1500:] + r.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert set(got) == set(BWD_SEQUENCES), (setting, sorted(got))
    for case, groups in BWD_SEQUENCES.items():
        want = next(seq for names, seq in groups if setting in names)
        recs = [tuple(rec) for rec in got[case]]
        print("%s / %s: %d launches" % (setting, case, len(recs)))
        assert recs == want, (setting, case, [(i, a, b) for i, (a, b) in enumerate(zip(recs, want)) if a != b][:3], len(recs), len(want))


# Ordered launch records of the entry points that test_backward_launch_sequence_per_switch does not cover, under the default environment:
# recorded with tests/_entry_sequence_child.py on the library of the commit before the host plan was split into units (cnr_plan.h).
ENTRY_SEQUENCES = {
    'background_forward': [
        ('prep_weight', 2, 0, 2496, 0, 0, 0), ('split_planes', 2, 0, 5408, 0, 0, 0), ('bg_embed', 2, 0, 640, 0, 0, 0),
        ('layer_gemm_ws', 0, 108, 640, 256, 84, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm', 0, 8, 640, 256, 340, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm', 0, 1, 640, 1, 256, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('layer_gemm', 0, 4, 640, 128, 283, 1), ('layer_gemm', 0, 1, 640, 3, 128, 1),
        ('bg_alpha', 2, 0, 640, 0, 0, 0),
    ],
    'background_backward': [
        ('bg_heads_bwd', 2, 0, 640, 0, 0, 0), ('dw_skinny', 1, 1, 640, 3, 128, 1), ('layer_gemm', 0, 4, 640, 128, 3, 1),
        ('dw_gemm_bx', 1, 4224, 640, 128, 256, 1), ('dw_gemm', 1, 8112, 640, 128, 27, 1), ('layer_gemm_ws', 0, 108, 640, 256, 128, 1),
        ('layer_gemm', 0, 1, 640, 27, 128, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('dw_skinny', 1, 1, 640, 1, 256, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('bg_join', 2, 0, 163840, 0, 0, 0), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1),
        ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 84, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1),
        ('layer_gemm', 0, 3, 640, 84, 256, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1),
        ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1),
        ('layer_gemm_ws', 0, 108, 640, 256, 256, 1), ('dw_gemm_bx', 1, 4224, 640, 256, 256, 1), ('layer_gemm_ws', 0, 108, 640, 256, 256, 1),
        ('dw_gemm_bx', 1, 4224, 640, 256, 84, 1), ('layer_gemm', 0, 3, 640, 84, 256, 1), ('finish_weight', 2, 0, 2436, 0, 0, 0),
        ('bg_embed_bwd', 2, 0, 640, 0, 0, 0), ('bg_rays_bwd', 2, 0, 16, 0, 0, 0),
    ],
    'forward_only_prune_tiny_sharp': [
        ('prep_weight', 2, 0, 544, 0, 0, 0), ('split_planes', 2, 0, 1184, 0, 0, 0), ('pack_frags', 2, 0, 176, 0, 0, 0),
        ('embed_z', 2, 0, 256, 0, 0, 0), ('layer_gemm', 0, 2, 256, 64, 39, 1), ('layer_gemm', 0, 2, 256, 64, 64, 1),
        ('layer_gemm', 0, 1, 256, 1, 64, 1), ('sampler_step', 2, 0, 16, 0, 0, 0), ('layer_gemm', 0, 2, 64, 64, 39, 1),
        ('layer_gemm', 0, 2, 64, 64, 64, 1), ('layer_gemm', 0, 1, 64, 1, 64, 1), ('sampler_step', 2, 0, 16, 0, 0, 0),
        ('layer_gemm', 0, 2, 64, 64, 39, 1), ('layer_gemm', 0, 2, 64, 64, 64, 1), ('layer_gemm', 0, 1, 64, 1, 64, 1),
        ('sampler_step', 2, 0, 16, 0, 0, 0), ('layer_gemm', 0, 2, 64, 64, 39, 1), ('layer_gemm', 0, 2, 64, 64, 64, 1),
        ('layer_gemm', 0, 1, 64, 1, 64, 1), ('sampler_step', 2, 0, 16, 0, 0, 0), ('merge', 2, 0, 16, 0, 0, 0), ('fine_setup', 2, 0, 512, 0, 0, 0),
        ('layer_gemm', 0, 2, 512, 64, 39, 1), ('layer_gemm', 0, 2, 512, 64, 64, 1), ('layer_gemm', 0, 1, 512, 1, 64, 1),
        ('layer_gemm', 0, 2, 512, 64, 64, 1), ('layer_gemm', 0, 2, 512, 64, 64, 1), ('layer_gemm', 0, 2, 512, 39, 64, 1),
        ('grad_finish', 2, 0, 512, 0, 0, 0), ('composite_fwd', 2, 0, 16, 0, 0, 0), ('prune_count', 2, 0, 16, 0, 0, 0),
        ('prune_scan', 2, 0, 16, 0, 0, 0), ('prune_gather', 2, 0, 16, 0, 0, 0), ('layer_gemm', 0, 2, 512, 64, 70, 1),
        ('layer_gemm', 0, 2, 512, 64, 64, 1), ('layer_gemm', 0, 1, 512, 3, 64, 1), ('layer_gemm', 0, 2, 512, 64, 33, 1),
        ('layer_gemm', 0, 2, 512, 64, 67, 1), ('layer_gemm', 0, 1, 512, 3, 64, 1), ('prune_scatter', 2, 0, 512, 0, 0, 0),
        ('composite_fwd', 2, 0, 16, 0, 0, 0), ('reduce_eik', 2, 0, 16, 0, 0, 0),
    ],
    'forward_only_prune_dtu_sharp': [
        ('prep_weight', 2, 0, 4448, 0, 0, 0), ('split_planes', 2, 0, 8992, 0, 0, 0), ('pack_frags', 2, 0, 3968, 0, 0, 0),
        ('embed_z', 2, 0, 1024, 0, 0, 0), ('chain_sdf_value', 3, 12, 1024, 1840, 256, 1), ('sampler_step', 2, 0, 16, 0, 0, 0),
        ('chain_sdf_value', 3, 12, 256, 1840, 256, 1), ('sampler_step', 2, 0, 16, 0, 0, 0), ('chain_sdf_value', 3, 12, 256, 1840, 256, 1),
        ('sampler_step', 2, 0, 16, 0, 0, 0), ('chain_sdf_value', 3, 12, 256, 1840, 256, 1), ('sampler_step', 2, 0, 16, 0, 0, 0),
        ('merge', 2, 0, 16, 0, 0, 0), ('fine_setup', 2, 0, 2048, 0, 0, 0), ('chain_sdf_fwd', 3, 11, 2048, 2096, 256, 1),
        ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
        ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 217, 1), ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1),
        ('layer_gemm_ws', 0, 108, 2048, 256, 256, 1), ('narrow_dx', 0, 301, 2048, 39, 256, 1), ('grad_finish', 2, 0, 2048, 0, 0, 0),
        ('composite_fwd', 2, 0, 16, 0, 0, 0), ('prune_count', 2, 0, 16, 0, 0, 0), ('prune_scan', 2, 0, 16, 0, 0, 0),
        ('prune_gather', 2, 0, 16, 0, 0, 0), ('chain_fwd', 3, 11, 2048, 1872, 256, 1), ('composite_fwd', 2, 0, 16, 0, 0, 0),
        ('reduce_eik', 2, 0, 16, 0, 0, 0),
    ],
    'extract_color': [
        ('prep_weight', 2, 0, 544, 0, 0, 0), ('split_planes', 2, 0, 1184, 0, 0, 0), ('pack_frags', 2, 0, 176, 0, 0, 0),
        ('embed_pts', 2, 0, 37, 0, 0, 0), ('layer_gemm', 0, 2, 37, 64, 39, 1), ('layer_gemm', 0, 2, 37, 64, 64, 1),
        ('layer_gemm', 0, 1, 37, 1, 64, 1), ('layer_gemm', 0, 2, 37, 64, 64, 1), ('layer_gemm', 0, 2, 37, 64, 64, 1),
        ('layer_gemm', 0, 2, 37, 39, 64, 1), ('grad_finish', 2, 0, 37, 0, 0, 0), ('layer_gemm', 0, 2, 37, 64, 70, 1),
        ('layer_gemm', 0, 2, 37, 64, 64, 1), ('layer_gemm', 0, 1, 37, 3, 64, 1),
    ],
    'extract_fields': [
        ('prep_weight', 2, 0, 224, 0, 0, 0), ('split_planes', 2, 0, 416, 0, 0, 0), ('pack_frags', 2, 0, 176, 0, 0, 0),
        ('embed_pts', 2, 0, 512, 0, 0, 0), ('layer_gemm', 0, 2, 512, 64, 39, 1), ('layer_gemm', 0, 2, 512, 64, 64, 1),
        ('layer_gemm', 0, 1, 512, 1, 64, 1),
    ],
    'query_forward': [
        ('prep_weight', 2, 0, 224, 0, 0, 0), ('split_planes', 2, 0, 416, 0, 0, 0), ('pack_frags', 2, 0, 176, 0, 0, 0),
        ('query_in', 2, 0, 384, 0, 0, 0), ('embed_pts', 2, 0, 128, 0, 0, 0), ('layer_gemm', 0, 2, 128, 64, 39, 1),
        ('layer_gemm', 0, 2, 128, 64, 64, 1), ('layer_gemm', 0, 1, 128, 1, 64, 1), ('layer_gemm', 0, 2, 128, 64, 64, 1),
        ('layer_gemm', 0, 2, 128, 64, 64, 1), ('layer_gemm', 0, 2, 128, 39, 64, 1), ('grad_finish', 2, 0, 128, 0, 0, 0),
        ('query_out', 2, 0, 148, 0, 0, 0),
    ],
    'query_backward': [
        ('query_seed', 2, 0, 2688, 0, 0, 0), ('gbar_finish', 2, 0, 128, 0, 0, 0), ('layer_gemm', 0, 2, 128, 64, 39, 1),
        ('layer_gemm', 0, 2, 128, 64, 64, 1), ('layer_gemm', 0, 2, 128, 64, 65, 1), ('layer_gemm', 0, 2, 128, 64, 64, 1),
        ('layer_gemm', 0, 2, 128, 39, 64, 1), ('dw_gemm', 1, 8112, 128, 64, 39, 2), ('dw_gemm', 1, 8112, 128, 64, 64, 2),
        ('dw_gemm', 1, 8112, 128, 65, 64, 2), ('finish_weight', 2, 0, 193, 0, 0, 0), ('pbar_finish', 2, 0, 128, 0, 0, 0),
        ('query_out', 2, 0, 111, 0, 0, 0),
    ],
}


@pytest.mark.gpu
def test_entry_point_launch_sequences(tmp_path):
    """Background forward + backward (tiny_outside, 16 rays), a forward-only render with prune_eps > 0 in both forms (tiny_sharp: compact
    copies + per-layer chains; dtu_sharp: the chain-fused launch through the index list; 16 rays each), extract_color on 37 vertices,
    extract_fields at resolution 8 and a point-query forward + backward with want_grad at 37 points, in one child process: the whole
    ordered list of launch records of every call equals the recorded one.  (The CPU emulation records no launches: GPU only.)"""
    import json
    import subprocess
    import sys
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_entry_sequence_child.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("CNR_")}
    out = os.path.join(str(tmp_path), "entries.json")
    r = subprocess.run([sys.executable, child, out], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-1500:] + r.stderr[-3000:])
    with open(out) as f:
        got = json.load(f)
    assert set(got) == set(ENTRY_SEQUENCES), sorted(got)
    for case, want in ENTRY_SEQUENCES.items():
        recs = [tuple(rec) for rec in got[case]]
        print("%s: %d launches" % (case, len(recs)))
        assert recs == want, (case, [(i, a, b) for i, (a, b) in enumerate(zip(recs, want)) if a != b][:3], len(recs), len(want))
