"""Every entry point on exact-size, poisoned, guarded buffers (tests/_guard.py).

The C interface's contract is that the caller owns all memory and a ``*_bytes`` query gives the size of a context / scratch buffer.  Three
things follow, and each case below checks them through the product route:

1. a size query is honest: no launch writes outside [base, base + bytes) -- the buffers come from ``_guard`` with 64 KiB of guard bytes on
   either side, the payload exactly as long as the query said;
2. the library writes everything it reads: the payload starts as 0xFF (NaN / -1) in one run and 0x00 in another, and the results of both
   equal those of a plainly allocated run TO THE BIT (the rule of test_results_do_not_depend_on_scratch_contents -- no tolerance);
3. buffers with a documented zero contract (the loss scratch) start zero and are all zero again after the call.

Each case is a function ``(library, device, guard, *args) -> {name: tensor}``; ``_run`` calls it three times -- guarded 0xFF, guarded
0x00, plain -- and holds the 0xFF run to the existing modules' own references, their rules and tolerances, nothing new: either the module's
helper runs once more under the 0xFF guard (``gate``: render, sdf / colour evaluation, point queries, background, compositor, loss, optimiser, ray
backward), or its reference is applied to the results of the 0xFF run (``check``: nearest neighbours, image metrics and panel, cameras, linear;
marching cubes, rasteriser and pixel table inside the case).  Without one, by lack of a reference in any module: the idr vertex colours, the loss
at 1025 rays, the loss-only / with-samples / sampler render layouts and the forward-only entry point (bitwise against the plain run, which the
existing modules tie to the saving forward).  The last tests assert that the guarded runs of this module met EVERY size
function of the binding (``_lib.SIGNATURES``): a new entry point with a size function fails there until it has a case.

The direct-call tests at the end (``test_direct_*``) put the typed INPUTS and OUTPUTS of the row-storing entry points into guarded tensors
as well: 0xFF around an input (a row read past its end is NaN), guard bytes around an output."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _guard
import _native as N
import color_neus_amd as cn
from color_neus_amd import _lib
from color_neus_amd._lib import param_array, ptr, stream_of

EMU = ("emu", N.EMU_LIB, "cpu")
HIP = ("hip", None, "cuda:0")
SEEN = {"emu": set(), "hip": set()}       # size functions met by the guarded runs, per build
_DONE = set()                             # (build, family name, args) of the cases that ran
REGISTRY = []                             # (family, args) of every case of section 2: the coverage tests run what has not run


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def _same_bits(name, a, b, what):
    assert set(a) == set(b), (name, what, set(a) ^ set(b))
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (name, what, k)
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            x, y = a[k].detach().cpu().reshape(-1), b[k].detach().cpu().reshape(-1)
            diff = (_bits(a[k]).reshape(x.numel(), -1) != _bits(b[k]).reshape(x.numel(), -1)).any(dim=1).nonzero().reshape(-1)
            raise AssertionError("%s: %s differs from the plain run under %s: %d of %d entries, first at %d (%r vs %r)"
                                 % (name, k, what, diff.numel(), x.numel(), int(diff[0]), x[int(diff[0])].item(), y[int(diff[0])].item()))


def _fresh_caches():
    """Scratch buffers the package keeps between calls are dropped, so that a guarded run allocates its own (and a later plain run too)."""
    from color_neus_amd import loss
    loss._SCRATCH.clear()


def _guarded_call(fn, fill):
    g = _guard.Guard(fill)
    _fresh_caches()
    try:
        with g.scratch_substituted():
            res = fn(g)
            g.check()
    finally:
        _fresh_caches()
    return res, g


def _run(build, family, *args, gate=None, check=None):
    """The three runs of one case and their assertions.  ``gate(library, device)``: an existing module's own helper that calls the library and checks
    by itself, run once more under the 0xFF guard; ``check(results)``: an existing module's reference applied to the results of the 0xFF run."""
    tag, library, dev = build
    if tag == "emu" and not os.path.isfile(N.EMU_LIB):
        pytest.skip("emulation library not built")
    name = "%s%r" % (family.__name__, args)
    # the guarded runs come first: a store outside a buffer is then reported by check() before any run could put it into memory that
    # belongs to something else
    res = {}
    for fill in (_guard.POISON, 0x00):
        res[fill], g = _guarded_call(lambda g: family(library, dev, g, *args), fill)
        SEEN[tag] |= g.names
    _fresh_caches()
    plain = family(library, dev, None, *args)
    assert plain and all(torch.is_tensor(v) for v in plain.values()), name
    for fill in (_guard.POISON, 0x00):
        _same_bits(name, plain, res[fill], "payload 0x%02X" % fill)
    if check is not None:
        check(res[_guard.POISON])
    if gate is not None:
        _, g = _guarded_call(lambda g: gate(library, dev), _guard.POISON)
        SEEN[tag] |= g.names
    _DONE.add((tag, family.__name__, args))


def _cases(family, argslist):
    REGISTRY.extend((family, a) for a in argslist)
    return argslist


def _coef(t):
    """A fixed cotangent of t's shape (no generator state: the three runs of a case see the same one)."""
    return torch.cos(torch.arange(t.numel(), dtype=torch.float32) * 0.37 + 0.1).reshape(t.shape).to(t.device)


# =====================================================================================================================================
# the render path
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _render_inputs(cfg_name, shape):
    """(oracle config, weights, batch, z_vals) of a render case, computed once and never modified.  ``shape``: a ray count for the DTU
    configurations of test_edge_batches (its _config / _batch recipe), "B" for the lattice configurations of test_width_lattice
    (67 rays x (12 + 9) samples: 1407 points, P % 32 = 31)."""
    from oracle import colorneus_oracle as O
    import test_edge_batches as EB
    import test_width_lattice as WL
    if shape == "B":
        R, ns, ni, steps = WL.SHAPES["B"]
        ocfg = WL.CONFIGS[cfg_name]()
        ocfg.n_samples, ocfg.n_importance, ocfg.up_sample_steps = ns, ni, steps
        batch = WL._batch(R, WL.SEEDS[cfg_name, "B"])
    else:
        ocfg = EB._config(cfg_name)
        batch = EB._batch(shape, 100 + shape)
    P = O.init_params(ocfg, seed=5, trained_like=True)
    o, d, near, far, t_rand, gt, mask = batch
    z = O.sample_z(P, ocfg, o, d, near, far, t_rand)
    return ocfg, P, batch, z


def _render(library, dev, g, cfg_name, shape, mode):
    """Render forward + backward.  mode: "saving" (the training dict, compute_loss), "loss_only" (training_outputs="loss_only", the fused
    loss), "with_samples" (the per-sample network outputs the N_OUTSIDE mixing takes; a fixed cotangent on every output), "sampler"
    (saving, no z_vals: the hierarchical sampler's scratch is live)."""
    from color_neus_amd import renderer as RR
    ocfg, P, (o, d, near, far, t_rand, gt, mask), z = _render_inputs(cfg_name, shape)
    r = N.make_renderer(ocfg, P, library, dev)
    dv = lambda t: t.to(dev)
    og, dg = dv(o).clone().requires_grad_(True), dv(d).clone().requires_grad_(True)      # (clone: on the CPU .to() is the cached tensor itself)
    if mode == "with_samples":
        params = r._ordered_params()
        res = RR._RenderFunction.apply(r, og, dg, dv(near), dv(far), None, dv(z), None, 0.0, 0.0, True, *params)
        out = {"out%d" % i: t for i, t in enumerate(res)}
        loss = sum((t * _coef(t)).sum() for t in res if t.requires_grad)
    elif mode == "loss_only":
        out = r(og, dg, dv(near), dv(far), z_vals=dv(z), training_outputs="loss_only")
        loss, _ = cn.compute_loss_fused(out, dv(gt), dv(mask), library=r._lib)
    elif mode == "sampler":
        out = r(og, dg, dv(near), dv(far), t_rand=t_rand)
        loss, _ = cn.compute_loss(out, dv(gt), dv(mask))
    else:
        out = r(og, dg, dv(near), dv(far), z_vals=dv(z))
        loss, _ = cn.compute_loss(out, dv(gt), dv(mask))
    loss.backward()
    res = {"out:" + k: v.detach() for k, v in out.items()}
    res["loss"] = loss.detach()
    res.update({"grad:" + k: p.grad for k, p in r.named_parameters() if p.grad is not None})
    res["grad:rays_o"], res["grad:rays_d"] = og.grad, dg.grad
    return res


def _gate_edge(R, cfg_name):
    """test_edge_batches' own float64 gate on the same configuration and rays (the helper renders and checks by itself)"""
    import test_edge_batches as EB
    return lambda library, dev: EB._check(R, library, torch.device(dev), cfg_name)


def _gate_lattice(name):
    """test_width_lattice's own gate (strict on the HIP build, loose on the emulation, as in that module)"""
    import test_width_lattice as WL
    return lambda library, dev: WL._check(name, "B", library, torch.device(dev), strict=library is None)


# DTU at 33 rays x (64 + 64): P = 4224, full tiles, the fused 256-wide launches, 7 empty partial-sum slots of 40; at 3 rays 6 of 8 slots are
# used; w48 / mixed / w208 / neus176 at shape B: the general layer kernel, the 3-tile kernel, tail fill behind an 89- or 9-wide skip layer,
# a ragged last tile everywhere; dtu_pe4: K padded from 27 to 32
RENDER = _cases(_render, [("dtu", 33, "saving"), ("dtu", 33, "loss_only"), ("dtu", 33, "with_samples"), ("dtu", 33, "sampler"),
                          ("dtu", 3, "saving"), ("dtu", 3, "loss_only"), ("dtu", 3, "with_samples"),
                          ("w48", "B", "saving"), ("w48", "B", "loss_only"), ("w48", "B", "with_samples"),
                          ("mixed", "B", "saving"), ("mixed", "B", "loss_only"), ("mixed", "B", "with_samples"),
                          ("w208", "B", "saving"), ("w208", "B", "loss_only"), ("w208", "B", "with_samples"),
                          ("dtu_pe4", 33, "saving"), ("dtu_pe4", 33, "loss_only"), ("dtu_pe4", 33, "with_samples"),
                          ("neus176", "B", "saving"), ("neus176", "B", "loss_only"), ("neus176", "B", "with_samples")])


def _render_gate(build, cfg_name, shape, mode):
    if mode != "saving":
        return None
    if shape == "B":
        return _gate_lattice(cfg_name)
    # the emulation build has its float64 gate at the tiny configuration only (test_edge_batches_emu); the DTU widths are gated on the HIP build
    return _gate_edge(shape, cfg_name) if build[0] == "hip" else None


@pytest.mark.parametrize("cfg_name,shape,mode", RENDER)
def test_render_emu(cfg_name, shape, mode):
    _run(EMU, _render, cfg_name, shape, mode, gate=_render_gate(EMU, cfg_name, shape, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,shape,mode", RENDER)
def test_render_hip(cfg_name, shape, mode):
    _run(HIP, _render, cfg_name, shape, mode, gate=_render_gate(HIP, cfg_name, shape, mode))


def _forward_only(library, dev, g, prune_eps):
    """cnr_render_forward_only at 33 rays (prune_eps 0 and > 0) and cnr_sample_z on the same rays"""
    ocfg, P, (o, d, near, far, t_rand, gt, mask), z = _render_inputs("dtu", 33)
    r = N.make_renderer(ocfg, P, library, dev)
    dv = lambda t: t.to(dev)
    with torch.no_grad():
        out = r(dv(o), dv(d), dv(near), dv(far), z_vals=dv(z), prune_eps=prune_eps)
        zs = r._sample_z(dv(o), dv(d), dv(near), dv(far), dv(t_rand))
    res = {"out:" + k: v for k, v in out.items()}
    res["sample_z"] = zs
    return res


FORWARD_ONLY = _cases(_forward_only, [(0.0,), (1e-3,)])


@pytest.mark.parametrize("prune_eps", [a[0] for a in FORWARD_ONLY])
def test_forward_only_and_sample_z_emu(prune_eps):
    _run(EMU, _forward_only, prune_eps)


@pytest.mark.gpu
@pytest.mark.parametrize("prune_eps", [a[0] for a in FORWARD_ONLY])
def test_forward_only_and_sample_z_hip(prune_eps):
    _run(HIP, _forward_only, prune_eps)


# =====================================================================================================================================
# evaluation: sdf, lattice, slab, vertex colours, marching cubes
# =====================================================================================================================================
def _eval_renderer(cfg_name, library, dev):
    shape = "B" if cfg_name == "neus176" else 33
    ocfg, P, _, _ = _render_inputs(cfg_name, shape)
    return N.make_renderer(ocfg, P, library, dev)


def _pts(n, seed=3):
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)) * 2.0 - 1.0


def _sdf_eval(library, dev, g, n):
    r = _eval_renderer("dtu", library, dev)
    pts = _pts(n).to(dev)
    if g is not None:
        pts = g.copy(pts, "cnr_sdf_eval points")
    return {"sdf": r.sdf(pts), "sdf_module": r.sdf_network.sdf(pts).detach()}


def _gate_eval(build, n):
    """test_edge_batches._check_eval_sizes (sdf() against the float64 oracle at 1e-4, sdf / extract_color prefixes against the full query) at
    this size, on the configuration that module gates each build at: DTU on the HIP build, tiny on the emulation"""
    import test_edge_batches as EB
    cfg_name = "dtu" if build[0] == "hip" else "tiny"
    return lambda library, dev: EB._check_eval_sizes(library, torch.device(dev), cfg_name, [n])


SDF_EVAL = _cases(_sdf_eval, [(1,), (33,), (4097,)])


@pytest.mark.parametrize("n", [a[0] for a in SDF_EVAL])
def test_sdf_eval_emu(n):
    _run(EMU, _sdf_eval, n, gate=_gate_eval(EMU, n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [a[0] for a in SDF_EVAL])
def test_sdf_eval_hip(n):
    _run(HIP, _sdf_eval, n, gate=_gate_eval(HIP, n))


def _grids(library, dev, g):
    """cnr_sdf_grid at resolution 13, cnr_sdf_grid_slab on x in [3, 7) (it equals the lattice's rows) and on an empty slab (refused)"""
    r = _eval_renderer("dtu", library, dev)
    b0, b1 = [-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]
    u = r.extract_fields(b0, b1, dev, 13)
    slab = r.extract_fields_slab(b0, b1, dev, 13, 3, 7)
    # an empty slab is refused with a message (parallel.sharded_extract_fields never asks for one): its scratch query says 0 bytes, and the
    # refused call writes nothing -- the zero-length guarded payload's neighbours are checked like every other buffer's
    with pytest.raises(RuntimeError, match="x_begin < x_end"):
        r.extract_fields_slab(b0, b1, dev, 13, 5, 5)
    assert torch.equal(_bits(slab), _bits(u[3:7])), "a slab holds the lattice's own rows"
    return {"grid": u, "slab": slab}


GRIDS = _cases(_grids, [()])


def test_sdf_grid_and_slab_emu():
    _run(EMU, _grids)


@pytest.mark.gpu
def test_sdf_grid_and_slab_hip():
    _run(HIP, _grids)


def _vertex_color(library, dev, g, cfg_name, n):
    r = _eval_renderer(cfg_name, library, dev)
    pts = _pts(n, seed=5).to(dev) * 0.7
    if g is not None:
        pts = g.copy(pts, "cnr_vertex_color points")
    return {"rgb": r.vertex_colors(pts)}


# dtu: Color_NeuS, no_view_dir; neus176: NeuS, idr (the view branch).  Gate: _check_eval_sizes as above (it queries extract_color too); no existing
# module holds a float64 reference of the vertex colours, so the idr cases have the bitwise rule alone
VERTEX_COLOR = _cases(_vertex_color, [("dtu", 1), ("dtu", 33), ("neus176", 1), ("neus176", 33)])


@pytest.mark.parametrize("cfg_name,n", VERTEX_COLOR)
def test_vertex_color_emu(cfg_name, n):
    _run(EMU, _vertex_color, cfg_name, n, gate=_gate_eval(EMU, n) if cfg_name == "dtu" else None)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,n", VERTEX_COLOR)
def test_vertex_color_hip(cfg_name, n):
    _run(HIP, _vertex_color, cfg_name, n, gate=_gate_eval(HIP, n) if cfg_name == "dtu" else None)


def _sphere_lattice(res, dev):
    import test_marching_cubes as MC
    return MC._lattice(res, lambda x, y, z: 0.6 - torch.sqrt(x * x + y * y + z * z), dev)


def _marching_cubes(library, dev, g):
    """cnr_mc_count / cnr_mc_emit at resolution 13 on the sphere of test_marching_cubes (and its closed-surface check)"""
    import test_marching_cubes as MC
    r = _eval_renderer("dtu", library, dev)
    u = _sphere_lattice(13, dev)
    if g is not None:
        u = g.copy(u, "lattice")
    v, t = r.marching_cubes(u, [-1, -1, -1], [1, 1, 1], 0.0)
    assert MC._mesh_checks(v.cpu().numpy().astype(np.float64), t.cpu().numpy()) == 2
    return {"vertices": v, "triangles": t}


MARCHING = _cases(_marching_cubes, [()])


def test_marching_cubes_emu():
    _run(EMU, _marching_cubes)


@pytest.mark.gpu
def test_marching_cubes_hip():
    _run(HIP, _marching_cubes)


# =====================================================================================================================================
# differentiable SDF point queries
# =====================================================================================================================================
def _sdf_query(library, dev, g, n, want_grad):
    import test_sdf_query as SQ
    r = _eval_renderer("dtu", library, dev)
    net = r.sdf_network
    x = SQ._points(n).float().to(dev)
    if g is not None:
        x = g.copy(x, "cnr_sdf_query points")
    x.requires_grad_(True)
    r.zero_grad(set_to_none=True)
    out = net(x)                                        # sdf + features: want_grad 0
    loss = (out * _coef(out)).sum()
    res = {"sdf_feat": out.detach()}
    if want_grad:
        gr = net.gradient(x)                            # want_grad 1, with the second-order backward
        res["gradient"] = gr.detach()
        loss = loss + (gr * _coef(gr)).sum() + ((gr.norm(dim=-1) - 1.0) ** 2).mean()
    loss.backward()
    res["grad:x"] = x.grad
    res.update({"grad:" + k: p.grad for k, p in net.named_parameters() if p.grad is not None})
    return res


def _gate_query(build, n, want_grad):
    """test_sdf_query._check_forward (1e-4 against the float64 oracle) and _check_backward (the strict check_grads_full rule) at this size, on
    the configuration that module gates each build at: DTU on the HIP build, mid on the emulation"""
    import _golden as G
    import test_sdf_query as SQ
    from oracle import colorneus_oracle as O

    def gate(library, dev):
        ocfg = O.dtu_config() if build[0] == "hip" else G.mid_config()
        SQ._check_forward(ocfg, build[0], n, seed=n)
        SQ._check_backward(ocfg, build[0], n, SQ.TERMS["all"] if want_grad else ("a", "B"), seed=n)
    return gate


SDF_QUERY = _cases(_sdf_query, [(n, wg) for n in (1, 33, 129) for wg in (0, 1)])


@pytest.mark.parametrize("n,want_grad", SDF_QUERY)
def test_sdf_query_emu(n, want_grad):
    _run(EMU, _sdf_query, n, want_grad, gate=_gate_query(EMU, n, want_grad))


@pytest.mark.gpu
@pytest.mark.parametrize("n,want_grad", SDF_QUERY)
def test_sdf_query_hip(n, want_grad):
    _run(HIP, _sdf_query, n, want_grad, gate=_gate_query(HIP, n, want_grad))


# =====================================================================================================================================
# one plain layer
# =====================================================================================================================================
LINEAR_SHAPES = [(5, 7, True), (84, 256, True), (340, 256, True), (272, 224, True), (256, 33, False), (256, 97, False)]
LINEAR_SIZES = [1, 33, 1280]


@functools.lru_cache(maxsize=None)
def _linear_inputs(n, k, n_out, relu):
    """x, W, b, dy of one layer (test_linear_op._check's recipe: with ReLU, rows holding a pre-activation closer to the kink than the tolerance
    on y are drawn again, so every gate is decided by y's check)"""
    g = torch.Generator().manual_seed(n * 1000 + k + n_out)
    x, w, b = torch.randn(n, k, generator=g), torch.randn(n_out, k, generator=g) / k ** 0.5, torch.randn(n_out, generator=g) * 0.1
    if relu:
        for _ in range(16):
            z = torch.nn.functional.linear(x.double(), w.double(), b.double())
            near = (z.abs() < 2e-5 * float(z.max())).any(dim=1)
            if not bool(near.any()):
                break
            x[near] = torch.randn(int(near.sum()), k, generator=g)
        assert not bool(near.any()), (n, k, n_out)
    return x, w, b, torch.randn(n, n_out, generator=g)


def _linear_call(lib, dev, g, x, w, b, dy, relu, alloc):
    """cnr_linear_forward + cnr_linear_backward by direct calls; ``alloc(shape, what)`` makes the outputs"""
    n, k, n_out = x.shape[0], x.shape[1], w.shape[0]
    y, dx, dW, db = alloc((n, n_out), "y"), alloc((n, k), "dx"), alloc((n_out, k), "dW"), alloc((n_out,), "db")
    s, nb = lib.scratch("cnr_linear_scratch_bytes", dev, n, k, n_out, 0)
    lib.call("cnr_linear_forward", ptr(x), n, k, ptr(w), ptr(b), n_out, int(relu), ptr(y), ptr(s), nb, stream_of(x))
    s2, nb2 = lib.scratch("cnr_linear_scratch_bytes", dev, n, k, n_out, 1)
    lib.call("cnr_linear_backward", ptr(x), ptr(y), ptr(dy), n, k, ptr(w), n_out, int(relu), ptr(dx), ptr(dW), ptr(db), ptr(s2), nb2, stream_of(x))
    return {"y": y, "dx": dx, "dW": dW, "db": db}


def _linear(library, dev, g, k, n_out, relu, n):
    lib = cn.load_library(library)
    x, w, b, dy = (t.to(dev) for t in _linear_inputs(n, k, n_out, relu))
    return _linear_call(lib, dev, g, x, w, b, dy, relu, lambda shape, what: torch.empty(shape, dtype=torch.float32, device=dev))


# No gate of test_linear_op is run under the guard: its HipLinear allocates its scratch with torch.empty itself (not through
# RenderLibrary.scratch), and its _check draws its own inputs.  Its rule is applied to these results instead: float64 autograd at 2e-5 of
# the tensor's maximum, with its redraw of rows whose pre-activation sits at the ReLU kink (_linear_inputs below does the same redraw).
def _check_linear(k, n_out, relu, n):
    def check(res):
        x, w, b, dy = (t.double().requires_grad_(i < 3) for i, t in enumerate(_linear_inputs(n, k, n_out, relu)))
        ref = torch.nn.functional.linear(x, w, b)
        ref = torch.relu(ref) if relu else ref
        gx, gw, gb = torch.autograd.grad(ref, [x, w, b], dy)
        for name, r in (("y", ref.detach()), ("dx", gx), ("dW", gw), ("db", gb)):
            err = float((res[name].cpu().double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
            assert err < 2e-5, (n, k, n_out, relu, name, err)
    return check


LINEAR = _cases(_linear, [(k, n_out, relu, n) for k, n_out, relu in LINEAR_SHAPES for n in LINEAR_SIZES])


@pytest.mark.parametrize("k,n_out,relu,n", LINEAR)
def test_linear_emu(k, n_out, relu, n):
    _run(EMU, _linear, k, n_out, relu, n, check=_check_linear(k, n_out, relu, n))


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_out,relu,n", LINEAR)
def test_linear_hip(k, n_out, relu, n):
    _run(HIP, _linear, k, n_out, relu, n, check=_check_linear(k, n_out, relu, n))


# =====================================================================================================================================
# N_OUTSIDE > 0: outside z, background network, compositor
# =====================================================================================================================================
def _rays_bg(R, g):
    import test_background_ops as BG
    return BG._rays(R, g)


def _outside_z(library, dev, g, perturb):
    """test_background_ops._outside_z's inputs (no scratch: the sorted feed and its source map are the outputs)"""
    from color_neus_amd import background as B
    lib = cn.load_library(library)
    gen = torch.Generator().manual_seed(1)
    R, M, n_out, S = 37, 24, 8, 16
    far = torch.rand(R, generator=gen) * 2 + 2.5
    z = torch.sort(torch.rand(R, M, generator=gen) * 2 + 0.7, dim=-1).values
    z[3, 5] = z[3, 4]
    t = torch.rand(R, n_out, generator=gen) if perturb else None
    fn, zn = far.to(dev).requires_grad_(True), z.to(dev).requires_grad_(True)
    z_feed, src = B.OutsideZ.apply(lib, fn, t.to(dev) if perturb else None, zn, S, n_out)
    (z_feed * _coef(z_feed)).sum().backward()
    return {"z_feed": z_feed.detach(), "src": src, "d_far": fn.grad, "d_z": zn.grad}


OUTSIDE_Z = _cases(_outside_z, [(False,), (True,)])


@pytest.mark.parametrize("perturb", [False, True])
def test_outside_z_emu(perturb):
    _run(EMU, _outside_z, perturb)


@pytest.mark.gpu
@pytest.mark.parametrize("perturb", [False, True])
def test_outside_z_hip(perturb):
    _run(HIP, _outside_z, perturb)


def _background(library, dev, g, small):
    """cnr_background_forward / _backward on test_background_ops._background's small (4 x 64) and w160 (3 x 160) networks: 80 points"""
    from color_neus_amd import background as B
    lib = cn.load_library(library)
    gen = torch.Generator().manual_seed(2)
    R, MF = 8, 10
    o, d = _rays_bg(R, gen)
    zf = torch.sort(torch.rand(R, MF, generator=gen) * 3.0 + 0.5, dim=-1).values
    zf[:, -4:] = zf[:, -4:] * 40.0
    kw = dict(D=3, W=160, multires=4, multires_view=1, skips=(1,)) if small == "w160" else dict(D=4, W=64, multires=6, multires_view=2, skips=(1,))
    torch.manual_seed(11)
    nerf = B.NeRF(**kw).to(dev)
    on, dn, zn = o.to(dev).requires_grad_(True), d.to(dev).requires_grad_(True), zf.to(dev).requires_grad_(True)
    alpha, color = B.Background.apply(lib, nerf.config(), 2.0 / 16, on, dn, zn, *nerf.ordered_params(lib))
    ((alpha * _coef(alpha)).sum() + (color * _coef(color)).sum()).backward()
    res = {"alpha": alpha.detach(), "color": color.detach(), "d_o": on.grad, "d_d": dn.grad, "d_z": zn.grad}
    res.update({"grad:" + k: p.grad for k, p in nerf.named_parameters() if p.grad is not None})
    return res


def _gate_background(small):
    import test_background_ops as BG
    return lambda library, dev: BG._background(library, dev, small)


BACKGROUND = _cases(_background, [(True,), ("w160",)])


@pytest.mark.parametrize("small", [True, "w160"])
def test_background_emu(small):
    _run(EMU, _background, small, gate=_gate_background(small))


@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, "w160"])
def test_background_hip(small):
    _run(HIP, _background, small, gate=_gate_background(small))


def _composite(library, dev, g, color_type):
    """cnr_composite_background_forward / _backward at 33 rays (test_background_ops._composite's recipe at that ray count)"""
    from color_neus_amd import background as B
    lib = cn.load_library(library)
    gen = torch.Generator().manual_seed(3)
    R, M, n_out = 33, 20, 6
    MF = M + n_out
    o, d = _rays_bg(R, gen)
    z = torch.sort(torch.rand(R, M, generator=gen) * 2.4 + 1.0, dim=-1).values
    zf = torch.sort(torch.cat([z, torch.rand(R, n_out, generator=gen) * 30 + 4.0], -1), -1).values
    sdf = torch.randn(R, M, generator=gen) * 0.05
    grads = torch.nn.functional.normalize(torch.randn(R, M, 3, generator=gen), dim=-1) * (1 + 0.2 * torch.randn(R, M, 1, generator=gen))
    col, gcol = torch.rand(R, M, 3, generator=gen), (torch.rand(R, M, 3, generator=gen) if color_type else None)
    bga, bgc = torch.rand(R, MF, generator=gen) * 0.3, torch.rand(R, MF, 3, generator=gen)
    vals = dict(rays_d=d, z=z, zf=zf, sdf=sdf, grads=grads, col=col, bga=bga, bgc=bgc, var=torch.tensor([0.35]), gcol=gcol)
    tn = {k: v.to(dev).requires_grad_(True) for k, v in vals.items() if v is not None}
    res = B.CompositeBg.apply(lib, 2.0 / 16, 0.3, torch.tensor([0.2, 0.5, 0.7]).to(dev), o.to(dev), tn["rays_d"], tn["z"], tn["zf"], tn["sdf"], tn["grads"],
                              tn["col"], tn.get("gcol"), tn["bga"], tn["bgc"], tn["var"])
    diff, non_diff = B.composite_output_names(color_type)
    outn = dict(zip(diff + non_diff, res))
    sum((t * _coef(t)).sum() for t in res if t.requires_grad).backward()
    out = {"out:" + k: v.detach() for k, v in outn.items()}
    out.update({"grad:" + k: v.grad for k, v in tn.items() if v.grad is not None})
    return out


def _gate_composite(color_type):
    import test_background_ops as BG
    return lambda library, dev: BG._composite(library, dev, color_type)


COMPOSITE = _cases(_composite, [(False,), (True,)])


@pytest.mark.parametrize("color_type", [False, True])
def test_composite_background_emu(color_type):
    _run(EMU, _composite, color_type, gate=_gate_composite(color_type))


@pytest.mark.gpu
@pytest.mark.parametrize("color_type", [False, True])
def test_composite_background_hip(color_type):
    _run(HIP, _composite, color_type, gate=_gate_composite(color_type))


# =====================================================================================================================================
# loss, optimiser
# =====================================================================================================================================
def _fused_loss(library, dev, g, R, use_mask, sharded):
    """The fused loss forms on test_fused_loss._case's inputs: the one-launch form (cnr_loss_forward / _backward) and the ray-sharded form
    (cnr_loss_shard_stats / _combine, one rank).  The loss scratch has a zero contract: the guarded runs start it as 0x00 and check() holds
    it to all zero after the calls.  Only the _hip cases can fail that assertion: the emulation's be_loss_forward / be_loss_shard_stats never
    touch the scratch or its counter (cnr_kernels_emu.cpp), the partial sums and their clearing exist in loss_forward_kernel alone."""
    import test_fused_loss as FL
    lib = cn.load_library(library)
    out, gt, mask = FL._case(dev, R=R)
    if sharded:
        out["eik_sums"] = torch.tensor([0.3 * R * 12, float(R * 12)], device=dev)
    loss, parts = cn.compute_loss_fused(out, gt, mask if use_mask else None, library=lib, n_rays_global=R if sharded else None)
    loss2, _ = cn.compute_loss_fused(out, gt, mask if use_mask else None, library=lib, n_rays_global=R if sharded else None)   # the scratch again, as left
    keys = [k for k in out if k != "eik_sums"]
    grads = torch.autograd.grad(loss + loss2, [out[k] for k in keys], allow_unused=True)
    res = {"loss": loss.detach(), "loss_again": loss2.detach()}
    res.update({"part:" + k: v.detach() for k, v in parts.items() if torch.is_tensor(v)})
    res.update({"grad:" + k: v for k, v in zip(keys, grads) if v is not None})
    return res


def _gate_fused_loss(R):
    """test_fused_loss' own checks under the guard: the golden loss vectors of the reference (_loss_goldens) and, at that module's R = 53,
    _compare against compute_loss over its variants.  1025 rays has no reference of its own there: the bitwise rule alone."""
    import test_fused_loss as FL

    def gate(library, dev):
        lib = cn.load_library(library)
        FL._loss_goldens(dev, lib)
        if R == 53:
            FL._compare(lib, dev)
    return gate


FUSED_LOSS = _cases(_fused_loss, [(R, m, s) for R in (53, 1025) for m in (True, False) for s in (False, True)])


@pytest.mark.parametrize("R,use_mask,sharded", FUSED_LOSS)
def test_fused_loss_emu(R, use_mask, sharded):
    _run(EMU, _fused_loss, R, use_mask, sharded, gate=_gate_fused_loss(R))


@pytest.mark.gpu
@pytest.mark.parametrize("R,use_mask,sharded", FUSED_LOSS)
def test_fused_loss_hip(R, use_mask, sharded):
    _run(HIP, _fused_loss, R, use_mask, sharded, gate=_gate_fused_loss(R))


def _clip_adam(library, dev, g, group="seven"):
    """One ClipAdam step on the tensor shapes of test_clip_adam._run ("seven"), or on that module's group of 73 tensors ("split": two
    launches of 64 and 9 tensors, the second one's chunk sums behind the first one's in the scratch, tensors of 64, 65 and 74 chunks --
    cnr_clip_adam_scratch_bytes of a split call, exact-size and poisoned)"""
    import test_clip_adam as CA
    gen = torch.Generator().manual_seed(3)
    shapes = [(257, 256), (256,), (256, 1), (1,), (3, 259), (217, 39), (65536 // 64, 70)] if group == "seven" else [(n,) for n in CA._group_sizes()]
    ps = [torch.randn(s, generator=gen).to(dev).requires_grad_(True) for s in shapes]
    opt = cn.ClipAdam(ps, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=0.05, library=library)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=gen).to(dev)
    opt.step()
    st = opt.state[ps[0]]
    res = {"p%d" % i: p.detach() for i, p in enumerate(ps)}
    res.update(exp_avg=st["exp_avg"], exp_avg_sq=st["exp_avg_sq"])
    return res


def _gate_clip_adam(group="seven"):
    import test_clip_adam as CA
    return (lambda library, dev: CA._run(library, dev, steps=2)) if group == "seven" else (lambda library, dev: CA._group_check(library, dev))


CLIP_ADAM = _cases(_clip_adam, [(), ("split",)])


def test_clip_adam_emu():
    _run(EMU, _clip_adam, gate=_gate_clip_adam())


@pytest.mark.gpu
def test_clip_adam_hip():
    _run(HIP, _clip_adam, gate=_gate_clip_adam())


def test_clip_adam_split_call_emu():
    _run(EMU, _clip_adam, "split", gate=_gate_clip_adam("split"))


@pytest.mark.gpu
def test_clip_adam_split_call_hip():
    _run(HIP, _clip_adam, "split", gate=_gate_clip_adam("split"))


# =====================================================================================================================================
# nearest neighbours, images, rasteriser
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _nn_inputs(n, m):
    gen = torch.Generator().manual_seed(n + m)
    return torch.randn(n, 3, generator=gen), torch.randn(m, 3, generator=gen)


def _nn_search(library, dev, g, n, m):
    q, t = (x.to(dev) for x in _nn_inputs(n, m))
    if g is not None:
        q, t = g.copy(q, "query"), g.copy(t, "target")
    d2, idx = cn.metrics.nearest_neighbors(q, t, library=library)
    return {"dist2": d2, "idx": idx}


def _check_nn(n, m):
    """test_nn_metrics' two references: bitwise against the float32 restatement, within its bounds of the float64 one"""
    import test_nn_metrics as NM

    def check(res):
        q, t = _nn_inputs(n, m)
        NM._assert_bitwise_r32(q, t, res["dist2"], res["idx"])
        NM._assert_r64_bounds(q, t, res["dist2"], res["idx"])
    return check


NN = _cases(_nn_search, [(1, 1), (1000, 777)])


@pytest.mark.parametrize("n,m", NN)
def test_nn_search_emu(n, m):
    _run(EMU, _nn_search, n, m, check=_check_nn(n, m))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", NN)
def test_nn_search_hip(n, m):
    _run(HIP, _nn_search, n, m, check=_check_nn(n, m))


@functools.lru_cache(maxsize=None)
def _image_inputs(channels):
    gen = torch.Generator().manual_seed(channels)
    x, y = torch.rand(2, channels, 37, 53, generator=gen), torch.rand(2, channels, 37, 53, generator=gen)
    return x, y, torch.rand(37, 53, generator=gen) * 3.0


def _image_metrics(library, dev, g, channels, layout):
    """cnr_image_metrics on 37 x 53 images with the SSIM map.  layout "nchw": [2, C, H, W]; "nhwc": the same pair in torch's channels-last
    memory format (C = 3; with one channel that format IS the contiguous one and the channels-last kernel is not reached); "hwc": one
    [H, W, C] image, which reaches the channels-last kernel with one channel too.  With 3 channels also cnr_image_panel and the depth map."""
    x, y, depth = _image_inputs(channels)
    if layout == "hwc":
        x, y = x[:1], y[:1]
        m = cn.imaging.image_metrics(x[0].permute(1, 2, 0).contiguous().to(dev), y[0].permute(1, 2, 0).contiguous().to(dev), return_map=True, library=library)
        smap = m["ssim_map"].permute(2, 0, 1)[None]
    else:
        if layout == "nhwc":
            x, y = x.contiguous(memory_format=torch.channels_last), y.contiguous(memory_format=torch.channels_last)
        m = cn.imaging.image_metrics(x.to(dev), y.to(dev), return_map=True, library=library)
        smap = m["ssim_map"]
    res = {"mse": m["mse"], "ssim": m["ssim"], "ssim_map": smap.contiguous()}      # the map as [B, C, H, W], whatever the layout
    if channels == 3:
        gt, rd = x[0].permute(1, 2, 0).contiguous().to(dev), y[0].permute(1, 2, 0).contiguous().to(dev)
        res["panel"] = cn.imaging.panel(gt, rd, depth.to(dev), library=library)
        res["cmap"] = cn.imaging.cmap(depth.to(dev), library=library)
    return res


def _check_image(channels, layout):
    """test_image_eval's rules: the map is the float32 specification to the bit, mse / ssim its float64 means within 1e-9; the panel is the
    hstack of the quantised images and the depth colour map, exactly"""
    import test_image_eval as IE

    def check(res):
        x, y, depth = _image_inputs(channels)
        if layout == "hwc":
            x, y = x[:1], y[:1]
        ref_map, d = IE._ssim_ref(x, y, torch.float32), x - y
        assert torch.equal(IE._bits(res["ssim_map"]), IE._bits(ref_map)), int((IE._bits(res["ssim_map"]) != IE._bits(ref_map)).sum())
        ref_mse, ref_ssim = (d * d).double().mean().item(), ref_map.double().mean().item()
        assert abs(res["mse"].item() - ref_mse) <= 1e-9 * ref_mse and abs(res["ssim"].item() - ref_ssim) <= 1e-9 * abs(ref_ssim)
        if channels == 3:
            gt, rd = x[0].permute(1, 2, 0).contiguous().numpy(), y[0].permute(1, 2, 0).contiguous().numpy()
            assert np.array_equal(res["cmap"].cpu().numpy(), IE._cmap_np(depth.numpy()))
            assert np.array_equal(res["panel"].cpu().numpy(), np.hstack([IE._quant_np(gt), IE._quant_np(rd), IE._cmap_np(depth.numpy())]))
    return check


IMAGE = _cases(_image_metrics, [(1, "nchw"), (1, "hwc"), (3, "nchw"), (3, "nhwc")])


@pytest.mark.parametrize("channels,layout", IMAGE)
def test_image_metrics_and_panel_emu(channels, layout):
    _run(EMU, _image_metrics, channels, layout, check=_check_image(channels, layout))


@pytest.mark.gpu
@pytest.mark.parametrize("channels,layout", IMAGE)
def test_image_metrics_and_panel_hip(channels, layout):
    _run(HIP, _image_metrics, channels, layout, check=_check_image(channels, layout))


def _mesh_raster(library, dev, g):
    """cnr_mesh_raster on the small sphere of test_mesh_raster at its own H0 x W0, against that module's bitwise specification"""
    import test_mesh_raster as MR
    V, Fc, col = MR._sphere()
    c2w = MR._camera(0)
    t = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)
    got = cn.rasterize_mesh(t(V, np.float32), t(Fc, np.int64), t(c2w, np.float32), t(np.asarray((MR.F0, MR.F0)), np.float32), MR.H0, MR.W0,
                            colors=t(col, np.float32), library=library)
    MR._same(got, MR._s32(V, Fc, col, c2w, (MR.F0, MR.F0), MR.H0, MR.W0))
    return {k: got[k] for k in ("rgb", "depth", "tri_id", "mask")}


RASTER = _cases(_mesh_raster, [()])


def test_mesh_raster_emu():
    _run(EMU, _mesh_raster)


@pytest.mark.gpu
def test_mesh_raster_hip():
    _run(HIP, _mesh_raster)


# =====================================================================================================================================
# pixel table, rays, cameras
# =====================================================================================================================================
def _pixel_table(library, dev, g):
    """cnr_pixel_table_build + cnr_choose_pixels on 3 images of 12 x 17, against test_pixel_sampler's references: the table is
    torch.nonzero's (ref_table), every draw the restatement's (ref_draw), exactly"""
    import test_pixel_sampler as PS
    gen = torch.Generator().manual_seed(12 * 17)
    hw = 12 * 17
    masks = (torch.rand(3, 12, 17, generator=gen) < 0.3).float()
    table = PS.ref_table(masks)
    s = cn.PixelSampler(masks.to(dev), seed=3, library=library)
    order, fg, bg = PS._np(s.order), PS._np(s.fg_count), PS._np(s.bg_count)
    for n, (wf, wb) in enumerate(table):
        assert (fg[n], bg[n]) == (len(wf), len(wb)), n
        assert np.array_equal(order[n, :fg[n]], wf) and np.array_equal(order[n, fg[n]:fg[n] + bg[n]], wb), n
    idx, t = s.draw(64, 0.5, jitter=True)
    PS._compare(s, (idx, t), PS.ref_draw(3, 0, 64, 3, hw, table, want_fg=32, B=3))
    cams, counts = s.last_cams.clone(), s.last_counts.clone()
    idx2 = s.draw(40, 0.9, images_per_step=2, jitter=False)
    PS._compare(s, idx2, PS.ref_draw(3, 1, 40, 3, hw, table, want_fg=int(0.9 * 40), B=2), jitter=False)
    return {"order": s.order * (torch.arange(hw, device=dev)[None] < (s.fg_count + s.bg_count)[:, None]), "fg": s.fg_count, "bg": s.bg_count,
            "idx": idx, "t": t, "idx2": idx2, "cams": cams, "counts": counts, "cams2": s.last_cams, "counts2": s.last_counts}


PIXELS = _cases(_pixel_table, [()])


def test_pixel_table_and_choose_pixels_emu():
    _run(EMU, _pixel_table)


@pytest.mark.gpu
def test_pixel_table_and_choose_pixels_hip():
    _run(HIP, _pixel_table)


def _gen_rays_backward(library, dev, g):
    """cnr_gen_rays_backward on test_rays._backward's inputs (its scratch, n_cams * 2 floats, is stated by the header, not by a size function)"""
    import _golden as G
    from color_neus_amd import rays
    fx = G.load("rays")
    gen = torch.Generator().manual_seed(2)
    H, W, n = 12, 17, 64
    idx = torch.randint(0, 3 * H * W, (n,), generator=gen)
    cd = torch.from_numpy(fx["c2w"]).clone().to(dev).requires_grad_(True)
    fd = torch.from_numpy(fx["focal"]).clone().to(dev).requires_grad_(True)
    o, d, _, _, near, far = rays._generate(rays._library(library), idx.to(dev), n, cd, fd, H, W, True, False, origin=torch.tensor([0.1, -0.2, 0.05]),
                                           radius=1.7, want_nearfar=True)
    sum((t * _coef(t)).sum() for t in (o, d, near, far)).backward()
    return {"o": o.detach(), "d": d.detach(), "near": near.detach(), "far": far.detach(), "d_c2w": cd.grad, "d_focal": fd.grad}


def _gate_rays():
    import test_rays as TR
    return lambda library, dev: TR._backward(library, dev)


GEN_RAYS = _cases(_gen_rays_backward, [()])


def test_gen_rays_backward_emu():
    _run(EMU, _gen_rays_backward, gate=_gate_rays())


@pytest.mark.gpu
def test_gen_rays_backward_hip():
    _run(HIP, _gen_rays_backward, gate=_gate_rays())


def _cameras(library, dev, g, mode):
    """cnr_camera_forward / _backward at 49 cameras (test_cameras' input family); no scratch: the guarded runs hold the results to the plain run"""
    import test_cameras as TC
    r, t, init, ids, probe = TC._pose_inputs(1, mode)
    net = TC._pose_net(library, dev, mode, r, t, init)
    c2w, dr, dt = TC._run_pose(net, ids.to(dev), probe, dev)
    return {"c2w": c2w, "d_r": dr, "d_t": dt}


def _check_cameras(mode):
    """test_cameras' float64 yardstick and its tolerance (min(1e-5, max(1e-6, 4 x the float32 yardstick's own error)))"""
    import test_cameras as TC

    def check(res):
        r, t, init, ids, probe = TC._pose_inputs(1, mode)
        y32, y64 = (TC._yardstick(r, t, init, ids, mode, probe, dt) for dt in (torch.float32, torch.float64))
        for k, a, b in zip(("c2w", "d_r", "d_t"), y32, y64):
            TC._check("%s %s" % (mode, k), res[k], a, b)
    return check


CAMERAS = _cases(_cameras, [("6d",), ("3d",)])


@pytest.mark.parametrize("mode", ["6d", "3d"])
def test_cameras_emu(mode):
    _run(EMU, _cameras, mode, check=_check_cameras(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["6d", "3d"])
def test_cameras_hip(mode):
    _run(HIP, _cameras, mode, check=_check_cameras(mode))


# =====================================================================================================================================
# coverage is a condition: every size function of the binding was met by a guarded run of this module
# =====================================================================================================================================
def _coverage(build):
    tag = build[0]
    for family, args in REGISTRY:
        if (tag, family.__name__, args) not in _DONE:      # (run on its own, this test runs the cases itself)
            _run(build, family, *args)
    want = {n for n in _lib.SIGNATURES if n.endswith("_bytes")}
    assert SEEN[tag] == want, ("size functions without a guarded case", sorted(want - SEEN[tag]), "unknown names", sorted(SEEN[tag] - want))


def test_every_size_function_has_a_guarded_case_emu():
    _coverage(EMU)


@pytest.mark.gpu
def test_every_size_function_has_a_guarded_case_hip():
    _coverage(HIP)


def test_the_harness_can_fail():
    """The guard itself: one byte written behind, one in front of a payload, and a zero-contract payload left non-zero are each reported
    with the buffer's name, arguments and offsets; an untouched guard passes."""
    g = _guard.Guard()
    a = g.bytes(1000, "cpu", "cnr_some_bytes", (3, 4))
    z = g.bytes(64, "cpu", "cnr_zero_bytes", (), zero=True)
    t = g.empty((5, 3), torch.float32, "cpu", "rows")
    assert a.data_ptr() % 256 == 0 and t.data_ptr() % 256 == 0 and a.numel() == 1000 and bool((a == 0xFF).all()) and bool(torch.isnan(t).all())
    g.check()
    reg = g.regions[0]
    reg.raw[reg.off + 1000 + 7] = 1
    with pytest.raises(AssertionError, match=r"cnr_some_bytes\(3, 4\) \(1000 bytes\): 1 guard byte\(s\) after the payload changed, offsets \+7 \.\. \+7"):
        g.check()
    reg.raw[reg.off + 1000 + 7] = _guard.GUARD_FILL
    reg.raw[reg.off - 2] = 0
    with pytest.raises(AssertionError, match=r"before the payload changed, offsets -1002 \.\. -1002"):
        g.check()
    reg.raw[reg.off - 2] = _guard.GUARD_FILL
    z[60] = 1
    with pytest.raises(AssertionError, match=r"cnr_zero_bytes.*left non-zero: 1 byte\(s\), payload offsets 60 \.\. 60"):
        g.check()


# =====================================================================================================================================
# alignment of a context / scratch base (include/colorneus_render.h: a multiple of 16 bytes): refused on the host, nothing is launched.
# Emulation build only -- the host code is shared, and no kernel is ever handed a misaligned buffer
# =====================================================================================================================================
@contextlib.contextmanager
def _misaligned(names):
    """RenderLibrary.scratch hands out base + 4 for the size functions in ``names``"""
    orig = _lib.RenderLibrary.scratch

    def scratch(lib, bytes_fn, device, *args, at_least=0, zero=False, nbytes=None):
        t, nb = orig(lib, bytes_fn, device, *args, at_least=at_least, zero=zero, nbytes=nbytes)
        if bytes_fn in names:
            big = torch.zeros(t.numel() + 64, dtype=torch.uint8, device=device)
            off = (-big.data_ptr()) % 16 + 4
            t = big[off:off + t.numel()]
        return t, nb

    _lib.RenderLibrary.scratch = scratch
    try:
        yield
    finally:
        _lib.RenderLibrary.scratch = orig


# size function -> a case that reaches its entry point: one per family that lays an arena over a caller's buffer
MISALIGNED = [("cnr_ctx_bytes", _render, ("dtu", 3, "saving")), ("cnr_bwd_scratch_bytes", _render, ("dtu", 3, "saving")),
              ("cnr_infer_scratch_bytes", _forward_only, (0.0,)), ("cnr_sdf_eval_scratch_bytes", _sdf_eval, (1,)),
              ("cnr_sdf_grid_scratch_bytes", _grids, ()), ("cnr_vertex_color_scratch_bytes", _vertex_color, ("dtu", 1)),
              ("cnr_sdf_query_ctx_bytes", _sdf_query, (1, 1)), ("cnr_sdf_query_bwd_scratch_bytes", _sdf_query, (1, 1)),
              ("cnr_linear_scratch_bytes", _linear, (5, 7, True, 1)), ("cnr_background_ctx_bytes", _background, (True,)),
              ("cnr_background_bwd_scratch_bytes", _background, (True,))]


@pytest.mark.parametrize("bytes_fn,family,args", MISALIGNED, ids=[m[0] for m in MISALIGNED])
def test_a_misaligned_base_is_refused_emu(bytes_fn, family, args):
    if not os.path.isfile(N.EMU_LIB):
        pytest.skip("emulation library not built")
    with _misaligned({bytes_fn}):
        with pytest.raises(RuntimeError, match="misaligned: its address must be a multiple of 16 bytes"):
            family(N.EMU_LIB, "cpu", None, *args)
    family(N.EMU_LIB, "cpu", None, *args)       # and the same call on the aligned buffer goes through


# =====================================================================================================================================
# 3. output and input sentinels by direct calls: the typed inputs and outputs of the row-storing entry points in guarded tensors
# =====================================================================================================================================
F32 = torch.float32


class _Plain:
    """The allocator of the plain run of a direct-call case: same interface as _guard.Guard, ordinary tensors"""

    def __init__(self):
        self._backing = []

    def empty(self, shape, dtype, device, what="tensor"):
        if 0 in tuple(shape):      # a zero-length output still has an address (the ABI takes no NULL there): no rows of a one-row allocation
            big = torch.empty((1,) + tuple(shape)[1:], dtype=dtype, device=device)
            self._backing.append((big[:0], big))
            return self._backing[-1][0]
        return torch.empty(shape, dtype=dtype, device=device)

    def addr(self, t):
        for u, big in self._backing:
            if u is t:
                return C.c_void_p(big.data_ptr())
        return C.c_void_p(t.data_ptr())

    def copy(self, t, what="input"):
        return t.detach().contiguous().clone()


def _run_direct(build, family, *args):
    """A direct-call case twice: plainly allocated, then with every input and output (and the scratch) guarded, 0xFF around / inside
    them; the results are equal to the bit and no guard byte changed."""
    tag, library, dev = build
    if tag == "emu" and not os.path.isfile(N.EMU_LIB):
        pytest.skip("emulation library not built")
    name = "%s%r" % (family.__name__, args)
    got, g = _guarded_call(lambda g: family(library, dev, g, *args), _guard.POISON)      # (first: see _run)
    plain = family(library, dev, _Plain(), *args)
    _same_bits(name, plain, got, "guarded inputs and outputs")


def _direct_linear(library, dev, A, k, n_out, relu, n):
    lib = cn.load_library(library)
    x, w, b, dy = (A.copy(t.to(dev), what) for t, what in zip(_linear_inputs(n, k, n_out, relu), ("x", "W", "b", "dy")))
    return _linear_call(lib, dev, A, x, w, b, dy, relu, lambda shape, what: A.empty(shape, F32, dev, what))


@pytest.mark.parametrize("k,n_out,relu,n", LINEAR)
def test_direct_linear_emu(k, n_out, relu, n):
    _run_direct(EMU, _direct_linear, k, n_out, relu, n)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n_out,relu,n", LINEAR)
def test_direct_linear_hip(k, n_out, relu, n):
    _run_direct(HIP, _direct_linear, k, n_out, relu, n)


def _direct_points(library, dev, A, cfg_name, n):
    """cnr_sdf_eval and cnr_vertex_color: points [n][3] in, [n][1] / [n][3] out"""
    r = _eval_renderer(cfg_name, library, dev)
    lib, ccfg = r._lib, r._ccfg
    plist, parr = r._param_array()
    pts = A.copy((_pts(n, seed=5) * 0.7).to(dev), "points")
    sdf, rgb = A.empty((n, 1), F32, dev, "sdf"), A.empty((n, 3), F32, dev, "rgb")
    s, nb = lib.scratch("cnr_sdf_eval_scratch_bytes", dev, C.byref(ccfg), n)
    lib.call("cnr_sdf_eval", C.byref(ccfg), parr, ptr(pts), n, 1.0, ptr(sdf), ptr(s), nb, stream_of(pts))
    s2, nb2 = lib.scratch("cnr_vertex_color_scratch_bytes", dev, C.byref(ccfg), n)
    lib.call("cnr_vertex_color", C.byref(ccfg), parr, ptr(pts), n, ptr(rgb), ptr(s2), nb2, stream_of(pts))
    return {"sdf": sdf, "rgb": rgb}


DIRECT_POINTS = [("dtu", 1), ("dtu", 33), ("dtu", 4097), ("neus176", 1), ("neus176", 33)]


@pytest.mark.parametrize("cfg_name,n", DIRECT_POINTS)
def test_direct_sdf_eval_and_vertex_color_emu(cfg_name, n):
    _run_direct(EMU, _direct_points, cfg_name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,n", DIRECT_POINTS)
def test_direct_sdf_eval_and_vertex_color_hip(cfg_name, n):
    _run_direct(HIP, _direct_points, cfg_name, n)


def _direct_render(library, dev, A, cfg_name, shape, mode):
    """cnr_render_forward with every output the mode asks for, then cnr_render_backward with every d_params tensor in a buffer of its own
    (not the flat one) and d_rays_o / d_rays_d; a fixed cotangent on every differentiable output"""
    from color_neus_amd import renderer as RR
    ocfg, P, (o, d, near, far, t_rand, gt, mask), z = _render_inputs(cfg_name, shape)
    r = N.make_renderer(ocfg, P, library, dev)
    lib, ccfg, cfg = r._lib, r._ccfg, r.rcfg
    R = o.shape[0]
    o_, d_, near_, far_ = (A.copy(t.to(dev).reshape(s), w) for t, s, w in ((o, (R, 3), "rays_o"), (d, (R, 3), "rays_d"), (near, (R,), "near"), (far, (R,), "far")))
    out = {k: (A.empty(t.shape, F32, dev, "out " + k) if t is not None else None) for k, t in RR._alloc_outputs(cfg, R, dev, mode).items()}
    out["z_vals"].copy_(z.to(dev))
    plist = [A.copy(p, "parameter") for p in r._ordered_params()]
    cin = RR._inputs(o_, d_, near_, far_, None, out["z_vals"])
    cout = _lib.CnrOutputs(**{k: ptr(out[k]) for k in _lib.OUTPUT_FIELDS})
    buf, nb = lib.scratch("cnr_ctx_bytes", dev, C.byref(ccfg), R)
    lib.call("cnr_render_forward", C.byref(ccfg), param_array(plist), C.byref(cin), C.byref(cout), ptr(buf), nb, stream_of(o_))
    gmap = {}
    for k in _lib.OUT_GRAD_FIELDS:
        if k == "delta_relight_per_ray":
            if out.get("delta_relight_ray_sum") is not None:
                gmap[k] = A.copy(_coef(out["delta_relight_ray_sum"]), "cotangent " + k)
        elif out.get(k) is not None:
            gmap[k] = A.copy(_coef(out[k]), "cotangent " + k)
    cg = _lib.CnrOutGrads(**{k: ptr(gmap.get(k)) for k in _lib.OUT_GRAD_FIELDS})
    dparams = [A.empty(p.shape, F32, dev, "d_params[%d]" % i) for i, p in enumerate(plist)]
    darr = param_array(dparams)
    d_o, d_d = A.empty((R, 3), F32, dev, "d_rays_o"), A.empty((R, 3), F32, dev, "d_rays_d")
    gin = _lib.CnrInGrads(d_params=C.cast(darr, C.POINTER(C.c_void_p)), d_rays_o=ptr(d_o), d_rays_d=ptr(d_d), d_near=None, d_far=None)
    cout_b = _lib.CnrOutputs(z_vals=ptr(out["z_vals"]), gradients=ptr(out["gradients"]))
    scratch, nbs = lib.scratch("cnr_bwd_scratch_bytes", dev, C.byref(ccfg), R)
    lib.call("cnr_render_backward", C.byref(ccfg), param_array(plist), C.byref(cin), C.byref(cout_b), ptr(buf), nb, C.byref(cg), C.byref(gin),
             ptr(scratch), nbs, stream_of(o_))
    res = {"out:" + k: v for k, v in out.items() if v is not None}
    res.update({"d_params[%d]" % i: t for i, t in enumerate(dparams)})
    res.update(d_rays_o=d_o, d_rays_d=d_d)
    return res


DIRECT_RENDER = [("dtu", 33, "saving"), ("dtu", 33, "loss_only"), ("dtu", 33, "with_samples"), ("dtu", 3, "saving"),
                 ("w48", "B", "saving"), ("mixed", "B", "loss_only"), ("w208", "B", "with_samples"), ("dtu_pe4", 33, "saving"), ("neus176", "B", "saving")]


@pytest.mark.parametrize("cfg_name,shape,mode", DIRECT_RENDER)
def test_direct_render_emu(cfg_name, shape, mode):
    _run_direct(EMU, _direct_render, cfg_name, shape, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,shape,mode", DIRECT_RENDER)
def test_direct_render_hip(cfg_name, shape, mode):
    _run_direct(HIP, _direct_render, cfg_name, shape, mode)


def _direct_background(library, dev, A, small):
    from color_neus_amd import background as B
    lib = cn.load_library(library)
    gen = torch.Generator().manual_seed(2)
    R, MF = 8, 10
    o, d = _rays_bg(R, gen)
    zf = torch.sort(torch.rand(R, MF, generator=gen) * 3.0 + 0.5, dim=-1).values
    zf[:, -4:] = zf[:, -4:] * 40.0
    kw = dict(D=3, W=160, multires=4, multires_view=1, skips=(1,)) if small == "w160" else dict(D=4, W=64, multires=6, multires_view=2, skips=(1,))
    torch.manual_seed(11)
    nerf = B.NeRF(**kw).to(dev)
    ncfg = nerf.config()
    plist = [A.copy(p.float(), "parameter") for p in nerf.ordered_params(lib)]
    o_, d_, zf_ = A.copy(o.to(dev), "rays_o"), A.copy(d.to(dev), "rays_d"), A.copy(zf.to(dev), "z_feed")
    alpha, color = A.empty((R, MF), F32, dev, "alpha"), A.empty((R, MF, 3), F32, dev, "color")
    buf, nb = lib.scratch("cnr_background_ctx_bytes", dev, C.byref(ncfg), R, MF)
    lib.call("cnr_background_forward", C.byref(ncfg), param_array(plist), ptr(o_), ptr(d_), ptr(zf_), R, MF, 2.0 / 16, ptr(alpha), ptr(color), ptr(buf), nb,
             stream_of(zf_))
    da, dc = A.copy(_coef(alpha), "d_alpha"), A.copy(_coef(color), "d_color")
    dparams = [A.empty(p.shape, F32, dev, "d_params[%d]" % i) for i, p in enumerate(plist)]
    d_o, d_d, d_zf = A.empty((R, 3), F32, dev, "d_rays_o"), A.empty((R, 3), F32, dev, "d_rays_d"), A.empty((R, MF), F32, dev, "d_z_feed")
    scratch, nbs = lib.scratch("cnr_background_bwd_scratch_bytes", dev, C.byref(ncfg), R, MF)
    lib.call("cnr_background_backward", C.byref(ncfg), param_array(plist), ptr(o_), ptr(d_), ptr(zf_), R, MF, 2.0 / 16, ptr(buf), nb, ptr(color), ptr(da), ptr(dc),
             param_array(dparams), ptr(d_o), ptr(d_d), ptr(d_zf), ptr(scratch), nbs, stream_of(zf_))
    res = {"alpha": alpha, "color": color, "d_o": d_o, "d_d": d_d, "d_zf": d_zf}
    res.update({"d_params[%d]" % i: t for i, t in enumerate(dparams)})
    return res


@pytest.mark.parametrize("small", [True, "w160"])
def test_direct_background_emu(small):
    _run_direct(EMU, _direct_background, small)


@pytest.mark.gpu
@pytest.mark.parametrize("small", [True, "w160"])
def test_direct_background_hip(small):
    _run_direct(HIP, _direct_background, small)


def _direct_samplers(library, dev, A, R):
    """cnr_sample_pdf (R x 17 bins -> 9 samples) and cnr_up_sample (R x 16 positions -> 8 new ones)"""
    lib = cn.load_library(library)
    gen = torch.Generator().manual_seed(R)
    n, ns = 17, 9
    bins = A.copy(torch.sort(torch.rand(R, n, generator=gen) * 2.0 + 0.5, dim=-1).values.to(dev), "bins")
    w = A.copy((torch.rand(R, n - 1, generator=gen) + 1e-3).to(dev), "weights")
    out = A.empty((R, ns), F32, dev, "samples")
    lib.call("cnr_sample_pdf", ptr(bins), ptr(w), R, n, ns, ptr(out), stream_of(bins))
    import test_background_ops as BG
    o, d = BG._rays(R, gen)
    m, ni = 16, 8
    z = A.copy(torch.sort(torch.rand(R, m, generator=gen) * 2.0 + 1.5, dim=-1).values.to(dev), "z_vals")
    sdf = A.copy((torch.randn(R, m, generator=gen) * 0.3).to(dev), "sdf")
    o_, d_ = A.copy(o.to(dev), "rays_o"), A.copy(d.to(dev), "rays_d")
    newz = A.empty((R, ni), F32, dev, "new z")
    lib.call("cnr_up_sample", ptr(o_), ptr(d_), ptr(z), ptr(sdf), R, m, ni, 64.0, ptr(newz), stream_of(z))
    return {"sample_pdf": out, "up_sample": newz}


@pytest.mark.parametrize("R", [1, 33, 67])
def test_direct_sample_pdf_and_up_sample_emu(R):
    _run_direct(EMU, _direct_samplers, R)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 33, 67])
def test_direct_sample_pdf_and_up_sample_hip(R):
    _run_direct(HIP, _direct_samplers, R)


def _direct_mc_emit(library, dev, A, threshold):
    """cnr_mc_count, then cnr_mc_emit into ``vertices`` / ``triangles`` sized exactly by the counted totals (not max(n, 1)); a threshold
    above the lattice's maximum gives an empty surface, i.e. zero-length outputs"""
    lib = cn.load_library(library)
    u = A.copy(_sphere_lattice(13, dev), "lattice")
    scratch, nb = lib.scratch("cnr_mc_scratch_bytes", dev, 13)
    totals = A.empty((2,), torch.int32, dev, "totals")
    lib.call("cnr_mc_count", ptr(u), 13, float(threshold), ptr(scratch), nb, ptr(totals), stream_of(u))
    nv, nt = (int(x) for x in totals.tolist())
    assert (nv > 0 and nt > 0) == (threshold < 0.6)
    verts, tris = A.empty((nv, 3), F32, dev, "vertices"), A.empty((nt, 3), torch.int32, dev, "triangles")
    lib.call("cnr_mc_emit", ptr(u), 13, float(threshold), _lib.float3([-1, -1, -1]), _lib.float3([1, 1, 1]), ptr(scratch), nb,
             A.addr(verts), A.addr(tris), stream_of(u))
    return {"totals": totals, "vertices": verts, "triangles": tris}


@pytest.mark.parametrize("threshold", [0.0, 5.0])
def test_direct_mc_emit_emu(threshold):
    _run_direct(EMU, _direct_mc_emit, threshold)


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.0, 5.0])
def test_direct_mc_emit_hip(threshold):
    _run_direct(HIP, _direct_mc_emit, threshold)
