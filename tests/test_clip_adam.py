"""Fused per-parameter clip + Adam (cnr_clip_adam_step) against the reference loop's two calls: clip_grad_norm_ on each parameter
tensor (lib/utils/net_utils.py:174-184) followed by torch.optim.Adam(betas=(0.9, 0.99), eps=1e-8) (net_utils.py:88)."""
import functools
import math
import os

import pytest
import torch

import _golden as G
import _native as N
import color_neus_amd as cn


def _run(library, device, steps=5, max_norm=0.05):
    g = torch.Generator().manual_seed(3)
    shapes = [(257, 256), (256,), (256, 1), (1,), (3, 259), (217, 39), (65536 // 64, 70)]
    ref = [torch.randn(s, generator=g).to(device).requires_grad_(True) for s in shapes]
    ours = [p.detach().clone().requires_grad_(True) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=5e-4, betas=(0.9, 0.99), eps=1e-8)
    o_our = cn.ClipAdam(ours, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=max_norm, library=library)
    for it in range(steps):
        scale = [1e-3, 1.0, 30.0, 1e-6, 0.2][it % 5]          # below / above the clip threshold, tiny gradients
        for p, q in zip(ref, ours):
            gr = (torch.randn(p.shape, generator=g) * scale).to(device)
            if it == 2:
                gr = gr * (torch.rand(p.shape, generator=g) < 0.1).to(device)   # sparse gradient
            p.grad = gr.clone()
            q.grad = gr.clone()
        o_ref.param_groups[0]["lr"] = o_our.param_groups[0]["lr"] = 5e-4 * (0.9 ** it)   # a scheduler changes lr every step
        for p in ref:
            torch.nn.utils.clip_grad_norm_(p, max_norm, 2)
        o_ref.step()
        o_our.step()
    for p, q in zip(ref, ours):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(p.detach().abs().max())), p.shape
    st = o_our.state[ours[0]]
    flat_m = torch.cat([o_ref.state[p]["exp_avg"].reshape(-1) for p in ref])
    flat_v = torch.cat([o_ref.state[p]["exp_avg_sq"].reshape(-1) for p in ref])
    assert float((st["exp_avg"] - flat_m).abs().max()) <= 1e-6 * float(flat_m.abs().max())
    assert float((st["exp_avg_sq"] - flat_v).abs().max()) <= 5e-6 * float(flat_v.abs().max())   # (the clip coefficient enters squared)
    assert st["steps"] == [steps] * len(ours)


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
@pytest.mark.parametrize("max_norm", [0.05, None])
def test_clip_adam_matches_torch_emu(max_norm):
    if max_norm is None:
        g = torch.Generator().manual_seed(1)
        p = torch.randn(300, generator=g).requires_grad_(True)
        q = p.detach().clone().requires_grad_(True)
        a, b = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.99)), cn.ClipAdam([q], lr=1e-3, library=N.EMU_LIB)
        for _ in range(3):
            gr = torch.randn(300, generator=g)
            p.grad, q.grad = gr.clone(), gr.clone()
            a.step(); b.step()
        assert float((p - q).abs().max()) < 1e-6
    else:
        _run(N.EMU_LIB, "cpu", max_norm=max_norm)


@pytest.mark.gpu
def test_clip_adam_matches_torch_hip():
    _run(None, "cuda:0")


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_backward_lays_gradients_out_in_one_flat_buffer():
    """All parameter gradients of a render backward tile one contiguous buffer in canonical order (what the in-place bucket
    all-reduce and the fused optimiser step rely on), and a training step through ClipAdam moves the parameters."""
    from color_neus_amd import optim
    fx, r, out, loss, grads, o, d = N.run_native("tiny_sharp", "jit", N.EMU_LIB, "cpu", fixed_z=True)
    params = r._ordered_params()
    flat = optim.flat_view_of_grads(params)
    assert flat is not None and flat.numel() == sum(p.numel() for p in params)
    off = 0
    for p in params:
        assert torch.equal(flat[off:off + p.numel()].view_as(p), p.grad)
        off += p.numel()
    before = [p.detach().clone() for p in params]
    opt = cn.ClipAdam(params, lr=1e-3, max_norm=1.0, library=N.EMU_LIB)
    opt.step()
    assert any(float((a - b.detach()).abs().max()) > 0 for a, b in zip(before, params))


def _run_intermittent(library, device):
    """A parameter that receives a gradient only on some steps (auxiliary / background parameters) keeps its moments and its own step
    count, exactly like torch.optim.Adam's per-parameter state; the others are unaffected by its absence."""
    g = torch.Generator().manual_seed(5)
    shapes = [(64, 33), (64,), (5, 7), (129,)]
    ref = [torch.randn(s, generator=g).to(device).requires_grad_(True) for s in shapes]
    ours = [p.detach().clone().requires_grad_(True) for p in ref]
    o_ref = torch.optim.Adam(ref, lr=1e-2, betas=(0.9, 0.99), eps=1e-8)
    o_our = cn.ClipAdam(ours, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, max_norm=None, library=library)
    for it in range(6):
        for i, (p, q) in enumerate(zip(ref, ours)):
            if (i == 2 and it % 2 == 1) or (i == 0 and it == 3):   # no gradient for these tensors on these steps (incl. the first one of the group)
                p.grad = None
                q.grad = None
                continue
            gr = torch.randn(p.shape, generator=g).to(device)
            p.grad = gr.clone()
            q.grad = gr.clone()
        o_ref.step()
        o_our.step()
    for p, q in zip(ref, ours):
        assert float((p.detach() - q.detach()).abs().max()) <= 2e-6 * max(1.0, float(p.detach().abs().max())), p.shape
    assert o_our.state[ours[0]]["steps"] == [5, 6, 3, 6]
    sd = o_our.state_dict()            # round trip: the scratch buffer is not part of the state
    assert set(sd["state"][0].keys()) == {"exp_avg", "exp_avg_sq", "steps"}
    o2 = cn.ClipAdam(ours, lr=1e-2, betas=(0.9, 0.99), eps=1e-8, max_norm=None, library=library)
    o2.load_state_dict(sd)
    assert o2.state[ours[0]]["steps"] == [5, 6, 3, 6]


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_clip_adam_intermittent_gradients_emu():
    _run_intermittent(N.EMU_LIB, "cpu")


@pytest.mark.gpu
def test_clip_adam_intermittent_gradients_hip():
    _run_intermittent(None, "cuda:0")


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_clip_adam_loads_state_of_the_previous_layout():
    """A state_dict saved by the build whose group state held ONE ``step`` count (and no ``steps`` list) resumes: the moments cover every
    parameter of the group there, so the per-parameter step counts are that count; a layout whose moments cover only a subset is refused
    with a clear message instead of a KeyError."""
    g = torch.Generator().manual_seed(4)
    ps = [torch.randn(40, 7, generator=g).requires_grad_(True), torch.randn(9, generator=g).requires_grad_(True)]
    a = cn.ClipAdam(ps, lr=1e-3, max_norm=1.0, library=N.EMU_LIB)
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g)
    a.step(); a.step()
    sd = a.state_dict()
    st = sd["state"][0]
    old = {"exp_avg": st["exp_avg"].clone(), "exp_avg_sq": st["exp_avg_sq"].clone(), "step": 2}   # the earlier layout
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    b = cn.ClipAdam(qs, lr=1e-3, max_norm=1.0, library=N.EMU_LIB)
    b.load_state_dict({"state": {0: old}, "param_groups": sd["param_groups"]})
    for p, q in zip(ps, qs):
        gr = torch.randn(p.shape, generator=g)
        p.grad, q.grad = gr.clone(), gr.clone()
    a.step(); b.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p.detach(), q.detach())
    assert b.state[qs[0]]["steps"] == [3, 3]
    c = cn.ClipAdam([q.detach().clone().requires_grad_(True) for q in qs], lr=1e-3, library=N.EMU_LIB)
    c.load_state_dict({"state": {0: {"exp_avg": old["exp_avg"][:280].clone(), "exp_avg_sq": old["exp_avg_sq"][:280].clone(), "step": 2}},
                       "param_groups": sd["param_groups"]})
    for q in c.param_groups[0]["params"]:
        q.grad = torch.zeros_like(q)
    with pytest.raises(RuntimeError, match="earlier layout"):
        c.step()


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_capturable_mode_reads_the_step_scalars_from_device_memory_emu():
    """ClipAdam(capturable=True) -- cnr_adam_config.hyper_dev (ABI 8): lr and the two bias corrections read from three device floats that
    prepare_step() refreshes, so that step() can sit in a captured HIP graph -- must produce the same bits as the by-value form, with a
    scheduler changing lr every step; step() without prepare_step() is an error."""
    g = torch.Generator().manual_seed(5)
    shapes = [(33, 7), (5,), (4100,)]
    w0 = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * sc for s in shapes] for sc in (1e-3, 1.0, 30.0, 0.2, 1e-6, 2.0)]

    def run(cap):
        ps = [w.clone().requires_grad_(True) for w in w0]
        opt = cn.ClipAdam(ps, lr=5e-4, betas=(0.9, 0.99), eps=1e-8, max_norm=0.05, library=N.EMU_LIB, capturable=cap)
        for it, gs in enumerate(grads):
            opt.param_groups[0]["lr"] = 5e-4 * (0.9 ** it)
            for p, gr in zip(ps, gs):
                p.grad = gr.clone()
            if cap:
                opt.prepare_step()
            opt.step()
        return [p.detach() for p in ps], opt.state[ps[0]]

    (a, sa), (b, sb) = run(False), run(True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]) and sa["steps"] == sb["steps"]
    p = torch.zeros(3, requires_grad=True)
    p.grad = torch.ones(3)
    with pytest.raises(RuntimeError, match="prepare_step"):
        cn.ClipAdam([p], library=N.EMU_LIB, capturable=True).step()


# =====================================================================================================================================
# beyond one loop trip: a group of 73 tensors (two launches of kAdamBatch = 64), tensors of more than 64 chunks (the second trip of the
# chunk-sum fold), every chunk edge -- against a float64 reference, every tensor on its own scale
# =====================================================================================================================================
# positions of the sizes that matter; the other 66 are drawn from [1, 9000).  4095 / 4096 / 4097: one chunk less one, one chunk, one chunk plus
# one; 262144 / 262145: 64 and 65 chunks (the fold's `c += 64` loop makes its second trip at 65); 300001: 74 chunks, ragged.  Tensors 3 and 40
# sit in the first launch of 64, tensor 66 in the second -- its chunk sums lie behind 150-odd chunks of the first launch in the scratch, and
# behind two small tensors of its own launch.  Tensors 10 and 64 (the first of the second launch) are the ones whose gradient goes missing.
SPECIAL_SIZES = {0: 4095, 1: 4096, 2: 4097, 3: 262145, 7: 1, 40: 262144, 66: 300001}
N_GROUP = 73
MISSING = {10: (0, 3), 64: (0, 1, 4)}          # tensor -> the steps on which it has no gradient (the first step among them)
STEPS = 5
LR0, BETAS, EPS, MAX_NORM = 5e-4, (0.9, 0.99), 1e-8, 0.05


def _group_sizes():
    g = torch.Generator().manual_seed(73)
    drawn = iter(torch.randint(1, 9000, (N_GROUP - len(SPECIAL_SIZES),), generator=g).tolist())
    return [SPECIAL_SIZES[i] if i in SPECIAL_SIZES else next(drawn) for i in range(N_GROUP)]


@functools.lru_cache(maxsize=None)
def _group_problem(intermittent):
    """Initial weights, the gradients of every step (None where a tensor has none) and the learning rates: drawn once, never modified.
    Odd tensors start from weights scaled by 1e-3, so that their total movement (~2e-3) is as large as they are and the weight check
    says something about the update; the gradient schedule is _run's (scales below and above the clip threshold, tiny gradients, one
    sparse step, lr changed every step) times a factor 1 + i % 7 of each tensor's own, so that a neighbour's clip coefficient is wrong by
    tens of percent."""
    g = torch.Generator().manual_seed(11)
    sizes = _group_sizes()
    w0 = [torch.randn(n, generator=g) * (1e-3 if i % 2 else 1.0) for i, n in enumerate(sizes)]
    grads = []
    for it in range(STEPS):
        scale = [1e-3, 1.0, 30.0, 1e-6, 0.2][it % 5]
        row = []
        for i, n in enumerate(sizes):
            gr = torch.randn(n, generator=g) * (scale * (1 + i % 7))
            if it == 2:
                gr = gr * (torch.rand(n, generator=g) < 0.1)
            row.append(None if intermittent and it in MISSING.get(i, ()) else gr)
        grads.append(row)
    lrs = [LR0 * 0.9 ** it for it in range(STEPS)]
    return sizes, w0, grads, lrs


@functools.lru_cache(maxsize=None)
def _group_reference(max_norm, intermittent):
    """The float64 reference of "clip each tensor, then Adam" (clip_grad_norm_ on one tensor: coef = min(1, max_norm / (||g|| + 1e-6));
    then torch.optim.Adam's exp_avg / exp_avg_sq / addcdiv formulas with the tensor's OWN step count), and, next to it, the distance of
    torch's own float32 clip_grad_norm_ + torch.optim.Adam from that reference on the same draw -- a second implementation of the same
    operation, the yardstick of the tolerances.  The betas are the float32 values of 0.9 and 0.99, as in cnr_clip_adam_step (its
    configuration holds floats): 0.99 as a float32 moves 1 - beta2 by 1e-6 relative, as much as the tolerance.
    Returns per tensor (w, exp_avg, exp_avg_sq, steps, total movement) and the two worst per-tensor distances of torch float32."""
    sizes, w0, grads, lrs = _group_problem(intermittent)
    b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in BETAS)
    ref = []
    for i, n in enumerate(sizes):
        w, m, v, t, moved = w0[i].double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), 0, 0.0
        for it in range(STEPS):
            if grads[it][i] is None:
                continue
            t += 1
            gr = grads[it][i].double()
            if max_norm is not None:
                gr = gr * min(1.0, max_norm / (float(gr.norm()) + 1e-6))
            m = m + (gr - m) * (1.0 - b1)
            v = v * b2 + (1.0 - b2) * gr * gr
            step = (lrs[it] / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + EPS)
            w = w - step
            moved += float(step.abs().max())
        ref.append((w, m, v, t, moved))
    ps = [w.clone().requires_grad_(True) for w in w0]
    opt = torch.optim.Adam(ps, lr=LR0, betas=BETAS, eps=EPS)
    for it in range(STEPS):
        for p, gr in zip(ps, grads[it]):
            p.grad = None if gr is None else gr.clone()
            if gr is not None and max_norm is not None:
                torch.nn.utils.clip_grad_norm_(p, max_norm, 2)
        opt.param_groups[0]["lr"] = lrs[it]
        opt.step()
    e_m = max(float((opt.state[p]["exp_avg"].double() - r[1]).abs().max() / r[1].abs().max()) for p, r in zip(ps, ref))
    e_v = max(float((opt.state[p]["exp_avg_sq"].double() - r[2]).abs().max() / r[2].abs().max()) for p, r in zip(ps, ref))
    return ref, e_m, e_v


def _group_steps(library, device, max_norm, intermittent, capturable=False):
    sizes, w0, grads, lrs = _group_problem(intermittent)
    ps = [w.clone().to(device).requires_grad_(True) for w in w0]
    opt = cn.ClipAdam(ps, lr=LR0, betas=BETAS, eps=EPS, max_norm=max_norm, library=library, capturable=capturable)
    for it in range(STEPS):
        for p, gr in zip(ps, grads[it]):
            p.grad = None if gr is None else gr.to(device)
        opt.param_groups[0]["lr"] = lrs[it]
        if capturable:
            opt.prepare_step()
        opt.step()
    st = opt.state[ps[0]]
    return [p.detach().cpu() for p in ps], st["exp_avg"].cpu(), st["exp_avg_sq"].cpu(), list(st["steps"])


def _group_check(library, device, max_norm=MAX_NORM, intermittent=False):
    """The 73-tensor group against the float64 reference, every tensor against its own largest reference entry.

    Moments: 4 x the worst per-tensor distance of torch's float32 clip_grad_norm_ + Adam from the reference on this draw (the HIP build
    sums the clip norm in another order than torch or the emulation do).  Measured on the CPU, 5 steps, worst tensor (exp_avg, exp_avg_sq):
    max_norm 0.05, with and without the missing gradients: torch float32 1.1e-6, 1.4e-6, the emulation build 5.1e-7, 7.1e-7; max_norm None:
    torch float32 2.9e-7, 1.1e-6, the emulation 1.6e-7, 1.5e-7.  The run prints its own figures before it asserts.
    Weights: a float32 weight is rounded once per step, at most half an ulp of the largest weight each time: steps * 2^-24 *
    2^ceil(log2 max|w|); on top of that the update lr / bc1 * m / (sqrt(v) / bc2 + eps) inherits the moments' relative error, e_m + e_v / 2
    to first order (the two moment tolerances), and six float32 roundings of its own (sqrt, two divisions, the sum, the quotient, the
    product: 6 * 2^-24), times the tensor's total movement (the sum over its steps of the largest step, from the reference).  The tensors
    that start from weights of 1e-3 move by about as much as they are: they are held to the relative term alone."""
    sizes, w0, grads, lrs = _group_problem(intermittent)
    ref, e_m, e_v = _group_reference(max_norm, intermittent)
    tol_m, tol_v = 4.0 * e_m, 4.0 * e_v
    rel_w = tol_m + 0.5 * tol_v + 6.0 * 2.0 ** -24
    ws, m, v, steps = _group_steps(library, device, max_norm, intermittent)
    assert steps == [r[3] for r in ref]
    if intermittent:
        assert steps == [STEPS - len(MISSING.get(i, ())) for i in range(N_GROUP)] and steps[10] == 3 and steps[64] == 2
    bad, worst, off = [], [0.0, 0.0, 0.0], 0
    for i, (n, (rw, rm, rv, t, moved)) in enumerate(zip(sizes, ref)):
        err_m = float((m[off:off + n].double() - rm).abs().max() / rm.abs().max())
        err_v = float((v[off:off + n].double() - rv).abs().max() / rv.abs().max())
        err_w = float((ws[i].double() - rw).abs().max())
        ulp = 0.0 if i % 2 else t * 2.0 ** -24 * 2.0 ** math.ceil(math.log2(float(rw.abs().max())))
        tol_w = ulp + rel_w * moved
        worst = [max(worst[0], err_m), max(worst[1], err_v), max(worst[2], err_w / tol_w)]
        for what, err, tol in (("exp_avg", err_m, tol_m), ("exp_avg_sq", err_v, tol_v), ("weight", err_w, tol_w)):
            if not err <= tol:
                bad.append("tensor %d (%d elements) %s: %.3g > %.3g" % (i, n, what, err, tol))
        off += n
    print("clip_adam group max_norm=%r intermittent=%r: torch float32 %.2e %.2e, library %.2e %.2e, weights at %.2f of their bound"
          % (max_norm, intermittent, e_m, e_v, worst[0], worst[1], worst[2]))
    assert not bad, "\n".join(bad)


GROUP_CASES = [(MAX_NORM, False), (None, False), (MAX_NORM, True)]


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
@pytest.mark.parametrize("max_norm,intermittent", GROUP_CASES)
def test_clip_adam_group_of_73_against_float64_emu(max_norm, intermittent):
    _group_check(N.EMU_LIB, "cpu", max_norm, intermittent)


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm,intermittent", GROUP_CASES)
def test_clip_adam_group_of_73_against_float64_hip(max_norm, intermittent):
    _group_check(None, "cuda:0", max_norm, intermittent)


def _group_capturable(library, device):
    """capturable=True (lr and the bias corrections read from device memory) on the 73-tensor group: the bits of the by-value form, in
    both launches of the split call."""
    a, b = _group_steps(library, device, MAX_NORM, False), _group_steps(library, device, MAX_NORM, False, capturable=True)
    for i, (x, y) in enumerate(zip(a[0], b[0])):
        assert torch.equal(x, y), i
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] == [STEPS] * N_GROUP


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_capturable_mode_on_the_group_of_73_emu():
    _group_capturable(N.EMU_LIB, "cpu")


@pytest.mark.gpu
def test_capturable_mode_on_the_group_of_73_hip():
    _group_capturable(None, "cuda:0")
