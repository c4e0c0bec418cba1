"""cnr_linear_forward / cnr_linear_backward (one plain nn.Linear (+ ReLU) on the render library's layer and weight-gradient kernels; the
shapes are those of the NeRF++ background network, fields.py:192-274, which cnr_background_forward chains internally) against torch.nn.functional.linear (+ ReLU) with autograd: every shape of the NeRF stack and ragged point counts."""
import os
import subprocess
import sys

import pytest
import torch

import _native as N

import ctypes as C


class HipLinear(torch.autograd.Function):
    """y = act(x W^T + b) through cnr_linear_forward / cnr_linear_backward (the render library's layer GEMM + weight-gradient GEMM)."""

    @staticmethod
    def forward(ctx, lib, x, weight, bias, relu):
        x2 = x.detach().reshape(-1, x.shape[-1]).contiguous().float()
        w, b = weight.detach().contiguous().float(), (bias.detach().contiguous().float() if bias is not None else None)
        n, k, n_out = x2.shape[0], x2.shape[1], w.shape[0]
        y = torch.empty(n, n_out, dtype=torch.float32, device=x2.device)
        if n > 0:
            nb = lib.lib.cnr_linear_scratch_bytes(n, k, n_out, 0)
            scratch = torch.empty(nb, dtype=torch.uint8, device=x2.device)
            stream = C.c_void_p(torch.cuda.current_stream(x2.device).cuda_stream) if x2.is_cuda else C.c_void_p(0)
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
            lib.check(lib.lib.cnr_linear_forward(p(x2), n, k, p(w), p(b), n_out, int(relu), p(y), p(scratch), nb, stream), "cnr_linear_forward")
        ctx.lib, ctx.relu, ctx.has_bias, ctx.xshape = lib, bool(relu), bias is not None, x.shape
        ctx.save_for_backward(x2, w, y)
        return y.reshape(*x.shape[:-1], n_out)

    @staticmethod
    def backward(ctx, dy):
        x2, w, y = ctx.saved_tensors
        lib = ctx.lib
        n, k, n_out = x2.shape[0], x2.shape[1], w.shape[0]
        dy2 = dy.reshape(-1, n_out).contiguous().float()
        dx = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        dW = torch.empty_like(w)
        db = torch.empty(n_out, dtype=torch.float32, device=w.device) if ctx.has_bias else None
        if n > 0:
            nb = lib.lib.cnr_linear_scratch_bytes(n, k, n_out, 1)
            scratch = torch.empty(nb, dtype=torch.uint8, device=x2.device)
            stream = C.c_void_p(torch.cuda.current_stream(x2.device).cuda_stream) if x2.is_cuda else C.c_void_p(0)
            p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
            lib.check(lib.lib.cnr_linear_backward(p(x2), p(y), p(dy2), n, k, p(w), n_out, int(ctx.relu), p(dx), p(dW), p(db), p(scratch), nb, stream),
                      "cnr_linear_backward")
        else:
            dW.zero_()
            if db is not None:
                db.zero_()
        return None, (dx.reshape(ctx.xshape) if dx is not None else None), dW, db, None


def _embed(x, multires):
    """get_embedder(multires, input_dims=d): [x, sin(2^k x), cos(2^k x)]_k (PositionEncoding.py:51-76)."""
    out = [x]
    for k in range(multires):
        out += [torch.sin(x * 2.0 ** k), torch.cos(x * 2.0 ** k)]


# (k, n_out, relu): pts_linears[0], pts_linears[i], the skip layer, alpha / feature heads, the view branch, the rgb head (NeRF(), fields.py:228-248)
SHAPES = [(84, 256, True), (256, 256, True), (340, 256, True), (256, 1, False), (256, 256, False), (283, 128, True), (128, 3, False), (5, 7, True)]
# widths between the tested 64 and 256 (tests/test_width_lattice.py runs whole networks of them; these isolate one forward, one backward and one
# weight-gradient launch per shape): the weight-stationary kernel with 128 / 96 weight rows and 8 / 7 k16 blocks, K = 240 (the boundary of its
# stream form) and K = 272 beyond it, an output one column either side of its 96-column threshold, an 80-wide output (3-tile general kernel),
# and outputs of exactly 32 and 33 columns (the row-tail boundary of the weight-gradient tiles)
SHAPES += [(128, 128, True), (112, 96, True), (240, 256, True), (48, 160, False), (272, 224, True), (256, 95, True), (256, 97, False), (80, 80, True),
           (256, 32, False), (256, 33, False)]


def _check(library, device, sizes, shapes=SHAPES):
    import color_neus_amd as cn
    lib = cn.load_library(library)
    g = torch.Generator().manual_seed(0)
    for n in sizes:
        for k, n_out, relu in shapes:
            x = torch.randn(n, k, generator=g)
            w = torch.randn(n_out, k, generator=g) / k ** 0.5
            b = torch.randn(n_out, generator=g) * 0.1
            if relu:
                # The derivative of ReLU is discontinuous at 0: a pre-activation closer to 0 than the tolerance on y may be gated the other way
                # by a y that passes, which moves its whole row of dx and dW by O(1) (met on the first draw of (1280, 272, 224): one unit at 4.1e-7,
                # y = 0 -- a wrong row in dx and dW at 7e-2).  Rows holding such a pre-activation (about 2 % of them) are drawn again, so every gate is decided by y's check.
                for _ in range(16):
                    z = torch.nn.functional.linear(x.double(), w.double(), b.double())
                    near = (z.abs() < 2e-5 * float(z.max())).any(dim=1)
                    if not bool(near.any()):
                        break
                    x[near] = torch.randn(int(near.sum()), k, generator=g)
                assert not bool(near.any()), (n, k, n_out)
            x, w, b = x.to(device).requires_grad_(True), w.to(device).requires_grad_(True), b.to(device).requires_grad_(True)
            dy = torch.randn(n, n_out, generator=g).to(device)
            ref = torch.nn.functional.linear(x.double(), w.double(), b.double())
            if relu:
                ref = torch.relu(ref)
            gx, gw, gb = torch.autograd.grad(ref, [x, w, b], dy.double())
            y = HipLinear.apply(lib, x, w, b, relu)
            hx, hw, hb = torch.autograd.grad(y, [x, w, b], dy)
            for name, a, r in (("y", y, ref), ("dx", hx, gx), ("dW", hw, gw), ("db", hb, gb)):
                den = max(float(r.abs().max()), 1e-30)
                err = float((a.double() - r).abs().max()) / den
                assert err < 2e-5, (n, k, n_out, relu, name, err)


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_linear_op_emu():
    _check(N.EMU_LIB, "cpu", [1, 33, 200])


@pytest.mark.gpu
def test_linear_op_hip():
    _check(None, "cuda:0", [1, 33, 1280, 5000])


# (k, n_out, relu) whose weight gradient has a 256 x 256 main tile: a full one, a partial one, a second column tile (k0 = 256), the row-tail boundary
FP32_SHAPES = [(256, 256, True), (80, 80, True), (340, 256, True), (256, 33, False)]
_FP32_CHILD = r"""
import sys, os
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import torch
import color_neus_amd as cn
import test_linear_op as T
lib = cn.load_library(None)
lib.timing_enable(True)
lib.timing_collect()
T._check(None, "cuda:0", [1, 33], T.FP32_SHAPES)
torch.cuda.synchronize()
names = [(rec[0], rec[2]) for rec in lib.timing_collect()]
assert ("dw_gemm", 4224) in names, names
assert not any(nm in ("dw_gemm_bx", "dw_gemm_hx") for nm, _ in names), names
print("fp32 main tiles:", sum(1 for r in names if r == ("dw_gemm", 4224)))
"""


@pytest.mark.gpu
def test_linear_op_fp32_main_tiles_hip():
    """CNR_DW_FP32=1 (read once per process: a child process) sends the 256 x 256 main tiles to dw_gemm_kernel<4, 2, 2, 4> -- the launch records
    show it -- whose staging and column sums no other test meets at ragged and sub-slab point counts: n = 1 leaves every workgroup but one
    without a slab, n = 33 ends inside one.  Same check as test_linear_op_hip: y, dx, dW, db against float64 autograd at 2e-5 of the tensor's maximum."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _FP32_CHILD, root], env=dict(os.environ, CNR_DW_FP32="1"), cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# (k, n_out): the split-f16 stream form of the layer kernel, a narrow input, K beyond 256
SCALE_SHAPES = [(256, 256), (84, 256), (272, 224)]


def _check_scale_rule(library, device):
    """The row scale of the split-f16 arithmetic is an exact power of two and is undone exactly, so multiplying a row of the input by 2^k multiplies
    the row of the output by 2^k to the bit -- a property of the design, not a tolerance -- and an all-zero row gives an exactly zero row.  Rows that
    are zero in either operand contribute exactly nothing to the weight gradient, which therefore keeps the file's 2e-5 of the tensor's maximum
    against float64 autograd with a third of the rows zeroed in each operand (both, only x, only dy, neither)."""
    import color_neus_amd as cn
    lib = cn.load_library(library)
    g = torch.Generator().manual_seed(1)
    for n in (33, 1280):   # a ragged last tile; several tiles
        rows = torch.arange(n)
        zx, zy = rows % 3 == 0, (rows % 6 == 0) | (rows % 6 == 1)
        for k, n_out in SCALE_SHAPES:
            x = torch.randn(n, k, generator=g)
            dy = torch.randn(n, n_out, generator=g)
            x[zx] = 0.0
            dy[zy] = 0.0
            w = torch.randn(n_out, k, generator=g) / k ** 0.5
            b = torch.randn(n_out, generator=g) * 0.1
            s = torch.ldexp(torch.ones(n), torch.randint(-40, 41, (n,), generator=g)).unsqueeze(1)   # 2^k_i, k_i in [-40, 40]
            x, dy, w, b, s = x.to(device), dy.to(device), w.to(device).requires_grad_(True), b.to(device).requires_grad_(True), s.to(device)

            def run(xin, dyin, bias):
                xin = xin.clone().requires_grad_(True)
                y = HipLinear.apply(lib, xin, w, bias, False)
                return (y.detach(),) + torch.autograd.grad(y, [xin, w] + ([bias] if bias is not None else []), dyin)

            y0, dx0, _ = run(x, dy, None)
            y1, _, _ = run(x * s, dy, None)
            _, dx1, _ = run(x, dy * s, None)
            assert torch.equal(y1, y0 * s), (n, k, n_out, "y", float((y1 - y0 * s).abs().max()))
            assert torch.equal(dx1, dx0 * s), (n, k, n_out, "dx", float((dx1 - dx0 * s).abs().max()))
            assert bool((y0[zx.to(device)] == 0).all()) and bool((y0[~zx.to(device)] != 0).any()), (n, k, n_out, "zero rows of y")
            assert bool((dx0[zy.to(device)] == 0).all()) and bool((dx0[~zy.to(device)] != 0).any()), (n, k, n_out, "zero rows of dx")
            _, _, hw, hb = run(x, dy, b)
            ref = torch.nn.functional.linear(x.double(), w.double(), b.double())
            gw, gb = torch.autograd.grad(ref, [w, b], dy.double())
            for name, a, r in (("dW", hw, gw), ("db", hb, gb)):
                err = float((a.double() - r).abs().max()) / max(float(r.abs().max()), 1e-30)
                assert err < 2e-5, (n, k, n_out, name, err)


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_scale_rule_is_exact_emu():
    _check_scale_rule(N.EMU_LIB, "cpu")


@pytest.mark.gpu
def test_scale_rule_is_exact_hip():
    _check_scale_rule(None, "cuda:0")


# (k, n_out, relu): K = 256 (the stream form of the layer kernel where n allows it), a narrow input, K beyond 256 (17 k16 blocks), no ReLU
TILE_SHAPES = [(256, 256, True), (84, 256, True), (272, 224, True), (256, 256, False)]


def _check_rows_do_not_depend_on_their_tile(library, device, pairs, want_ws):
    """Row r of y is a function of row r of x, W and b alone (the row scale is per row, the summation order over K is fixed), and row r of dx of
    row r of dy, y and W alone.  So a short call on the first rows of a long call's input returns the long call's first rows to the bit, whichever
    workgroup, wave group, LDS buffer, staging register set, walk direction (it alternates from launch to launch) or ragged last tile a row met.
    Both calls of a pair must take the same kernels: the launch records of the two calls are the same sequence of (name, kind, nt, N, K).  The
    records do not tell the stream form of layer_gemm_ws from the general one (same name and nt); the host picks between them by K, the epilogue
    and `n % 32 == 0` only (ws_stream_ok), so a pair is two multiples of 32 or two ragged counts, which is asserted as well."""
    import color_neus_amd as cn
    lib = cn.load_library(library)
    g = torch.Generator().manual_seed(2)
    lib.timing_enable(True)
    try:
        for k, n_out, relu in TILE_SHAPES:
            w = (torch.randn(n_out, k, generator=g) / k ** 0.5).to(device).requires_grad_(True)
            b = (torch.randn(n_out, generator=g) * 0.1).to(device).requires_grad_(True)
            for n_short, n_long in pairs:
                assert (n_short % 32 == 0) == (n_long % 32 == 0), (n_short, n_long)
                x = torch.randn(n_long, k, generator=g).to(device)
                dy = torch.randn(n_long, n_out, generator=g).to(device)

                def run(n):
                    lib.timing_collect()
                    xin = x[:n].clone().requires_grad_(True)
                    y = HipLinear.apply(lib, xin, w, b, relu)
                    (dx,) = torch.autograd.grad(y, [xin], dy[:n].contiguous())
                    if xin.is_cuda:
                        torch.cuda.synchronize()
                    return y.detach(), dx, [(rec[0], rec[1], rec[2], rec[4], rec[5]) for rec in lib.timing_collect()]

                ys, dxs, recs_s = run(n_short)
                yl, dxl, recs_l = run(n_long)
                print("rows / tile:", (k, n_out, relu), (n_short, n_long), recs_l)
                assert recs_s == recs_l, (k, n_out, relu, n_short, n_long, recs_s, recs_l)
                if want_ws:
                    assert any(rec[0] in ("layer_gemm_ws", "layer_dw") for rec in recs_l), recs_l
                assert torch.equal(ys, yl[:n_short]), (k, n_out, relu, n_short, n_long, "y", float((ys - yl[:n_short]).abs().max()))
                assert torch.equal(dxs, dxl[:n_short]), (k, n_out, relu, n_short, n_long, "dx", float((dxs - dxl[:n_short]).abs().max()))
                assert bool((yl != 0).any()) and bool((dxl != 0).any())
    finally:
        lib.timing_enable(False)


@pytest.mark.skipif(not os.path.isfile(N.EMU_LIB), reason="emulation library not built")
def test_rows_do_not_depend_on_their_tile_emu():
    _check_rows_do_not_depend_on_their_tile(N.EMU_LIB, "cpu", [(37, 200), (64, 192)], False)


@pytest.mark.gpu
def test_rows_do_not_depend_on_their_tile_hip():
    # 513 tiles: 3 tiles per workgroup, both LDS buffers and both staging sets | a 5-row last tile against a 3-row one
    _check_rows_do_not_depend_on_their_tile(None, "cuda:0", [(64, 16416), (37, 16419)], True)
