"""The pixel-pair Winograd form of the stride-(1,2) 3x3 layers (csrc/wino.hip: k_wino_conv_strided) BIT FOR BIT against the float64
reference and against the direct entry points, on small-integer data in poisoned arenas (the method of tests/test_gpu_conv_exact.py).

Exactness is by construction: the rearranged kernel holds the layer's own integer weights and zeros, so U = G g G^T lives on the grid
1/4, V = B^T d B holds integers, every channel sum stays below 2^23 grid steps (``conv_ref.headroom`` asserts it for the pair view's 2C
reduction channels -- an upper bound: half of them carry one tap column instead of two), and the planes the kernel leaves out are exact
zeros.  tanh is the same ``dl_tanh`` on the same value in both paths, so a forward pass with tanh must equal the direct kernel's bit
for bit although neither equals float64.

Shapes are given as the pair view H' x W' the kernel tiles (the layer's image is H' x 2W'):
  4x64   one 2x32 tile group, wrapping onto itself        8x32   one 4x16 group
  4x128  two groups across the wrap                       8x64   two 4x16 groups side by side, zero rows at the image edge only
with 64 -> 128 and 128 -> 64 channels: the boundary between the even- and the odd-pixel channels then falls inside a workgroup's
chunk range, and the input gradient has one and two 64-channel output blocks per pixel phase (only the even-pixel blocks add the
down-sampling branch's gradient).  Stride (2,2) is not built: layer4.0 stays on the direct kernel.
"""
import numpy as np
import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv_exact import ACT, ADD_GRID, DACT, RELU, TANH, Run, _dev, _guarded, _p, _stream

pytestmark = pytest.mark.gpu

XMAX, WMAX = 4, 3
VIEWS = [(4, 64), (8, 32), (4, 128), (8, 64)]
CHANNELS = [(64, 128), (128, 64)]
CASES = [cc.Case(2, h, 2 * w, c, k, 3, (1, 2), xmax=XMAX, wmax=WMAX) for (h, w) in VIEWS for (c, k) in CHANNELS]
FWD = [(0, 0), (ACT, RELU), (ACT, TANH)]
BWD = [(0, 0, None), (ADD_GRID, 0, None), (ADD_GRID | DACT, TANH, "tanh"), (ADD_GRID | DACT, RELU, "relu")]


def _strided_weights(r):
    c = r.c
    n = int(r.lib.dl_wino_strided_weights_floats(c.K, c.C, 1, 2))
    assert n == 16 * c.K * 2 * c.C
    uf, ub = r.out((n,), torch.float32, "u_fwd", 0), r.out((n,), torch.float32, "u_bwd", 0)
    r.ok(r.lib.dl_wino_strided_weights_f32(_p(r.w_d), _p(uf), _p(ub), c.K, c.C, 1, 2, _stream()), "dl_wino_strided_weights_f32")
    torch.cuda.synchronize()
    r.A.check(f"{c.id} weight preparation")
    for t in (uf, ub):
        r.A.check_output(t, f"{c.id} weight preparation")
        r.A.freeze(t)
    return uf, ub


def run_strided(case, dev):
    r = Run(case, dev)
    c, lib = case, r.lib
    # the pair view's sums: 2C reduction channels forward, K backward, the grid operand (<= 3) and tanh' on top
    cr.headroom("wino_conv", 2 * c.C, c.xmax, c.wmax, add=3, dact_tanh=True)
    cr.headroom("wino_conv", c.K, c.xmax, c.wmax, add=3, dact_tanh=True)
    assert lib.dl_wino_strided_takes(c.N, c.H, c.W, c.C, c.K, 1, 2, 1) == 1, "the case must be one the dispatch can take"
    uf, ub = _strided_weights(r)
    yshape, xshape = tuple(r.y0.shape), tuple(r.x.shape)
    for flags, act in FWD:
        y_new, y_dir = r.out(yshape, name="y (pixel-pair Winograd)"), r.out(yshape, name="y (direct)")
        r.ok(lib.dl_wino_strided_conv3x3_nhwc_f32(_p(r.x_d), _p(uf), _p(y_new), c.N, c.H, c.W, c.C, c.K, 1, 2, act, flags, _stream()),
             "dl_wino_strided_conv3x3_nhwc_f32")
        r.ok(lib.dl_conv2d_nhwc_f32(_p(r.x_d), _p(r.w_d), _p(y_dir), None, None, c.N, c.H, c.W, c.C, c.K, 3, 1, 2, 0, act, flags, _stream()),
             "dl_conv2d_nhwc_f32")
        what = f"forward, tail {flags}/{act}"
        if act == TANH:                                  # not exact against float64; the two kernels must still agree to the bit
            torch.cuda.synchronize()
            r.A.check(f"{c.id} {what}")
            r.A.check_output(y_new, f"{c.id} {what}")
            r.A.check_output(y_dir, f"{c.id} {what}")
        else:
            ref = cr.epilogue(r.y0, flags, act)
            r.compare(y_new, ref, "pixel-pair Winograd " + what)
            r.compare(y_dir, ref, "direct " + what, (8, 64))
        r.bad += cr.mismatches(y_new, y_dir.detach().cpu(), f"{c.id} pixel-pair Winograd against direct, {what}")
    gshape = (c.N, c.Ho, c.Wo, c.C)
    for i, (flags, act, kind) in enumerate(BWD):
        _, sv, _, sv_d = r.tail_operands(xshape, flags, kind, 50 + 2 * i)
        addg = cr.ints(gshape, 3, c.seed(60 + i)) if flags & ADD_GRID else None
        addg_d = r.A.arena(gshape, r.dt, addg, "add_grid") if addg is not None else None
        ref = cr.epilogue(r.dx0, flags, act, None, sv, addg, c.stride)
        dx_new, dx_dir = r.out(xshape, name="dx (pixel-pair Winograd)"), r.out(xshape, name="dx (direct)")
        r.ok(lib.dl_wino_strided_dgrad3x3_nhwc_f32(_p(r.g_d), _p(ub), _p(dx_new), _p(addg_d), _p(sv_d), c.N, c.H, c.W, c.K, c.C, 1, 2, act, flags,
                                                   _stream()), "dl_wino_strided_dgrad3x3_nhwc_f32")
        r.ok(lib.dl_conv2d_dgrad_strided_nhwc_f32(_p(r.g_d), _p(r.w_d), _p(dx_dir), _p(addg_d), _p(sv_d), c.N, c.H, c.W, c.K, c.C, 3, 1, 2, 0, act,
                                                  flags, None, _stream()), "dl_conv2d_dgrad_strided_nhwc_f32")
        what = f"input gradient, tail {flags}/{act}"
        r.compare(dx_new, ref, "pixel-pair Winograd " + what)
        r.compare(dx_dir, ref, "direct " + what, (8, 64))
        assert torch.equal(dx_new, dx_dir), f"{c.id}: the two input gradients differ from each other ({what})"
    return r.bad


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pixel_pair_winograd_equals_float64_and_the_direct_kernel(case):
    dev = _dev()
    bad = _guarded(run_strided, case, dev)
    util.measured(f"strided Winograd exact {case.id}: elements that differ", bad, bound=0)


def test_all_ones_weights_against_numpy_box_sums():
    """With every weight 1 the layer is a box sum: rows h-1..h+1 inside the image, columns 2j-1..2j+1 around the wrap, all channels.
    The expected values come from numpy alone, so the comparison does not lean on the direct kernel or on torch's convolution."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    N, H, W, C, K = 2, 8, 128, 64, 64
    cr.headroom("wino_conv", 2 * C, XMAX, 1)
    x = cr.ints((N, H, W, C), XMAX, 4242)
    g = cr.ints((N, H, W // 2, K), XMAX, 4243)
    xs = x.numpy().sum(axis=3)                                                  # [N,H,W]
    cols = np.roll(xs, 1, axis=2) + xs + np.roll(xs, -1, axis=2)                # columns w-1..w+1 (wrapped)
    rows = cols.copy()
    rows[:, 1:] += cols[:, :-1]
    rows[:, :-1] += cols[:, 1:]
    y_ref = np.repeat(rows[:, :, 0::2, None], K, axis=3)                         # output column j sits on image column 2j
    gs = g.numpy().sum(axis=3)                                                  # [N,H,W/2]
    up = np.zeros((N, H, W))
    up[:, :, 0::2] = gs                                                         # g on the image grid, then the same box sum (the box is symmetric)
    cols = np.roll(up, 1, axis=2) + up + np.roll(up, -1, axis=2)
    rows = cols.copy()
    rows[:, 1:] += cols[:, :-1]
    rows[:, :-1] += cols[:, 1:]
    dx_ref = np.repeat(rows[:, :, :, None], C, axis=3)
    A = cr.Arenas(dev)
    x_d, g_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(g.shape, torch.float32, g, "g")
    w_d = A.arena((K, 3, 3, C), torch.float32, torch.ones((K, 3, 3, C), dtype=torch.float64), "w", 0)
    n = int(lib.dl_wino_strided_weights_floats(K, C, 1, 2))
    uf, ub = A.arena((n,), torch.float32, None, "u_fwd", 0), A.arena((n,), torch.float32, None, "u_bwd", 0)
    y_d, dx_d = A.arena(y_ref.shape, torch.float32, None, "y"), A.arena(dx_ref.shape, torch.float32, None, "dx")
    _lib.check(lib.dl_wino_strided_weights_f32(_p(w_d), _p(uf), _p(ub), K, C, 1, 2, _stream()), "dl_wino_strided_weights_f32")
    _lib.check(lib.dl_wino_strided_conv3x3_nhwc_f32(_p(x_d), _p(uf), _p(y_d), N, H, W, C, K, 1, 2, 0, 0, _stream()), "dl_wino_strided_conv3x3_nhwc_f32")
    _lib.check(lib.dl_wino_strided_dgrad3x3_nhwc_f32(_p(g_d), _p(ub), _p(dx_d), None, None, N, H, W, K, C, 1, 2, 0, 0, _stream()),
               "dl_wino_strided_dgrad3x3_nhwc_f32")
    torch.cuda.synchronize()
    A.check("all-ones weights")
    for t in (uf, ub, y_d, dx_d):
        A.check_output(t, "all-ones weights")
    bad = cr.mismatches(y_d, torch.from_numpy(y_ref).float(), "all-ones weights, forward against numpy box sums")
    bad += cr.mismatches(dx_d, torch.from_numpy(dx_ref).float(), "all-ones weights, input gradient against numpy box sums")
    util.measured("strided Winograd exact, all-ones weights against numpy box sums: elements that differ", bad, bound=0)
