"""The operand fetch of the direct fp32 convolutions (csrc/conv.hip) goes through buffer descriptors: a zero row, a column beside
a pass that does not wrap and a surplus pixel are offsets the descriptor's range check rejects, the advance from chunk to chunk is a
scalar offset.  What that addressing can get wrong, on the smallest shapes that reach it --
bit for bit against the float64 reference on the small-integer data of tests/conv_ref.py, every buffer inside a poisoned arena:

  * zero rows and image edges (one row, W = 2, W = 3, an odd width with its seam, overhanging tiles);
  * a NaN at element 0 and in the last element of an operand reaches only the outputs whose stencil touches it;
  * one descriptor per image: with three images, whose last one ends where the arena's poison begins, a read behind an image's end
    would show;
  * the 1x1 layers at their chunk depth (16 channels), four to thirty-two chunks, C = 160 included;
  * tiles that hang over the image by more than two image widths.
"""
import ctypes

import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv_exact import Run, _dev, _guarded, _p, _stream, _wgrad_layer, run_case

pytestmark = pytest.mark.gpu

C = cc.Case
CASES = [
    # zero rows and edges through the range check: forward, strided input gradient, weight gradients (run_case runs them all)
    C(2, 1, 2, 64, 64, 3, (1, 2), why="one row: both neighbours are zero rows; W = 2"),
    C(1, 3, 3, 64, 64, 3, (2, 2), why="W = 3: odd, the narrowest seam"),
    C(2, 19, 45, 64, 64, 3, (2, 2), why="odd width: phases that do not wrap + seam, two row tiles, overhang"),
    # one descriptor per image: three images, the operand's last image ends where the poison begins
    C(3, 5, 6, 64, 64, 3, (2, 2), why="three images"), C(3, 3, 34, 64, 64, 3, (1, 2), why="three images, two chunks per row"),
    C(3, 4, 6, 64, 64, 1, (2, 2), why="three images, 1x1"),
    # 1x1 at its chunk depth of 16 channels: 4, 10 and 32 chunks forward, 4 and 32 in the dense input gradient (its reduction runs over K)
    C(1, 8, 128, 64, 64, 1, (1, 2)), C(1, 8, 128, 160, 64, 1, (1, 2)), C(1, 8, 128, 512, 64, 1, (1, 2)), C(1, 8, 128, 64, 512, 1, (1, 2)),
    C(1, 8, 45, 64, 64, 1, (2, 2)), C(1, 8, 45, 160, 64, 1, (2, 2)), C(1, 8, 45, 512, 64, 1, (2, 2)),
    # tiles that overhang beyond 2W: the column wrap is two conditional steps, not a modulo
    C(1, 7, 23, 128, 64, 3, (1, 1), why="width 23 under 32-column tiles"), C(1, 7, 2, 128, 64, 3, (1, 1), why="W = 2 under 16-column tiles: 8 W"),
]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_addressing_case_equals_the_float64_reference(case):
    dev = _dev()
    bad = _guarded(run_case, case, dev)
    util.measured(f"conv addressing {case.id}: elements that differ from float64", bad, bound=0)


def _nan_ends(t):
    t = t.clone()
    t.view(-1)[0] = float("nan")
    t.view(-1)[-1] = float("nan")
    return t


def _check_nan_pass(got, ref, what, rows_axis=1):
    """Outside the reference's NaNs: bit-exact and finite; inside: NaN.  The first and the last output row must hold finite pixels."""
    got = got.detach().cpu().double()
    touched = torch.isnan(ref)
    assert 0 < int(touched.sum()) < ref.numel() // 4, what
    clean = ~touched
    assert bool(torch.isfinite(got[clean]).all()), f"{what}: a NaN leaked into {int((~torch.isfinite(got[clean])).sum())} outputs whose stencil does not touch it"
    bad = int((got[clean] != ref[clean]).sum())
    missing = int((~torch.isnan(got[touched])).sum())
    first, last = clean.select(rows_axis, 0), clean.select(rows_axis, ref.shape[rows_axis] - 1)
    assert int(first.sum()) > first.numel() // 2 and int(last.sum()) > last.numel() // 2, what
    return bad + missing


def _nan_contract(dev):
    from delora_amd import _lib
    lib = _lib.load()
    c = C(2, 19, 45, 64, 64, 3, (2, 2))
    r = Run(c, dev)
    bad = 0
    # forward: NaN in x
    xn = _nan_ends(r.x)
    xn_d = r.A.arena(xn.shape, torch.float32, xn, "x with NaN")
    y_d = r.out(tuple(r.y0.shape), name="y")
    r.ok(lib.dl_conv2d_nhwc_f32(_p(xn_d), _p(r.w_d), _p(y_d), _p(None), _p(None), c.N, c.H, c.W, c.C, c.K, 3, 2, 2, 0, 0, 0, _stream()), "dl_conv2d_nhwc_f32")
    torch.cuda.synchronize()
    r.A.check("NaN contract, forward")
    bad += _check_nan_pass(y_d, cr.conv(xn, r.w, c.stride), "forward")
    # gradients: NaN in g
    gn = _nan_ends(r.g)
    gn_d = r.A.arena(gn.shape, torch.float32, gn, "g with NaN")
    dx0, dw0 = cr.conv_grads(r.x, r.w, gn, c.stride)
    dx_d = r.out(tuple(r.x.shape), name="dx")
    seam = r.out((c.N, c.H, 2, c.C), torch.float32, "seam_ws", 0)
    r.ok(lib.dl_conv2d_dgrad_strided_nhwc_f32(_p(gn_d), _p(r.w_d), _p(dx_d), _p(None), _p(None), c.N, c.H, c.W, c.K, c.C, 3, 2, 2, 0, 0, 0, _p(seam),
                                              _stream()), "dl_conv2d_dgrad_strided_nhwc_f32")
    torch.cuda.synchronize()
    r.A.check("NaN contract, strided input gradient")
    bad += _check_nan_pass(dx_d, dx0, "strided input gradient")
    # weight gradient (single and merged).  NaNs in g: g[.., k] with k = 0 and k = K - 1 carry them -- every other row of dW is exact.
    # NaNs in x: x[0, 0, 0, 0] and the last element of the last image, next to the zero rows above and below the image that rest on
    # the range check (a clamped read instead of a rejected one would fetch them) -- only dW's columns c = 0 and c = C - 1 may see them.
    g_d = r.g_d
    _, dw0x = cr.conv_grads(xn, r.w, r.g, c.stride)
    for side, xs_d, gs_d, ref, ax in (("g", r.x_d, gn_d, dw0, 0), ("x", xn_d, g_d, dw0x, 3)):
        r.x_d, r.g_d = xs_d, gs_d
        n_ax = ref.shape[ax]
        assert bool(torch.isnan(ref.select(ax, 0)).any()) and bool(torch.isnan(ref.select(ax, n_ax - 1)).any())
        assert bool(torch.isfinite(ref.narrow(ax, 1, n_ax - 2)).all())
        for merged in (False, True):
            dw = r.out(tuple(ref.shape), torch.float32, "dw", 0)
            if merged:
                arr = _wgrad_layer(r, dw)
                ap = ctypes.cast(arr, ctypes.c_void_p)
                ws = r.ws(int(lib.dl_conv2d_wgrad_batch_workspace_bytes(ap, 1)))
                r.ok(lib.dl_conv2d_wgrad_batch_nhwc_f32(ap, 1, _p(ws), _stream()), "dl_conv2d_wgrad_batch_nhwc_f32")
            else:
                ws = r.ws(int(lib.dl_conv2d_wgrad_workspace_bytes(c.N, c.H, c.W, c.C, c.K, 3, 2, 2)))
                r.ok(lib.dl_conv2d_wgrad_nhwc_f32(_p(r.x_d), _p(r.g_d), _p(dw), _p(ws), c.N, c.H, c.W, c.C, c.K, 3, 2, 2, _stream()), "dl_conv2d_wgrad_nhwc_f32")
            torch.cuda.synchronize()
            r.A.check(f"NaN contract, weight gradient, NaNs in {side}")
            got = dw.detach().cpu().double().narrow(ax, 1, n_ax - 2)
            assert bool(torch.isfinite(got).all()), f"weight gradient: a NaN of {side} leaked into entries of dW that do not read it"
            bad += int((got != ref.narrow(ax, 1, n_ax - 2)).sum())
    return bad


def test_a_nan_at_either_end_of_an_operand_stays_in_its_stencil():
    dev = _dev()
    bad = _guarded(_nan_contract, dev)
    util.measured("conv addressing, NaN at element 0 and in the last element: outputs that differ from float64", bad, bound=0)
