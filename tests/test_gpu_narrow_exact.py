"""The narrow family's members for narrow pose networks (csrc/narrow.hip: stride (1,2), 1x1 filters, residual add, the strided layers'
input gradient) against a float64 CPU reference, BIT FOR BIT, on small-integer data in poisoned arenas -- the method of
tests/test_gpu_tower_exact.py: ``headroom`` proves per case that every product and partial sum is an fp32 number, so no tile shape,
chunking, zero insertion or slab plan may change a bit; every pointer is a view inside a NaN-filled allocation.

Cases (N, H, W, C, K, ksize, stride):
  (1,1,4,8,16,3,(1,2))      the smallest image: both wrap taps hit live columns; one row (both zero rows)
  (2,5,7,16,32,3,(1,2))     odd width: the last output's right tap wraps; a fifth row overhangs the 4-row tile
  (1,4,130,32,64,3,(1,2))   65 output columns: a tile seam (tiles are 32 output columns at stride 2), the wrap read from the far tile
  (2,3,8,8,32,3,(1,2))      the stem's channel pair
  (2,3,6,32,64,1,(1,2)), (1,6,258,16,32,1,(1,2))   the 1x1 shortcut, small and across a seam
  (2,5,66,32,32,3,(1,1)), (1,1,1,16,16,3,(1,1))    the residual epilogue; a one-pixel ring that wraps onto itself
"""
import ctypes

import pytest
import torch

from tests import conv_ref as cr
from tests import util

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 4, 8, 16, 3, (1, 2)), (2, 5, 7, 16, 32, 3, (1, 2)), (1, 4, 130, 32, 64, 3, (1, 2)), (2, 3, 8, 8, 32, 3, (1, 2)),
         (2, 3, 6, 32, 64, 1, (1, 2)), (1, 6, 258, 16, 32, 1, (1, 2)), (2, 5, 66, 32, 32, 3, (1, 1)), (1, 1, 1, 16, 16, 3, (1, 1))]
IDS = [f"{n}x{h}x{w}-{c}to{k}-k{ks}-s{s[1]}" for (n, h, w, c, k, ks, s) in CASES]
AMAX = 8
ADD, ACT, DACT, ADD_GRID = cr.EPI_ADD, cr.EPI_ACT, cr.EPI_DACT, cr.EPI_ADD_GRID


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _finish(A, out, ref, what):
    _sync()
    A.check(what)
    A.check_output(out, what)
    return cr.mismatches(out, ref.float(), what, (4, 32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_equals_float64(case):
    """Plain, with relu in the epilogue, and -- where the layer closes a residual block (stride 1, C == K) -- with ADD and ADD | ACT."""
    dev = _dev()
    L, lib = _lib()
    N, H, W, C, K, ks, stride = case
    cr.headroom("direct", C, AMAX, AMAX, taps=ks * ks, add=AMAX)
    sd = 7000 + 100 * C + 10 * W + H + ks
    x, w = cr.ints((N, H, W, C), AMAX, sd + 1), cr.ints((K, ks, ks, C), AMAX, sd + 2)
    pre = cr.conv(x, w, stride)
    assert pre.shape == (N, H, cr.out_size(W, 2) if stride[1] == 2 else W, K)
    A = cr.Arenas(dev)
    x_d, w_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(w.shape, torch.float32, w, "w", row_elems=0)
    runs = [(0, 0, None), (ACT, cr.ACT_RELU, None)]
    if stride == (1, 1) and C == K:
        res = cr.ints(pre.shape, AMAX, sd + 3)
        runs += [(ADD, 0, res), (ADD | ACT, cr.ACT_RELU, res)]
    bad = 0
    for flags, act, res in runs:
        res_d = A.arena(res.shape, torch.float32, res, "add") if res is not None else None
        y_d = A.arena(pre.shape, torch.float32, None, "y")
        L.check(lib.dl_narrow_conv2d_nhwc_f32(_p(x_d), _p(w_d), _p(y_d), _p(res_d), None, N, H, W, C, K, ks, stride[0], stride[1], 0, act, flags,
                                              _stream()), "dl_narrow_conv2d_nhwc_f32")
        bad += _finish(A, y_d, cr.epilogue(pre, flags, act, add=res), f"narrow forward {case} tail {flags}/{act}")
    util.measured(f"narrow exact forward {IDS[CASES.index(case)]}: elements that differ from float64", bad, bound=0)


@pytest.mark.parametrize("case", [c for c in CASES if c[3] != 8], ids=[i for c, i in zip(CASES, IDS) if c[3] != 8])
def test_input_gradient_equals_float64_autograd(case):
    """Plain and with DACT on a saved relu / tanh map; as the trunk calls it: a stride-1 layer with ADD | DACT (the shortcut's gradient),
    a strided 3x3 layer with ADD_GRID | DACT (the 1x1 branch's gradient on the even columns), a strided 1x1 layer dense on the grid --
    and at full resolution, where every odd column is zero."""
    dev = _dev()
    L, lib = _lib()
    N, H, W, C, K, ks, stride = case
    Wo = cr.out_size(W, stride[1])
    sd = 8000 + 100 * C + 10 * W + H + ks
    g, w = cr.ints((N, H, Wo, K), AMAX, sd + 1), cr.ints((K, ks, ks, C), AMAX, sd + 2)
    dx0 = cr.conv_dx((N, H, W, C), w, g, stride)
    A = cr.Arenas(dev)
    g_d, w_d = A.arena(g.shape, torch.float32, g, "g"), A.arena(w.shape, torch.float32, w, "w", row_elems=0)
    sv_r, sv_t = cr.saved_relu(dx0.shape, sd + 5), cr.saved_tanh(dx0.shape, sd + 6)
    addend = cr.ints(dx0.shape if stride == (1, 1) else (N, H, Wo, C), AMAX, sd + 7)
    f_add = ADD if stride == (1, 1) else ADD_GRID
    runs = [(0, 0, None, None), (DACT, cr.ACT_RELU, sv_r, None), (DACT, cr.ACT_TANH, sv_t, None)]
    if ks == 3:
        runs += [(f_add, 0, None, addend), (f_add | DACT, cr.ACT_RELU, sv_r, addend), (f_add | DACT, cr.ACT_TANH, sv_t, addend)]
    bad = 0
    for flags, act, sv, add in runs:
        cr.headroom("direct", K, AMAX, AMAX, taps=ks * ks, add=AMAX if add is not None else 0, dact_tanh=act == cr.ACT_TANH)
        sv_d = A.arena(sv.shape, torch.float32, sv, "dsrc") if sv is not None else None
        add_d = A.arena(add.shape, torch.float32, add, "add") if add is not None else None
        dx_d = A.arena(dx0.shape, torch.float32, None, "dx")
        if stride == (1, 1):
            L.check(lib.dl_narrow_conv2d_nhwc_f32(_p(g_d), _p(w_d), _p(dx_d), _p(add_d), _p(sv_d), N, H, W, K, C, ks, 1, 1, 1, act, flags, _stream()),
                    "dl_narrow_conv2d_nhwc_f32")
            ref = cr.epilogue(dx0, flags, act, add=add, dsrc=sv)
        else:
            L.check(lib.dl_narrow_dgrad_strided_nhwc_f32(_p(g_d), _p(w_d), _p(dx_d), _p(add_d), _p(sv_d), N, H, W, K, C, ks, stride[0], stride[1], 0,
                                                         act, flags, _stream()), "dl_narrow_dgrad_strided_nhwc_f32")
            ref = cr.epilogue(dx0, flags, act, dsrc=sv, add_grid=add, stride=stride)
        bad += _finish(A, dx_d, ref, f"narrow input gradient {case} tail {flags}/{act}")
    if ks == 1 and stride != (1, 1):
        assert float(dx0[:, :, 1::2].abs().max()) == 0.0               # (only phase (0,0) receives gradient)
        dense = A.arena((N, H, Wo, C), torch.float32, None, "dx dense")
        L.check(lib.dl_narrow_dgrad_strided_nhwc_f32(_p(g_d), _p(w_d), _p(dense), None, None, N, H, W, K, C, ks, stride[0], stride[1], 1, 0, 0,
                                                     _stream()), "dl_narrow_dgrad_strided_nhwc_f32")
        bad += _finish(A, dense, dx0[:, :, ::2].contiguous(), f"narrow input gradient {case} dense")
    util.measured(f"narrow exact input gradient {IDS[CASES.index(case)]}: elements that differ from float64 autograd", bad, bound=0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weight_gradient_equals_float64_autograd_and_repeats_bitwise(case):
    dev = _dev()
    L, lib = _lib()
    N, H, W, C, K, ks, stride = case
    Wo = cr.out_size(W, stride[1])
    cr.headroom("wgrad", N * H * Wo, AMAX, AMAX)
    sd = 9000 + 100 * C + 10 * W + H + ks
    x, g = cr.ints((N, H, W, C), AMAX, sd + 1), cr.ints((N, H, Wo, K), AMAX, sd + 2)
    _, dw0 = cr.conv_grads(x, torch.zeros((K, ks, ks, C), dtype=torch.float64), g, stride)
    A = cr.Arenas(dev)
    x_d, g_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(g.shape, torch.float32, g, "g")
    nbytes = int(lib.dl_narrow_wgrad_workspace_bytes(N, H, W, C, K, ks, stride[0], stride[1]))
    assert nbytes > 0 and nbytes % 4 == 0
    outs, bad = [], 0
    for poison in (None, 12345.0):
        ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)          # exactly what the query promised
        if poison is not None:
            ws.fill_(poison)                                                                  # a differently poisoned workspace
        dw = A.arena(dw0.shape, torch.float32, None, "dw", row_elems=0)
        L.check(lib.dl_narrow_wgrad_nhwc_f32(_p(x_d), _p(g_d), _p(dw), _p(ws), N, H, W, C, K, ks, stride[0], stride[1], _stream()),
                "dl_narrow_wgrad_nhwc_f32")
        bad += _finish(A, dw, dw0, f"narrow weight gradient {case}")
        outs.append(dw)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs of the weight gradient differ bitwise"
    util.measured(f"narrow exact weight gradient {IDS[CASES.index(case)]}: elements that differ from float64 autograd", bad, bound=0)
