"""The narrow convolution family (csrc/tower.hip) against a float64 CPU reference, BIT FOR BIT, on small-integer data in poisoned
arenas -- the method of tests/test_gpu_conv_exact.py: on the data of tests/conv_ref.py every product and partial sum is an fp32
number (``headroom`` proves it per case), so no tile shape, chunking or slab plan may change a bit.  Every pointer is a view inside
a NaN-filled allocation: a write beside a buffer, an unwritten element and a workspace assumed to be zero all show.

The kernels tile an image in 4 rows x 64 columns (a tile never leaves its image) and walk the weight gradient in 256-column
segments of a row.  Shapes: the four of the issue, a width of exactly one tile (64), a tile + 4 (68, among the four), and (1, 4)
with N = 3, whose whole batch is smaller than one tile; 260 crosses a weight-gradient segment.  Together: the wrap seam, the zero
rows, overhang in both directions, several images.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import util

pytestmark = pytest.mark.gpu

N_IMG = 3
SHAPES = [(1, 4), (3, 20), (6, 68), (5, 132), (4, 64), (2, 260)]
FWD_PAIRS = [(4, 8), (8, 16), (16, 24), (24, 32), (32, 40)]
WIDE_PAIRS = [(48, 64), (64, 48)]                            # the upper end of the domain: four 16-channel tiles either way
BWD_PAIRS = [(40, 32), (32, 24), (24, 16), (16, 8)]           # (reduction channels = the layer's outputs, result channels)
AMAX = 8
ACT, DACT = cr.EPI_ACT, cr.EPI_DACT
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _view(pitch, offset=0, group=1):
    return (ctypes.c_int32 * 3)(pitch, offset, group)


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def _conv(lib, x, w, y, dsrc, N, H, W, C, K, xv, yv, dv, transposed, act, flags):
    return lib.dl_tower_conv3x3_nhwc_f32(_p(x), _p(w), _p(y), _p(dsrc), N, H, W, C, K, xv, yv, dv, transposed, act, flags, _stream())


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
    return cr.mismatches(out, ref.float(), what, (4, 64))


def _ulps(got, ref64):
    """Largest distance of fp32 ``got`` from the float64 values ``ref64`` in units of the fp32 spacing at the reference."""
    ref32 = ref64.float().numpy()
    err = np.abs(got.detach().cpu().double().numpy() - ref64.numpy())
    return float((err / np.spacing(np.maximum(np.abs(ref32), np.float32(2.0 ** -126)))).max())


@pytest.mark.parametrize("hw,pair", [(hw, p) for p in FWD_PAIRS for hw in SHAPES] + [((6, 68), p) for p in WIDE_PAIRS],
                         ids=[f"{h}x{w}-{c}to{k}" for (c, k) in FWD_PAIRS for (h, w) in SHAPES] + [f"6x68-{c}to{k}" for c, k in WIDE_PAIRS])
def test_forward_equals_float64(hw, pair):
    """act none and relu: ``==``; tanh on the same integer pre-activations: within 2 ulp of tanh in float64 (the bound csrc/common.h
    documents for dl_tanh)."""
    dev = _dev()
    L, lib = _lib()
    (H, W), (C, K), N = hw, pair, N_IMG
    cr.headroom("direct", C, AMAX, AMAX)
    sd = 1000 * C + 10 * W + H
    x, w = cr.ints((N, H, W, C), AMAX, sd + 1), cr.ints((K, 3, 3, C), AMAX, sd + 2)
    pre = cr.conv(x, w)
    A = cr.Arenas(dev)
    x_d, w_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(w.shape, torch.float32, w, "w", row_elems=0)
    bad = 0
    for act, flags, ref in ((0, 0, pre), (cr.ACT_RELU, ACT, torch.relu(pre))):
        y_d = A.arena(pre.shape, torch.float32, None, "y")
        L.check(_conv(lib, x_d, w_d, y_d, None, N, H, W, C, K, _view(C), _view(K), None, 0, act, flags), "dl_tower_conv3x3_nhwc_f32")
        bad += _finish(A, y_d, ref, f"tower forward {C}->{K} {H}x{W} act {act}")
    util.measured(f"tower exact forward {C}->{K} {H}x{W}: elements that differ from float64", bad, bound=0)
    y_d = A.arena(pre.shape, torch.float32, None, "y tanh")
    L.check(_conv(lib, x_d, w_d, y_d, None, N, H, W, C, K, _view(C), _view(K), None, 0, cr.ACT_TANH, ACT), "dl_tower_conv3x3_nhwc_f32")
    _sync()
    A.check("tanh")
    A.check_output(y_d, "tanh")
    util.measured(f"tower forward with tanh {C}->{K} {H}x{W}: ulp from tanh in float64", _ulps(y_d, torch.tanh(pre)), bound=2.0)


@pytest.mark.parametrize("hw,pair", [(hw, p) for p in BWD_PAIRS for hw in SHAPES] + [((6, 68), p) for p in WIDE_PAIRS],
                         ids=[f"{h}x{w}-{k}to{c}" for (k, c) in BWD_PAIRS for (h, w) in SHAPES] + [f"6x68-{k}to{c}" for k, c in WIDE_PAIRS])
def test_input_gradient_equals_float64_autograd(hw, pair):
    dev = _dev()
    L, lib = _lib()
    (H, W), (K, C), N = hw, pair, N_IMG             # the layer: C -> K channels; its input gradient reduces over K
    sd = 2000 * K + 10 * W + H
    g, w = cr.ints((N, H, W, K), AMAX, sd + 1), cr.ints((K, 3, 3, C), AMAX, sd + 2)
    dx0, _ = cr.conv_grads(torch.zeros((N, H, W, C), dtype=torch.float64), w, g)
    A = cr.Arenas(dev)
    g_d, w_d = A.arena(g.shape, torch.float32, g, "g"), A.arena(w.shape, torch.float32, w, "w", row_elems=0)
    bad = 0
    for flags, act, kind in ((0, 0, None), (DACT, cr.ACT_RELU, "relu"), (DACT, cr.ACT_TANH, "tanh")):
        cr.headroom("direct", K, AMAX, AMAX, dact_tanh=kind == "tanh")
        sv = sv_d = None
        if kind:
            sv = cr.saved_tanh(dx0.shape, sd + 5) if kind == "tanh" else cr.saved_relu(dx0.shape, sd + 6)
            sv_d = A.arena(sv.shape, torch.float32, sv, "dsrc")
        ref = dx0 * cr.dact(sv, act) if kind else dx0
        dx_d = A.arena(dx0.shape, torch.float32, None, "dx")
        L.check(_conv(lib, g_d, w_d, dx_d, sv_d, N, H, W, K, C, _view(K), _view(C), _view(C) if kind else None, 1, act, flags),
                "dl_tower_conv3x3_nhwc_f32")
        bad += _finish(A, dx_d, ref, f"tower input gradient {K}->{C} {H}x{W} tail {flags}/{act}")
    util.measured(f"tower exact input gradient {K}->{C} {H}x{W}: elements that differ from float64 autograd", bad, bound=0)


@pytest.mark.parametrize("hw,pair", [(hw, p) for p in FWD_PAIRS for hw in SHAPES] + [((6, 68), p) for p in WIDE_PAIRS],
                         ids=[f"{h}x{w}-{c}to{k}" for (c, k) in FWD_PAIRS for (h, w) in SHAPES] + [f"6x68-{c}to{k}" for c, k in WIDE_PAIRS])
def test_weight_gradient_equals_float64_autograd_and_repeats_bitwise(hw, pair):
    dev = _dev()
    L, lib = _lib()
    (H, W), (C, K), N = hw, pair, N_IMG
    cr.headroom("wgrad", N * H * W, AMAX, AMAX)
    sd = 3000 * C + 10 * W + H
    x, g = cr.ints((N, H, W, C), AMAX, sd + 1), cr.ints((N, H, W, K), AMAX, sd + 2)
    _, dw0 = cr.conv_grads(x, torch.zeros((K, 3, 3, C), dtype=torch.float64), g)
    A = cr.Arenas(dev)
    x_d, g_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(g.shape, torch.float32, g, "g")
    nbytes = int(lib.dl_tower_wgrad_workspace_bytes(N, H, W, C, K))
    assert nbytes > 0 and nbytes % 4 == 0
    outs, bad = [], 0
    for poison in (None, 12345.0):
        ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)          # exactly what the query promised
        if poison is not None:
            ws.fill_(poison)                                                                  # a differently poisoned workspace
        dw = A.arena(dw0.shape, torch.float32, None, "dw", row_elems=0)
        L.check(lib.dl_tower_wgrad3x3_nhwc_f32(_p(x_d), _p(g_d), _p(dw), _p(ws), N, H, W, C, K, _view(C), _view(K), _stream()),
                "dl_tower_wgrad3x3_nhwc_f32")
        bad += _finish(A, dw, dw0, f"tower weight gradient {C}->{K} {H}x{W}")
        outs.append(dw)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs of the weight gradient differ bitwise"
    util.measured(f"tower exact weight gradient {C}->{K} {H}x{W}: elements that differ from float64 autograd", bad, bound=0)


def _poison_left(buf, used_channels):
    """Words of a [.., 128] arena outside channels [0, used_channels) that no longer hold the arena's NaN pattern."""
    word = cr._as_i32(cr.NAN_WORD[torch.float32])
    return int((buf.view(torch.int32)[..., used_channels:] != word).sum())


@pytest.mark.parametrize("mode", ["one launch, group 2", "two launches, offsets 0 and 40"])
@pytest.mark.parametrize("hw", [(3, 20), (6, 68)], ids=["3x20", "6x68"])
def test_layer_five_writes_both_slices_of_a_wide_buffer_and_the_backward_reads_them(hw, mode):
    """The fifth layer of two images of a sample writes channels 0..39 and 40..79 of a NaN-filled [B,H,W,128] buffer through its
    view: both slices exact, every other word still poison.  The input gradient and the weight gradient then read their operand
    from such slices of a buffer that holds NaN everywhere else."""
    dev = _dev()
    L, lib = _lib()
    (H, W), (C, K), B = hw, (32, 40), 2
    N = 2 * B
    grouped = mode.startswith("one")
    cr.headroom("direct", C, AMAX, AMAX)
    cr.headroom("direct", K, AMAX, AMAX, dact_tanh=True)
    cr.headroom("wgrad", N * H * W, AMAX, AMAX)
    sd = 4000 + 10 * W + H
    # image order: grouped -> n = 2 b + j (the planar [B,8,H,W] pair seen as [2B,4,H,W]); else j-major, one launch per j
    x, w = cr.ints((N, H, W, C), AMAX, sd + 1), cr.ints((K, 3, 3, C), AMAX, sd + 2)
    y0 = torch.relu(cr.conv(x, w))
    img = (lambda b, j: 2 * b + j) if grouped else (lambda b, j: j * B + b)
    wide0 = torch.stack([torch.cat([y0[img(b, 0)], y0[img(b, 1)]], dim=-1) for b in range(B)])          # [B,H,W,80]
    A = cr.Arenas(dev)
    x_d, w_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(w.shape, torch.float32, w, "w", row_elems=0)
    wide = A.arena((B, H, W, 128), torch.float32, None, "wide")

    def launches():
        return [(0, N, _view(128, 0, 2))] if grouped else [(0, B, _view(128, 0, 1)), (B, B, _view(128, 40, 1))]

    for n0, nn, yv in launches():
        L.check(_conv(lib, x_d[n0:], w_d, wide, None, nn, H, W, C, K, _view(C), yv, None, 0, cr.ACT_RELU, ACT), "dl_tower_conv3x3_nhwc_f32")
    _sync()
    A.check("layer five into the wide buffer")
    bad = cr.mismatches(wide[..., :80], wide0.float(), f"layer five slices, {mode}", (4, 64))
    left = _poison_left(wide, 80)
    assert left == 0, f"{left} words outside channels 0..79 were written"
    # ---- the backward reads from the slices: g lives in a NaN-filled wide buffer
    g = cr.ints((N, H, W, K), AMAX, sd + 3)
    gw0 = torch.stack([torch.cat([g[img(b, 0)], g[img(b, 1)]], dim=-1) for b in range(B)])
    gw = A.arena((B, H, W, 128), torch.float32, None, "g wide")
    gw[..., :80] = gw0.float().to(dev)
    A.freeze(gw)
    dx0, dw0 = cr.conv_grads(x, w, g)
    sv = cr.saved_tanh(dx0.shape, sd + 4)
    sv_d = A.arena(sv.shape, torch.float32, sv, "dsrc")
    dx = A.arena(dx0.shape, torch.float32, None, "dx")
    for n0, nn, gv in launches():
        L.check(_conv(lib, gw, w_d, dx[n0:], sv_d[n0:], nn, H, W, K, C, gv, _view(C), _view(C), 1, cr.ACT_TANH, DACT), "dl_tower_conv3x3_nhwc_f32")
    bad += _finish(A, dx, dx0 * cr.dact(sv, cr.ACT_TANH), f"input gradient from a slice, {mode}")
    if grouped:
        nbytes = int(lib.dl_tower_wgrad_workspace_bytes(N, H, W, C, K))
        ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
        dw = A.arena(dw0.shape, torch.float32, None, "dw", row_elems=0)
        L.check(lib.dl_tower_wgrad3x3_nhwc_f32(_p(x_d), _p(gw), _p(dw), _p(ws), N, H, W, C, K, _view(C), _view(128, 0, 2), _stream()),
                "dl_tower_wgrad3x3_nhwc_f32")
        bad += _finish(A, dw, dw0, f"weight gradient from a slice, {mode}")
    else:
        for j, (n0, nn, gv) in enumerate(launches()):
            _, dwj = cr.conv_grads(x[n0:n0 + nn], w, g[n0:n0 + nn])
            nbytes = int(lib.dl_tower_wgrad_workspace_bytes(nn, H, W, C, K))
            ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
            dw = A.arena(dw0.shape, torch.float32, None, "dw", row_elems=0)
            L.check(lib.dl_tower_wgrad3x3_nhwc_f32(_p(x_d[n0:]), _p(gw), _p(dw), _p(ws), nn, H, W, C, K, _view(C), gv, _stream()),
                    "dl_tower_wgrad3x3_nhwc_f32")
            bad += _finish(A, dw, dwj, f"weight gradient from slice {j}, {mode}")
    util.measured(f"tower exact wide buffer {H}x{W}, {mode}: elements that differ from float64", bad, bound=0)


def test_refusals_name_the_entry_point_and_launch_nothing():
    dev = _dev()
    L, lib = _lib()
    N, H, W = 1, 3, 20
    A = cr.Arenas(dev)
    x = A.arena((N, H, W, 64), torch.float32, torch.zeros((N, H, W, 64)), "x")
    w = A.arena((72, 3, 3, 64), torch.float32, torch.zeros((72, 3, 3, 64)), "w", row_elems=0)
    y = A.arena((N, H, W, 72), torch.float32, None, "y")
    ws = A.arena((1 << 16,), torch.float32, None, "workspace", row_elems=0)
    unsupported, invalid = -3, -1                     # DL_ERR_UNSUPPORTED, DL_ERR_INVALID_ARGUMENT

    def refused(rc, code, name):
        assert rc == code, (rc, code, lib.dl_last_error())
        assert name.encode() in lib.dl_last_error(), lib.dl_last_error()

    for C, K in ((6, 8), (4, 12), (4, 72)):
        refused(_conv(lib, x, w, y, None, N, H, W, C, K, _view(C), _view(K), None, 0, 0, 0), unsupported, "dl_tower_conv3x3_nhwc_f32")
        refused(lib.dl_tower_wgrad3x3_nhwc_f32(_p(x), _p(y), _p(w), _p(ws), N, H, W, C, K, _view(C), _view(K), _stream()), unsupported,
                "dl_tower_wgrad3x3_nhwc_f32")
        assert lib.dl_tower_wgrad_workspace_bytes(N, H, W, C, K) == 0
    refused(_conv(lib, None, w, y, None, N, H, W, 4, 8, _view(4), _view(8), None, 0, 0, 0), invalid, "dl_tower_conv3x3_nhwc_f32")
    refused(_conv(lib, x, w, None, None, N, H, W, 4, 8, _view(4), _view(8), None, 0, 0, 0), invalid, "dl_tower_conv3x3_nhwc_f32")
    refused(_conv(lib, x, w, y, None, N, H, W, 4, 8, _view(4), _view(8), None, 0, cr.ACT_TANH, DACT), invalid, "dl_tower_conv3x3_nhwc_f32")
    refused(_conv(lib, x, w, y, None, N, H, W, 4, 8, _view(4), _view(6), None, 0, 0, 0), invalid, "dl_tower_conv3x3_nhwc_f32")
    refused(lib.dl_tower_wgrad3x3_nhwc_f32(_p(x), _p(y), _p(w), None, N, H, W, 4, 8, _view(4), _view(8), _stream()), invalid,
            "dl_tower_wgrad3x3_nhwc_f32")
    refused(lib.dl_tower_wgrad3x3_nhwc_f32(None, _p(y), _p(w), _p(ws), N, H, W, 4, 8, _view(4), _view(8), _stream()), invalid,
            "dl_tower_wgrad3x3_nhwc_f32")
    _sync()
    A.check("refusals")
    word = cr._as_i32(cr.NAN_WORD[torch.float32])
    assert int((y.view(torch.int32) != word).sum()) == 0 and int((ws.view(torch.int32) != word).sum()) == 0, "a refused call wrote"
