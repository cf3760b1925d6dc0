"""The Winograd-domain weight gradient of the stride-(1,2) 3x3 layers on the pixel-pair view (csrc/wino.hip: k_wino_wgrad_strided_batch,
12 live planes for the odd-pixel channel blocks, 8 for the even-pixel ones) BIT FOR BIT against the float64 reference and against the
direct kernel, on small-integer data in poisoned arenas (the method of tests/test_gpu_wino_strided_exact.py).

Exactness is by construction: B^T d B and A g A^T of integer data are integers, their sums over the pair view's 2x2 tiles stay below
2^23 (``conv_ref.headroom("wino_wgrad", tiles, ...)``), the output transform's halves keep the result on the grid 1/4, and the planes the
kernel leaves out multiply rows of G that are zero.  A dead plane that was needed, a live plane stored to the wrong place or a slab left
out of the sum all change integers; a plane that is stored although dead lands in the NaN-filled workspace behind what the size
function promised, or in its guard.

Pair views H' x W' (the layer's image is H' x 2W'):
  2x16   one chunk per image: both zero-row edges at once, the first DMA piece of a row is also its last (wraps onto itself)
  4x16   two tile rows: the top and the bottom edge fall in different chunks
  4x32   two chunks per tile row: the first and the last chunk of a row differ
  6x48   a middle chunk and a middle tile row
with 64 -> 128 and 128 -> 64 channels (one and two 64-channel blocks per pixel phase), and 1 x 8x128, 256 -> 256, whose workgroups
run the steady-state loop (at least three chunks per slab; the 2x16 case has exactly one, so only prologue and epilogue run there).
"""
import ctypes

import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv_exact import Run, _dev, _guarded, _p, _stream, _wgrad_layer

pytestmark = pytest.mark.gpu

XMAX, WMAX = 4, 3
VIEWS = [(2, 16), (4, 16), (4, 32), (6, 48)]
CHANNELS = [(64, 128), (128, 64)]
CASES = [cc.Case(2, h, 2 * w, c, k, 3, (1, 2), xmax=XMAX, wmax=WMAX) for (h, w) in VIEWS for (c, k) in CHANNELS]
LONG = cc.Case(1, 8, 2 * 128, 256, 256, 3, (1, 2), xmax=XMAX, wmax=WMAX)


def _tiles(c):
    return c.N * (c.H // 2) * (c.W // 4)               # 2x2 tiles of the pair view


def _chunks_per_slab(lib, c):
    """(odd, even) chunks per slab of a one-layer call, from the host-side plan the launcher uses."""
    chunks = c.N * (c.H // 2) * (c.W // 32)
    tiles = (c.K // 64) * (c.C // 64)
    t, ch, ns = (ctypes.c_int32 * 2)(tiles, tiles), (ctypes.c_int32 * 2)(chunks, (3 * chunks + 3) // 4), (ctypes.c_int32 * 2)()
    assert lib.dl_wgrad_batch_plan(ctypes.cast(t, ctypes.c_void_p), ctypes.cast(ch, ctypes.c_void_p), 2, 256, 10, ctypes.cast(ns, ctypes.c_void_p)) > 0
    return tuple(-(-chunks // min(int(n), chunks)) for n in ns)


def test_headroom_and_slab_plan_of_the_cases_on_the_host():
    """No GPU needed for this part, but it belongs with the cases: every sum stays exact, the shortest case runs one chunk per slab
    and the long one at least three."""
    from delora_amd import _lib
    lib = _lib.load()
    for c in CASES + [LONG]:
        cr.headroom("wino_wgrad", _tiles(c), c.xmax, c.xmax)
        assert lib.dl_wino_strided_wgrad_takes(c.N, c.H, c.W, c.C, c.K, 1, 2) == 1, c.id
    assert _chunks_per_slab(lib, CASES[0]) == (1, 1)
    assert min(_chunks_per_slab(lib, LONG)) >= 3


def run_wgrad(case, dev, skew=0):
    r = Run(case, dev, skew)
    c, lib = case, r.lib
    cr.headroom("wino_wgrad", _tiles(c), c.xmax, c.xmax)
    assert lib.dl_wino_strided_wgrad_takes(c.N, c.H, c.W, c.C, c.K, 1, 2) == 1
    dshape = tuple(r.dw0.shape)
    dw_new, dw_dir = r.out(dshape, torch.float32, "dw (pixel-pair Winograd)", 0), r.out(dshape, torch.float32, "dw (direct)", 0)
    arr = _wgrad_layer(r, dw_new)
    ap = ctypes.cast(arr, ctypes.c_void_p)
    nbytes = int(lib.dl_wino_strided_wgrad3x3_batch_workspace_bytes(ap, 1))
    assert nbytes > 0
    ws = r.ws(nbytes)
    r.ok(lib.dl_wino_strided_wgrad3x3_batch_nhwc_f32(ap, 1, _p(ws), _stream()), "dl_wino_strided_wgrad3x3_batch_nhwc_f32")
    r.compare(dw_new, r.dw0, "pixel-pair Winograd weight gradient")
    r.A.check_output(ws, f"{c.id} workspace: every promised word is a live plane that was written")
    first = dw_new.clone()
    r.ok(lib.dl_wino_strided_wgrad3x3_batch_nhwc_f32(ap, 1, _p(ws), _stream()), "dl_wino_strided_wgrad3x3_batch_nhwc_f32")
    torch.cuda.synchronize()
    assert torch.equal(first, dw_new), f"{c.id}: two runs of the same call differ"
    wsd = r.ws(int(lib.dl_conv2d_wgrad_workspace_bytes(c.N, c.H, c.W, c.C, c.K, 3, 1, 2)), "direct workspace")
    r.ok(lib.dl_conv2d_wgrad_nhwc_f32(_p(r.x_d), _p(r.g_d), _p(dw_dir), _p(wsd), c.N, c.H, c.W, c.C, c.K, 3, 1, 2, _stream()), "dl_conv2d_wgrad_nhwc_f32")
    r.compare(dw_dir, r.dw0, "direct weight gradient")
    assert torch.equal(dw_new, dw_dir), f"{c.id}: the two weight gradients differ from each other"
    return r.bad


@pytest.mark.parametrize("case", CASES + [LONG], ids=[c.id for c in CASES + [LONG]])
def test_pixel_pair_weight_gradient_equals_float64_and_the_direct_kernel(case):
    dev = _dev()
    bad = _guarded(run_wgrad, case, dev)
    util.measured(f"strided Winograd wgrad exact {case.id}: elements that differ", bad, bound=0)


def test_minimum_documented_alignment_of_the_pixel_pair_weight_gradient():
    """x, g, dw and the workspace 16 bytes -- the documented minimum -- past a 256-byte boundary (pair view 4x32, 128 -> 64)."""
    dev = _dev()
    case = cc.Case(2, 4, 2 * 32, 128, 64, 3, (1, 2), xmax=XMAX, wmax=WMAX)
    bad = _guarded(run_wgrad, case, dev, 16)
    util.measured(f"strided Winograd wgrad exact {case.id}, bases 16 bytes past a 256-byte boundary: elements that differ", bad, bound=0)


def test_two_layers_in_one_launch():
    """The merged launch: two layers of different shapes (four items, both bodies, different slab counts) in one table; each exact,
    and two runs of the same call identical (the slab sums run in a fixed order)."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    shapes = [(2, 4, 64, 64, 128), (1, 6, 96, 128, 64)]
    A = cr.Arenas(dev)
    arr = (_lib.WgradLayer * len(shapes))()
    refs, dws = [], []
    for j, (N, H, W, C, K) in enumerate(shapes):
        c = cc.Case(N, H, W, C, K, 3, (1, 2), xmax=XMAX, wmax=WMAX)
        cr.headroom("wino_wgrad", _tiles(c), XMAX, XMAX)
        x, g = cr.ints((N, H, W, C), XMAX, c.seed(1)), cr.ints((N, H, W // 2, K), XMAX, c.seed(3))
        refs.append(cr.conv_grads(x, torch.zeros((K, 3, 3, C), dtype=torch.float64), g, (1, 2))[1])
        x_d, g_d = A.arena(x.shape, torch.float32, x, f"x{j}"), A.arena(g.shape, torch.float32, g, f"g{j}")
        dws.append(A.arena((K, 3, 3, C), torch.float32, None, f"dw{j}", 0))
        arr[j].x, arr[j].g, arr[j].dw = x_d.data_ptr(), g_d.data_ptr(), dws[j].data_ptr()
        arr[j].N, arr[j].H, arr[j].W, arr[j].C, arr[j].K, arr[j].ksize, arr[j].stride_h, arr[j].stride_w = N, H, W, C, K, 3, 1, 2
    ap = ctypes.cast(arr, ctypes.c_void_p)
    nbytes = int(lib.dl_wino_strided_wgrad3x3_batch_workspace_bytes(ap, len(shapes)))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", 0)

    def call():
        _lib.check(lib.dl_wino_strided_wgrad3x3_batch_nhwc_f32(ap, len(shapes), _p(ws), _stream()), "merged strided weight gradient")
        torch.cuda.synchronize()

    _guarded(call)
    A.check("merged strided weight gradient")
    A.check_output(ws, "merged strided weight gradient, workspace")
    bad = 0
    for j, (dw, ref) in enumerate(zip(dws, refs)):
        A.check_output(dw, f"merged strided layer {j}")
        bad += cr.mismatches(dw, ref.float(), f"merged strided weight gradient, layer {j} {shapes[j]}")
    first = [dw.clone() for dw in dws]
    _guarded(call)
    assert all(torch.equal(a, b) for a, b in zip(first, dws)), "two runs of the same merged call differ"
    util.measured(f"strided Winograd wgrad exact, {len(shapes)} layers in one launch: elements that differ", bad, bound=0)
