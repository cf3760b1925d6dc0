"""Host side of the stride-(1,2) 3x3 weight gradient on the pixel-pair view (csrc/wino.hip: k_wino_wgrad_strided_batch): which
layers ``dl_wino_strided_wgrad_takes`` answers yes for, that ``dl_wino_strided_wgrad3x3_batch_workspace_bytes`` is 0 exactly where it
says no, and that the shape rule restated in ``ring_conv.wino_strided_wgrad_ok`` agrees with the library.  No GPU is touched.
"""
import ctypes
import itertools

import pytest

from delora_amd import _lib
from delora_amd.models import ring_conv as rc


def _table(N, H, W, C, K, ks, sh, sw):
    arr = (_lib.WgradLayer * 1)()
    arr[0].x = arr[0].g = arr[0].dw = 0
    arr[0].N, arr[0].H, arr[0].W, arr[0].C, arr[0].K, arr[0].ksize, arr[0].stride_h, arr[0].stride_w = N, H, W, C, K, ks, sh, sw
    return arr


def _bytes(lib, *layer):
    return int(lib.dl_wino_strided_wgrad3x3_batch_workspace_bytes(ctypes.cast(_table(*layer), ctypes.c_void_p), 1))


GRID = [(N, H, W, C, K, st) for N, H, W, C, K, st in itertools.product(
    (1, 8), (2, 7, 64), (16, 32, 48, 100, 256, 512), (32, 64, 96, 128), (64, 100, 256), ((1, 2), (2, 2), (1, 1), (2, 1)))]
HUGE = [(8, 64, 2 ** 16, 256, 256, (1, 2)),          # N H (W/2) 2C = 2^33 elements
        (1, 1024, 2 ** 12, 256, 64, (1, 2))]          # one sample of the pair view: 2^30 elements


def test_the_query_takes_the_two_layers_of_the_step_and_refuses_what_the_kernel_cannot_tile():
    lib = _lib.load()
    q = lib.dl_wino_strided_wgrad_takes
    assert q(8, 64, 512, 64, 128, 1, 2) == 1            # layer2.0.conv1 at B = 8
    assert q(8, 64, 256, 128, 256, 1, 2) == 1           # layer3.0.conv1
    assert q(8, 64, 512, 64, 128, 2, 2) == 0, "stride (2,2) stays on the direct kernel"
    assert q(8, 64, 512, 64, 128, 1, 1) == 0, "stride (1,1) has its own entry point"
    assert q(8, 63, 512, 64, 128, 1, 2) == 0, "odd H"
    assert q(8, 64, 496, 64, 128, 1, 2) == 0, "W % 32 != 0"
    assert q(8, 64, 512, 96, 128, 1, 2) == 0, "C % 64 != 0"
    assert q(8, 64, 512, 64, 100, 1, 2) == 0, "K % 64 != 0"
    for N, H, W, C, K, st in HUGE:
        assert q(N, H, W, C, K, *st) == 0, "past the 32-bit offsets of the kernel"
    assert q(1, 1024, 2 ** 11, 256, 64, 1, 2) == 1      # (half of the second HUGE shape is inside)


def test_workspace_bytes_is_zero_exactly_where_the_query_says_no_and_python_restates_the_rule():
    lib = _lib.load()
    yes = 0
    for N, H, W, C, K, st in GRID + HUGE:
        takes = int(lib.dl_wino_strided_wgrad_takes(N, H, W, C, K, st[0], st[1]))
        nbytes = _bytes(lib, N, H, W, C, K, 3, st[0], st[1])
        assert (nbytes > 0) == (takes == 1), (N, H, W, C, K, st, takes, nbytes)
        assert rc.wino_strided_wgrad_ok(N, H, W, C, K, st) == (takes == 1), (N, H, W, C, K, st)
        yes += takes
    assert 0 < yes < len(GRID)
    assert _bytes(lib, 8, 64, 512, 64, 128, 1, 1, 2) == 0, "a 1x1 layer is not this kernel's"


@pytest.mark.parametrize("field, layer", [("ksize", (2, 8, 64, 64, 128, 1, 1, 2)), ("stride", (2, 8, 64, 64, 128, 3, 2, 2)), ("H", (2, 7, 64, 64, 128, 3, 1, 2)),
                                          ("W", (2, 8, 48, 64, 128, 3, 1, 2)), ("C", (2, 8, 64, 96, 128, 3, 1, 2)), ("K", (2, 8, 64, 64, 100, 3, 1, 2))])
def test_a_refused_layer_is_named_with_its_field(field, layer):
    lib = _lib.load()
    assert _bytes(lib, *layer) == 0
    msg = (lib.dl_last_error() or b"").decode()
    assert "layer 0" in msg and field in msg, msg


def test_the_workspace_holds_live_planes_only():
    """12 planes for the odd-pixel channel blocks and 8 for the even-pixel ones, per slab and once more for their sum: never the 16 K 2C
    of the stride-1 form.  The slab counts are those of dl_wgrad_batch_plan for (odd, even) items with the even chunks weighed 3/4."""
    lib = _lib.load()
    N, H, W, C, K = 8, 64, 512, 64, 128
    chunks = N * (H // 2) * (W // 32)
    tiles = (K // 64) * (C // 64)
    t = (ctypes.c_int32 * 2)(tiles, tiles)
    c = (ctypes.c_int32 * 2)(chunks, (3 * chunks + 3) // 4)
    ns = (ctypes.c_int32 * 2)()
    assert lib.dl_wgrad_batch_plan(ctypes.cast(t, ctypes.c_void_p), ctypes.cast(c, ctypes.c_void_p), 2, 256, 10, ctypes.cast(ns, ctypes.c_void_p)) > 0
    floats = 0
    for planes, want in ((12, ns[0]), (8, ns[1])):
        per = -(-chunks // want)
        slabs = -(-chunks // per)
        floats += ((slabs if slabs > 1 else 0) + 1) * planes * K * C
    assert _bytes(lib, N, H, W, C, K, 3, 1, 2) == 4 * floats


def test_the_dispatch_takes_the_layers_of_the_step_and_leaves_the_rest(monkeypatch):
    import torch
    calls = []

    def fake(items, size_fn, run_fn, what, *extra):
        calls.append((run_fn, [tuple(x.shape) + (ks,) + tuple(st) for x, g, ks, st in items]))
        return [run_fn for _ in items]

    monkeypatch.setattr(rc, "_wgrad_batch_call", fake)
    shapes = [(8, 64, 512, 64, 128, 3, (1, 2)), (8, 64, 256, 128, 256, 3, (1, 2)), (8, 64, 128, 256, 512, 3, (2, 2)), (8, 64, 512, 64, 128, 1, (1, 2)),
              (8, 63, 512, 64, 128, 3, (1, 2)), (2, 8, 64, 128, 256, 3, (1, 2)), (8, 64, 512, 128, 128, 3, (1, 1))]
    items = [(torch.empty((N, H, W, C), device="meta"), torch.empty((N, rc.out_size(H, st[0]), rc.out_size(W, st[1]), K), device="meta"), ks, st)
             for (N, H, W, C, K, ks, st) in shapes]
    new, direct, wino = "dl_wino_strided_wgrad3x3_batch_nhwc_f32", "dl_conv2d_wgrad_batch_nhwc_f32", "dl_wino_wgrad3x3_batch_nhwc_f32"
    assert rc.USE_WINOGRAD and rc.USE_WINOGRAD_STRIDED_WGRAD
    assert rc.wgrad_batch(items) == [new, new, direct, direct, direct, direct, wino]      # (the sixth is below WINO_STRIDED_WGRAD_MIN_CHUNKS)
    assert sorted(fn for fn, _ in calls) == sorted([new, direct, wino]), "one call per family, none per layer"
    for flag in ("USE_WINOGRAD_STRIDED_WGRAD", "USE_WINOGRAD"):
        monkeypatch.setattr(rc, flag, False)
        assert rc.wgrad_batch(items) == [direct] * 6 + [wino]
        monkeypatch.setattr(rc, flag, True)
