"""The Winograd-domain weight gradient of the stride-(1,2) 3x3 layers (pixel-pair view, live planes only) on random float data:
against the float64 reference of tests/conv_ref.py at the bound tests/test_gpu_conv.py applies to the stride-1 Winograd-domain weight
gradient (TIGHT, relative to the largest element), next to the direct kernel on the same data, and one RingSegment backward with
``USE_WINOGRAD_STRIDED_WGRAD`` on and off."""
import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv import TIGHT, _dev, _rel

pytestmark = pytest.mark.gpu


def test_weight_gradient_against_the_float64_reference(monkeypatch):
    """N = 2, pair view 8x64 (image 8x128), 64 -> 128: the new path and the direct kernel, each against float64."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    N, H, W, C, K = 2, 8, 128, 64, 128
    gen = torch.Generator(device="cpu").manual_seed(N + H + W + C + K)
    x = torch.randn((N, H, W, C), generator=gen)
    g = torch.randn((N, H, W // 2, K), generator=gen)
    _, dw_ref = cr.conv_grads(x.double(), torch.zeros((K, 3, 3, C), dtype=torch.float64), g.double(), (1, 2))
    x_d, g_d = x.to(dev), g.to(dev)
    monkeypatch.setattr(rc, "WINO_STRIDED_WGRAD_MIN_CHUNKS", 0)
    assert rc.wino_strided_wgrad_ok(N, H, W, C, K, (1, 2))
    monkeypatch.setattr(rc, "USE_WINOGRAD_STRIDED_WGRAD", True)
    dw_new = rc.wgrad_batch([(x_d, g_d, 3, (1, 2))])[0]
    monkeypatch.setattr(rc, "USE_WINOGRAD_STRIDED_WGRAD", False)
    dw_dir = rc.wgrad_batch([(x_d, g_d, 3, (1, 2))])[0]
    tag = f"strided winograd wgrad {N}x{H}x{W} {C}->{K}"
    e_new, e_dir = _rel(dw_new.cpu().double(), dw_ref), _rel(dw_dir.cpu().double(), dw_ref)
    util.measured(f"{tag}: direct kernel vs float64 (relative)", e_dir, bound=TIGHT)
    util.measured(f"{tag}: pixel-pair Winograd vs float64 (relative)", e_new, bound=TIGHT)
    assert not torch.equal(dw_new, dw_dir)              # the two paths really are different kernels


def test_segment_backward_with_the_switch_on_and_off(monkeypatch):
    """One RingSegment of one ``down (1,2)`` block (N = 2, 8x128 input, 64 -> 128, tanh), forward and backward.  With the switch on the
    weight gradient of conv1 comes from k_wino_wgrad_strided (the size threshold of the dispatch is lifted for this small image); with
    it off the launches are the ones the module made before the switch existed -- no kernel of the new family in the profile."""
    from delora_amd import _lib
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    N, H, W = 2, 8, 128
    blocks = ((64, 128, (1, 2), True),)
    gen = torch.Generator(device="cpu").manual_seed(78)
    x0 = torch.tanh(torch.randn((N, H, W, 64), generator=gen)).to(dev)
    shapes = [(128, 64, 3), (128, 128, 3), (128, 64, 1)]
    ws = [(torch.randn((k, c, ks, ks), generator=gen) * (0.7 / np.sqrt(ks * ks * c))).contiguous(memory_format=torch.channels_last).to(dev) for k, c, ks in shapes]
    dy = torch.randn((N, H, W // 2, 128), generator=gen).to(dev)
    monkeypatch.setattr(rc, "WINO_STRIDED_WGRAD_MIN_CHUNKS", 0)
    res = {}
    for on in (True, False):
        monkeypatch.setattr(rc, "USE_WINOGRAD_STRIDED_WGRAD", on)
        params = [w.clone().requires_grad_(True) for w in ws]
        x = x0.clone().requires_grad_(True)
        _lib.profile_begin(64)
        y = rc.RingSegment.apply(x, rc.ACT["tanh"], blocks, False, True, *params)
        y.backward(dy)
        torch.cuda.synchronize()
        rows, _ = _lib.profile_end()
        res[on] = (y.detach(), x.grad, [p.grad for p in params], [r["name"] for r in rows])
    assert [n for n in res[True][3] if n.startswith("k_wino_wgrad_strided")], res[True][3]
    assert not [n for n in res[False][3] if n.startswith("k_wino_wgrad_strided")], res[False][3]
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])     # nothing but weight gradients changes
    for (k, c, ks), a, b in zip(shapes, res[True][2], res[False][2]):
        util.measured(f"strided segment: weight gradient {c}->{k} {ks}x{ks}, wgrad switch on vs off (relative)", _rel(a, b), bound=TIGHT)
    assert torch.equal(res[True][2][1], res[False][2][1])     # conv2 keeps its launch (the 1x1 branch's direct launch loses a neighbour: its slab plan may differ)
