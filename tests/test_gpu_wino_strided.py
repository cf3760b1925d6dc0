"""The pixel-pair Winograd form of the stride-(1,2) 3x3 layers on random float data: against the float64 reference of
tests/conv_ref.py at the bound tests/test_gpu_conv.py applies to the Winograd layers (TIGHT, relative to the largest element), its
transformed weights against a torch-CPU G g G^T of the rearranged kernel, and one RingSegment with the switch on and off."""
import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv import TIGHT, _dev, _rel

pytestmark = pytest.mark.gpu

G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], dtype=torch.float64)


def _pair_kernel(w):
    """w [K,3,3,C] -> the stride-1 kernel [K,3,3,2C] of the pixel-pair view (even pixel's channels first)."""
    K, _, _, C = w.shape
    w2 = torch.zeros((K, 3, 3, 2 * C), dtype=w.dtype)
    w2[:, :, 0, C:] = w[:, :, 0]
    w2[:, :, 1, :C] = w[:, :, 1]
    w2[:, :, 1, C:] = w[:, :, 2]
    return w2


def _unpack(u, rows, red):
    """The wn_u_index layout (csrc/wino.hip) -> [16][rows][red]: reduction index in chunks of 8, rows in blocks of 64, the 16-byte halves
    of a row's eight swapped where bit 3 of the row is set."""
    v = u.view(red // 8, rows // 64, 16, 64, 2, 4).clone()
    swap = ((torch.arange(64) >> 3) & 1).bool()
    v[:, :, :, swap] = v[:, :, :, swap].flip(4)
    return v.reshape(red // 8, rows // 64, 16, 64, 8).permute(2, 1, 3, 0, 4).reshape(16, rows, red)


@pytest.mark.parametrize("ck", [(64, 128), (128, 64)])
def test_transformed_weights_are_g_w_gt_of_the_rearranged_kernel(ck):
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    C, K = ck
    gen = torch.Generator(device="cpu").manual_seed(C + 2 * K)
    w = torch.randn((K, 3, 3, C), generator=gen) * 0.1                                     # [K,r,s,C]
    w_param = w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).to(dev)
    uf, ub = rc.wino_strided_weights(w_param, (1, 2))
    w2 = _pair_kernel(w.double())                                                           # [K,3,3,2C]
    # forward: U[xi = 4a + b][k][c'] = (G g G^T)[a][b];  input gradient: the taps flipped, rows c', reduction k
    U = torch.einsum("ar,krsc,bs->abkc", G, w2, G).reshape(16, K, 2 * C)
    Ub = torch.einsum("ar,krsc,bs->abck", G, w2.flip(1, 2), G).reshape(16, 2 * C, K)
    got_f, got_b = _unpack(uf.cpu(), K, 2 * C), _unpack(ub.cpu(), 2 * C, K)
    util.measured(f"strided Winograd weights {C}->{K}: u_fwd vs float64 G g G^T (relative)", _rel(got_f.double(), U), bound=1e-6)
    util.measured(f"strided Winograd weights {C}->{K}: u_bwd vs float64 G g G^T (relative)", _rel(got_b.double(), Ub), bound=1e-6)
    # the planes the kernel never reads are exact zeros, and so is xi-column 0 (3) of the even-pixel half of u_fwd (u_bwd)
    col = torch.arange(16) % 4
    assert int((got_f[col == 3] != 0).sum()) == 0 and int((got_b[col == 0] != 0).sum()) == 0
    assert int((got_f[col == 0][:, :, :C] != 0).sum()) == 0 and int((got_b[col == 3][:, :C] != 0).sum()) == 0
    assert float(got_f[col == 1].abs().min()) > 0 and float(got_b[col == 1].abs().min()) > 0


@pytest.mark.parametrize("shape", [(2, 8, 128, 64, 128), (2, 4, 256, 128, 64), (1, 16, 64, 128, 128)])
def test_forward_and_input_gradient_against_the_float64_reference(shape):
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    N, H, W, C, K = shape
    gen = torch.Generator(device="cpu").manual_seed(sum(shape))
    x = torch.randn((N, H, W, C), generator=gen)
    w = torch.randn((K, 3, 3, C), generator=gen) * (0.5 / np.sqrt(9 * C))
    g = torch.randn((N, H, W // 2, K), generator=gen)
    y_ref = cr.conv(x.double(), w.double(), (1, 2))
    dx_ref, _ = cr.conv_grads(x.double(), w.double(), g.double(), (1, 2))
    w_param = w.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).to(dev)
    uf, ub = rc.wino_strided_weights(w_param, (1, 2))
    tag = f"strided winograd {N}x{H}x{W} {C}->{K}"
    x_d, g_d = x.to(dev), g.to(dev)
    y = rc.wino_strided_conv(x_d, uf, K, (1, 2))
    util.measured(f"{tag}: forward vs float64 (relative)", _rel(y.cpu().double(), y_ref), bound=TIGHT)
    y2 = rc.wino_strided_conv(x_d, uf, K, (1, 2), act=rc.ACT["tanh"], epilogue=rc.EPI_ACT)
    util.measured(f"{tag}: forward + tanh vs float64 (absolute)", float((y2.cpu().double() - torch.tanh(y_ref)).abs().max()), bound=2e-5)
    dx = rc.wino_strided_dgrad(g_d, ub, C, (1, 2), (H, W))
    util.measured(f"{tag}: input gradient vs float64 autograd (relative)", _rel(dx.cpu().double(), dx_ref), bound=TIGHT)
    addg = torch.randn((N, H, W // 2, C), generator=gen)
    ysave = torch.tanh(torch.randn((N, H, W, C), generator=gen))
    dx2 = rc.wino_strided_dgrad(g_d, ub, C, (1, 2), (H, W), act=rc.ACT["tanh"], epilogue=rc.EPI_ADD_GRID | rc.EPI_DACT, add_grid=addg.to(dev),
                                dsrc=ysave.to(dev))
    want = cr.epilogue(dx_ref, cr.EPI_ADD_GRID | cr.EPI_DACT, cr.ACT_TANH, None, ysave.double(), addg.double(), (1, 2))
    util.measured(f"{tag}: fused (dgrad + grid gradient) * tanh' vs float64 (relative)", _rel(dx2.cpu().double(), want), bound=TIGHT)
    y_direct = rc.conv_nhwc(x_d, rc.weight_storage(w_param), stride=(1, 2))
    util.measured(f"{tag}: pixel-pair Winograd vs the direct MFMA kernel (relative)", _rel(y, y_direct), bound=TIGHT)


def test_segment_with_the_switch_on_and_off(monkeypatch):
    """One RingSegment (N = 2, 8x128 input; blocks 64 -> 128 stride (1,2) and 128 -> 256 stride (2,2); tanh), forward and backward.
    With the switch on the first block's conv1 runs as pixel-pair Winograd, forward and input gradient (the plan query is asked as
    for a one-CU device: on the real CU count a launch this small stays direct); its weight gradient comes from the unchanged kernel,
    fed with x and the new g1.  The stride-(2,2) block stays on the direct kernel either way."""
    from delora_amd import _lib
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    N, H, W = 2, 8, 128
    blocks = ((64, 128, (1, 2), True), (128, 256, (2, 2), True))
    gen = torch.Generator(device="cpu").manual_seed(77)
    x0 = torch.tanh(torch.randn((N, H, W, 64), generator=gen)).to(dev)
    shapes = [(128, 64, 3), (128, 128, 3), (128, 64, 1), (256, 128, 3), (256, 256, 3), (256, 128, 1)]
    ws = [(torch.randn((k, c, ks, ks), generator=gen) * (0.7 / np.sqrt(ks * ks * c))).contiguous(memory_format=torch.channels_last).to(dev) for k, c, ks in shapes]
    dy = torch.randn((N, H // 2, W // 4, 256), generator=gen).to(dev)
    monkeypatch.setattr(rc, "STRIDED_PLAN_CUS", 1)
    assert rc.wino_strided_ok(N, H, W, 64, 128, (1, 2)) and not rc.wino_strided_ok(N, H, W // 2, 128, 256, (2, 2))
    res = {}
    for on in (True, False):
        monkeypatch.setattr(rc, "USE_WINOGRAD_STRIDED", on)
        params = [w.clone().requires_grad_(True) for w in ws]
        x = x0.clone().requires_grad_(True)
        _lib.profile_begin(64)
        y = rc.RingSegment.apply(x, rc.ACT["tanh"], blocks, False, True, *params)      # not first: the returned gradient carries tanh'(x0)
        y.backward(dy)
        torch.cuda.synchronize()
        rows, _ = _lib.profile_end()
        res[on] = (y.detach(), x.grad, [p.grad for p in params], [r["name"] for r in rows])
    tagged = [n for n in res[True][3] if n.startswith("k_wino_conv ") and n.endswith("s(1,2)")]
    assert tagged and not [n for n in res[False][3] if n.startswith("k_wino_conv ") and n.endswith("s(1,2)")], (res[True][3], res[False][3])
    util.measured("strided segment: output, switch on vs off (relative)", _rel(res[True][0], res[False][0]), bound=TIGHT)
    util.measured("strided segment: returned gradient, switch on vs off (relative)", _rel(res[True][1], res[False][1]), bound=TIGHT)
    for (k, c, ks), a, b in zip(shapes, res[True][2], res[False][2]):
        util.measured(f"strided segment: weight gradient {c}->{k} {ks}x{ks}, switch on vs off (relative)", _rel(a, b), bound=TIGHT)
