"""Dropout on the HIP pose CNN (delora_amd/csrc/dropout.hip, the ``_drop`` heads, ``ring_conv.ChannelDropout``): ``use_dropout: True`` in
training mode keeps the channels-last MFMA path.

The masks come from the library's own counter-based stream, so every one of them is recomputed here by the numpy replica of
tests/test_dropout_host.py (Philox4x32-10; contract in include/delora_hip.h).  Reference semantics: src/models/resnet_modified.py:33-38,
:95-118 (element-wise dropout on the stacked input and on the fc output, Dropout2d on layer3's output, p = 0.2, training only)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util
from tests.test_dropout_host import SITE_CHANNELS, SITE_FC, SITE_INPUT, site_scales

pytestmark = pytest.mark.gpu
SIZES = [(16, 1024), (64, 720)]
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}      # ulp/2 of the storage type, rounded up (tests/test_gpu_convh.py)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _seed_tensor(value, dev):
    v = int(value) & (2 ** 64 - 1)
    return torch.tensor([v - 2 ** 64 if v >= 2 ** 63 else v], dtype=torch.int64, device=dev)


def _model(size, act="tanh", use_dropout=True, impl="hip", seed=5, device="cuda:0"):
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(size[0], size[1], device=device, activation_fct=act, use_dropout=use_dropout, cnn_impl=impl)
    torch.manual_seed(seed)
    m = OdometryModel(cfg).to(cfg["device"])
    if impl == "hip":
        m.resnet.trunk_weights_channels_last()
    return m


def _loss(t, q):
    return t.float().square().sum() + (q.float() * torch.arange(1, 5, device=q.device, dtype=torch.float32)).sum()


def _run(m, x, amp=None, seed=None):
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    if amp is None:
        t, q = m(x)
    else:
        with torch.autocast("cuda", dtype=amp):
            t, q = m(x)
    _loss(t, q).backward()
    return t.detach().float(), q.detach().float(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------ 4, 5: the stream
@pytest.mark.parametrize("seed", [1234, (7 << 32) | 1234, 0xF234_5678_9ABC_DEF1])
def test_scale_kernel_equals_the_host_replica(seed):
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    st = _seed_tensor(seed, dev)
    for n in (1, 5, 2048, 2 * 1000):
        for site in (SITE_INPUT, SITE_CHANNELS, SITE_FC):
            got = rc.dropout_scale(st, site, 0.2, n).cpu().numpy()
            want = site_scales(seed, site, n)
            assert got.dtype == np.float32 and np.array_equal(got, want), (seed, site, n)
    assert bool((rc.dropout_scale(st, SITE_FC, 0.0, 2000) == 1.0).all())


def test_input_kernel_mask_order_and_exact_copy():
    """All-ones image: the zero pattern of the channels-last output is the replica's site-1 mask in flat index order and every kept
    value is exactly 1.25f; p = 0 is an exact transposing copy."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    for (N, H, W), seed in (((2, 16, 1024), 99), ((2, 64, 720), (3 << 32) + 17), ((1, 3, 20), 5)):
        st = _seed_tensor(seed, dev)
        y = rc.stem_input_drop(torch.ones((N, 8, H, W), device=dev), st, 0.2)
        assert y.shape == (N, H, W, 8)
        want = site_scales(seed, SITE_INPUT, N * H * W * 8).reshape(N, H, W, 8)
        assert np.array_equal(y.cpu().numpy(), want)
        assert set(np.unique(y.cpu().numpy()).tolist()) == {0.0, 1.25}
        x = torch.randn((N, 8, H, W), device=dev)
        assert torch.equal(rc.stem_input_drop(x, st, 0.0), x.permute(0, 2, 3, 1).contiguous())
        # and with values: the product, element by element
        assert torch.equal(rc.stem_input_drop(x, st, 0.2), x.permute(0, 2, 3, 1).contiguous() * torch.from_numpy(want).to(dev))


def test_keep_rates():
    """Keep fraction within 6 sigma of 0.8, sigma = sqrt(0.16 / n): the B = 8, 64x2048 input mask, a [8][256] channel mask, a [8][1000] fc mask."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    st = _seed_tensor((7 << 32) | 1234, dev)
    y = rc.stem_input_drop(torch.ones((8, 8, 64, 2048), device=dev), st, 0.2)
    n = y.numel()
    assert n == 8388608
    util.measured("dropout keep rate, input mask B=8 64x2048: |rate - 0.8| in sigmas", abs(float((y > 0).float().mean()) - 0.8) / np.sqrt(0.16 / n), bound=6.0)
    for name, site, n in (("channel mask [8][256]", SITE_CHANNELS, 2048), ("fc mask [8][1000]", SITE_FC, 8000)):
        s = rc.dropout_scale(st, site, 0.2, n)
        util.measured(f"dropout keep rate, {name}: |rate - 0.8| in sigmas", abs(float((s > 0).float().mean()) - 0.8) / np.sqrt(0.16 / n), bound=6.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_channel_scale_kernels_against_torch(dtype, act):
    """``ChannelDropout``: forward ``x * scale[n][c]``, backward ``g * scale[n][c] * act'(x)`` in one pass; fp32 arithmetic on the stored
    values, one rounding of the result."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(8)
    N, H, W, C = 2, 5, 23, 256
    x = torch.tanh(torch.randn((N, H, W, C), generator=g)) if act == "tanh" else torch.relu(torch.randn((N, H, W, C), generator=g))
    x = x.to(dtype).to(dev).requires_grad_(True)
    gy = torch.randn((N, H, W, C), generator=g).to(dtype).to(dev)
    scale = rc.dropout_scale(_seed_tensor(11, dev), SITE_CHANNELS, 0.2, N * C).view(N, C)
    y = rc.ChannelDropout.apply(x, scale, rc.ACT[act])
    y.backward(gy)
    s = scale.view(N, 1, 1, C)
    xf = x.detach().float()
    assert torch.equal(y.detach(), (xf * s).to(dtype))
    dact = (1.0 - xf * xf) if act == "tanh" else (xf > 0).float()
    assert torch.equal(x.grad, ((gy.float() * s) * dact).to(dtype))


# ------------------------------------------------------------------------------------------------------------ 6: p = 0
@pytest.mark.parametrize("size", SIZES, ids=["16x1024", "64x720"])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("amp", [None, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_p_zero_through_the_dropout_plumbing_is_the_plain_hip_path(amp, act, size):
    """The whole dropout plumbing (copy kernel, extra cut + ChannelDropout, ``_drop`` heads) with p = 0, i.e. scales of exactly 1.0f:
    poses equal to the plain HIP path bit for bit; every parameter gradient to the order of the merged weight-gradient sums (the cut
    merges other sets of layers: 2e-5 of the gradient's largest element, the bound of tests/test_gpu_convh.py for another cut of the
    same computation).  A wrong first / last convention at the new cut shows here."""
    dev = _dev()
    m_plain, m_drop = _model(size, act, use_dropout=False), _model(size, act, use_dropout=True)
    m_drop.load_state_dict(m_plain.state_dict())
    m_drop.resnet.dropout_p = 0.0
    m_plain.train(), m_drop.train()
    x = (torch.randn((2, 8, size[0], size[1]), generator=torch.Generator().manual_seed(2)) * 3.0).to(dev)
    t0, q0, g0 = _run(m_plain, x, amp)
    t1, q1, g1 = _run(m_drop, x, amp)
    assert bool((m_drop.resnet.last_dropout["channels"] == 1.0).all()) and bool((m_drop.resnet.last_dropout["fc"] == 1.0).all())
    assert not hasattr(m_plain.resnet, "last_dropout")
    assert torch.equal(t0, t1) and torch.equal(q0, q1)
    worst = max((_rel(g1[k], g0[k]), k) for k in g0)
    tag = f"p=0 plumbing vs plain HIP path [{'fp32' if amp is None else str(amp)[6:]},{act},{size[0]}x{size[1]}]"
    util.measured(f"{tag}: worst parameter-gradient difference, relative to the gradient's largest element ({worst[1]})", worst[0], bound=2e-5)


# ------------------------------------------------------------------------------------------------------------ 7: first=True + shortcut
def _ref_conv(x_nchw, w, stride, ks):
    if ks == 3:
        return F.conv2d(F.pad(x_nchw, (1, 1, 0, 0), mode="circular"), w, stride=stride, padding=(1, 0))
    return F.conv2d(x_nchw, w, stride=stride)


def _torch_grads(x_nhwc, w, stride, ks, gy_nhwc):
    """(dL/dx [N,H,W,C], dL/dw [K,C,k,k]) of the reference's layer by torch autograd, fp32, from channels-last operands."""
    xr = x_nhwc.float().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    wr = w.detach().clone().float().requires_grad_(True)
    y = _ref_conv(xr, wr, stride, ks)
    gx, gw = torch.autograd.grad(y, (xr, wr), gy_nhwc.float().permute(0, 3, 1, 2).contiguous())
    return gx.permute(0, 2, 3, 1), gw


def _act_fns(act):
    if act == "tanh":
        return torch.tanh, lambda y: 1.0 - y * y
    return torch.relu, lambda y: (y > 0).float()


BLOCKS = [((2, 16, 64), 256, 512, (2, 2)), ((2, 8, 90), 128, 256, (1, 2))]


@pytest.mark.parametrize("shape", BLOCKS, ids=["256-512-s22", "128-256-s12"])
def test_first_segment_with_shortcut_convolution_fp32(shape):
    """One strided block WITH a down-sampling branch run as a segment with ``first=True, last=True`` (``EPI_ADD_GRID`` without
    ``EPI_DACT`` in the strided input gradient -- the mode the cut in front of layer4 uses): output, the true dL/dx and the three
    weight gradients against torch autograd on ``F.conv2d(F.pad(circular))``.  Bounds of tests/test_gpu_conv.py (1e-5 relative to the
    largest element; weight gradients 2e-5).  tanh: ``first`` only removes the activation derivative of the segment's INPUT, and a relu
    mask that two evaluations round to different sides of zero is not an error of the epilogue."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    act = "tanh"
    (N, H, W), C, K, stride = shape
    g = torch.Generator(device="cpu").manual_seed(C + K)
    fn, _ = _act_fns(act)
    x = fn(torch.randn((N, C, H, W), generator=g)).to(dev)
    w1 = (torch.randn((K, C, 3, 3), generator=g) / np.sqrt(9 * C)).to(dev).contiguous(memory_format=torch.channels_last)
    w2 = (torch.randn((K, K, 3, 3), generator=g) / np.sqrt(9 * K)).to(dev).contiguous(memory_format=torch.channels_last)
    wd = (torch.randn((K, C, 1, 1), generator=g) / np.sqrt(C)).to(dev).contiguous(memory_format=torch.channels_last)
    ref_in = [t.detach().clone().requires_grad_(True) for t in (x, w1, w2, wd)]
    y_ref = fn(_ref_conv(fn(_ref_conv(ref_in[0], ref_in[1], stride, 3)), ref_in[2], (1, 1), 3) + _ref_conv(ref_in[0], ref_in[3], stride, 1))
    gy = torch.randn(y_ref.shape, generator=g).to(dev)
    y_ref.backward(gy)
    ours = [x.permute(0, 2, 3, 1).contiguous().requires_grad_(True)] + [t.detach().clone().requires_grad_(True) for t in (w1, w2, wd)]
    y = rc.RingSegment.apply(ours[0], rc.ACT[act], ((C, K, stride, True),), True, True, *ours[1:])
    y.backward(gy.permute(0, 2, 3, 1).contiguous())
    tag = f"first+last segment fp32 {C}->{K} s{stride} {act}"
    util.measured(f"{tag}: output vs torch (relative)", _rel(y.detach().permute(0, 3, 1, 2), y_ref.detach()), bound=1e-5)
    util.measured(f"{tag}: true dL/dx vs torch autograd (relative)", _rel(ours[0].grad.permute(0, 3, 1, 2), ref_in[0].grad), bound=1e-5)
    for name, a, b in (("conv1", ours[1], ref_in[1]), ("conv2", ours[2], ref_in[2]), ("downsample", ours[3], ref_in[3])):
        util.measured(f"{tag}: {name} weight gradient vs torch autograd (relative)", _rel(a.grad, b.grad), bound=2e-5)


def _worst(got, want, eps, abs_tol):
    got, want = got.float(), want.float()
    return float(((got - want).abs() / (eps * want.abs() + abs_tol)).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", BLOCKS, ids=["256-512-s22", "128-256-s12"])
def test_first_segment_with_shortcut_convolution_half(shape, dtype):
    """The same block as ``RingSegmentH`` with ``first=True, last=True``.  As in tests/test_gpu_convh.py every result is compared with
    torch fp32 autograd evaluated ON THE SAME ROUNDED INPUTS, so that what is bounded is the accumulation order plus ONE rounding of
    the stored result: the half-precision intermediates a gradient depends on (y1, the pre-activation gradient g1, the branch
    gradient on the grid) are produced by the library's own operator calls -- the launches the segment makes, bit for bit -- and
    handed to torch; each of those operators is itself bounded against torch the same way (here for the 1x1 grid gradient, in
    tests/test_gpu_convh.py for the rest).  A reference that re-derived the intermediates in fp32 would differ from the kernels' by
    rounding flips (one half-precision ulp of one term of a weight-gradient sum is already 2e-5 of its largest element)."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    act = "tanh"
    (N, H, W), C, K, stride = shape
    eps = EPS[dtype]
    g = torch.Generator(device="cpu").manual_seed(C + K + 1)
    x = torch.tanh(torch.randn((N, H, W, C), generator=g)).to(dtype).to(dev)
    mk = lambda k, c, ks: (torch.randn((k, c, ks, ks), generator=g) / np.sqrt(ks * ks * c)).to(dtype).float().to(dev).contiguous(memory_format=torch.channels_last)   # noqa: E731
    w1, w2, wd = mk(K, C, 3), mk(K, K, 3), mk(K, C, 1)
    Ho, Wo = rc.out_size(H, stride[0]), rc.out_size(W, stride[1])
    gy = torch.randn((N, Ho, Wo, K), generator=g).to(dtype).to(dev)
    ours = [x.clone().requires_grad_(True)] + [t.detach().clone().requires_grad_(True) for t in (w1, w2, wd)]
    y = rc.RingSegmentH.apply(ours[0], rc.ACT[act], ((C, K, stride, True),), True, True, *ours[1:])
    y.backward(gy)
    # the segment's own intermediates, from the same launches
    (w1f, w1b), (w2f, w2b), (wdf, wdb) = rc.weights_h(w1, dtype), rc.weights_h(w2, dtype), rc.weights_h(wd, dtype)
    y1 = rc.conv_nhwc_h(x, w1f, 3, stride=stride, act=rc.ACT[act], epilogue=rc.EPI_ACT)
    sc = rc.conv_nhwc_h(x, wdf, 1, stride=stride)
    assert torch.equal(y.detach(), rc.conv_nhwc_h(y1, w2f, 3, act=rc.ACT[act], epilogue=rc.EPI_ADD | rc.EPI_ACT, add=sc))
    yf = y.detach().float()
    g2 = (gy.float() * (1.0 - yf * yf)).to(dtype)                      # last=True: act' of the block's own output, applied by the segment
    g1 = rc.conv_nhwc_h(g2, w2b, 3, act=rc.ACT[act], epilogue=rc.EPI_DACT, dsrc=y1, transposed=True)
    dxb = rc.dgrad_strided_h(g2, wdb, 1, stride, (H, W), dense=True)
    tag = f"first+last segment {str(dtype)[6:]} {C}->{K} s{stride}"
    abs_tol = 2e-5 * np.sqrt(9 * max(C, K))
    # forward against torch on the rounded intermediates
    pre = _ref_conv(y1.float().permute(0, 3, 1, 2), w2, (1, 1), 3) + sc.float().permute(0, 3, 1, 2)
    util.measured(f"{tag}: output vs torch fp32 on the same inputs (units of one rounding)", _worst(y.detach().permute(0, 3, 1, 2), torch.tanh(pre), eps, 3e-5), bound=1.0)
    # weight gradients (fp32)
    for name, got, (inp, w, st, ks, gout) in (("conv2", ours[2].grad, (y1, w2, (1, 1), 3, g2)), ("conv1", ours[1].grad, (x, w1, stride, 3, g1)),
                                              ("downsample", ours[3].grad, (x, wd, stride, 1, g2))):
        want = _torch_grads(inp, w, st, ks, gout)[1]
        assert got.dtype == torch.float32
        util.measured(f"{tag}: {name} weight gradient (fp32) vs torch autograd (relative to its largest element)", _rel(got, want), bound=2e-5)
    # the branch gradient on the grid, then the true dL/dx = dgrad(g1, w1) + branch gradient: NO activation derivative (first=True)
    ref_b = _torch_grads(x, wd, stride, 1, g2)[0][:, ::stride[0], ::stride[1]]
    util.measured(f"{tag}: 1x1 branch gradient on the grid (units of one rounding)", _worst(dxb, ref_b, eps, abs_tol), bound=1.0)
    ref_dx = _torch_grads(x, w1, stride, 3, g1)[0].clone()
    ref_dx[:, ::stride[0], ::stride[1]] += dxb.float()
    util.measured(f"{tag}: true dL/dx, all phases + branch gradient, no act' (units of one rounding)", _worst(ours[0].grad, ref_dx, eps, abs_tol), bound=1.0)


# ------------------------------------------------------------------------------------------------------------ 8: parity, fp32
class _Masks(torch.nn.Module):
    """Stands in for a torch dropout module: multiplies the k-th call's input by the k-th mask."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = list(masks), 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m.to(x.dtype)


def _with_masks(m_mod, last, x_shape, device, dtype=torch.float32):
    """Replace the three dropout sites of a module-path model by the masks the HIP model drew (site 1 recomputed by the replica)."""
    N, _, H, W = x_shape
    seed = int(last["seed"].item())
    m_in = torch.from_numpy(site_scales(seed, SITE_INPUT, N * H * W * 8).reshape(N, H, W, 8)).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(last["channels"].cpu().numpy().reshape(-1), site_scales(seed, SITE_CHANNELS, last["channels"].numel()))
    assert np.array_equal(last["fc"].cpu().numpy().reshape(-1), site_scales(seed, SITE_FC, last["fc"].numel()))
    m_mod.resnet.dropout_values = _Masks([m_in.to(device, dtype), last["fc"].to(device, dtype)])          # input first, fc output second
    m_mod.resnet.dropout_channels = _Masks([last["channels"].to(device, dtype)[:, :, None, None]])


@pytest.mark.parametrize("size", SIZES, ids=["16x1024", "64x720"])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_dropout_hip_path_matches_module_path_with_the_same_masks(act, size):
    """HIP model in train() with ``use_dropout: True`` against the module path (library convolutions) whose three dropout modules are
    replaced by multiplications with the masks the HIP model used.  Bounds and their reasons are those of
    tests/test_gpu_conv.py::test_hip_trunk_matches_module_path -- a multiplication by 0 or 1.25 adds at most one rounding."""
    dev = _dev()
    m_hip = _model(size, act, use_dropout=True)
    m_mod = _model(size, act, use_dropout=True, impl="modules")
    m_mod.load_state_dict(m_hip.state_dict())
    m_hip.train(), m_mod.train()
    x = torch.randn((2, 8, size[0], size[1]), generator=torch.Generator().manual_seed(6)).to(dev)
    t0, q0, g0 = _run(m_hip, x, seed=21)
    last = m_hip.resnet.last_dropout
    assert 0.5 < float((last["channels"] > 0).float().mean()) < 0.97 and last["p"] == 0.2
    _with_masks(m_mod, last, x.shape, dev)
    t1, q1, g1 = _run(m_mod, x)
    assert m_mod.resnet.dropout_values.calls == 2 and m_mod.resnet.dropout_channels.calls == 1
    tagn = f"dropout[{act},{size[0]}x{size[1]}]"
    util.measured(f"{tagn}: translation hip vs modules with the same masks (relative)", _rel(t0, t1), bound=1e-5)
    util.measured(f"{tagn}: quaternion hip vs modules with the same masks (relative)", _rel(q0, q1), bound=1e-5)
    referee = {}
    if size == (64, 720):
        # the library's weight gradient of the 8-channel conv1 deviates at this size (tests/test_gpu_conv.py:183-198): float64 CPU referee
        m_cpu = _model(size, act, use_dropout=True, impl="modules", device="cpu").double()
        m_cpu.load_state_dict({k: v.detach().cpu().double() for k, v in m_hip.state_dict().items()})
        m_cpu.train()
        _with_masks(m_cpu, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in last.items()}, x.shape, "cpu", torch.float64)
        t, q = m_cpu(x.cpu().double())
        (t.square().sum() + (q * torch.arange(1, 5, dtype=torch.float64)).sum()).backward()
        referee = {"resnet.conv1.weight": m_cpu.resnet.conv1.weight.grad.float().to(dev)}
    errs, worst, name = [], 0.0, ""
    for k in g0:
        if k in referee:
            ref = referee[k]
            # tanh: the referee's bound of tests/test_gpu_conv.py.  relu: that test has no relu case at this size; a pre-activation that
            # fp32 on the GPU and float64 on the CPU round to different sides of zero is a flipped mask, which that test documents at
            # 1.3e-3 for conv1 (:205-212) -- the relu bound of the other parameter gradients applies to this one as well
            util.measured(f"{tagn}: {k} gradient, HIP stem vs torch-CPU float64 (relative)", float((g0[k] - ref).norm() / ref.norm()),
                          bound=(5e-5 if act == "tanh" else 5e-3))
            util.measured(f"{tagn}: {k} gradient, module path (library convolution) vs torch-CPU float64 (relative)", float((g1[k] - ref).norm() / ref.norm()))
            continue
        e = float((g0[k] - g1[k]).norm() / g1[k].norm().clamp_min(1e-30))
        errs.append(e)
        if e > worst:
            worst, name = e, k
    util.measured(f"{tagn}: worst relative parameter-gradient difference hip vs modules ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))
    util.measured(f"{tagn}: 25th percentile of the relative parameter-gradient differences hip vs modules", float(np.quantile(errs, 0.25)), bound=1e-5)


# ------------------------------------------------------------------------------------------------------------ 9: parity, half
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_dropout_half_network_against_the_fp32_network_with_the_same_masks(dtype):
    """Same ``torch.manual_seed`` -> same library seed -> same masks in fp32 and inside autocast (the decision index does not depend on
    the storage type): the autocast dropout network against the fp32 dropout network at 64x720, bounds of
    tests/test_gpu_convh.py::test_half_precision_network_against_the_fp32_network_at_full_size."""
    dev = _dev()
    B, H, W = 2, 64, 720
    m = _model((H, W), "tanh", use_dropout=True, seed=3)
    m.train()
    g = torch.Generator(device="cpu").manual_seed(5)
    az = torch.linspace(-np.pi, np.pi, W).view(1, 1, 1, W)
    el = torch.linspace(-0.4, 0.05, H).view(1, 1, H, 1)
    rng = 8.0 + 6.0 * torch.sin(3 * az + torch.rand((B, 2, 1, 1), generator=g)) + 2.0 * torch.rand((B, 2, H, W), generator=g)
    xyz = torch.stack((rng * torch.cos(el) * torch.cos(az), rng * torch.cos(el) * torch.sin(az), rng * torch.sin(el).expand_as(rng), rng), dim=2)
    x = (xyz * (torch.rand((B, 2, 1, H, W), generator=g) > 0.05)).reshape(B, 8, H, W).to(dev)
    t32, q32, g32 = _run(m, x, seed=77)
    last32 = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in m.resnet.last_dropout.items()}
    th, qh, gh = _run(m, x, amp=dtype, seed=77)
    lasth = m.resnet.last_dropout
    assert torch.equal(last32["seed"], lasth["seed"]) and torch.equal(last32["channels"], lasth["channels"]) and torch.equal(last32["fc"], lasth["fc"])
    name = str(dtype)[6:]
    rel_pose = {torch.bfloat16: 5e-2, torch.float16: 8e-3}[dtype]
    rel_grad = {torch.bfloat16: 1.5e-1, torch.float16: 3e-2}[dtype]
    util.measured(f"dropout half network {name} vs fp32 @{H}x{W}: translation (relative to its largest element)", _rel(th, t32), bound=rel_pose)
    util.measured(f"dropout half network {name} vs fp32 @{H}x{W}: quaternion (relative to its largest element)", _rel(qh, q32), bound=rel_pose)
    worst = max(float((gh[k] - g32[k]).norm() / g32[k].norm().clamp_min(1e-30)) for k in g32)
    util.measured(f"dropout half network {name} vs fp32 @{H}x{W}: worst parameter gradient |dg| / |g|", worst, bound=rel_grad)
    assert all(bool(torch.isfinite(a).all()) for a in gh.values())


# ------------------------------------------------------------------------------------------------------------ 10: determinism
def test_dropout_is_deterministic_under_manual_seed_fresh_per_pass_and_off_in_eval():
    dev = _dev()
    size = (16, 1024)
    m = _model(size, "tanh", use_dropout=True)
    m.train()
    x = torch.randn((2, 8, size[0], size[1]), generator=torch.Generator().manual_seed(6)).to(dev)
    ta, qa, ga = _run(m, x, seed=31)
    seed_a = m.resnet.last_dropout["seed"].clone()
    tb, qb, gb = _run(m, x, seed=31)
    assert torch.equal(seed_a, m.resnet.last_dropout["seed"])
    assert torch.equal(ta, tb) and torch.equal(qa, qb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    # two consecutive passes without reseeding: new masks
    ch1 = m.resnet.last_dropout["channels"].clone()
    with torch.no_grad():
        m(x)
    assert not torch.equal(ch1, m.resnet.last_dropout["channels"])
    # the masks act: the poses differ from the network without dropout
    m_plain = _model(size, "tanh", use_dropout=False)
    m_plain.load_state_dict(m.state_dict())
    m.eval(), m_plain.eval()
    del m.resnet.last_dropout
    state = torch.cuda.get_rng_state(dev)
    with torch.no_grad():
        (te, qe), (tp, qp) = m(x), m_plain(x)
    assert torch.equal(te, tp) and torch.equal(qe, qp)
    assert torch.equal(state, torch.cuda.get_rng_state(dev)), "eval() must not draw a seed"
    assert not hasattr(m.resnet, "last_dropout")
    assert not torch.equal(ta, tp)
    # the list-returning reference interface draws the same masks from the same seed as the fused-heads interface
    m.train()
    torch.manual_seed(31)
    out = m.resnet(x)[-1]
    assert torch.equal(seed_a, m.resnet.last_dropout["seed"])
    t2, q2 = m._heads(out)
    util.measured("dropout: fused heads vs torch heads on the masked fc output, translation (relative)", _rel(t2.detach(), ta), bound=1e-5)
    util.measured("dropout: fused heads vs torch heads on the masked fc output, quaternion (relative)", _rel(q2.detach(), qa), bound=1e-5)


# ------------------------------------------------------------------------------------------------------------ 11: the step
def _trainer(size, B, **over):
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(size[0], size[1], device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=B, learning_rate=1e-5,
                           use_dropout=True, **over)
    ds = SyntheticPairDataset(cfg, "kitti", B, rings=size[0], azimuth_steps=max(600, size[1] + size[1] // 4))
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    return tr, tr.to_device([ds[i] for i in range(B)])


@pytest.mark.parametrize("amp", [None, "bfloat16"], ids=["fp32", "bf16"])
def test_training_step_with_dropout_stays_on_the_hip_path(amp, monkeypatch):
    """A ``Trainer`` on a synthetic 64x720 dataset with ``use_dropout: True``: no module path, the segment backward passes and the
    channel dropout's run, fc runs inside the fused heads, losses finite, weights moved."""
    from delora_amd.models import ring_conv
    _dev()
    monkeypatch.setattr(ring_conv, "TRUNK_SEGMENTS", "mono")          # one process: [layer1..layer3] dropout [layer4]
    tr, batch = _trainer((64, 720), 2, **({"amp_dtype": amp} if amp else {}))
    model = tr.raw_model
    assert model.training and model.resnet.use_dropout
    fired = []
    model.resnet.fc.register_forward_hook(lambda *a: fired.append(1))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    trace = []
    monkeypatch.setattr(ring_conv, "BACKWARD_TRACE", trace)
    losses = []
    for _ in range(3):
        tr.optimizer.zero_grad(set_to_none=True)
        ep, _ = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses())
        losses.append(float(ep["loss_epoch"]))
    assert not getattr(model.resnet, "_module_path_noted", None)
    assert sum(1 for e in trace if e[0] == "segment") == 3 * 2 and trace.count(("channel_dropout", 256)) == 3, trace
    assert not fired, "fc must run inside the fused heads"
    assert all(np.isfinite(v) for v in losses)
    last = model.resnet.last_dropout
    assert tuple(last["channels"].shape) == (2, 256) and tuple(last["fc"].shape) == (2, model.resnet.fc.out_features)
    moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))


# ------------------------------------------------------------------------------------------------------------ 12: graph replay
def test_graph_replay_draws_fresh_masks_from_the_static_seed():
    """``use_dropout: True`` inside a captured step: the seed tensor is drawn by torch's generator inside the capture, so every replay
    writes a new seed into the static tensor and the kernels, which read it from device memory, draw new masks."""
    from delora_amd.deploy.graph_step import GraphedStep
    _dev()
    tr, batch = _trainer((16, 512), 2)
    model = tr.raw_model
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    gs = GraphedStep(tr, batch, warmup=3)
    losses, seen = [], []
    for _ in range(3):
        ep, _ = gs()
        torch.cuda.synchronize()
        losses.append(float(ep["loss_epoch"]))
        last = model.resnet.last_dropout
        seen.append((int(last["seed"].item()), last["channels"].clone(), last["fc"].clone()))
    assert all(np.isfinite(v) for v in losses)
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())
    print(f"[graph] captured = {gs.captured}, replayed steps = {gs.replayed_steps}, fallback steps = {gs.fallback_steps}")
    if not gs.captured:
        return                                   # GraphedStep printed the reason; the eager steps it fell back to trained (asserted above)
    assert gs.replayed_steps == 3
    for seed, ch, fc in seen:
        assert np.array_equal(ch.cpu().numpy().reshape(-1), site_scales(seed, SITE_CHANNELS, ch.numel()))
        assert np.array_equal(fc.cpu().numpy().reshape(-1), site_scales(seed, SITE_FC, fc.numel()))
    assert len({s for s, _, _ in seen}) == 3, "every replay must draw a fresh seed"
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1])


# ------------------------------------------------------------------------------------------------------------ 13: ranks
def test_two_ranks_with_equal_torch_seeds_drop_differently():
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    masks = []
    for rank in (0, 1):
        torch.manual_seed(123)
        seed = rc.mix_rank(rc.draw_seed(dev), rank, 2)
        ch = rc.dropout_scale(seed, SITE_CHANNELS, 0.2, 8 * 256)
        assert np.array_equal(ch.cpu().numpy(), site_scales(int(seed.item()), SITE_CHANNELS, 8 * 256))
        masks.append(ch)
    assert not torch.equal(masks[0], masks[1])
    util.measured("two ranks, equal torch seeds: fraction of channel decisions that agree (independent masks: 0.68)",
                  float((masks[0] == masks[1]).float().mean()), bound=0.68 + 6.0 * np.sqrt(0.68 * 0.32 / 2048))
