"""``use_dropout`` together with ``pre_feature_extraction`` on the HIP path: the two element-wise kernels that put the site-1 mask on
the 80 tower channels (bit for bit against the host replica of tests/test_dropout_host.py, in NaN-filled arenas with guard zones),
p = 0 through the whole plumbing against the plain tower path, the model against the float64 module model WITH THE SAME MASKS,
autocast, determinism / fresh masks / eval(), and the training step (eager, and as a replayed graph)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as cr
from tests import util
from tests.test_dropout_host import SITE_CHANNELS, SITE_FC, SITE_INPUT, site_scales

pytestmark = pytest.mark.gpu

SIZES = [(16, 128), (9, 100)]                        # those of tests/test_gpu_tower_model.py
SIZE_IDS = ["16x128", "9x100"]
# (B, H, W) of the kernel tests: one pixel row of four, an odd batch with partial workgroups, a width above 64 that 64 does not divide
KERNEL_SHAPES = [(1, 1, 4), (3, 3, 20), (2, 5, 68)]
SEEDS = [1234, (7 << 32) | 1234]
CH, PITCH = 40, 128
ACT = {"none": 0, "tanh": 1, "relu": 2}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed_tensor(value, dev):
    return torch.tensor([int(value)], dtype=torch.int64, device=dev)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _wide(y5, B):
    """compact ``[2B,H,W,40]`` (image n = 2 b + k) -> the logical ``[B,H,W,80]`` tensor of the stem input"""
    _, H, W, C = y5.shape
    return y5.reshape(B, 2, H, W, C).permute(0, 2, 3, 1, 4).reshape(B, H, W, 2 * C)


def _compact(xw80):
    """the inverse of ``_wide``"""
    B, H, W, C2 = xw80.shape
    return xw80.reshape(B, H, W, 2, C2 // 2).permute(0, 3, 1, 2, 4).reshape(2 * B, H, W, C2 // 2)


# ------------------------------------------------------------------------------------------------------------ 1, 2: the kernels
@pytest.mark.parametrize("p", [0.2, 0.5])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_forward_kernel_equals_the_host_replica_bit_for_bit(shape, seed, p):
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    B, H, W = shape
    y5 = torch.randn((2 * B, H, W, CH), generator=torch.Generator().manual_seed(B * 100 + W))
    A = cr.Arenas(dev)
    y_d = A.arena(y5.shape, torch.float32, y5, "y5")
    sd = A.arena((2,), torch.int32, _seed_tensor(seed, "cpu").view(torch.int32), "seed", row_elems=0)
    xw = A.arena((B, H, W, PITCH), torch.float32, None, "xw")
    _lib.check(lib.dl_tower_wide_drop_f32(_p(y_d), _p(sd), p, B, H, W, CH, PITCH, _p(xw), _stream()), "dl_tower_wide_drop_f32")
    torch.cuda.synchronize()
    A.check(f"tower wide drop {shape}")
    got = xw.cpu().numpy()
    s = site_scales(seed, SITE_INPUT, B * H * W * 2 * CH, p).reshape(B, H, W, 2 * CH)
    assert set(np.unique(s).tolist()) <= {0.0, float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))}
    want = _wide(y5, B).numpy() * s                                              # one fp32 product per element
    assert want.dtype == np.float32
    assert np.array_equal(got[..., :2 * CH], want)
    assert np.array_equal(got[..., 2 * CH:], np.zeros((B, H, W, PITCH - 2 * CH), dtype=np.float32))


@pytest.mark.parametrize("act", ["none", "tanh", "relu"])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_kernel_equals_numpy_bit_for_bit(shape, seed, act):
    """y5 on the grid 1/8 in [-1, 1], integer gradients in [-4, 4], scales 0 / 1.25: ``g s`` lies on the grid 1/4, ``1 - y^2`` on the grid
    1/64, and their product needs 12 bits -- every intermediate is an fp32 number whether or not the compiler contracts ``1 - y y``."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    B, H, W = shape
    g = torch.Generator().manual_seed(B * 100 + W + 7)
    y5 = torch.randint(-8, 9, (2 * B, H, W, CH), generator=g).float() / 8.0
    gx = torch.full((B, H, W, PITCH), float("nan"))
    gx[..., :2 * CH] = torch.randint(-4, 5, (B, H, W, 2 * CH), generator=g).float()
    A = cr.Arenas(dev)
    gx_d, y_d = A.arena(gx.shape, torch.float32, gx, "gx"), A.arena(y5.shape, torch.float32, y5, "y5")
    sd = A.arena((2,), torch.int32, _seed_tensor(seed, "cpu").view(torch.int32), "seed", row_elems=0)
    g5 = A.arena(y5.shape, torch.float32, None, "g5")
    _lib.check(lib.dl_tower_wide_drop_bwd_f32(_p(gx_d), _p(y_d), _p(sd), 0.2, ACT[act], B, H, W, CH, PITCH, _p(g5), _stream()),
               "dl_tower_wide_drop_bwd_f32")
    torch.cuda.synchronize()
    A.check(f"tower wide drop backward {shape} {act}")
    s = _compact(torch.from_numpy(site_scales(seed, SITE_INPUT, B * H * W * 2 * CH).reshape(B, H, W, 2 * CH))).numpy()
    gc, y = _compact(gx[..., :2 * CH]).numpy(), y5.numpy()
    one = np.float32(1.0)
    dact = {"none": np.ones_like(y), "tanh": one - y * y, "relu": (y > 0).astype(np.float32)}[act]
    want = (gc * s) * dact
    assert want.dtype == np.float32 and 0 < float((s == 0).mean()) < 0.5
    got = g5.cpu().numpy()
    assert not np.isnan(got).any(), "channels 80..127 of gx reached g5"
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ the models
def _models(dev, H, W, act, cpu=False, **over):
    """(HIP model with both switches, the plain HIP tower model, float64 CPU module model or None) with the same weights."""
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(H, W, device="cuda:0", activation_fct=act, pre_feature_extraction=True, **over)
    torch.manual_seed(5)
    m_drop = OdometryModel(dict(cfg, cnn_impl="hip", use_dropout=True)).to(dev)
    assert m_drop.resnet.hip_path_takes(H, W, batch=2)
    m_drop.resnet.trunk_weights_channels_last()
    m_plain = OdometryModel(dict(cfg, cnn_impl="hip", use_dropout=False)).to(dev)
    m_plain.load_state_dict(m_drop.state_dict())
    m_plain.resnet.trunk_weights_channels_last()
    m_cpu = None
    if cpu:
        m_cpu = OdometryModel(dict(util.repo_config(H, W, device="cpu", activation_fct=act, pre_feature_extraction=True, use_dropout=True, **over),
                                   cnn_impl="modules")).double()
        m_cpu.load_state_dict({k: v.detach().cpu().double() for k, v in m_drop.state_dict().items()})
    return m_drop.train(), m_plain.train(), m_cpu


def _loss(t, q):
    """The loss of tests/test_gpu_tower_model.py."""
    return t.square().sum() + (q * torch.arange(1, 5, device=q.device, dtype=q.dtype)).sum()


def _run(m, x, amp=None, seed=None):
    m.zero_grad(set_to_none=True)
    if seed is not None:
        torch.manual_seed(seed)
    if amp is None:
        t, q = m(x)
    else:
        with torch.autocast("cuda", dtype=amp):
            t, q = m(x)
    t, q = t.float(), q.float()
    _loss(t, q).backward()
    return t.detach(), q.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------------------ 3: p = 0
@pytest.mark.parametrize("segments", ["layer", "mono"])
@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_p_zero_through_the_dropout_plumbing_is_the_plain_tower_path(size, act, amp, segments, monkeypatch):
    """Scales of exactly 1.0f everywhere: the compact fifth layer + ``dl_tower_wide_drop_f32`` must give the wide buffer of the plain
    ``RingTower``, so the poses are equal bit for bit.  Backward, relu: act' is 0 or 1, a product with it is exact wherever it is
    formed, so every parameter gradient is equal bit for bit.  tanh: ``1 - y^2`` moves from the epilogue of the stem's input gradient
    into ``dl_tower_wide_drop_bwd_f32``; a difference of more than 1e-6 of a gradient's norm is an error.

    ``trunk_segments: layer`` (what the trainer selects under DDP) already cuts the trunk in front of layer4, where the channel
    dropout sits: both models then run the same Functions and the comparison above holds for EVERY parameter.  In the default
    ``mono`` mode the dropout's cut changes which layers of the TRUNK share a merged weight-gradient launch, i.e.
    the summation order of some trunk weight gradients -- measured on the MI355X at 16x128: 3 (fp32) / 9 (bf16) trunk weights differ,
    by at most 1.5e-7 of their norm, for relu as for tanh; every parameter outside the trunk (tower, conv1, fc, heads) is bitwise
    equal for both activations.  So in ``mono`` the parameters outside the trunk are held to bit equality and the trunk's to the bound
    tests/test_gpu_dropout.py asserts for the same cut without the tower (2e-5 of the gradient's largest element)."""
    from delora_amd.models import ring_conv
    dev = _dev()
    monkeypatch.setattr(ring_conv, "TRUNK_SEGMENTS", segments)
    H, W = size
    m_drop, m_plain, _ = _models(dev, H, W, act)
    m_drop.resnet.dropout_p = 0.0
    x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(2)).to(dev)
    t0, q0, g0 = _run(m_plain, x, amp)
    t1, q1, g1 = _run(m_drop, x, amp)
    last = m_drop.resnet.last_dropout
    assert bool((last["channels"] == 1.0).all()) and bool((last["fc"] == 1.0).all()) and not hasattr(m_plain.resnet, "last_dropout")
    assert not getattr(m_drop.resnet, "_module_path_noted", None)
    assert torch.equal(t0, t1) and torch.equal(q0, q1)
    trunk = {k for k in g0 if k.startswith("resnet.layer")}
    differing = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    worst = max((float((g1[k] - g0[k]).norm() / g0[k].norm().clamp_min(1e-30)), k) for k in g0)
    tag = f"tower p=0 plumbing vs plain tower path [{segments},{'fp32' if amp is None else 'bf16'},{act},{H}x{W}]"
    util.measured(f"{tag}: parameter gradients that are not bitwise equal", len(differing))
    assert not [k for k in differing if k not in trunk], [k for k in differing if k not in trunk]
    if segments == "layer":
        util.measured(f"{tag}: worst relative parameter-gradient difference ({worst[1]})", worst[0], bound=0.0)
        assert not differing, differing                 # (tanh turned out bitwise as well: measured on the MI355X, all sixteen cases)
    else:
        util.measured(f"{tag}: worst relative parameter-gradient difference ({worst[1]})", worst[0])
        w_trunk = max((_rel(g1[k], g0[k]), k) for k in trunk)
        util.measured(f"{tag}: worst trunk weight gradient, relative to the gradient's largest element ({w_trunk[1]})", w_trunk[0], bound=2e-5)


# ------------------------------------------------------------------------------------------------------------ 4: parity
class _Masks(torch.nn.Module):
    """Stands in for a torch dropout module: multiplies the k-th call's input by the k-th mask (tests/test_gpu_dropout.py)."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = list(masks), 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m.to(x.dtype)


def _with_masks(m_mod, last, B, H, W, dtype=torch.float64):
    """The three dropout sites of a CPU module model become the masks the HIP model drew; site 1 is the replica's 80-channel mask."""
    seed = int(last["seed"].item())
    m_in = torch.from_numpy(site_scales(seed, SITE_INPUT, B * H * W * 80, last["p"]).reshape(B, H, W, 80)).permute(0, 3, 1, 2).contiguous()
    assert np.array_equal(last["channels"].cpu().numpy().reshape(-1), site_scales(seed, SITE_CHANNELS, last["channels"].numel(), last["p"]))
    assert np.array_equal(last["fc"].cpu().numpy().reshape(-1), site_scales(seed, SITE_FC, last["fc"].numel(), last["p"]))
    m_mod.resnet.dropout_values = _Masks([m_in.to(dtype), last["fc"].cpu().to(dtype)])                     # input first, fc output second
    m_mod.resnet.dropout_channels = _Masks([last["channels"].cpu().to(dtype)[:, :, None, None]])


POOL_MARGIN = 2e-6


def _pool_margin(m_cpu, x64, act):
    """Smallest gap between the largest and the second largest value of a 3x3 / stride (1,2) pooling window of conv1's activation in
    the float64 referee (tower, site-1 mask, conv1 written out with torch functions).  Max-pooling routes a window's gradient to ONE
    pixel: where two candidates are closer than the fp32 rounding error of the activation, fp32 and float64 may pick different ones,
    and one such pick moves one of the 65 536 gradient elements of the pooled map -- sqrt(2 / 65536) = 5.5e-3 of the gradient norm
    of EVERY parameter upstream (conv1 and the tower), whatever computes it.  Seen with the generator seed 6 at 16x128: conv1 and
    the five tower layers 2.4e-3 .. 3.0e-3 from float64, ``RingStemWide`` alone on that input 4.6e-3 / 5.0e-3 with a pooled output
    3.1e-7 from float64, every trunk and head parameter below 2e-5.  It is the pooling's analogue of a flipped relu mask and says
    nothing about the kernels, so the comparison runs on an input whose referee has no such near-tie."""
    fe = m_cpu.feature_extractor
    f = m_cpu.resnet.dropout_values.masks[0] * torch.cat((fe(x64[:, :4]), fe(x64[:, 4:])), dim=1)
    a = F.conv2d(F.pad(f, (1, 1, 0, 0), mode="circular"), m_cpu.resnet.conv1.weight, stride=(1, 2), padding=(1, 0))
    a = torch.tanh(a) if act == "tanh" else torch.relu(a)
    a = F.pad(F.pad(a, (1, 1, 0, 0), mode="circular"), (0, 0, 1, 1), value=float("-inf"))
    N, C, Hp, Wp = a.shape
    win = F.unfold(a.reshape(N * C, 1, Hp, Wp), kernel_size=3, stride=(1, 2))          # [N C, 9, windows]
    top = win.topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    if act == "relu":                               # two zeros tie exactly in every arithmetic, and carry no gradient
        gap = torch.where(top[:, 0] > 0, gap, torch.full_like(gap, float("inf")))
    return float(gap.min())


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_dropout_tower_model_against_float64_with_the_same_masks(size, act):
    """The HIP model in train() with both switches and ``cnn_impl: hip`` against the module model in float64 on the CPU whose three
    dropout modules multiply by the masks the HIP model used.  Bounds: those of
    tests/test_gpu_tower_model.py::test_whole_model_with_the_tower_against_float64 for the same size and activation -- a
    multiplication by 0 or 1.25 adds at most one rounding.

    The input is the first of the generator seeds 6, 7, 8, ... whose float64 referee keeps every pooling window's two largest values
    ``POOL_MARGIN`` = 2e-6 apart (``_pool_margin``; decided on the referee alone): conv1's activation is a tanh / relu of a 720-term fp32
    dot product, measured 3.1e-7 from float64 at this size, so a gap of 2e-6 cannot be reversed by rounding on either side.  relu takes
    seed 6 as it is: its bound is the one that allows for isolated flipped decisions, and its activations lie too densely near zero
    for such an input to exist (smallest gaps of 1e-7 on every seed)."""
    _parity(size, act)


def test_torch_heads_behind_the_dropout_tower_apply_the_fc_mask():
    """``fused_heads: False`` (as a batch above 16 would): ``forward_tower`` then runs ``fc`` and the heads as torch modules and
    multiplies the fc output by the mask itself.  The same comparison and bounds, relu at 9x100; ``fc`` must have run as a module."""
    _parity((9, 100), "relu", fused_heads=False)


def _parity(size, act, **over):
    dev = _dev()
    H, W = size
    m_hip, _, m_cpu = _models(dev, H, W, act, cpu=True, **over)
    m_cpu.train()
    fired = []
    m_hip.resnet.fc.register_forward_hook(lambda *a: fired.append(1))
    for xseed in range(6, 30):
        x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(xseed)).to(dev)
        t0, q0, g0 = _run(m_hip, x, seed=21)
        last = m_hip.resnet.last_dropout
        _with_masks(m_cpu, last, 2, H, W)
        with torch.no_grad():
            margin = _pool_margin(m_cpu, x.cpu().double(), act)
        print(f"generator seed {xseed}: smallest pooling gap of the referee {margin:.3g}")
        if margin >= POOL_MARGIN or act == "relu":
            break
    else:
        raise AssertionError("no input without a near-tie in a pooling window")
    assert not getattr(m_hip.resnet, "_module_path_noted", None), "the HIP model took the module path"
    assert bool(fired) == (over.get("fused_heads", True) is False), "fc ran on the wrong side of the fused heads"
    assert last["p"] == 0.2 and 0.5 < float((last["channels"] > 0).float().mean()) < 0.97
    t, q = m_cpu(x.cpu().double())
    _loss(t, q).backward()
    assert m_cpu.resnet.dropout_values.calls == 2 and m_cpu.resnet.dropout_channels.calls == 1
    tag = f"dropout tower model[{act},{H}x{W}{',torch heads' if over else ''}]"
    util.measured(f"{tag}: translation hip vs float64 with the same masks (relative)", _rel(t0.cpu().double(), t.detach()), bound=1e-5)
    util.measured(f"{tag}: quaternion hip vs float64 with the same masks (relative)", _rel(q0.cpu().double(), q.detach()), bound=1e-5)
    errs, worst, name = [], 0.0, ""
    for k, pr in m_cpu.named_parameters():
        ref = pr.grad
        e = float((g0[k].cpu().double() - ref).norm() / ref.norm().clamp_min(1e-30))
        errs.append(e)
        if e > worst:
            worst, name = e, k
    util.measured(f"{tag}: worst relative parameter-gradient difference hip vs float64 ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))
    util.measured(f"{tag}: 25th percentile of the relative parameter-gradient differences hip vs float64", float(np.quantile(errs, 0.25)), bound=1e-5)


def test_near_tie_input_agrees_once_the_pooling_picks_the_same_pixels():
    """The direct check behind ``_pool_margin``: the input the parity test passes over (generator seed 6, tanh, 16x128, masks of torch
    seed 21), through ``RingStemWide`` alone.  Against a float64 referee that pools with ITS OWN arg-max the gradients are recorded
    (4.6e-3 / 5.0e-3 when this was written); against the same referee pooling at the pixels the fp32 activation selects -- nothing
    else changed -- weight and input gradient must meet the bounds of
    tests/test_gpu_tower_model.py::test_wide_stem_function_against_torch.  A defect in a kernel would survive the alignment."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    H, W = 16, 128
    m, _, _ = _models(dev, H, W, "tanh")
    x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(6)).to(dev)
    torch.manual_seed(21)
    seed = rc.draw_seed(dev)
    with torch.no_grad():
        xw0 = rc.RingTowerDrop.apply(x, rc.ACT["tanh"], seed, 0.2, *m._tower_weights())
    w1 = m.resnet.conv1.weight.detach().clone().requires_grad_(True)
    xw = xw0.clone().requires_grad_(True)
    y = rc.RingStemWide.apply(xw, w1, rc.ACT["tanh"], False)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).to(dev)
    y.backward(gy)

    def pad(a):
        return F.pad(a, (1, 1, 0, 0), mode="circular")

    def referee(idx):
        xr = xw0[..., :80].permute(0, 3, 1, 2).cpu().double().requires_grad_(True)
        wr = w1.detach().cpu().double().requires_grad_(True)
        ap = pad(torch.tanh(F.conv2d(pad(xr), wr, stride=(1, 2), padding=(1, 0))))
        if idx is None:
            yr, idx = F.max_pool2d(ap, kernel_size=3, stride=(1, 2), padding=(1, 0), return_indices=True)
        else:
            yr = ap.flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
        yr.backward(gy.permute(0, 3, 1, 2).cpu().double())
        return yr.detach(), wr.grad, xr.grad, idx

    with torch.no_grad():                               # the pixels the fp32 activation selects (torch's rule, the kernel's rule)
        wp = torch.zeros((64, 3, 3, rc.TOWER_PITCH), device=dev)
        wp[..., :80] = w1.detach().permute(0, 2, 3, 1)
        a32 = rc.conv_nhwc(xw0, wp, stride=(1, 2), act=rc.ACT["tanh"], epilogue=rc.EPI_ACT).permute(0, 3, 1, 2)
        y32, idx32 = F.max_pool2d(pad(a32), kernel_size=3, stride=(1, 2), padding=(1, 0), return_indices=True)
        assert torch.equal(y32, y.detach().permute(0, 3, 1, 2)), "the pooling kernel does not return the maximum of its window"
    y_own, dw_own, gx_own, idx_own = referee(None)
    y_al, dw_al, gx_al, _ = referee(idx32.cpu())
    got_y, got_dw, got_gx = y.detach().permute(0, 3, 1, 2).cpu().double(), w1.grad.cpu().double(), xw.grad[..., :80].permute(0, 3, 1, 2).cpu().double()
    rel = lambda a, b: float((a - b).norm() / b.norm())                                 # noqa: E731
    tag = "wide stem on the near-tie input (seed 6)"
    util.measured(f"{tag}: windows where fp32 and float64 select different pixels", int((idx_own != idx32.cpu()).sum()))
    util.measured(f"{tag}: weight gradient vs the referee's own arg-max (relative, norm)", rel(got_dw, dw_own))
    util.measured(f"{tag}: input gradient vs the referee's own arg-max (relative, norm)", rel(got_gx, gx_own))
    util.measured(f"{tag}: pooled output vs float64 (absolute)", float((got_y - y_own).abs().max()), bound=2e-5)
    util.measured(f"{tag}: weight gradient, arg-max aligned (relative)", _rel(got_dw, dw_al), bound=1e-5)
    util.measured(f"{tag}: input gradient, arg-max aligned (relative)", _rel(got_gx, gx_al), bound=1e-5)


# ------------------------------------------------------------------------------------------------------------ 5: autocast
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_autocast_dropout_tower_model_against_the_fp32_hip_model_with_the_same_seed(dtype):
    """Same ``torch.manual_seed`` -> same masks in fp32 and inside autocast; input and bounds of
    tests/test_gpu_tower_model.py::test_autocast_tower_model_against_the_fp32_hip_model.

    One of those bounds is on the RELATIVE error of the loss, a sum of terms of either sign, and says something only where the fp32
    loss does not cancel: with the masks of torch seed 77 the fp32 model's loss is a small remainder of its terms and poses that
    agree to 1.2e-2 / 9.1e-3 (bound 5e-2) give a loss 0.77 off.  So the masks are those of the first torch seed 77, 78, ... for which
    the fp32 model's |loss| is at least half the sum of the magnitudes of its terms -- decided on the fp32 reference alone; the
    relative error of the loss is then at most twice that of its terms."""
    dev = _dev()
    H, W, B = 16, 128, 2
    m, _, _ = _models(dev, H, W, "tanh")
    g = torch.Generator(device="cpu").manual_seed(5)
    az = torch.linspace(-np.pi, np.pi, W).view(1, 1, 1, W)
    el = torch.linspace(-0.4, 0.05, H).view(1, 1, H, 1)
    rng = 8.0 + 6.0 * torch.sin(3 * az + torch.rand((B, 2, 1, 1), generator=g)) + 2.0 * torch.rand((B, 2, H, W), generator=g)
    xyz = torch.stack((rng * torch.cos(el) * torch.cos(az), rng * torch.cos(el) * torch.sin(az), rng * torch.sin(el).expand_as(rng), rng), dim=2)
    xyz = xyz * (torch.rand((B, 2, 1, H, W), generator=g) > 0.05)
    x = xyz.reshape(B, 8, H, W).to(dev)
    wq = torch.tensor([0.3, -0.2, 0.5, 1.0], device=dev)

    def run(amp, seed):
        m.zero_grad(set_to_none=True)
        torch.manual_seed(seed)
        if amp is None:
            t, q = m(x)
        else:
            with torch.autocast("cuda", dtype=amp):
                t, q = m(x)
            t, q = t.float(), q.float()
        loss = t.square().sum() + (q * wq).sum()
        loss.backward()
        last = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in m.resnet.last_dropout.items()}
        terms = float((t.square().sum() + (q * wq).abs().sum()).detach())
        return t.detach(), q.detach(), float(loss.detach()), [p.grad.detach().clone() for p in m.parameters()], last, terms

    for seed in range(77, 97):
        t32, q32, l32, g32, last32, terms = run(None, seed)
        print(f"torch seed {seed}: fp32 loss {l32:.4g}, sum of the magnitudes of its terms {terms:.4g}")
        if abs(l32) >= 0.5 * terms:
            break
    else:
        raise AssertionError("no masks with a loss that does not cancel")
    th, qh, lh, gh, lasth, _ = run(dtype, seed)
    assert not getattr(m.resnet, "_module_path_noted", None), "autocast took the module path"
    assert torch.equal(last32["seed"], lasth["seed"]) and torch.equal(last32["channels"], lasth["channels"]) and torch.equal(last32["fc"], lasth["fc"])
    name = str(dtype)[6:]
    rel_pose = {torch.bfloat16: 5e-2, torch.float16: 8e-3}[dtype]
    rel_grad = {torch.bfloat16: 1.5e-1, torch.float16: 3e-2}[dtype]
    tag = f"dropout tower model {name} vs fp32 @{H}x{W}"
    util.measured(f"{tag}: translation (relative to its largest element)", float((th - t32).abs().max() / t32.abs().max()), bound=rel_pose)
    util.measured(f"{tag}: quaternion (relative to its largest element)", float((qh - q32).abs().max() / q32.abs().max()), bound=rel_pose)
    util.measured(f"{tag}: loss (relative)", abs(lh - l32) / abs(l32), bound=rel_pose)
    worst, worst_cos = 0.0, 1.0
    for a, b in zip(gh, g32):
        worst = max(worst, float((a - b).norm() / b.norm().clamp_min(1e-30)))
        worst_cos = min(worst_cos, float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0)))
    util.measured(f"{tag}: worst parameter gradient |dg| / |g|", worst, bound=rel_grad)
    util.measured(f"{tag}: 1 - worst cosine between parameter gradients", 1.0 - worst_cos, bound=rel_grad ** 2)
    assert all(torch.isfinite(a).all() for a in gh)


# ------------------------------------------------------------------------------------------------------------ 6: behaviour
def test_deterministic_under_manual_seed_fresh_per_pass_off_in_eval_and_the_keep_rate():
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    H, W = 16, 128
    m, m_plain, _ = _models(dev, H, W, "tanh")
    x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(6)).to(dev)
    ta, qa, ga = _run(m, x, seed=31)
    seed_a = m.resnet.last_dropout["seed"].clone()
    tb, qb, gb = _run(m, x, seed=31)
    assert torch.equal(seed_a, m.resnet.last_dropout["seed"])
    assert torch.equal(ta, tb) and torch.equal(qa, qb) and all(torch.equal(ga[k], gb[k]) for k in ga)
    # the stem's input of that pass, made again from its seed: zeros exactly where the replica drops (tanh of a random image is never
    # exactly zero), channels 80.. zero
    with torch.no_grad():
        xw = rc.RingTowerDrop.apply(x, rc.ACT["tanh"], seed_a, 0.2, *m._tower_weights()).cpu().numpy()
    s = site_scales(int(seed_a.item()), SITE_INPUT, 2 * H * W * 80).reshape(2, H, W, 80)
    assert xw.shape == (2, H, W, 128) and np.array_equal(xw[..., :80] == 0, s == 0) and not xw[..., 80:].any()
    keep = float((xw[..., :80] != 0).mean())
    util.measured(f"dropout behind the tower: |site-1 keep rate - 0.8| over one 16x128, B = 2 pass ({s.size} decisions)", abs(keep - 0.8), bound=0.01)
    # two consecutive passes without reseeding: new masks
    ch1 = m.resnet.last_dropout["channels"].clone()
    with torch.no_grad():
        m(x)
    assert not torch.equal(ch1, m.resnet.last_dropout["channels"]) and not torch.equal(seed_a, m.resnet.last_dropout["seed"])
    # eval(): the non-dropout model bit for bit, no seed drawn
    m.eval(), m_plain.eval()
    del m.resnet.last_dropout
    state = torch.cuda.get_rng_state(dev)
    with torch.no_grad():
        (te, qe), (tp, qp) = m(x), m_plain(x)
    assert torch.equal(te, tp) and torch.equal(qe, qp)
    assert torch.equal(state, torch.cuda.get_rng_state(dev)), "eval() must not draw a seed"
    assert not hasattr(m.resnet, "last_dropout") and not torch.equal(ta, tp)
    assert not getattr(m.resnet, "_module_path_noted", None)


# ------------------------------------------------------------------------------------------------------------ 7: the step
def _trainer(size, **over):
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(size[0], size[1], device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=2, learning_rate=1e-5,
                           use_dropout=True, pre_feature_extraction=True, **over)
    ds = SyntheticPairDataset(cfg, "kitti", 2, rings=size[0], azimuth_steps=600)
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    assert tr.raw_model.resnet.hip_path_takes(size[0], size[1], batch=2)
    return tr, tr.to_device([ds[0], ds[1]])


@pytest.mark.parametrize("amp", [None, "bfloat16"], ids=["fp32", "bf16"])
def test_training_steps_with_both_switches_stay_on_the_hip_path_and_repeat_bitwise(amp, monkeypatch, capsys):
    from delora_amd.models import ring_conv
    _dev()
    over = {"amp_dtype": amp} if amp else {}
    trace = []
    monkeypatch.setattr(ring_conv, "BACKWARD_TRACE", trace)
    states, all_losses = [], []
    for _ in range(2):
        tr, batch = _trainer((16, 128), **over)
        model = tr.raw_model
        assert model.training and model.resnet.use_dropout and model.pre_feature_extraction
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        losses = []
        for _ in range(2):
            tr.optimizer.zero_grad(set_to_none=True)
            ep, _ = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses())
            losses.append(float(ep["loss_epoch"]))
        assert all(np.isfinite(v) for v in losses), losses
        assert not getattr(model.resnet, "_module_path_noted", None), "the training step took the module path"
        moved = [k for k, v in model.state_dict().items() if not torch.equal(v, before[k])]
        assert len(moved) == len(before), sorted(set(before) - set(moved))
        states.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        all_losses.append(losses)
    assert "MODULE path" not in capsys.readouterr().out
    assert trace.count(("tower_drop", 4, 40, 5)) == 4 and trace.count(("channel_dropout", 256)) == 4 and ("tower", 4, 40, 5) not in trace, trace
    assert all_losses[0] == all_losses[1], all_losses
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), f"{k}: two trainers from the same seed differ after two steps"


def test_graph_replay_with_both_switches_draws_fresh_masks():
    """``tests/test_gpu_dropout.py::test_graph_replay_draws_fresh_masks_from_the_static_seed`` with the tower in front: every replay
    writes a new seed into the static tensor, and the tower's two mask kernels read it from device memory like the others."""
    from delora_amd.deploy.graph_step import GraphedStep
    _dev()
    tr, batch = _trainer((16, 512))
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
    assert not getattr(model.resnet, "_module_path_noted", None)
    print(f"[graph] captured = {gs.captured}, replayed steps = {gs.replayed_steps}, fallback steps = {gs.fallback_steps}")
    if not gs.captured:
        return                                   # GraphedStep printed the reason; the eager steps it fell back to trained (asserted above)
    assert gs.replayed_steps == 3
    for seed, ch, fc in seen:
        assert np.array_equal(ch.cpu().numpy().reshape(-1), site_scales(seed, SITE_CHANNELS, ch.numel()))
        assert np.array_equal(fc.cpu().numpy().reshape(-1), site_scales(seed, SITE_FC, fc.numel()))
    assert len({s for s, _, _ in seen}) == 3, "every replay must draw a fresh seed"
    assert not torch.equal(seen[0][1], seen[1][1]) and not torch.equal(seen[1][1], seen[2][1])
