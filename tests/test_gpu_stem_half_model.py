"""The half-precision stem in the model (config key ``amp_stem`` under ``amp_dtype``): ``ring_conv.RingStemH`` against the three entry
points and the derived weight-gradient bound, the whole network against the fp32 network inside the project's bounds for a few
roundings of the storage type, which entry points a training step calls with the key and without it, two trainers from one seed, and
the gate that keeps dropout and inputs that require a gradient on the fp32 stem."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import stem_half_ref as hr
from tests import stem_ref as sr
from tests import util

pytestmark = pytest.mark.gpu

DT = pytest.mark.parametrize("dtype", hr.DTYPES, ids=[hr.NAME[d] for d in hr.DTYPES])
NEW = ("dl_stem_input_nhwc_h", "dl_stem_conv1_h", "dl_stem_pool_fwd_h", "dl_stem_wgrad_h")
FP32_STEM = ("dl_conv2d_nhwc_f32", "dl_pool3x3s12_nhwc_fwd", "dl_stem_wgrad_f32", "dl_cast_f32_to_h")
H, W, B = 16, 128, 2


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _model(dev, act="tanh", seed=3, **over):
    from delora_amd.models.model import OdometryModel
    h, w = over.pop("hw", (H, W))
    cfg = util.repo_config(h, w, device=str(dev), activation_fct=act, cnn_impl=over.pop("cnn_impl", "hip"), **over)
    torch.manual_seed(seed)
    m = OdometryModel(cfg).to(dev)
    m.resnet.trunk_weights_channels_last()
    return m


def _range_image(dev, b=B, h=H, w=W, seed=5):
    """The input of tests/test_gpu_convh.py's full-size comparison: xyz + range in metres, smooth along the image, with empty pixels."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    az = torch.linspace(-np.pi, np.pi, w).view(1, 1, 1, w)
    el = torch.linspace(-0.4, 0.05, h).view(1, 1, h, 1)
    rng = 8.0 + 6.0 * torch.sin(3 * az + torch.rand((b, 2, 1, 1), generator=g)) + 2.0 * torch.rand((b, 2, h, w), generator=g)
    xyz = torch.stack((rng * torch.cos(el) * torch.cos(az), rng * torch.cos(el) * torch.sin(az), rng * torch.sin(el).expand_as(rng), rng), dim=2)
    xyz = xyz * (torch.rand((b, 2, 1, h, w), generator=g) > 0.05)
    return xyz.reshape(b, 8, h, w).to(dev)


def _loss(t, q):
    return t.float().square().sum() + (q.float() * torch.tensor([0.3, -0.2, 0.5, 1.0], device=q.device)).sum()


def _run(m, x, amp):
    m.zero_grad(set_to_none=True)
    if amp is None:
        t, q = m(x)
    else:
        with torch.autocast("cuda", dtype=amp):
            t, q = m(x)
    loss = _loss(t, q)
    loss.backward()
    return t.detach().float(), q.detach().float(), float(loss.detach()), [p.grad.detach().clone() for p in m.parameters()]


class _Recorder:
    """The bound library with the name of every entry point that is called appended to ``calls``."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("dl_"):
            return f

        def call(*a):
            self.calls.append(name)
            return f(*a)
        return call


def _record(monkeypatch):
    from delora_amd import _lib
    rec = _Recorder(_lib.load())
    monkeypatch.setattr(_lib, "load", lambda: rec)
    return rec


# ====================================================================================================== 9. the Function


@DT
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_ring_stem_h_equals_its_three_entry_points_and_its_gradient_holds_the_bound(act, dtype):
    from delora_amd import _lib
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    lib = _lib.load()
    code, a_code = hr.CODE[dtype], rc.ACT[act]
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = _range_image(dev)
    torch.manual_seed(11)
    w1 = (torch.randn((64, 8, 3, 3), device=dev) * (0.5 / (10.0 * np.sqrt(72.0)))).requires_grad_(True)
    y = rc.RingStemH.apply(x, w1, a_code, dtype)
    assert y.dtype == dtype and tuple(y.shape) == (B, H, W // 4, 64)
    # the composition, by hand
    x8h = torch.empty((B, H, W, 8), dtype=dtype, device=dev)
    a = torch.empty((B, H, W // 2, 64), dtype=dtype, device=dev)
    y2, win = torch.empty_like(y), torch.empty(y.shape, dtype=torch.int8, device=dev)
    ws_w = w1.detach().permute(0, 2, 3, 1).contiguous()
    _lib.check(lib.dl_stem_input_nhwc_h(_p(x), B, H, W, code, _p(x8h), st), "dl_stem_input_nhwc_h")
    _lib.check(lib.dl_stem_conv1_h(_p(x8h), _p(ws_w), B, H, W, a_code, code, _p(a), st), "dl_stem_conv1_h")
    _lib.check(lib.dl_stem_pool_fwd_h(_p(a), B, H, W // 2, 64, code, _p(y2), _p(win), st), "dl_stem_pool_fwd_h")
    assert torch.equal(y.detach().view(torch.int16), y2.view(torch.int16)), "RingStemH.forward is not the three entry points"
    assert torch.equal(x8h.view(torch.int16), x.permute(0, 2, 3, 1).contiguous().to(dtype).view(torch.int16))
    g = torch.randn(y.shape, device=dev).to(dtype)
    y.backward(g)
    assert w1.grad.dtype == torch.float32 and w1.grad.shape == w1.shape and tuple(w1.grad.stride()) == tuple(w1.stride())
    a64, win_np, g64, x64 = a.cpu().double().numpy(), win.cpu().numpy(), g.cpu().double().numpy(), x8h.cpu().double().numpy()
    ref, bound = hr.wgrad_ref_and_bound(hr.gc_half(g64, a64, win_np, a_code, dtype), x64, B, H, W)
    util.measured(f"RingStemH {hr.NAME[dtype]} {act} {H}x{W}: dw against float64 autograd of the rounded operands, worst error / bound",
                  float((np.abs(w1.grad.cpu().double().numpy() - ref) / np.maximum(bound, 1e-300)).max()), bound=1.0)
    with pytest.raises(_lib.DeloraHipError):
        rc.RingStemH.apply(x.clone().requires_grad_(True), w1, a_code, dtype)


# ====================================================================================================== 10. the whole network


@DT
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_network_with_half_stem_against_the_fp32_network(act, dtype):
    """The construction and the bounds of test_half_precision_network_against_the_fp32_network_at_full_size (tests/test_gpu_convh.py:
    a few roundings of the storage type), at the 64x720, B = 2 shape of that test.  Recorded next to them, unbounded: the same deviations
    with the fp32 stem (``amp_stem: false``) and of the module path under autocast, whose library conv1 rounds its operands the same way.

    Not at 16x128: there the fp32-stem network itself leaves the bounds (measured on the MI355X, bf16 / tanh: relative loss 0.076 against
    0.05 -- the loss is a difference of sums and nearly cancels on so small a map; the module path: 0.20; the half stem: 0.25)."""
    dev = _dev()
    H, W = 64, 720
    m = _model(dev, act, hw=(H, W))
    x = _range_image(dev, h=H, w=W)
    name = hr.NAME[dtype]
    rel_pose = {torch.bfloat16: 5e-2, torch.float16: 8e-3}[dtype]
    rel_grad = {torch.bfloat16: 1.5e-1, torch.float16: 3e-2}[dtype]
    t32, q32, l32, g32 = _run(m, x, None)

    def deviations(run):
        th, qh, lh, gh = run
        worst, worst_cos = 0.0, 1.0
        for a, b in zip(gh, g32):
            worst = max(worst, float((a - b).norm() / b.norm().clamp_min(1e-30)))
            worst_cos = min(worst_cos, float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0)))
        assert all(torch.isfinite(a).all() for a in gh)
        return {"translation (relative to its largest element)": float((th - t32).abs().max() / t32.abs().max()),
                "quaternion (relative to its largest element)": float((qh - q32).abs().max() / q32.abs().max()),
                "loss (relative)": abs(lh - l32) / abs(l32), "worst parameter gradient |dg| / |g|": worst,
                "1 - worst cosine between parameter gradients": 1.0 - worst_cos}

    off = deviations(_run(m, x, dtype))
    mm = _model(dev, act, cnn_impl="modules", hw=(H, W))
    mm.load_state_dict(m.state_dict())
    mod = deviations(_run(mm, x, dtype))
    m.resnet.amp_stem = True
    with torch.autocast("cuda", dtype=dtype):
        assert m.resnet.hip_half_stem_applicable(x) == dtype
    on = deviations(_run(m, x, dtype))
    for k in on:
        util.measured(f"network {name} {act} @{H}x{W}, amp_stem false (fp32 stem) vs fp32: {k}", off[k])
        util.measured(f"network {name} {act} @{H}x{W}, module path under autocast vs fp32: {k}", mod[k])
    bounds = {"translation (relative to its largest element)": rel_pose, "quaternion (relative to its largest element)": rel_pose,
              "loss (relative)": rel_pose, "worst parameter gradient |dg| / |g|": rel_grad,
              "1 - worst cosine between parameter gradients": rel_grad ** 2}
    for k in on:
        util.measured(f"network {name} {act} @{H}x{W}, amp_stem true vs fp32: {k}", on[k], bound=bounds[k])


# ====================================================================================================== 11. what a step calls


def test_training_step_calls_the_half_stem_and_nothing_of_the_fp32_stem(monkeypatch):
    """A training step under autocast, by the names of the library's entry points it calls (each launches its own kernels and nothing
    else) and, for library convolutions, by the operator names under the profiler.  With the key: the four half-stem entry points once
    each, no fp32 conv1, no fp32 pooling, no fp32 fused weight gradient, no ``dl_cast_f32_to_h``, no library convolution.  Without it:
    none of the new entry points, the fp32 stem's once each -- and everything that is not the stem is the same list in the same order."""
    dev = _dev()
    m = _model(dev)
    m.train()
    x = _range_image(dev)
    rec = _record(monkeypatch)

    def step(key):
        m.resnet.amp_stem = key
        rec.calls.clear()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            _run(m, x, torch.bfloat16)
            torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        assert names, "the profiler recorded nothing"
        library = sorted(n for n in names if n.startswith("aten::convolution") or n.startswith("aten::_convolution") or n.startswith("aten::miopen_")
                         or n.startswith("aten::cudnn_") or "conv2d" in n)
        assert not library, f"library convolutions ran: {library}"
        return list(rec.calls)

    off = step(False)
    on = step(True)
    for n in NEW:
        assert on.count(n) == 1, (n, on)
        assert n not in off, (n, off)
    for n in FP32_STEM:
        assert n not in on, f"{n} was called with amp_stem on"
        assert off.count(n) == 1, (n, off)
    assert "dl_stem_wgrad_h_workspace_bytes" in on
    # everything that is not the stem is the same list of calls, in the same order
    stem = set(NEW) | set(FP32_STEM) | {"dl_stem_wgrad_h_workspace_bytes", "dl_stem_wgrad_workspace_bytes"}
    assert [n for n in on if n not in stem] == [n for n in off if n not in stem]
    assert not getattr(m.resnet, "_module_path_noted", None)


# ====================================================================================================== 12. the trainer


def _trainer(dtype, **over):
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(H, W, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=2, learning_rate=1e-4,
                           amp_dtype=str(dtype)[6:], **over)
    ds = SyntheticPairDataset(cfg, "kitti", 2, rings=16, azimuth_steps=160)
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    return tr, tr.to_device([ds[0], ds[1]])


def _steps(tr, batch, n=4):
    losses = []
    for _ in range(n):
        tr.optimizer.zero_grad(set_to_none=True)
        ep, _ = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses())
        losses.append(float(ep["loss_epoch"]))
    return losses


@DT
def test_two_trainers_with_the_half_stem_agree_bitwise(dtype, monkeypatch, capsys):
    _dev()
    rec = _record(monkeypatch)
    tr_a, batch_a = _trainer(dtype, amp_stem=True)
    assert tr_a.raw_model.resnet.amp_stem is True
    w0 = tr_a.raw_model.resnet.conv1.weight.detach().clone()
    first = _steps(tr_a, batch_a)
    assert all(np.isfinite(v) for v in first), first
    assert rec.calls.count("dl_stem_wgrad_h") == len(first) and "dl_stem_wgrad_f32" not in rec.calls
    tr_b, batch_b = _trainer(dtype, amp_stem=True)
    again = _steps(tr_b, batch_b)
    assert again == first, (again, first)
    for (k, a), (_, b) in zip(tr_a.raw_model.state_dict().items(), tr_b.raw_model.state_dict().items()):
        assert torch.equal(a, b), f"{k}: two trainers from the same seed differ"
    w1 = tr_a.raw_model.resnet.conv1.weight.detach()
    assert torch.isfinite(w1).all() and not torch.equal(w1, w0), "conv1.weight has not moved"
    assert "MODULE path" not in capsys.readouterr().out


# ====================================================================================================== 13. the gate


@pytest.mark.parametrize("why", ["dropout", "input gradient"])
def test_gate_keeps_the_fp32_stem(why, monkeypatch):
    """Active dropout, or an input that requires a gradient: a model with the key takes the fp32 stem -- the parent's entry points --
    and computes what the model without the key computes, bit for bit."""
    dev = _dev()
    over = {"use_dropout": True} if why == "dropout" else {}
    m_key, m_ref = _model(dev, **over, amp_stem=True), _model(dev, **over)
    m_ref.load_state_dict(m_key.state_dict())
    assert m_key.resnet.amp_stem is True and m_ref.resnet.amp_stem is False
    for m in (m_key, m_ref):
        m.train()
    x = _range_image(dev)
    rec = _record(monkeypatch)
    # the gradient with respect to the image comes from the library's convolution backward (RingStem, both models): its deterministic
    # algorithms, and one discarded pass so that its algorithm search lies behind both compared passes
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)
    if why == "input gradient":
        _run(m_ref, x.clone().requires_grad_(True), torch.bfloat16)
    runs, calls = [], []
    for m in (m_key, m_ref):
        xx = x.clone().requires_grad_(True) if why == "input gradient" else x
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert m.resnet.hip_half_stem_applicable(xx) is None and m.resnet.hip_half_applicable(xx) == torch.bfloat16
        torch.manual_seed(21)                            # (the dropout seed of the pass is drawn from torch's generator)
        rec.calls.clear()
        t, q, loss, grads = _run(m, xx, torch.bfloat16)
        calls.append(list(rec.calls))
        runs.append([t, q] + grads + ([xx.grad.detach().clone()] if why == "input gradient" else []))
    assert calls[0] == calls[1]
    assert not set(NEW) & set(calls[0]) and "dl_cast_f32_to_h" in calls[0] and "dl_pool3x3s12_nhwc_fwd" in calls[0]
    assert ("dl_stem_input_nhwc_drop_f32" if why == "dropout" else "dl_pool3x3s12_nhwc_bwd") in calls[0]
    for a, b in zip(*runs):
        assert torch.equal(a, b), "the gated model differs from the model without the key"
    # the same model in eval (dropout inactive), or on a plain input: the half stem
    m_key.eval()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert m_key.resnet.hip_half_stem_applicable(x) == torch.bfloat16
