"""``pre_feature_extraction`` on the HIP path: the 80-channel stem Function, the ``RingTower`` Function and the whole model against
torch autograd in float64 on the CPU (the referee; the library path on the GPU is recorded next to it, without a bound), run-to-run
determinism, autocast, the training step (eager twice, and as a replayed graph) and the reference checkpoint layout."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import util

pytestmark = pytest.mark.gpu

SIZES = [(16, 128), (9, 100)]
SIZE_IDS = ["16x128", "9x100"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _ring_conv(x_nchw, w, stride):
    return F.conv2d(F.pad(x_nchw, (1, 1, 0, 0), mode="circular"), w, stride=stride, padding=(1, 0))


def _ref_stem(x, w1, act):
    """The operator chain of ``_ref_stem`` in tests/test_gpu_conv.py."""
    a = _ring_conv(x, w1, (1, 2))
    a = torch.tanh(a) if act == "tanh" else torch.relu(a)
    return F.max_pool2d(F.pad(a, (1, 1, 0, 0), mode="circular"), kernel_size=3, stride=(1, 2), padding=(1, 0))


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_wide_stem_function_against_torch(size, act):
    """``RingStemWide`` (conv1 80 -> 64 on the zero-padded 128-channel buffer + activation + pooling; backward: pooling gather, weight
    gradient and INPUT gradient on the direct kernels) against the same ops under torch autograd in float64 on the CPU, with the bounds
    ``test_stem_function_against_torch`` asserts for the 8-channel stem."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    H, W = size
    g = torch.Generator(device="cpu").manual_seed(19)
    x = torch.randn((2, 80, H, W), generator=g) * 0.5
    w1 = (torch.randn((64, 80, 3, 3), generator=g) * 0.05).to(dev).requires_grad_(True)
    assert rc.stem_supported((2, 80, H, W), 64)
    xw = torch.zeros((2, H, W, rc.TOWER_PITCH), device=dev)
    xw[..., :80] = x.permute(0, 2, 3, 1).to(dev)
    xw.requires_grad_(True)
    y = rc.RingStemWide.apply(xw, w1, rc.ACT[act], False)                              # [N,H,W/4,64]; False: a true dL/dx comes back
    gy = torch.randn(y.shape, generator=g).to(dev)
    y.backward(gy)
    xr = x.double().requires_grad_(True)
    w1r = w1.detach().cpu().double().requires_grad_(True)
    y_ref = _ref_stem(xr, w1r, act)
    y_ref.backward(gy.permute(0, 3, 1, 2).cpu().double())
    tag = f"wide stem[{act},{H}x{W}]"
    util.measured(f"{tag}: pooled output vs torch float64 (absolute)", float((y.detach().permute(0, 3, 1, 2).cpu() - y_ref.detach().float()).abs().max()),
                  bound=2e-5)
    util.measured(f"{tag}: conv1 weight gradient vs torch autograd (relative)", _rel(w1.grad.cpu(), w1r.grad.float()), bound=1e-5)
    util.measured(f"{tag}: input gradient vs torch autograd (relative)", _rel(xw.grad[..., :80].permute(0, 3, 1, 2).cpu(), xr.grad.float()), bound=1e-5)
    assert float(xw.grad[..., 80:].abs().max()) == 0.0, "the zero-padded channels received a gradient"


def _tower_modules(act):
    """The five CircularPad + Conv2d + activation modules of the model itself (a narrow network: only the tower is used)."""
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(16, 128, pre_feature_extraction=True, activation_fct=act, factor_fewer_resnet_channels=8, resnet_outputs=64)
    torch.manual_seed(23)
    return OdometryModel(cfg).feature_extractor.double()


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_ring_tower_function_against_the_modules(size, act):
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    H, W = size
    B = 2
    tower = _tower_modules(act)
    convs = [m for m in tower if isinstance(m, torch.nn.Conv2d)]
    g = torch.Generator(device="cpu").manual_seed(29)
    x = torch.randn((B, 8, H, W), generator=g)
    assert rc.tower_supported(tuple(x.shape))
    ws = [c.weight.detach().float().to(dev).requires_grad_(True) for c in convs]
    xw = rc.RingTower.apply(x.to(dev), rc.ACT[act], True, *ws)                           # True: a true dL/dy goes in
    assert tuple(xw.shape) == (B, H, W, rc.TOWER_PITCH) and float(xw.detach()[..., 80:].abs().max()) == 0.0
    gy = torch.randn((B, H, W, rc.TOWER_PITCH), generator=g)
    xw.backward(gy.to(dev))
    y_ref = torch.cat((tower(x[:, :4].double()), tower(x[:, 4:].double())), dim=1)      # [B,80,H,W]
    y_ref.backward(gy[..., :80].permute(0, 3, 1, 2).double())
    tag = f"tower[{act},{H}x{W}]"
    util.measured(f"{tag}: output vs the modules in float64 (absolute)",
                  float((xw.detach()[..., :80].permute(0, 3, 1, 2).cpu() - y_ref.detach().float()).abs().max()), bound=2e-5)
    worst = 0.0
    for i, (w, c) in enumerate(zip(ws, convs)):
        assert w.grad is not None and w.grad.shape == w.shape
        e = _rel(w.grad.cpu(), c.weight.grad.float())
        worst = max(worst, e)
        util.measured(f"{tag}: weight gradient of layer {i + 1} vs torch autograd (relative)", e, bound=1e-5 if act == "tanh" else None)
    util.measured(f"{tag}: worst weight gradient of the five layers (relative)", worst, bound=1e-5 if act == "tanh" else None)


def _models(dev, H, W, act):
    """(HIP model, module-path model on the GPU, float64 CPU referee) with the same weights."""
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(H, W, device="cuda:0", activation_fct=act, pre_feature_extraction=True)
    torch.manual_seed(5)
    m_hip = OdometryModel(dict(cfg, cnn_impl="hip")).to(dev)
    assert m_hip.resnet.hip_path_takes(H, W, batch=2)
    m_hip.resnet.trunk_weights_channels_last()
    m_mod = OdometryModel(dict(cfg, cnn_impl="modules")).to(dev)
    m_mod.load_state_dict(m_hip.state_dict())
    m_cpu = OdometryModel(dict(util.repo_config(H, W, device="cpu", activation_fct=act, pre_feature_extraction=True), cnn_impl="modules")).double()
    m_cpu.load_state_dict({k: v.detach().cpu().double() for k, v in m_hip.state_dict().items()})
    return m_hip, m_mod, m_cpu


def _loss(t, q):
    """The loss of ``test_hip_trunk_matches_module_path``."""
    return t.square().sum() + (q * torch.arange(1, 5, device=q.device, dtype=q.dtype)).sum()


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_whole_model_with_the_tower_against_float64(size, act):
    dev = _dev()
    H, W = size
    m_hip, m_mod, m_cpu = _models(dev, H, W, act)
    x = torch.randn((2, 8, H, W), device=dev)
    out = []
    for m, xx in ((m_hip, x), (m_mod, x), (m_cpu, x.cpu().double())):
        t, q = m(xx)
        _loss(t, q).backward()
        out.append((t.detach().cpu().double(), q.detach().cpu().double()))
    assert not getattr(m_hip.resnet, "_module_path_noted", None), "the HIP model took the module path"
    tag = f"tower model[{act},{H}x{W}]"
    for i, nm in enumerate(("translation", "quaternion")):
        util.measured(f"{tag}: {nm} hip vs float64 (relative)", _rel(out[0][i], out[2][i]), bound=1e-5)
        util.measured(f"{tag}: {nm} module path (library convolutions) vs float64 (relative)", _rel(out[1][i], out[2][i]))
    errs, errs_mod, worst, name = [], [], 0.0, ""
    for (k, p), (_, p2), (_, pr) in zip(m_hip.named_parameters(), m_mod.named_parameters(), m_cpu.named_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, k
        ref = pr.grad
        e = float((p.grad.cpu().double() - ref).norm() / ref.norm().clamp_min(1e-30))
        errs.append(e)
        errs_mod.append(float((p2.grad.cpu().double() - ref).norm() / ref.norm().clamp_min(1e-30)))
        if e > worst:
            worst, name = e, k
        if e > 2e-5:
            print(f"  gradient of {k}: relative difference {e:.3e}")
    util.measured(f"{tag}: worst relative parameter-gradient difference, module path vs float64", max(errs_mod))
    util.measured(f"{tag}: worst relative parameter-gradient difference hip vs float64 ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))
    util.measured(f"{tag}: 25th percentile of the relative parameter-gradient differences hip vs float64", float(np.quantile(errs, 0.25)), bound=1e-5)


def test_two_passes_of_the_tower_model_are_bitwise_equal():
    dev = _dev()
    m_hip, _, _ = _models(dev, 16, 128, "tanh")
    x = torch.randn((2, 8, 16, 128), device=dev)
    runs = []
    for _ in range(2):
        m_hip.zero_grad(set_to_none=True)
        t, q = m_hip(x)
        _loss(t, q).backward()
        runs.append([t.detach().clone(), q.detach().clone()] + [p.grad.detach().clone() for p in m_hip.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two passes on the same input differ"
    # the reference's forward(image_1, image_2) takes the same path to the same bits
    t2, q2 = m_hip(x[:, :4], x[:, 4:])
    assert torch.equal(t2, runs[0][0]) and torch.equal(q2, runs[0][1])
    assert not getattr(m_hip.resnet, "_module_path_noted", None)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_autocast_tower_model_against_the_fp32_hip_model(dtype):
    """The quantities and per-dtype bounds of ``test_half_precision_network_against_the_fp32_network_at_full_size``; tower and stem stay
    fp32 inside autocast, the trunk runs on the half-precision kernels."""
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

    def run(amp):
        m.zero_grad(set_to_none=True)
        if amp is None:
            t, q = m(x)
        else:
            with torch.autocast("cuda", dtype=amp):
                t, q = m(x)
            t, q = t.float(), q.float()
        loss = (t.square().sum() + (q * torch.tensor([0.3, -0.2, 0.5, 1.0], device=dev)).sum())
        loss.backward()
        return t.detach(), q.detach(), float(loss.detach()), [p.grad.detach().clone() for p in m.parameters()]

    t32, q32, l32, g32 = run(None)
    th, qh, lh, gh = run(dtype)
    assert not getattr(m.resnet, "_module_path_noted", None), "autocast took the module path"
    name = str(dtype)[6:]
    rel_pose = {torch.bfloat16: 5e-2, torch.float16: 8e-3}[dtype]
    rel_grad = {torch.bfloat16: 1.5e-1, torch.float16: 3e-2}[dtype]
    util.measured(f"tower model {name} vs fp32 @{H}x{W}: translation (relative to its largest element)",
                  float((th - t32).abs().max() / t32.abs().max()), bound=rel_pose)
    util.measured(f"tower model {name} vs fp32 @{H}x{W}: quaternion (relative to its largest element)",
                  float((qh - q32).abs().max() / q32.abs().max()), bound=rel_pose)
    util.measured(f"tower model {name} vs fp32 @{H}x{W}: loss (relative)", abs(lh - l32) / abs(l32), bound=rel_pose)
    worst, worst_cos = 0.0, 1.0
    for a, b in zip(gh, g32):
        worst = max(worst, float((a - b).norm() / b.norm().clamp_min(1e-30)))
        worst_cos = min(worst_cos, float(F.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0)))
    util.measured(f"tower model {name} vs fp32 @{H}x{W}: worst parameter gradient |dg| / |g|", worst, bound=rel_grad)
    util.measured(f"tower model {name} vs fp32 @{H}x{W}: 1 - worst cosine between parameter gradients", 1.0 - worst_cos, bound=rel_grad ** 2)
    assert all(torch.isfinite(a).all() for a in gh)


def _trainer():
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(16, 512, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=2, learning_rate=1e-5,
                           pre_feature_extraction=True)
    ds = SyntheticPairDataset(cfg, "kitti", 2, rings=16, azimuth_steps=600)
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    assert tr.raw_model.resnet.hip_path_takes(16, 512, batch=2)
    return tr, tr.to_device([ds[0], ds[1]])


def _eager_steps(tr, batch, n=4):
    losses = []
    for _ in range(n):
        tr.optimizer.zero_grad(set_to_none=True)
        ep, _ = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses())
        losses.append(float(ep["loss_epoch"]))
    return losses


def test_trainer_steps_with_the_tower_repeat_bitwise_and_replay_as_a_graph():
    from delora_amd.deploy.graph_step import GraphedStep
    _dev()
    tr_a, batch_a = _trainer()
    eager = _eager_steps(tr_a, batch_a)
    assert all(np.isfinite(v) for v in eager), eager
    assert not getattr(tr_a.raw_model.resnet, "_module_path_noted", None), "the training step took the module path"
    tr_b, batch_b = _trainer()
    again = _eager_steps(tr_b, batch_b)
    assert again == eager, (again, eager)
    for (k, a), (_, b) in zip(tr_a.raw_model.state_dict().items(), tr_b.raw_model.state_dict().items()):
        assert torch.equal(a, b), f"{k}: two trainers from the same seed differ after four steps"
    tr_g, batch_g = _trainer()
    gs = GraphedStep(tr_g, batch_g, warmup=3)
    assert gs.captured
    got = []
    for _ in range(4):
        ep, _ = gs()
        got.append(float(ep["loss_epoch"]))
    # the bounds of test_graphed_step_equals_eager_step_on_the_hip_trunk
    util.measured("graph replay vs eager with the tower (16x512, full width): worst relative loss difference over four steps",
                  float(np.max(np.abs(np.array(got) - np.array(eager)) / np.abs(np.array(eager)))), bound=2e-6)
    worst = max(float((a - b).abs().max()) for a, b in zip(tr_g.raw_model.state_dict().values(), tr_a.raw_model.state_dict().values()))
    util.measured("graph replay vs eager with the tower: largest weight difference after four steps", worst, bound=2e-7)


def test_reference_checkpoint_with_the_tower_loads_strictly():
    """The names did not move: the ``sd::`` entries of the reference's tower checkpoint load with ``strict=True`` (a narrow network,
    which runs on the module path)."""
    from delora_amd.models.model import OdometryModel
    dev = _dev()
    g = util.load_golden("model_tower_relu")
    over = {k[5:]: v for k, v in g.items() if k.startswith("cfg::")}
    over = {k: (str(v) if k == "activation_fct" else (bool(v) if k in ("pre_feature_extraction", "use_single_mlp_at_output") else int(v)))
            for k, v in over.items()}
    m = OdometryModel(util.repo_config(16, 128, device="cuda:0", **over)).to(dev)
    sd = {k[4:]: torch.from_numpy(v).to(dev) for k, v in g.items() if k.startswith("sd::")}
    m.load_state_dict(sd, strict=True)
    assert {f"feature_extractor.{i}.weight" for i in (1, 4, 7, 10, 13)} <= set(sd)
