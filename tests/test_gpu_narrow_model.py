"""Narrow pose networks (``factor_fewer_resnet_channels`` 2 and 4) on the HIP path: the whole model against the same modules in float64
on the CPU (the referee; the module path on the GPU is recorded beside it, without a bound) with the bounds
``tests/test_gpu_tower_model.py::test_whole_model_with_the_tower_against_float64`` applies, no library convolution left in a forward +
backward, run-to-run determinism, and training steps that two trainers built from the same seed repeat bit for bit."""
import numpy as np
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu

SIZES = [(16, 128, 2), (5, 36, 3)]
SIZE_IDS = ["16x128-b2", "5x36-b3"]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _models(dev, H, W, B, act, f, referees=True):
    """(HIP model, module-path model on the GPU, float64 CPU referee) with the same weights."""
    from delora_amd.models.model import OdometryModel
    over = dict(activation_fct=act, factor_fewer_resnet_channels=f)
    cfg = util.repo_config(H, W, device="cuda:0", **over)
    torch.manual_seed(5)
    m_hip = OdometryModel(dict(cfg, cnn_impl="hip")).to(dev)
    assert m_hip.resnet.hip_path_takes(H, W, batch=B)
    m_hip.resnet.trunk_weights_channels_last()
    if not referees:
        return m_hip, None, None
    m_mod = OdometryModel(dict(cfg, cnn_impl="modules")).to(dev)
    m_mod.load_state_dict(m_hip.state_dict())
    m_cpu = OdometryModel(dict(util.repo_config(H, W, device="cpu", **over), cnn_impl="modules")).double()
    m_cpu.load_state_dict({k: v.detach().cpu().double() for k, v in m_hip.state_dict().items()})
    return m_hip, m_mod, m_cpu


def _loss(t, q):
    """The loss of ``test_hip_trunk_matches_module_path``."""
    return t.square().sum() + (q * torch.arange(1, 5, device=q.device, dtype=q.dtype)).sum()


@pytest.mark.parametrize("act", ["tanh", "relu"])
@pytest.mark.parametrize("f", [2, 4], ids=["factor2", "factor4"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_whole_narrow_model_against_float64(size, f, act):
    dev = _dev()
    H, W, B = size
    m_hip, m_mod, m_cpu = _models(dev, H, W, B, act, f)
    m_hip.train()
    x = torch.randn((B, 8, H, W), device=dev)
    out = []
    for m, xx in ((m_hip, x), (m_mod, x), (m_cpu, x.cpu().double())):
        t, q = m(xx)
        _loss(t, q).backward()
        out.append((t.detach().cpu().double(), q.detach().cpu().double()))
    assert not getattr(m_hip.resnet, "_module_path_noted", None), "the HIP model took the module path"
    tag = f"narrow model[factor {f},{act},{H}x{W}]"
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
    for i, nm in enumerate(("translation", "quaternion")):
        util.measured(f"{tag}: {nm} module path (library convolutions) vs float64 (relative)", _rel(out[1][i], out[2][i]))
    util.measured(f"{tag}: worst relative parameter-gradient difference, module path vs float64", max(errs_mod))
    for i, nm in enumerate(("translation", "quaternion")):
        util.measured(f"{tag}: {nm} hip vs float64 (relative)", _rel(out[0][i], out[2][i]), bound=1e-5)
    util.measured(f"{tag}: worst relative parameter-gradient difference hip vs float64 ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))


@pytest.mark.parametrize("f", [2, 4], ids=["factor2", "factor4"])
def test_no_library_convolution_runs_in_forward_and_backward(f):
    """Under the profiler (CPU activities: the operator names) a training-mode forward + backward dispatches no ``aten::convolution*`` and
    no ``aten::miopen_*`` operator -- the stem's backward included -- and prints no MODULE-path line."""
    dev = _dev()
    H, W, B = 16, 128, 2
    m_hip, _, _ = _models(dev, H, W, B, "tanh", f, referees=False)
    m_hip.train()
    x = torch.randn((B, 8, H, W), device=dev)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        t, q = m_hip(x)
        _loss(t, q).backward()
        torch.cuda.synchronize()
    names = {e.key for e in prof.key_averages()}
    assert names, "the profiler recorded nothing"
    library = sorted(n for n in names if n.startswith("aten::convolution") or n.startswith("aten::_convolution") or n.startswith("aten::miopen_")
                     or n.startswith("aten::cudnn_") or "conv2d" in n)
    assert not library, f"library convolutions ran: {library}"
    assert not getattr(m_hip.resnet, "_module_path_noted", None)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m_hip.parameters())


@pytest.mark.parametrize("f", [2, 4], ids=["factor2", "factor4"])
def test_two_passes_of_a_narrow_model_are_bitwise_equal(f):
    dev = _dev()
    m_hip, _, _ = _models(dev, 16, 128, 2, "tanh", f, referees=False)
    m_hip.train()
    x = torch.randn((2, 8, 16, 128), device=dev)
    runs = []
    for _ in range(2):
        m_hip.zero_grad(set_to_none=True)
        t, q = m_hip(x)
        _loss(t, q).backward()
        runs.append([t.detach().clone(), q.detach().clone()] + [p.grad.detach().clone() for p in m_hip.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two passes on the same input differ"
    # eval takes the same path to the same poses
    m_hip.eval()
    with torch.no_grad():
        t2, q2 = m_hip(x)
    assert torch.equal(t2, runs[0][0]) and torch.equal(q2, runs[0][1])
    assert not getattr(m_hip.resnet, "_module_path_noted", None)


def _trainer(use_dropout):
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(16, 128, device="cuda:0", factor_fewer_resnet_channels=4, resnet_outputs=128, unsupervised_at_start=True,
                           inference_only=False, batch_size=2, learning_rate=1e-4, use_dropout=use_dropout)
    ds = SyntheticPairDataset(cfg, "kitti", 2, rings=16, azimuth_steps=160)          # no normal lists: online normals
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    assert tr.raw_model.resnet.hip_path_takes(16, 128, batch=2)
    return tr, tr.to_device([ds[0], ds[1]])


def _steps(tr, batch, n=3):
    losses = []
    for _ in range(n):
        tr.optimizer.zero_grad(set_to_none=True)
        ep, _ = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses())
        losses.append(float(ep["loss_epoch"]))
    return losses


@pytest.mark.parametrize("use_dropout", [False, True], ids=["plain", "dropout"])
def test_two_trainers_from_one_seed_agree_bitwise_after_three_steps(use_dropout, capsys):
    """What the module path cannot give (its weight gradients add with atomics): losses and every entry of the state_dict bit-equal."""
    _dev()
    tr_a, batch_a = _trainer(use_dropout)
    first = _steps(tr_a, batch_a)
    assert all(np.isfinite(v) for v in first), first
    assert not getattr(tr_a.raw_model.resnet, "_module_path_noted", None), "the training step took the module path"
    tr_b, batch_b = _trainer(use_dropout)
    again = _steps(tr_b, batch_b)
    assert again == first, (again, first)
    for (k, a), (_, b) in zip(tr_a.raw_model.state_dict().items(), tr_b.raw_model.state_dict().items()):
        assert torch.equal(a, b), f"{k}: two trainers from the same seed differ after three steps"
    assert "MODULE path" not in capsys.readouterr().out
