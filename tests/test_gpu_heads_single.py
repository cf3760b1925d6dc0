"""The single-MLP head (``use_single_mlp_at_output``) as ``dl_heads_single_fwd`` / ``dl_heads_single_bwd``: against a float64 torch
replica of the chain, one case bit for bit on small integers, the autograd Function against the torch modules at the bound of
tests/test_gpu_conv.py::test_fused_heads_against_the_torch_modules, and the whole model (also behind the tower, with dropout)
against the module path.  Device buffers live in NaN-filled arenas with guard zones; the workspace has exactly the promised size."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import tail_ref as tr
from tests import util
from tests.test_dropout_host import SITE_CHANNELS, SITE_FC, SITE_INPUT, site_scales
from tests.test_gpu_tail_exact import Bufs, _p, _stream

pytestmark = pytest.mark.gpu

TIGHT = 1e-5                                          # tests/test_gpu_conv.py: the operator-level bound of the two-head Function
HIDDEN = (512, 512, 256, 64)                          # reference src/models/model.py:59-72


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _actf(v, act):
    return torch.tanh(v) if act == 1 else (torch.relu(v) if act == 2 else v)


def single_ref(x, W, b, act, scale=None, g_t=None, g_r=None):
    """The chain in the dtype of its arguments under autograd: dict of the five activated outputs ``a0..a4``, ``rot_raw``,
    ``translation``, ``rotation``, ``norm`` and, with g_t / g_r, the gradients of sum(translation g_t) + sum(rotation g_r):
    ``d_w0..5``, ``d_b0..5``, ``grad_x``."""
    x = x.detach().clone().requires_grad_(True)
    W = [w.detach().clone().requires_grad_(True) for w in W]
    b = [v.detach().clone().requires_grad_(True) for v in b]
    out, a = {}, x
    for l in range(5):
        pre = a @ W[l].t() + b[l]
        if l == 0 and scale is not None:
            pre = pre * scale
        a = _actf(pre, act)
        out[f"a{l}"] = a
    raw = a @ W[5].t() + b[5]
    out["rot_raw"], out["translation"] = raw[:, :4], raw[:, 4:]
    out["norm"] = out["rot_raw"].norm().reshape(1)
    out["rotation"] = out["rot_raw"] / out["norm"]
    if g_t is not None:
        ((out["translation"] * g_t).sum() + (out["rotation"] * g_r).sum()).backward()
        out["grad_x"] = x.grad
        for l in range(6):
            out[f"d_w{l}"], out[f"d_b{l}"] = W[l].grad, b[l].grad
    return {k: v.detach() for k, v in out.items()}


FWD_OUT = ("a0", "a1", "a2", "a3", "a4", "rot_raw", "translation", "rotation", "norm")
BWD_OUT = tuple(f"d_{k}{l}" for l in range(6) for k in "wb") + ("grad_x",)


class SingleRun:
    """One case on the device through the C ABI."""

    def __init__(self, x, W, b, scale, dev):
        from delora_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.B = x.shape[0]
        self.sizes = [x.shape[1]] + [w.shape[0] for w in W[:5]]                       # F, R, H1..H4
        self.widths = self.sizes[1:]
        B = self.B
        self.bufs = bf = Bufs(dev)
        self.x = bf.inp(x, name="x")
        self.W, self.b = [bf.inp(w, name=f"w{l}") for l, w in enumerate(W)], [bf.inp(v, name=f"b{l}") for l, v in enumerate(b)]
        self.scale = bf.inp(scale, name="fc_scale")
        self.params = self.struct(self.W, self.b)
        self.fo = {"acts": bf.out((B * sum(self.widths),), name="acts"), "rot_raw": bf.out((B, 4), name="rot_raw"),
                   "translation": bf.out((B, 3), name="translation"), "rotation": bf.out((B, 4), name="rotation"), "norm": bf.out((1,), name="norm")}
        self.dW, self.db = [bf.out(tuple(w.shape), name=f"d_w{l}") for l, w in enumerate(W)], [bf.out(tuple(v.shape), name=f"d_b{l}") for l, v in enumerate(b)]
        self.grads = self.struct(self.dW, self.db)
        self.gx = bf.out(tuple(x.shape), name="grad_x")
        nbytes = int(self.lib.dl_heads_single_bwd_workspace_bytes(B, *self.sizes))
        assert nbytes > 0
        self.wsp = bf.ws(nbytes)

    def struct(self, W, b):
        s = self.L.HeadsSingleParams()
        for l in range(6):
            s.w[l], s.b[l] = W[l].data_ptr(), b[l].data_ptr()
        return s

    def split(self, acts):
        out, o = {}, 0
        for l, n in enumerate(self.widths):
            out[f"a{l}"] = acts[o:o + self.B * n].view(self.B, n)
            o += self.B * n
        return out

    def fwd(self, act, use_scale):
        s, o = self, self.fo
        s.bufs.poison()
        s.L.check(s.lib.dl_heads_single_fwd(_p(s.x), ctypes.byref(s.params), s.B, *s.sizes, act, _p(s.scale if use_scale else None), _p(o["acts"]),
                                            _p(o["rot_raw"]), _p(o["translation"]), _p(o["rotation"]), _p(o["norm"]), _stream()), "dl_heads_single_fwd")
        s.bufs.written(f"single head fwd B={s.B} {s.sizes} act {act}", only=tuple(o.values()))
        out = {k: v.cpu() for k, v in o.items() if k != "acts"}
        out.update(s.split(o["acts"].cpu()))
        return out

    def bwd(self, act, use_scale, ref, g_t, g_r):
        s = self
        s.bufs.poison()
        acts = s.bufs.inp(torch.cat([ref[f"a{l}"].reshape(-1) for l in range(5)]), name="saved acts")
        rr, nm = s.bufs.inp(ref["rot_raw"], name="saved rot_raw"), s.bufs.inp(ref["norm"], name="saved norm")
        gt_d, gr_d = s.bufs.inp(g_t, name="grad_translation"), s.bufs.inp(g_r, name="grad_rotation")
        s.L.check(s.lib.dl_heads_single_bwd(_p(s.x), ctypes.byref(s.params), s.B, *s.sizes, act, _p(s.scale if use_scale else None), _p(acts), _p(rr),
                                            _p(nm), _p(gt_d), _p(gr_d), ctypes.byref(s.grads), _p(s.gx), _p(s.wsp), _stream()), "dl_heads_single_bwd")
        s.bufs.written(f"single head bwd B={s.B} {s.sizes} act {act}", only=tuple(s.dW) + tuple(s.db) + (s.gx,))
        out = {f"d_w{l}": v.cpu() for l, v in enumerate(s.dW)}
        out.update({f"d_b{l}": v.cpu() for l, v in enumerate(s.db)})
        out["grad_x"] = s.gx.cpu()
        return out


def _case_real(B, F, R, seed=0):
    r = np.random.default_rng([seed, B, F, R])
    f = lambda v: torch.from_numpy(v.astype(np.float32).astype(np.float64))               # noqa: E731
    n = (F, R) + HIDDEN + (7,)
    W = [f(r.normal(size=(n[l + 1], n[l])) / np.sqrt(n[l])) for l in range(6)]
    b = [f(r.normal(size=(n[l + 1],)) * 0.1) for l in range(6)]
    scale = f(np.where(r.random((B, R)) < 0.2, 0.0, 1.25))
    scale[0, 0] = 1.25
    return f(r.normal(size=(B, F))), W, b, scale, f(r.normal(size=(B, 3))), f(r.normal(size=(B, 4)))


@pytest.mark.parametrize("R", [1000, 70])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_single_head_against_float64(B, R):
    """F = 512, the reference's hidden widths, tanh and relu, with and without ``fc_scale``: the nine forward outputs, the twelve
    parameter gradients and ``grad_x`` against the float64 replica, each within 1e-5 of the output's largest element -- the bound of
    the two-head Function's test.  (The per-element worst-case bound tests/tail_ref.py derives for the two-head kernels is no check
    at this depth: it grows by the absolute row sums of a weight matrix, about 18 at these widths, per layer, and passes the values
    themselves at the fourth.)  The backward is handed the replica's saved tensors rounded to fp32, as in tests/test_gpu_tail_exact.py,
    so a relu decision cannot differ.  The torch fp32 chain's deviation from the same replica is recorded in the same unit: it was
    at most 1.5e-6 on these cases when the test was written."""
    dev = _dev()
    x, W, b, scale, g_t, g_r = _case_real(B, 512, R)
    run = SingleRun(x, W, b, scale, dev)
    worst, worst_torch = {}, 0.0
    for act in (1, 2):
        for use in (False, True):
            sc = scale if use else None
            ref = single_ref(x, W, b, act, sc, g_t, g_r)
            got = run.fwd(act, use)
            got.update(run.bwd(act, use, {k: ref[k].to(torch.float32) for k in FWD_OUT}, g_t, g_r))
            f32 = single_ref(x.float(), [w.float() for w in W], [v.float() for v in b], act, None if sc is None else sc.float(), g_t.float(), g_r.float())
            for k in FWD_OUT + BWD_OUT:
                assert got[k].shape == ref[k].shape and not bool(torch.isnan(got[k]).any()), k
                worst[k] = max(worst.get(k, 0.0), _rel(got[k].double(), ref[k]))
                worst_torch = max(worst_torch, _rel(f32[k].double(), ref[k]))
    run.bufs.written("single head float64", only=())
    name = f"B={B} R={R}"
    util.measured(f"single head {name}: torch fp32 chain on the CPU vs float64, worst output (relative)", worst_torch)
    for k in FWD_OUT + BWD_OUT:
        util.measured(f"single head {name} vs float64: {k} (relative)", worst[k], bound=TIGHT)


def _case_exact(B, n, seed):
    r = np.random.default_rng([seed, B] + list(n))

    def w(shape, nnz):
        v = r.integers(1, 3, shape) * r.choice([-1, 1], shape)
        return torch.from_numpy((v * (r.random(shape) < min(1.0, nnz / shape[-1]))).astype(np.float64))
    W = [w((n[l + 1], n[l]), (24, 8, 6, 5, 4, 3)[l]) for l in range(6)]
    b = [torch.from_numpy(r.integers(-1, 2, (n[l + 1],)).astype(np.float64)) for l in range(6)]
    x = torch.from_numpy(r.integers(-2, 3, (B, n[0])).astype(np.float64))
    scale = torch.from_numpy(np.where(r.random((B, n[1])) < 0.2, 0.0, 1.25))
    g_t = torch.from_numpy(r.integers(-2, 3, (B, 3)).astype(np.float64))
    return x, W, b, scale, g_t


def _exact_headroom(x, W, b, scale, g_t):
    """Every value lives on the grid 1/4 (the mask's 1.25); the majorants of all sums (absolute values through the layers, relu
    bounded by the identity) times 4 stay below 2^24, so every order of summation gives the same fp32 number."""
    maj = tr._maj
    m, sums = x, []
    ms = []
    for l in range(6):
        m = maj(m, W[l], b[l]) * (scale.abs() if l == 0 else 1.0)
        ms.append(m)
    sums += ms
    g = torch.cat((torch.zeros(x.shape[0], 4, dtype=torch.float64), g_t.abs()), 1)
    for l in range(5, -1, -1):
        a = ms[l - 1] if l else x.abs()
        sums += [g.t() @ a, g.sum(0, keepdim=True)]
        g = g @ W[l].abs() * (scale.abs() if l == 1 else 1.0)
        sums.append(g)
    worst = max(float(s.max()) for s in sums) * 4.0
    assert worst < tr.LIMIT, f"{worst:.0f} grid steps: the case would not be exact"
    return worst / tr.LIMIT


def test_single_head_exact_on_small_integers():
    """Integer inputs, sparse integer weights, relu, the 0 / 1.25 mask, widths that are no multiples of anything (the layer sizes are
    arguments, not constants): a case is searched whose raw quaternions' batch sum of squares is a PERFECT SQUARE, so that the norm
    and, rotation being the correctly rounded quotient, every output is determined bit for bit.  With grad_rotation = 0 the rotation
    rows of the last layer's gradient are exactly zero and everything else equals the float64 reference."""
    dev = _dev()
    B, n = 3, (70, 41, 24, 20, 12, 10, 7)
    for seed in range(4000):
        x, W, b, scale, g_t = _case_exact(B, n, seed)
        ref = single_ref(x, W, b, 2, scale)
        ss = float((ref["rot_raw"] ** 2).sum()) * 16.0                       # rot_raw lives on the grid 1/4
        root = round(ss ** 0.5)
        if not (ss > 0 and root * root == ss and len({tuple(r) for r in ref["rot_raw"].tolist()}) == B):
            continue
        back = single_ref(x, W, b, 2, scale, g_t, torch.zeros(B, 4, dtype=torch.float64))
        if all(int((back[k] != 0).sum()) >= 8 for k in ("grad_x", "d_w0", "d_w1", "d_w2", "d_w3", "d_w4")):
            break
    else:
        raise AssertionError("no exact case with a perfect-square norm")
    _exact_headroom(x, W, b, scale, g_t)
    zero = torch.zeros(B, 4, dtype=torch.float64)
    ref = single_ref(x, W, b, 2, scale, g_t, zero)
    norm = ref["norm"].to(torch.float32)
    assert float(norm.double() ** 2) == float((ref["rot_raw"] ** 2).sum()), "the norm of the case is not an fp32 number"
    exp = {k: v.to(torch.float32) for k, v in ref.items()}
    exp["rotation"] = (ref["rot_raw"] / norm.double()).to(torch.float32)          # the correctly rounded fp32 quotient
    run = SingleRun(x, W, b, scale, dev)
    got = run.fwd(2, True)
    bad = [(k, m) for k in FWD_OUT if (m := cr.mismatches(got[k], exp[k], f"single head exact: {k}"))]
    gb = run.bwd(2, True, {k: exp[k] for k in FWD_OUT}, g_t, zero)
    assert not bool(exp["d_w5"][:4].any()) and not bool(exp["d_b5"][:4].any())
    bad += [(k, m) for k in BWD_OUT if (m := cr.mismatches(gb[k], exp[k], f"single head exact: {k}"))]
    run.bufs.written("single head exact", only=())
    assert not bad, f"mismatching elements (output, count): {bad}"
    assert int((gb["grad_x"] != 0).sum()) > 0 and int((gb["d_w0"] != 0).sum()) > 0, "the case's gradients died on the way down"


def _single_names():
    return ["resnet.fc.weight", "resnet.fc.bias"] + [f"fully_connected_rot_trans.{i}.{k}" for i in (1, 3, 5, 7, 9) for k in ("weight", "bias")]


@pytest.mark.parametrize("act,B", [("tanh", 8), ("relu", 3), ("tanh", 1), ("tanh", 16)])
def test_fused_single_head_function_against_the_torch_modules(act, B):
    """``FusedHeadsSingle`` against ``fc`` + the module chain + slice + whole-batch norm under torch autograd: the cases and the bound
    of tests/test_gpu_conv.py::test_fused_heads_against_the_torch_modules."""
    from delora_amd.models.model import OdometryModel
    from delora_amd.models import model_parts
    dev = _dev()
    cfg = util.repo_config(64, 2048, device="cuda:0", activation_fct=act, use_single_mlp_at_output=True)
    torch.manual_seed(3)
    m = OdometryModel(cfg).to(dev)
    g = torch.Generator(device="cpu").manual_seed(B)
    feat = torch.randn((B, 512), generator=g).to(dev)
    gt, gr = torch.randn((B, 3), generator=g).to(dev), torch.randn((B, 4), generator=g).to(dev)
    names = _single_names()
    params = dict(m.named_parameters())
    assert set(names) == {k for k in params if not k.startswith("resnet.") or k.startswith("resnet.fc.")}
    x1 = feat.clone().requires_grad_(True)
    t1, r1 = m._heads(m.resnet.fc(x1))
    ((t1 * gt).sum() + (r1 * gr).sum()).backward()
    ref = {n: params[n].grad.clone() for n in names}
    gx_ref = x1.grad.clone()
    m.zero_grad(set_to_none=True)
    x2 = feat.clone().requires_grad_(True)
    t2, r2 = model_parts.FusedHeadsSingle.apply(x2, 2 if act == "relu" else 1, *[params[n] for n in names])
    ((t2 * gt).sum() + (r2 * gr).sum()).backward()
    tag = f"fused single head[{act},B={B}]"
    util.measured(f"{tag}: translation vs torch modules (relative)", _rel(t2, t1.detach()), bound=TIGHT)
    util.measured(f"{tag}: rotation vs torch modules (relative)", _rel(r2, r1.detach()), bound=TIGHT)
    util.measured(f"{tag}: gradient of the pooled feature (relative)", _rel(x2.grad, gx_ref), bound=TIGHT)
    for n in names:
        assert params[n].grad is not None and params[n].grad.shape == params[n].shape and params[n].grad.is_contiguous(), n
    worst = max((_rel(params[n].grad, ref[n]), n) for n in names)
    util.measured(f"{tag}: worst parameter gradient vs torch autograd (relative) ({worst[1]})", worst[0], bound=TIGHT)


def _count_applications(monkeypatch):
    from delora_amd.models import model_parts
    calls = []
    fwd = model_parts.FusedHeadsSingle.forward
    monkeypatch.setattr(model_parts.FusedHeadsSingle, "forward", staticmethod(lambda ctx, *a: (calls.append(len(a)), fwd(ctx, *a))[1]))
    return calls


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_whole_model_with_the_single_head_matches_the_module_path(act, monkeypatch):
    """``use_single_mlp_at_output: True`` at 16x128, B = 2: the HIP model (stem + trunk + ``FusedHeadsSingle``) against the module path
    with the same weights, at the bounds of tests/test_gpu_conv.py::test_hip_trunk_matches_module_path."""
    from delora_amd.models.model import OdometryModel
    dev = _dev()
    H, W = 16, 128
    cfg = util.repo_config(H, W, device="cuda:0", activation_fct=act, use_single_mlp_at_output=True)
    torch.manual_seed(5)
    m_hip = OdometryModel(dict(cfg, cnn_impl="hip")).to(dev)
    assert m_hip.resnet.hip_path_takes(H, W, batch=2)
    m_hip.resnet.trunk_weights_channels_last()
    m_mod = OdometryModel(dict(cfg, cnn_impl="modules")).to(dev)
    m_mod.load_state_dict(m_hip.state_dict())
    assert set(m_hip.state_dict()) == set(m_mod.state_dict()) and {f"fully_connected_rot_trans.{i}.weight" for i in (1, 3, 5, 7, 9)} <= set(m_hip.state_dict())
    calls = _count_applications(monkeypatch)
    fired = []
    m_hip.resnet.fc.register_forward_hook(lambda *a: fired.append(1))
    x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(4)).to(dev)
    out = []
    for m in (m_hip, m_mod):
        t, q = m(x)
        (t.square().sum() + (q * torch.arange(1, 5, device=dev)).sum()).backward()
        out.append((t.detach(), q.detach()))
    assert calls == [14] and not fired, (calls, fired)            # x, act, twelve parameters -- once, and fc ran inside it
    assert not getattr(m_hip.resnet, "_module_path_noted", None)
    tagn = f"single head model[{act},{H}x{W}]"
    util.measured(f"{tagn}: translation hip vs modules (relative)", _rel(out[0][0], out[1][0]), bound=1e-5)
    util.measured(f"{tagn}: quaternion hip vs modules (relative)", _rel(out[0][1], out[1][1]), bound=1e-5)
    errs, worst, name = [], 0.0, ""
    for (k, p), (_, p2) in zip(m_hip.named_parameters(), m_mod.named_parameters()):
        assert p.grad is not None and p.grad.shape == p.shape, k
        e = float((p.grad - p2.grad).norm() / p2.grad.norm().clamp_min(1e-30))
        errs.append(e)
        if e > worst:
            worst, name = e, k
    util.measured(f"{tagn}: worst relative parameter-gradient difference hip vs modules ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))
    util.measured(f"{tagn}: 25th percentile of the relative parameter-gradient differences hip vs modules", float(np.quantile(errs, 0.25)), bound=1e-5)


class _Masks(torch.nn.Module):
    """Stands in for a torch dropout module: multiplies the k-th call's input by the k-th mask (tests/test_gpu_dropout.py)."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.calls = list(masks), 0

    def forward(self, x):
        m = self.masks[self.calls % len(self.masks)]
        self.calls += 1
        return x * m.to(x.dtype)


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_whole_model_with_single_head_tower_and_dropout_matches_the_module_path(act, monkeypatch):
    """All three switches at 16x128, B = 2, in train(): the HIP model (``RingTowerDrop``, wide stem, trunk with the channel mask,
    ``FusedHeadsSingle`` with ``fc_scale``) against the module path on the GPU whose dropout modules multiply by the masks the HIP
    model drew; same bounds."""
    from delora_amd.models.model import OdometryModel
    dev = _dev()
    H, W = 16, 128
    cfg = util.repo_config(H, W, device="cuda:0", activation_fct=act, use_single_mlp_at_output=True, pre_feature_extraction=True, use_dropout=True)
    torch.manual_seed(5)
    m_hip = OdometryModel(dict(cfg, cnn_impl="hip")).to(dev)
    m_hip.resnet.trunk_weights_channels_last()
    m_mod = OdometryModel(dict(cfg, cnn_impl="modules")).to(dev)
    m_mod.load_state_dict(m_hip.state_dict())
    m_hip.train(), m_mod.train()
    calls = _count_applications(monkeypatch)
    x = torch.randn((2, 8, H, W), generator=torch.Generator().manual_seed(4)).to(dev)
    torch.manual_seed(21)
    t0, q0 = m_hip(x)
    (t0.square().sum() + (q0 * torch.arange(1, 5, device=dev)).sum()).backward()
    assert calls == [15], calls                                   # ... plus fc_scale
    assert not getattr(m_hip.resnet, "_module_path_noted", None)
    last = m_hip.resnet.last_dropout
    seed = int(last["seed"].item())
    m_in = torch.from_numpy(site_scales(seed, SITE_INPUT, 2 * H * W * 80).reshape(2, H, W, 80)).permute(0, 3, 1, 2).contiguous().to(dev)
    assert np.array_equal(last["channels"].cpu().numpy().reshape(-1), site_scales(seed, SITE_CHANNELS, last["channels"].numel()))
    assert np.array_equal(last["fc"].cpu().numpy().reshape(-1), site_scales(seed, SITE_FC, last["fc"].numel()))
    m_mod.resnet.dropout_values = _Masks([m_in, last["fc"]])
    m_mod.resnet.dropout_channels = _Masks([last["channels"][:, :, None, None]])
    t1, q1 = m_mod(x)
    (t1.square().sum() + (q1 * torch.arange(1, 5, device=dev)).sum()).backward()
    assert m_mod.resnet.dropout_values.calls == 2 and m_mod.resnet.dropout_channels.calls == 1
    tagn = f"single head + tower + dropout model[{act},{H}x{W}]"
    util.measured(f"{tagn}: translation hip vs modules with the same masks (relative)", _rel(t0.detach(), t1.detach()), bound=1e-5)
    util.measured(f"{tagn}: quaternion hip vs modules with the same masks (relative)", _rel(q0.detach(), q1.detach()), bound=1e-5)
    errs, worst, name = [], 0.0, ""
    for (k, p), (_, p2) in zip(m_hip.named_parameters(), m_mod.named_parameters()):
        e = float((p.grad - p2.grad).norm() / p2.grad.norm().clamp_min(1e-30))
        errs.append(e)
        if e > worst:
            worst, name = e, k
    util.measured(f"{tagn}: worst relative parameter-gradient difference hip vs modules ({name})", worst, bound=(5e-5 if act == "tanh" else 5e-3))
    util.measured(f"{tagn}: 25th percentile of the relative parameter-gradient differences hip vs modules", float(np.quantile(errs, 0.25)), bound=1e-5)
