"""The torch-free inference path on the GPU (include/delora_hip.h: dl_pose_net_*, dl_odometry_push; deploy/native_infer.py;
tools/odometry_demo.hip) against the eval-mode Python path, BIT FOR BIT: both enqueue the same entry points with the same operands,
and the ABI promises deterministic results, so a differing bit is an orchestration bug -- there is no tolerance anywhere in this file.
Full-width network, random weights, trunk weights in channels-last storage; inputs are real projected pairs (empty pixels present)."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from delora_amd import geometry
from delora_amd.data import synthetic
from delora_amd.deploy import native_infer
from delora_amd.models import model as model_module
from delora_amd.ros_utils import odometry
from tests import util
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# B = 1 takes the split-K Winograd plan; 5 x 36 gives feature maps 9, 5, 3 and 2 wide with odd heights and partial tiles everywhere;
# 64 x 720 is the shipped image with its 45- and 23-wide maps
SHAPES = ((1, 16, 128), (2, 16, 128), (3, 5, 36), (1, 64, 720))


def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(H, W, act):
    cfg = util.repo_config(H, W, device="cuda:0", activation_fct=act, integrate_odometry=True)
    torch.manual_seed(11)
    model = model_module.OdometryModel(config=cfg).to(_dev()).eval()
    model.resnet.trunk_weights_channels_last()
    return model, cfg, geometry.Sensor.from_config(cfg, "kitti")


def _pairs(B, sensor, seed=40):
    """(image_prev, image_cur) ``[B,4,H,W]`` of B synthetic scan pairs through the HIP projection."""
    dev = _dev()
    scans = []
    for b in range(B):
        s1, s2, _ = synthetic.make_pair(seed + b, rings=16, azimuth_steps=140)
        scans += [torch.from_numpy(s1), torch.from_numpy(s2)]
    offs = torch.tensor(np.cumsum([0] + [s.shape[1] for s in scans]), dtype=torch.int32, device=dev)
    img = geometry.project(torch.cat(scans, dim=1).contiguous().to(dev), offs, max(s.shape[1] for s in scans), sensor)["image4"]
    prev, cur = img[0::2].contiguous(), img[1::2].contiguous()
    assert bool((prev[:, 3] != 0).any()) and bool((cur[:, 3] != 0).any())
    if sensor.H >= 16:                                           # (a 5 x 36 image may be fully occupied by 2240 points)
        assert bool((prev[:, 3] == 0).any()) and bool((cur[:, 3] == 0).any())      # empty pixels are present
    return prev, cur


def _python_path(model, prev, cur):
    """The reference of every test: the model's own eval forward on the stacked pair + the quaternion -> T kernel."""
    with torch.no_grad():
        t, q = model(torch.cat((prev, cur), dim=1))
        T = model.geometry_handler.get_transformation_matrix_quaternion(translation=t, quaternion=q, device=_dev())
    return t.clone(), q.clone(), T.clone()


@functools.lru_cache(maxsize=None)
def _case(B, H, W, act):
    """One (model, inputs, Python result) per shape and activation, shared by the tests below and never modified."""
    model, cfg, sensor = _model(H, W, act)
    prev, cur = _pairs(B, sensor)
    return model, sensor, prev, cur, _python_path(model, prev, cur)


def _same(got, want):
    for name, a, b in zip(("translation", "quaternion", "T"), got, want):
        assert a.shape == b.shape and torch.equal(a, b), (name, (a - b).abs().max().item())


@pytest.mark.parametrize("act", ("tanh", "relu"))
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_forward_equals_the_python_eval_path_bit_for_bit(B, H, W, act):
    model, _, prev, cur, want = _case(B, H, W, act)
    assert all(torch.isfinite(t).all() for t in want) and float(want[0].abs().max()) > 0
    net = native_infer.NativePoseNet(model, B, H, W)
    _same(net.forward(prev, cur), want)
    _same(net.forward(prev, cur), want)                         # and again on the used workspace


def test_strided_inputs_from_two_parent_buffers():
    """image_prev and image_cur are slices of two different larger buffers with different scan strides (6 and 9 planes per scan)."""
    B, H, W = 2, 16, 128
    model, _, prev, cur, want = _case(B, H, W, "tanh")
    pa = torch.full((B, 6, H, W), float("nan"), device=_dev())
    pb = torch.full((B, 9, H, W), float("nan"), device=_dev())
    pa[:, :4] = prev
    pb[:, 3:7] = cur
    a, b = pa[:, :4], pb[:, 3:7]
    assert a.stride(0) == 6 * H * W and b.stride(0) == 9 * H * W and not a.is_contiguous()
    _same(native_infer.NativePoseNet(model, B, H, W).forward(a, b), want)


@pytest.mark.parametrize("B,H,W", ((1, 16, 128), (3, 5, 36)))
def test_poisoned_arena_guards_intact_and_nothing_read_before_written(B, H, W):
    """Workspace and prepared weights are carved out of one buffer filled with a NaN bit pattern, 4 KiB guard bands around each; the
    outputs start as NaN.  Afterwards the guards hold their sentinel, the outputs are finite and equal those of a run on a zero-filled
    workspace (and the Python path's): nothing reads scratch it did not write, nothing writes outside what it was given."""
    model, _, prev, cur, want = _case(B, H, W, "tanh")
    probe = native_infer.NativePoseNet(model, B, H, W)
    wb, pb, G = probe.workspace_bytes, probe.prepared_bytes, 4096
    assert wb % 256 == 0 and pb % 256 == 0
    arena = torch.empty((G + wb + G + pb + G,), dtype=torch.uint8, device=_dev())
    assert arena.data_ptr() % 256 == 0
    arena.view(torch.int32).fill_(-1)                            # 0xffffffff: a NaN in every float
    guards = [arena[:G], arena[G + wb:2 * G + wb], arena[2 * G + wb + pb:]]
    for g in guards:
        g.fill_(0xA5)
    ws, prepared = arena[G:G + wb], arena[2 * G + wb:2 * G + wb + pb].view(torch.float32)
    out = tuple(torch.full((B,) + s, float("nan"), device=_dev()) for s in ((3,), (4,), (4, 4)))
    net = native_infer.NativePoseNet(model, B, H, W, prepared=prepared, workspace=ws)
    got = net.forward(prev, cur, out=out)
    torch.cuda.synchronize()
    assert all(bool((g == 0xA5).all()) for g in guards)
    assert all(bool(torch.isfinite(t).all()) for t in got) and got[0].data_ptr() == out[0].data_ptr()
    assert bool(torch.isfinite(prepared).all())
    clean = native_infer.NativePoseNet(model, B, H, W, workspace=torch.zeros((wb,), dtype=torch.uint8, device=_dev()))
    _same(got, clean.forward(prev, cur))
    _same(got, want)


def test_weights_are_prepared_once_and_the_cache_is_real():
    """Two forward passes on different inputs after a SINGLE prepare each equal the Python path.  Then a Winograd layer's weight is
    changed in place WITHOUT preparing again: the native result does not move (that layer still runs on the transformed weights made
    before the change -- the cache is real, nothing re-derives them per forward), while the Python path, which transforms the weights
    on every forward, does; after ``prepare()`` the two agree again."""
    B, H, W = 1, 16, 128
    model, cfg, sensor = _model(H, W, "tanh")
    model = model_module.OdometryModel(config=cfg).to(_dev()).eval()          # a private copy: this test changes a weight
    model.load_state_dict(_model(H, W, "tanh")[0].state_dict())
    model.resnet.trunk_weights_channels_last()
    net = native_infer.NativePoseNet(model, B, H, W)
    prev, cur = _pairs(B, sensor)
    prev2, cur2 = _pairs(B, sensor, seed=77)
    assert not torch.equal(cur, cur2)
    first = net.forward(prev, cur)
    _same(first, _python_path(model, prev, cur))
    _same(net.forward(prev2, cur2), _python_path(model, prev2, cur2))
    first = tuple(t.clone() for t in net.forward(prev, cur))
    with torch.no_grad():
        model.resnet.layer2[1].conv1.weight.mul_(0.5)            # a stride-1 3x3 layer: Winograd
    moved = _python_path(model, prev, cur)
    assert not torch.equal(moved[0], first[0])
    _same(net.forward(prev, cur), first)                         # stale prepared weights: the old result, to the bit
    net.prepare()
    _same(net.forward(prev, cur), moved)


def _scans(n):
    """Raw ``[1,3,N]`` scans as the existing odometry test takes them, and the filtered clouds the engines end up with."""
    raw = [synthetic.make_pair(300 + i, rings=16, azimuth_steps=140)[i % 2][None] for i in range(n)]
    clouds = [torch.from_numpy(odometry.filter_scans(np.asarray(s, dtype=np.float32)))[:, :3].to(_dev()).float() for s in raw]
    return raw, clouds


def test_streaming_native_engine_equals_the_torch_engine():
    H, W = 16, 128
    model, cfg, sensor = _model(H, W, "tanh")
    native = odometry.ScanToScanOdometry(cfg, model=model, engine="native")
    eager = odometry.ScanToScanOdometry(cfg, model=model, engine="torch")
    raw, clouds = _scans(5)
    assert native.push(raw[0]) is None and eager.push(raw[0]) is None
    for k in range(1, 5):
        a, b = native.push(raw[k]), eager.push(raw[k])
        pair = odometry._project_pair_hip(clouds[k - 1], clouds[k], sensor)
        assert torch.equal(native.native.image_t_1, pair[0]) and torch.equal(native.native.image_t, pair[1])
        assert sorted(a) == sorted(b)
        for key in ("transformation", "T_0_t", "translation", "quaternion", "global_translation", "global_quaternion"):
            assert np.array_equal(a[key], b[key]), (k, key)


def test_demo_program_prints_the_native_engines_bits(tmp_path):
    """tools/bin/odometry_demo (no Python, no torch: hipMalloc + the C ABI) on an exported weight file and three raw scans, in a child
    process of its own: its hex ``T`` lines are the native engine's tensors."""
    H, W = 16, 128
    model, _, sensor = _model(H, W, "tanh")
    binary = os.path.join(ROOT, "tools", "bin", "odometry_demo")
    assert os.path.exists(binary), "tools/bin/odometry_demo is not built (make -C tools)"
    blob = str(tmp_path / "net.dlpose")
    native_infer.export_pose_net(model, blob, sensor)
    _, clouds = _scans(3)
    files = []
    for i, c in enumerate(clouds):
        files.append(str(tmp_path / f"scan{i}.bin"))
        c[0].contiguous().cpu().numpy().astype("<f4").tofile(files[-1])
    out = str(tmp_path / "poses.txt")
    run = subprocess.run(["timeout", "-k", "10", "120", binary, blob, out] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = open(out).read().strip().split("\n")
    assert len(lines) == 2
    engine = native_infer.NativeOdometry(model, sensor)
    assert engine.push(clouds[0][0].contiguous()) is None
    pose = np.eye(4)
    for k in (1, 2):
        T = engine.push(clouds[k][0].contiguous())[2][0].cpu().numpy()
        words = lines[k - 1].split()
        assert words[0] == str(k) and words[1] == "T" and words[18] == "pose" and len(words) == 31
        assert [int(w, 16) for w in words[2:18]] == [int(v) for v in T.reshape(-1).view(np.uint32)]
        pose = pose @ T.astype(np.float64)
        assert np.allclose([float(w) for w in words[19:]], pose[:3].reshape(-1), rtol=1e-8, atol=1e-12)
    # a weight file that is cut short is refused with a non-zero exit code
    cut = str(tmp_path / "cut.dlpose")
    open(cut, "wb").write(open(blob, "rb").read()[:-4096])
    bad = subprocess.run(["timeout", "-k", "10", "60", binary, cut, out] + files, capture_output=True, text=True)
    assert bad.returncode == 1 and "truncated" in bad.stderr
