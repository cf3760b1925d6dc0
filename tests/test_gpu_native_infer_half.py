"""The half-precision inference family on the GPU (include/delora_hip.h: dl_pose_net_*_h, dl_odometry_*_h; deploy/native_infer.py with
``dtype=``; ros_utils/odometry.py with ``precision=``; tools/odometry_demo --half) against the model's eval forward inside
``torch.autocast``, BIT FOR BIT: both enqueue the same entry points on the same operands (half precision has one kernel family, so at
every shape), and the only difference by construction -- the pooling writes half precision directly where the Python path pools in
fp32 and casts -- is pinned to the bit by tests/test_gpu_pool_half_exact.py.  No tolerance in this file except the last test, which
records how far half precision is from fp32.  Models, inputs and scans are those of tests/test_gpu_native_infer.py."""
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from delora_amd.deploy import native_infer
from delora_amd.models import model as model_module
from delora_amd.ros_utils import odometry
from tests import util
from tests.conftest import ROOT
from tests.test_gpu_native_infer import SHAPES, _dev, _model, _pairs, _same, _scans
from tests.test_gpu_odometry_records import _messages

pytestmark = pytest.mark.gpu

DTYPES = (torch.bfloat16, torch.float16)
IDS = ("bf16", "fp16")
PRECISION = {torch.bfloat16: "bfloat16", torch.float16: "float16"}


def _python_path(model, prev, cur, dtype):
    """The reference of every test: the model's own eval forward on the stacked pair inside autocast (the half-precision HIP trunk:
    ResNetModified.pooled_features_drop, half branch, + the fused heads) and the quaternion -> T kernel."""
    stacked = torch.cat((prev, cur), dim=1)
    with torch.no_grad():
        with torch.autocast("cuda", dtype=dtype):
            assert model.resnet.hip_half_applicable(stacked) == dtype and model._fused_heads_ok(stacked)
            t, q = model(stacked)
        assert t.dtype == torch.float32 and q.dtype == torch.float32
        t, q = t.float(), q.float()
        T = model.geometry_handler.get_transformation_matrix_quaternion(translation=t, quaternion=q, device=_dev())
    return t.clone(), q.clone(), T.clone()


@functools.lru_cache(maxsize=None)
def _case(B, H, W, act, dtype):
    """One (model, inputs, Python result) per shape, activation and storage type, shared by the tests below and never modified."""
    model, cfg, sensor = _model(H, W, act)
    prev, cur = _pairs(B, sensor)
    return model, sensor, prev, cur, _python_path(model, prev, cur, dtype)


# both activations at the two small single-purpose shapes, tanh elsewhere
FORWARD_CASES = [(B, H, W, act) for (B, H, W) in SHAPES for act in (("tanh", "relu") if (B, H, W) in ((1, 16, 128), (3, 5, 36)) else ("tanh",))]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H,W,act", FORWARD_CASES)
def test_forward_equals_the_python_autocast_path_bit_for_bit(B, H, W, act, dtype):
    model, _, prev, cur, want = _case(B, H, W, act, dtype)
    assert all(torch.isfinite(t).all() for t in want) and float(want[0].abs().max()) > 0
    net = native_infer.NativePoseNet(model, B, H, W, dtype=dtype)
    assert net.prepared.dtype == torch.uint8 and net.prepared.numel() == net.prepared_bytes
    _same(net.forward(prev, cur), want)
    _same(net.forward(prev, cur), want)                         # and again on the used workspace


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_strided_inputs_from_two_parent_buffers(dtype):
    """image_prev and image_cur are slices of two different larger buffers with different scan strides (6 and 9 planes per scan)."""
    B, H, W = 2, 16, 128
    model, _, prev, cur, want = _case(B, H, W, "tanh", dtype)
    pa = torch.full((B, 6, H, W), float("nan"), device=_dev())
    pb = torch.full((B, 9, H, W), float("nan"), device=_dev())
    pa[:, :4] = prev
    pb[:, 3:7] = cur
    a, b = pa[:, :4], pb[:, 3:7]
    assert a.stride(0) == 6 * H * W and b.stride(0) == 9 * H * W and not a.is_contiguous()
    _same(native_infer.NativePoseNet(model, B, H, W, dtype=dtype).forward(a, b), want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("B,H,W", ((1, 16, 128), (3, 5, 36)))
def test_poisoned_arena_guards_intact_and_nothing_read_before_written(B, H, W, dtype):
    """Workspace and prepared weights are carved out of one buffer filled with a NaN bit pattern (0xffff is a NaN in both half types,
    0xffffffff in fp32), 4 KiB guard bands around each; the outputs start as NaN.  Afterwards the guards hold their sentinel, the outputs
    are finite and equal those of a run on a zero-filled workspace (and the Python path's)."""
    model, _, prev, cur, want = _case(B, H, W, "tanh", dtype)
    probe = native_infer.NativePoseNet(model, B, H, W, dtype=dtype)
    wb, pb, G = probe.workspace_bytes, probe.prepared_bytes, 4096
    assert wb % 256 == 0 and pb % 256 == 0
    arena = torch.empty((G + wb + G + pb + G,), dtype=torch.uint8, device=_dev())
    assert arena.data_ptr() % 256 == 0
    arena.view(torch.int32).fill_(-1)
    guards = [arena[:G], arena[G + wb:2 * G + wb], arena[2 * G + wb + pb:]]
    for g in guards:
        g.fill_(0xA5)
    ws, prepared = arena[G:G + wb], arena[2 * G + wb:2 * G + wb + pb]
    out = tuple(torch.full((B,) + s, float("nan"), device=_dev()) for s in ((3,), (4,), (4, 4)))
    net = native_infer.NativePoseNet(model, B, H, W, prepared=prepared, workspace=ws, dtype=dtype)
    got = net.forward(prev, cur, out=out)
    torch.cuda.synchronize()
    assert all(bool((g == 0xA5).all()) for g in guards)
    assert all(bool(torch.isfinite(t).all()) for t in got) and got[0].data_ptr() == out[0].data_ptr()
    assert bool(torch.isfinite(prepared.view(dtype).float()).all())          # every element of the prepared buffer was written
    clean = native_infer.NativePoseNet(model, B, H, W, workspace=torch.zeros((wb,), dtype=torch.uint8, device=_dev()), dtype=dtype)
    _same(got, clean.forward(prev, cur))
    _same(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_weights_are_prepared_once_and_the_cache_is_real(dtype):
    """Two forward passes on different inputs after a SINGLE prepare each equal the Python path.  Then a trunk weight is changed in
    place WITHOUT preparing again: the native result does not move (the whole trunk runs on the copies converted before the change),
    while the Python path, which converts the weights on every forward, does; after ``prepare()`` the two agree again."""
    B, H, W = 1, 16, 128
    _, cfg, sensor = _model(H, W, "tanh")
    model = model_module.OdometryModel(config=cfg).to(_dev()).eval()          # a private copy: this test changes a weight
    model.load_state_dict(_model(H, W, "tanh")[0].state_dict())
    model.resnet.trunk_weights_channels_last()
    net = native_infer.NativePoseNet(model, B, H, W, dtype=dtype)
    prev, cur = _pairs(B, sensor)
    prev2, cur2 = _pairs(B, sensor, seed=77)
    assert not torch.equal(cur, cur2)
    _same(net.forward(prev, cur), _python_path(model, prev, cur, dtype))
    _same(net.forward(prev2, cur2), _python_path(model, prev2, cur2, dtype))
    first = tuple(t.clone() for t in net.forward(prev, cur))
    with torch.no_grad():
        model.resnet.layer3[0].conv1.weight.mul_(0.5)            # a strided layer: in fp32 it reads the raw parameter, here the copy
    moved = _python_path(model, prev, cur, dtype)
    assert not torch.equal(moved[0], first[0])
    _same(net.forward(prev, cur), first)                         # stale prepared weights: the old result, to the bit
    net.prepare()
    _same(net.forward(prev, cur), moved)


def _dicts_equal(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert sorted(a) == sorted(b), what
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_streaming_native_engine_equals_the_torch_engine(dtype):
    H, W = 16, 128
    model, cfg, sensor = _model(H, W, "tanh")
    p = PRECISION[dtype]
    native = odometry.ScanToScanOdometry(cfg, model=model, engine="native", precision=p)
    eager = odometry.ScanToScanOdometry(cfg, model=model, engine="torch", precision=p)
    assert native.native.pose.dtype == dtype
    raw, clouds = _scans(4)
    assert native.push(raw[0]) is None and eager.push(raw[0]) is None
    fp32 = odometry.ScanToScanOdometry(cfg, model=model, engine="torch")
    fp32.push(raw[0])
    for k in range(1, 4):
        a, b = native.push(raw[k]), eager.push(raw[k])
        pair = odometry._project_pair_hip(clouds[k - 1], clouds[k], sensor)
        assert torch.equal(native.native.image_t_1, pair[0]) and torch.equal(native.native.image_t, pair[1])
        _dicts_equal(a, b, f"push {k}")
        assert not np.array_equal(a["translation"], fp32.push(raw[k])["translation"])      # (it is not the fp32 network that ran)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_push_records_equals_push_on_the_host_filtered_scan(dtype):
    """KITTI-layout float32 [N,4] messages through ``push_records`` (dl_odometry_push_records_h: the filter runs inside the projection)
    against ``push`` of the same engine on the host-filtered scan."""
    H, W = 16, 128
    model, cfg, _ = _model(H, W, "tanh")
    msgs = _messages(3)
    ref = odometry.ScanToScanOdometry(cfg, model=model, engine="native", precision=PRECISION[dtype])
    node = odometry.ScanToScanOdometry(cfg, model=model, engine="native", precision=PRECISION[dtype])
    for k, m in enumerate(msgs):
        want = ref.push(np.ascontiguousarray(m.T)[None])
        assert (want is None) == (k == 0)
        _dicts_equal(node.push_records(m), want, f"message {k}")
        assert torch.equal(node.native.image_t, ref.native.image_t)
    assert node.native.count == 3 and node.native.pose.dtype == dtype


def test_demo_program_with_half_prints_the_native_engines_bits(tmp_path):
    """tools/bin/odometry_demo --half bf16 on an exported (fp32) weight file and three raw scans, in a child process of its own: its hex
    ``T`` lines are the tensors of NativeOdometry(dtype=torch.bfloat16)."""
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
    run = subprocess.run(["timeout", "-k", "10", "120", binary, "--half", "bf16", blob, out] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = open(out).read().strip().split("\n")
    assert len(lines) == 2
    engine = native_infer.NativeOdometry(model, sensor, dtype=torch.bfloat16)
    assert engine.push(clouds[0][0].contiguous()) is None
    for k in (1, 2):
        T = engine.push(clouds[k][0].contiguous())[2][0].cpu().numpy()
        words = lines[k - 1].split()
        assert words[0] == str(k) and words[1] == "T" and words[18] == "pose" and len(words) == 31
        assert [int(w, 16) for w in words[2:18]] == [int(v) for v in T.reshape(-1).view(np.uint32)]
    # an unknown storage type ends the program before anything is read
    bad = subprocess.run(["timeout", "-k", "10", "60", binary, "--half", "fp8", blob, out] + files, capture_output=True, text=True)
    assert bad.returncode == 1 and "--half" in bad.stderr


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_half_against_fp32_at_the_shipped_image_for_the_record(dtype):
    """The native half outputs against the native fp32 outputs at 64 x 720, B = 1, with the definitions and bounds of
    tests/test_gpu_convh.py::test_half_precision_network_against_the_fp32_network_at_full_size: the difference relative to the output's
    largest element, 5e-2 for bf16 and 8e-3 for fp16 (a few roundings of the storage type through 17 layers)."""
    B, H, W = 1, 64, 720
    model, _, prev, cur, _ = _case(B, H, W, "tanh", dtype)
    half = native_infer.NativePoseNet(model, B, H, W, dtype=dtype).forward(prev, cur)
    full = native_infer.NativePoseNet(model, B, H, W).forward(prev, cur)
    bound = {torch.bfloat16: 5e-2, torch.float16: 8e-3}[dtype]
    name = str(dtype)[6:]
    for what, a, b in zip(("translation", "quaternion", "T"), half, full):
        util.measured(f"native half {name} vs native fp32 @{H}x{W}: {what} (relative to its largest element)",
                      float((a - b).abs().max() / b.abs().max()), bound=bound)
