"""Host side of the half-precision inference family (include/delora_hip.h: dl_pose_net_*_h, dl_odometry_*_h; deploy/native_infer.py,
ros_utils/odometry.py): the size arithmetic written out by hand, and the refusals -- the fp32 family's, with the same words, plus the
storage type's.  No GPU: the size functions are host arithmetic, and a refused call touches none of its pointers (host dummies here,
as in tests/test_native_infer_host.py, whose network and helpers this file uses)."""
import ctypes

import pytest
import torch

from delora_amd import _lib, geometry
from delora_amd.deploy import native_infer
from delora_amd.ros_utils import odometry
from tests.test_native_infer_host import BLOCKS, F, HD, R, _cpu_model, dummy_address, make_net, plan_restated, up

UNSUPPORTED, INVALID = -3, -1
F16, BF16 = 1, 2
SHAPES = ((1, 16, 128), (2, 16, 128), (3, 5, 36), (1, 64, 720), (8, 64, 2048))
# the reference network and four others that leave the slot rotation at every phase: one block, an end on a strided block, five blocks
# (the rotation past a full turn), a strided first block
BLOCK_LISTS = (BLOCKS, BLOCKS[:1], BLOCKS[:3], BLOCKS[:5], ((64, 128, (2, 2), True), (128, 128, (1, 1), False)))


def prepared_restated_h(blocks):
    """Every trunk convolution as w_fwd [taps][K][C] in 2-byte elements, each array rounded up to 256 bytes."""
    return sum(up(9 * cout * cin * 2) + up(9 * cout * cout * 2) + (up(1 * cout * cin * 2) if has_ds else 0) for (cin, cout, _, has_ds) in blocks)


def plan_restated_h(blocks, B, H, W, sizes=(F, R, HD)):
    """Workspace bytes of the half-precision family: the liveness walk of ``plan_restated`` (tests/test_native_infer_host.py) with the
    interleaved input and conv1's output (slots 0 and 1) in 4-byte elements, the pooled map and every block tensor in 2-byte elements, no
    window plane and no split-K scratch; then the fp32 pooled feature and the heads' four saved tensors; every part rounded up to 256."""
    slots = [0, 0, 0, 0]

    def hold(s, nbytes):
        slots[s % 4] = max(slots[s % 4], nbytes)

    hold(0, 4 * B * H * W * 8)
    hold(1, 4 * B * H * (W // 2) * 64)
    hold(2, 2 * B * H * (W // 4) * 64)
    s, h, w = 2, H, W // 4
    for (cin, cout, (sh, sw), has_ds) in blocks:
        ho, wo = -(-h // sh), -(-w // sw)
        hold(s + 1, 2 * B * ho * wo * cout)
        if has_ds:
            hold(s + 2, 2 * B * ho * wo * cout)
        hold(s + 3, 2 * B * ho * wo * cout)
        s, h, w = s + 3, ho, wo
    f, r, hd = sizes
    return sum(up(p) for p in slots + [4 * B * f, 4 * B * r, 4 * B * 2 * hd, 4 * B * 4, 4])


def test_abi_version_is_unchanged():
    assert _lib.load().dl_abi_version() == 10 and _lib.ABI_VERSION == 10


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_prepared_bytes_are_the_trunks_forward_weights_in_half_precision(B, H, W, dtype):
    """Every trunk convolution as w_fwd [taps][K][C] in 2-byte elements, each array rounded up to 256 bytes: 3x3 conv1 and conv2 of every
    block, the 1x1 shortcut of the three strided ones.  The image size does not enter."""
    lib = _lib.load()
    _, p = make_net()
    want = prepared_restated_h(BLOCKS)
    assert lib.dl_pose_net_prepared_bytes_h(p, B, H, W, dtype) == want, lib.dl_last_error()
    # by hand for the reference network: sixteen 3x3 layers and three 1x1 shortcuts, all multiples of 256 bytes already
    by_hand = 2 * (9 * (4 * 64 * 64 + 128 * 64 + 3 * 128 * 128 + 256 * 128 + 3 * 256 * 256 + 512 * 256 + 3 * 512 * 512)
                   + 128 * 64 + 256 * 128 + 512 * 256)
    assert want == by_hand


@pytest.mark.parametrize("dtype", (F16, BF16))
def test_workspace_is_smaller_than_the_fp32_one(dtype):
    lib = _lib.load()
    _, p = make_net()
    for (B, H, W) in SHAPES:
        ws = lib.dl_pose_net_workspace_bytes_h(p, B, H, W, dtype)
        assert ws > 0 and ws % 256 == 0, lib.dl_last_error()
        assert ws < lib.dl_pose_net_workspace_bytes(p, B, H, W)
        assert ws > 4 * B * H * (W // 2) * 64                        # conv1's fp32 output lives in it
    sensor = geometry.Sensor(64, 720, (-0.4, 0.03), (-3.1, 3.1))
    for n in (0, 1000):
        want = lib.dl_pose_net_workspace_bytes_h(p, 1, 64, 720, dtype) + up(64 * 720 * 4) + up(lib.dl_project_workspace_bytes(1, 64, 720, n, 3))
        assert lib.dl_odometry_workspace_bytes_h(p, ctypes.byref(sensor.struct), n, 64, 720, dtype) == want


@pytest.mark.parametrize("dtype", (F16, BF16))
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_workspace_equals_the_restated_half_plan(B, H, W, dtype):
    lib = _lib.load()
    _, p = make_net()
    assert lib.dl_pose_net_workspace_bytes_h(p, B, H, W, dtype) == plan_restated_h(BLOCKS, B, H, W), lib.dl_last_error()


@pytest.mark.parametrize("blocks", BLOCK_LISTS[1:], ids=("one", "three", "five", "strided_first"))
def test_other_block_lists_equal_the_restated_plans_in_both_families(blocks):
    """Shorter networks (F = the last block's channels) start and end the slot rotation at other phases: both workspace restatements,
    the fp32 prepared bytes and the half prepared bytes, at every shape and in both storage types."""
    lib = _lib.load()
    sizes = (blocks[-1][1], R, HD)
    _, p = make_net(blocks, sizes=sizes)
    for (B, H, W) in SHAPES:
        ws, prepared = plan_restated(lib, blocks, B, H, W, sizes)
        assert lib.dl_pose_net_workspace_bytes(p, B, H, W) == ws, lib.dl_last_error()
        assert lib.dl_pose_net_prepared_bytes(p, B, H, W) == prepared, lib.dl_last_error()
        for dtype in (F16, BF16):
            assert lib.dl_pose_net_workspace_bytes_h(p, B, H, W, dtype) == plan_restated_h(blocks, B, H, W, sizes), lib.dl_last_error()
            assert lib.dl_pose_net_prepared_bytes_h(p, B, H, W, dtype) == prepared_restated_h(blocks), lib.dl_last_error()


def _calls(lib, p, dtype, B=1, H=16, W=128, prepared=None, workspace=None, sensor=None):
    """name -> a call of every *_h entry point on net ``p`` with dummy addresses (size functions return 0 when they refuse)."""
    d = dummy_address()
    prepared = d if prepared is None else prepared
    workspace = d if workspace is None else workspace
    sensor = geometry.Sensor(H, W, (-0.4, 0.03), (-3.1, 3.1)) if sensor is None else sensor
    sp = ctypes.byref(sensor.struct)
    layout = ctypes.byref(odometry.record_layout(16, (0, 4, 8)))
    return {
        "dl_pose_net_prepared_bytes_h": lambda: lib.dl_pose_net_prepared_bytes_h(p, B, H, W, dtype),
        "dl_pose_net_workspace_bytes_h": lambda: lib.dl_pose_net_workspace_bytes_h(p, B, H, W, dtype),
        "dl_pose_net_prepare_h": lambda: lib.dl_pose_net_prepare_h(p, B, H, W, dtype, prepared, None),
        "dl_pose_net_forward_h": lambda: lib.dl_pose_net_forward_h(p, prepared, d, 4 * H * W, d, 4 * H * W, B, H, W, dtype, workspace, d, d, d, None),
        "dl_odometry_workspace_bytes_h": lambda: lib.dl_odometry_workspace_bytes_h(p, sp, 100, sensor.H, sensor.W, dtype),
        "dl_odometry_push_h": lambda: lib.dl_odometry_push_h(p, prepared, sp, d, 10, 10, d, d, d, dtype, workspace, d, d, d, None),
        "dl_odometry_push_records_h": lambda: lib.dl_odometry_push_records_h(p, prepared, sp, d, 10, layout, d, d, d, dtype, workspace, d, d, d, None),
    }


SIZE_FUNCTIONS = ("dl_pose_net_prepared_bytes_h", "dl_pose_net_workspace_bytes_h", "dl_odometry_workspace_bytes_h")


def _refused(lib, name, call, code, *words):
    got = call()
    assert got == (0 if name in SIZE_FUNCTIONS else code), (name, got, lib.dl_last_error())
    text = lib.dl_last_error()
    assert name.encode() + b":" in text, (name, text)
    for w in words:
        assert w in text, (name, w, text)


def test_every_entry_point_refuses_other_storage_types_and_a_null_net():
    lib = _lib.load()
    _, good = make_net()
    for dtype in (0, 3):
        for name, call in _calls(lib, good, dtype).items():
            _refused(lib, name, call, UNSUPPORTED, f"dtype={dtype}".encode())
    for name, call in _calls(lib, None, BF16).items():
        _refused(lib, name, call, INVALID, b"null net")


def test_misaligned_buffers_and_a_width_of_30():
    lib = _lib.load()
    _, good = make_net()
    for dtype in (F16, BF16):
        calls = _calls(lib, good, dtype, prepared=dummy_address(misalign=16))
        for name in ("dl_pose_net_prepare_h", "dl_pose_net_forward_h", "dl_odometry_push_h", "dl_odometry_push_records_h"):
            _refused(lib, name, calls[name], INVALID, b"prepared must be")
        calls = _calls(lib, good, dtype, workspace=dummy_address(misalign=64))
        for name in ("dl_pose_net_forward_h", "dl_odometry_push_h", "dl_odometry_push_records_h"):
            _refused(lib, name, calls[name], INVALID, b"workspace must be 256-byte aligned")
        bad = geometry.Sensor(16, 30, (-0.4, 0.03), (-3.1, 3.1))
        for name, call in _calls(lib, good, dtype, W=30, sensor=bad).items():
            _refused(lib, name, call, UNSUPPORTED, b"W=30")


def _fp32_text(lib, p):
    d = dummy_address()
    assert lib.dl_pose_net_forward(p, d, d, 4 * 16 * 128, d, 4 * 16 * 128, 1, 16, 128, d, d, d, d, None) == UNSUPPORTED
    return lib.dl_last_error().split(b": ", 1)[1]


def test_networks_outside_the_scope_are_refused_with_the_fp32_familys_words():
    """A narrow block (either side), a 1x1 shortcut on a stride-1 block (what a feature tower's or any other foreign trunk looks like to
    the struct), heads of another width: the text behind the entry point's name is the fp32 family's, character for character."""
    lib = _lib.load()
    cases = []
    narrow = list(BLOCKS)
    narrow[3] = (128, 32, (1, 1), True)
    cases.append((make_net(tuple(narrow)), b"blocks[3].cout=32"))
    narrow[3] = (32, 128, (1, 1), True)
    cases.append((make_net(tuple(narrow)), b"blocks[3].cin=32"))
    odd = list(BLOCKS)
    odd[1] = (64, 64, (1, 1), True)
    cases.append((make_net(tuple(odd)), b"blocks[1].has_downsample=1"))
    cases.append((make_net(sizes=(256, R, HD)), b"F=256"))
    cases.append((make_net(act=0), b"act=0"))
    for (net, p), word in cases:
        want = _fp32_text(lib, p)
        assert word in want
        for dtype in (F16, BF16):
            for name, call in _calls(lib, p, dtype).items():
                _refused(lib, name, call, UNSUPPORTED, word)
                assert lib.dl_last_error() == name.encode() + b": " + want


def test_python_wrappers_refuse_what_the_fp32_wrappers_refuse_and_unknown_precisions():
    model, cfg = _cpu_model()
    with pytest.raises(ValueError, match="float64"):
        native_infer.NativePoseNet(model, 1, 16, 128, dtype=torch.float64)
    with pytest.raises(ValueError, match="int8"):
        odometry.ScanToScanOdometry(cfg, model=model, precision="int8")
    with pytest.raises(ValueError, match="int8"):
        odometry.ScanToScanOdometry(cfg, model=model, engine="native", precision="int8")
    for over, word in ((dict(normalization_scaling=True), "normalization_scaling"), (dict(pre_feature_extraction=True), "pre_feature_extraction"),
                       (dict(factor_fewer_resnet_channels=4), "narrow"), (dict(use_single_mlp_at_output=True), "use_single_mlp_at_output")):
        m, c = _cpu_model(**over)
        for precision in ("bfloat16", "float16"):
            with pytest.raises(ValueError, match=word):
                odometry.ScanToScanOdometry(c, model=m, engine="native", precision=precision)
        if word != "normalization_scaling":
            with pytest.raises(ValueError, match=word):
                native_infer.NativePoseNet(m, 1, 16, 128, dtype=torch.bfloat16)
    # the training config's amp_dtype is deliberately not read: the default stays fp32
    node = odometry.ScanToScanOdometry(dict(cfg, amp_dtype="bfloat16"), model=model)
    assert node.precision == "float32" and node.dtype == torch.float32 and node.native is None
    assert odometry.ScanToScanOdometry(cfg, model=model, precision="bfloat16").dtype == torch.bfloat16
