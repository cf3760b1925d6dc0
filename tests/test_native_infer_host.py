"""Host side of the torch-free inference path (include/delora_hip.h: dl_pose_net_*, dl_odometry_*; deploy/native_infer.py): the
workspace arithmetic against a plain restatement of the plan, the refusals, and the weight file's round trip.  No GPU: the size
functions are host arithmetic, and a refused call touches none of its pointers (they are host dummies here, as in test_abi.py)."""
import ctypes

import numpy as np
import pytest
import torch

from delora_amd import _lib
from delora_amd.deploy import native_infer
from tests import util

# the reference network (src/models/resnet_modified.py: layers [2,2,2,2], strides (1,2) in layer2 / layer3 and (2,2) in layer4)
BLOCKS = ((64, 64, (1, 1), False), (64, 64, (1, 1), False), (64, 128, (1, 2), True), (128, 128, (1, 1), False),
          (128, 256, (1, 2), True), (256, 256, (1, 1), False), (256, 512, (2, 2), True), (512, 512, (1, 1), False))
F, R, HD = 512, 1000, 100
SHAPES = ((1, 16, 128), (2, 16, 128), (3, 5, 36), (1, 64, 720), (8, 64, 2048))

_keep = []


def dummy_address(_name=None, misalign=0):
    """A 256-byte aligned HOST address: good enough for every check that precedes a launch."""
    buf = (ctypes.c_char * 1024)()
    _keep.append(buf)
    return (ctypes.addressof(buf) + 255) // 256 * 256 + misalign


def make_net(blocks=BLOCKS, act=1, sizes=(F, R, HD), address=dummy_address):
    net = native_infer.fill_pose_net(_lib.PoseNet(), act, blocks, sizes, address)
    return net, ctypes.cast(ctypes.pointer(net), ctypes.c_void_p)


def up(n):
    return (n + 255) // 256 * 256


def plan_restated(lib, blocks, B, H, W, sizes=(F, R, HD)):
    """(workspace bytes, prepared bytes) by a liveness walk over the blocks: four rotating slots -- the stem's interleaved input, conv1
    output and pooled map in slots 0, 1, 2; a block with its input in slot s writes y1 to s+1, its shortcut to s+2, y2 to s+3 -- each as
    large as the largest tensor it ever holds; then the pooling's int8 window plane, the largest split-K scratch, the pooled feature and
    the heads' four saved tensors; everything rounded up to 256 bytes."""
    slots = [0, 0, 0, 0]

    def hold(s, floats):
        slots[s % 4] = max(slots[s % 4], 4 * floats)

    hold(0, B * H * W * 8)
    hold(1, B * H * (W // 2) * 64)
    hold(2, B * H * (W // 4) * 64)
    win = B * H * (W // 4) * 64
    s, h, w, split, prepared = 2, H, W // 4, 0, 0
    for (cin, cout, (sh, sw), has_ds) in blocks:
        ho, wo = -(-h // sh), -(-w // sw)
        hold(s + 1, B * ho * wo * cout)
        if has_ds:
            hold(s + 2, B * ho * wo * cout)
        hold(s + 3, B * ho * wo * cout)
        if (sh, sw) == (1, 1):
            split = max(split, lib.dl_wino_conv3x3_workspace_bytes(B, h, w, cin, cout))
            prepared += 4 * lib.dl_wino_weights_floats(cout, cin)
        split = max(split, lib.dl_wino_conv3x3_workspace_bytes(B, ho, wo, cout, cout))
        prepared += 4 * lib.dl_wino_weights_floats(cout, cout)
        s, h, w = s + 3, ho, wo
    f, r, hd = sizes
    parts = slots + [win, split, 4 * B * f, 4 * B * r, 4 * B * 2 * hd, 4 * B * 4, 4]
    return sum(up(p) for p in parts), prepared


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_workspace_and_prepared_bytes_equal_the_restated_plan(B, H, W):
    lib = _lib.load()
    _, p = make_net()
    ws, prepared = plan_restated(lib, BLOCKS, B, H, W)
    assert lib.dl_pose_net_workspace_bytes(p, B, H, W) == ws, lib.dl_last_error()
    assert lib.dl_pose_net_prepared_bytes(p, B, H, W) == prepared
    # thirteen stride-1 3x3 layers of the reference network, 16 K C floats each
    assert prepared == 4 * 16 * (4 * 64 * 64 + 128 * 128 * 3 + 256 * 256 * 3 + 512 * 512 * 3)
    assert ws % 256 == 0 and ws > 4 * B * H * (W // 2) * 64


def test_odometry_workspace_is_forward_plus_pixel_map_plus_projection_scratch():
    lib = _lib.load()
    _, p = make_net()
    from delora_amd import geometry
    sensor = geometry.Sensor(64, 720, (-0.4, 0.03), (-3.1, 3.1))
    for n in (0, 1000, 130000):
        want = lib.dl_pose_net_workspace_bytes(p, 1, 64, 720) + up(64 * 720 * 4) + up(lib.dl_project_workspace_bytes(1, 64, 720, n, 3))
        assert lib.dl_odometry_workspace_bytes(p, ctypes.byref(sensor.struct), n, 64, 720) == want
    assert lib.dl_odometry_workspace_bytes(p, ctypes.byref(sensor.struct), 1000, 64, 716) == 0 and b"sensor" in lib.dl_last_error()


def _forward(lib, p, B, H, W, workspace=None, prepared=None):
    d = dummy_address()
    return lib.dl_pose_net_forward(p, prepared if prepared is not None else d, d, 4 * H * W, d, 4 * H * W, B, H, W,
                                   workspace if workspace is not None else d, d, d, d, None)


def test_refusals_name_the_entry_point_and_the_field():
    lib = _lib.load()
    UNSUPPORTED, INVALID = -3, -1
    _, good = make_net()
    # a block with 32 channels
    narrow = list(BLOCKS)
    narrow[3] = (128, 32, (1, 1), True)
    _, p = make_net(tuple(narrow))
    assert _forward(lib, p, 1, 16, 128) == UNSUPPORTED
    assert b"dl_pose_net_forward" in lib.dl_last_error() and b"blocks[3].cout=32" in lib.dl_last_error()
    assert lib.dl_pose_net_workspace_bytes(p, 1, 16, 128) == 0 and b"dl_pose_net_workspace_bytes: blocks[3].cout=32" in lib.dl_last_error()
    assert lib.dl_pose_net_prepared_bytes(p, 1, 16, 128) == 0 and b"blocks[3].cout=32" in lib.dl_last_error()
    assert lib.dl_pose_net_prepare(p, 1, 16, 128, dummy_address(), None) == UNSUPPORTED and b"dl_pose_net_prepare" in lib.dl_last_error()
    narrow[3] = (32, 128, (1, 1), True)
    _, p = make_net(tuple(narrow))
    assert _forward(lib, p, 1, 16, 128) == UNSUPPORTED and b"blocks[3].cin=32" in lib.dl_last_error()
    # a width of 30
    assert _forward(lib, good, 1, 16, 30) == UNSUPPORTED and b"dl_pose_net_forward: W=30" in lib.dl_last_error()
    assert lib.dl_pose_net_workspace_bytes(good, 1, 16, 30) == 0 and b"W=30" in lib.dl_last_error()
    # B = 17
    assert _forward(lib, good, 17, 16, 128) == UNSUPPORTED and b"dl_pose_net_forward: B=17" in lib.dl_last_error()
    # a null weight pointer: a convolution's, the shortcut's, a head's
    for field, name in (("w2", b"blocks[5].w2 is null"), ("wd", b"blocks[4].wd is null")):
        net, p = make_net()
        setattr(net.blocks[5 if field == "w2" else 4], field, None)
        assert _forward(lib, p, 1, 16, 128) == INVALID and name in lib.dl_last_error() and b"dl_pose_net_forward" in lib.dl_last_error()
    net, p = make_net()
    net.heads.t3_w = None
    assert _forward(lib, p, 1, 16, 128) == INVALID and b"heads.t3_w is null" in lib.dl_last_error()
    net, p = make_net()
    net.conv1_w = None
    assert _forward(lib, p, 1, 16, 128) == INVALID and b"conv1_w is null" in lib.dl_last_error()
    # a misaligned workspace / prepared buffer, a weight that is not 16-byte aligned
    assert _forward(lib, good, 1, 16, 128, workspace=dummy_address(misalign=64)) == INVALID
    assert b"dl_pose_net_forward: workspace must be 256-byte aligned" in lib.dl_last_error()
    assert _forward(lib, good, 1, 16, 128, prepared=dummy_address(misalign=16)) == INVALID and b"prepared must be 256-byte aligned" in lib.dl_last_error()
    net, p = make_net()
    net.blocks[0].w1 = dummy_address(misalign=4)
    assert _forward(lib, p, 1, 16, 128) == INVALID and b"blocks[0].w1 is not 16-byte aligned" in lib.dl_last_error()
    # the rest of the scope: activation, the single shortcut rule, the feature width, a scan stride below the dense image
    _, p = make_net(act=0)
    assert _forward(lib, p, 1, 16, 128) == UNSUPPORTED and b"act=0" in lib.dl_last_error()
    odd = list(BLOCKS)
    odd[1] = (64, 64, (1, 1), True)
    _, p = make_net(tuple(odd))
    assert _forward(lib, p, 1, 16, 128) == UNSUPPORTED and b"blocks[1].has_downsample=1" in lib.dl_last_error()
    _, p = make_net(sizes=(256, R, HD))
    assert _forward(lib, p, 1, 16, 128) == UNSUPPORTED and b"F=256" in lib.dl_last_error()
    d = dummy_address()
    assert lib.dl_pose_net_forward(good, d, d, 4 * 16 * 128 - 1, d, 4 * 16 * 128, 1, 16, 128, d, d, d, d, None) == INVALID
    assert b"prev_ss" in lib.dl_last_error()
    assert lib.dl_pose_net_forward(None, d, d, 0, d, 0, 1, 16, 128, d, d, d, d, None) == INVALID and b"null net" in lib.dl_last_error()


def test_odometry_push_refusals():
    lib = _lib.load()
    from delora_amd import geometry
    _, good = make_net()
    sensor = geometry.Sensor(16, 128, (-0.4, 0.03), (-3.1, 3.1))
    d = dummy_address()
    sp = ctypes.byref(sensor.struct)
    assert lib.dl_odometry_push(good, d, sp, d, 10, 20, d, d, d, d, d, d, d, None) == -1 and b"dl_odometry_push: bad sizes n_points=20" in lib.dl_last_error()
    assert lib.dl_odometry_push(good, d, sp, d, 10, 10, None, d, d, d, d, d, d, None) == -1 and b"dl_odometry_push: null pointer" in lib.dl_last_error()
    assert lib.dl_odometry_push(good, d, sp, d, 10, 10, d, d, d, dummy_address(misalign=128), d, d, d, None) == -1 and b"workspace" in lib.dl_last_error()
    assert lib.dl_odometry_push(good, d, sp, d, 10, 10, d, d, d, d, None, d, d, None) == -1 and b"translation" in lib.dl_last_error()
    bad = geometry.Sensor(16, 30, (-0.4, 0.03), (-3.1, 3.1))
    assert lib.dl_odometry_push(good, d, ctypes.byref(bad.struct), d, 10, 10, d, d, d, d, d, d, d, None) == -3 and b"W=30" in lib.dl_last_error()


def _cpu_model(**over):
    from delora_amd.models import model as model_module
    cfg = util.repo_config(16, 128, **over)
    torch.manual_seed(3)
    return model_module.OdometryModel(config=cfg), cfg


def test_supported_mirrors_the_c_scope():
    model, _ = _cpu_model()
    assert native_infer.NativePoseNet.supported(model, 64, 720) and native_infer.NativePoseNet.supported(model, 5, 36, B=3)
    assert not native_infer.NativePoseNet.supported(model, 16, 30) and not native_infer.NativePoseNet.supported(model, 16, 128, B=17)
    for over, word in ((dict(factor_fewer_resnet_channels=2), "narrow"), (dict(use_single_mlp_at_output=True), "use_single_mlp_at_output"),
                       (dict(pre_feature_extraction=True), "pre_feature_extraction")):
        m, _ = _cpu_model(**over)
        assert word in native_infer.why_unsupported(m, 16, 128)
    # the blocks this test file writes out by hand are the model's own
    assert tuple(model.resnet._trunk_blocks()[0]) == BLOCKS


def test_native_engine_refuses_configs_outside_its_scope():
    from delora_amd.ros_utils import odometry
    for over, word in ((dict(normalization_scaling=True), "normalization_scaling"), (dict(pre_feature_extraction=True), "pre_feature_extraction"),
                       (dict(factor_fewer_resnet_channels=4), "narrow"), (dict(use_single_mlp_at_output=True), "use_single_mlp_at_output")):
        model, cfg = _cpu_model(**over)
        with pytest.raises(ValueError, match=word):
            odometry.ScanToScanOdometry(cfg, model=model, engine="native")
    model, cfg = _cpu_model()
    with pytest.raises(ValueError, match="engine"):
        odometry.ScanToScanOdometry(cfg, model=model, engine="fast")
    assert odometry.ScanToScanOdometry(cfg, model=model).native is None          # the default engine is the torch path


def test_blob_round_trip_is_bit_exact_and_bad_files_are_rejected(tmp_path):
    from delora_amd import geometry
    from delora_amd.models import ring_conv
    model, cfg = _cpu_model(activation_fct="relu")
    model.resnet.trunk_weights_channels_last()
    sensor = geometry.Sensor.from_config(cfg, "kitti")
    path = str(tmp_path / "net.dlpose")
    header = native_infer.export_pose_net(model, path, sensor)
    got_header, arrays = native_infer.load_pose_net_blob(path)
    assert got_header == header and header["activation"] == "relu" and (header["F"], header["R"], header["Hd"]) == (F, R, HD)
    assert [(b["cin"], b["cout"], tuple(b["stride"]), b["has_downsample"]) for b in header["blocks"]] == list(BLOCKS)
    assert header["sensor"] == {"H": 16, "W": 128, "hfov": list(sensor.hfov), "vfov": list(sensor.vfov)}
    assert header["data_offset"] % 256 == 0 and all(e["offset"] % 256 == 0 for e in header["arrays"].values())
    # every array, bit for bit, in the C layout
    blocks, weights = model.resnet._trunk_blocks()
    want = {"conv1_w": model.resnet.conv1.weight.detach().permute(0, 2, 3, 1)}
    wi = 0
    for i, (_, _, _, has_ds) in enumerate(blocks):
        for j, name in enumerate(("w1", "w2", "wd")[:3 if has_ds else 2]):
            want[f"blocks.{i}.{name}"] = weights[wi + j].detach().permute(0, 2, 3, 1)
        wi += 3 if has_ds else 2
    for name, t in zip(native_infer.HEAD_NAMES, native_infer._head_tensors(model)):
        want["heads." + name] = t.detach()
    assert set(arrays) == set(want) and len(want) == 1 + 19 + 10
    for name, t in want.items():
        a = t.contiguous().numpy()
        assert arrays[name].shape == a.shape and arrays[name].dtype == np.float32
        assert np.array_equal(arrays[name].view(np.uint32), a.view(np.uint32)), name
    assert arrays["conv1_w"].shape == (64, 3, 3, 8) and arrays["blocks.2.wd"].shape == (128, 1, 1, 64) and arrays["heads.r3_w"].shape == (4, HD)
    # no sensor is allowed; an unsupported model is not written
    assert native_infer.export_pose_net(model, str(tmp_path / "nosensor.dlpose"))["sensor"] is None
    with pytest.raises(ValueError, match="narrow"):
        native_infer.export_pose_net(_cpu_model(factor_fewer_resnet_channels=2)[0], str(tmp_path / "narrow.dlpose"))
    # a truncated file (inside the data, inside the header, inside the preamble) and a wrong magic / version are rejected
    raw = open(path, "rb").read()
    assert len(raw) == header["data_offset"] + header["data_bytes"]
    for cut in (len(raw) - 1, header["data_offset"] + 5, 100, 10):
        bad = str(tmp_path / f"cut{cut}.dlpose")
        open(bad, "wb").write(raw[:cut])
        with pytest.raises(ValueError, match="truncated|not a pose-network"):
            native_infer.load_pose_net_blob(bad)
    bad = str(tmp_path / "magic.dlpose")
    open(bad, "wb").write(b"DLPOSNEX" + raw[8:])
    with pytest.raises(ValueError, match="magic"):
        native_infer.load_pose_net_blob(bad)
    open(bad, "wb").write(raw[:8] + (2).to_bytes(4, "little") + raw[12:])
    with pytest.raises(ValueError, match="format version 2"):
        native_infer.load_pose_net_blob(bad)
    assert ring_conv.weight_storage(weights[0]).data_ptr() == weights[0].data_ptr()          # (the trunk's arrays were views, not copies)
