"""Host side of dropout behind the feature tower and of the single-MLP head: argument checks and workspace queries of the new
entry points (nothing is launched: every refusal happens before a pointer is touched), and the run-time gate for CPU tensors."""
import ctypes

import torch

from tests import util

SIZES = (512, 1000, 512, 512, 256, 64)               # F, R, H1..H4 of the reference's single MLP behind the full-width network


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def test_single_head_workspace_query():
    _, lib = _lib()
    ws = lib.dl_heads_single_bwd_workspace_bytes
    for B in range(1, 17):
        b = ws(B, *SIZES)
        # the five pre-activation gradients, then the partial input gradients of the layer that needs most: Linear(1000 -> 512) has
        # ceil(512 / 40) = 13 chunks of [B][1000] (fc: 25 chunks of [B][512], which is less)
        assert b == (B * (1000 + 512 + 512 + 256 + 64) + 13 * B * 1000) * 4, (B, b)
    assert ws(3, 512, 70, 512, 512, 256, 64) > 0 and ws(1, 8, 8, 8, 8, 8, 8) > 0
    assert ws(0, *SIZES) == 0 and ws(17, *SIZES) == 0 and ws(-1, *SIZES) == 0
    for i in range(6):
        sizes = list(SIZES)
        sizes[i] = 0
        assert ws(2, *sizes) == 0, sizes


def test_single_head_entry_points_reject_null_pointers_and_bad_sizes():
    L, lib = _lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))              # host memory: never dereferenced, the checks come first
    null = ctypes.c_void_p(0)
    full, empty = L.HeadsSingleParams(), L.HeadsSingleParams()
    for l in range(6):
        full.w[l] = full.b[l] = ctypes.addressof(buf)
    fwd = lambda x, st, B=2, sizes=SIZES, act=1, acts=p: lib.dl_heads_single_fwd(x, ctypes.byref(st), B, *sizes, act, null, acts, p, p, p, p, null)   # noqa: E731
    bwd = lambda x, st, gs, B=2, sizes=SIZES, ws=p: lib.dl_heads_single_bwd(x, ctypes.byref(st), B, *sizes, 1, null, p, p, p, p, p,            # noqa: E731
                                                                            ctypes.byref(gs), p, ws, null)
    for rc in (fwd(null, full), fwd(p, empty), fwd(p, full, acts=null)):
        assert rc < 0 and b"dl_heads_single_fwd: null pointer" in lib.dl_last_error()
    assert lib.dl_heads_single_fwd(p, None, 2, *SIZES, 1, null, p, p, p, p, p, null) < 0 and b"dl_heads_single_fwd" in lib.dl_last_error()
    for rc in (bwd(null, full, full), bwd(p, empty, full), bwd(p, full, empty), bwd(p, full, full, ws=null)):
        assert rc < 0 and b"dl_heads_single_bwd: null pointer" in lib.dl_last_error()
    for kw in (dict(B=0), dict(B=17), dict(act=3), dict(sizes=(512, 0, 512, 512, 256, 64)), dict(sizes=(512, 1000, 512, 512, 256, -4))):
        assert fwd(p, full, **kw) < 0 and b"dl_heads_single_fwd: bad size" in lib.dl_last_error(), kw
    assert bwd(p, full, full, B=17) < 0 and b"dl_heads_single_bwd: bad size" in lib.dl_last_error()


def test_tower_drop_kernels_reject_bad_channel_counts_and_null_pointers():
    _, lib = _lib()
    buf = (ctypes.c_float * 16)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)
    fwd = lambda CH, pitch, y5=p, seed=p, xw=p, B=1, prob=0.2: lib.dl_tower_wide_drop_f32(y5, seed, prob, B, 2, 4, CH, pitch, xw, null)    # noqa: E731
    bwd = lambda CH, pitch, gx=p, y5=p, seed=p, g5=p, act=1: lib.dl_tower_wide_drop_bwd_f32(gx, y5, seed, 0.2, act, 1, 2, 4, CH, pitch, g5, null)  # noqa: E731
    for name, fn in ((b"dl_tower_wide_drop_f32", fwd), (b"dl_tower_wide_drop_bwd_f32", bwd)):
        for CH, pitch in ((38, 128), (42, 128), (1, 128), (0, 128), (40, 76), (68, 128), (40, 126)):       # CH % 4, 2 CH > pitch, pitch % 4
            assert fn(CH, pitch) < 0 and name + b": bad size" in lib.dl_last_error(), (CH, pitch)
    for kw in (dict(y5=null), dict(seed=null), dict(xw=null)):
        assert fwd(40, 128, **kw) < 0 and b"dl_tower_wide_drop_f32: null pointer" in lib.dl_last_error()
    for kw in (dict(gx=null), dict(y5=null), dict(seed=null), dict(g5=null)):
        assert bwd(40, 128, **kw) < 0 and b"dl_tower_wide_drop_bwd_f32: null pointer" in lib.dl_last_error()
    assert fwd(40, 128, B=0) < 0 and fwd(40, 128, prob=1.0) < 0 and b"p must lie in [0, 1)" in lib.dl_last_error()
    assert bwd(40, 128, act=3) < 0 and b"act outside" in lib.dl_last_error()
    # the 2^31-element bound of ``tower_supported``: B * H * W * pitch
    assert lib.dl_tower_wide_drop_f32(p, p, 0.2, 1 << 22, 2, 4, 40, 128, p, null) < 0 and b"2^31" in lib.dl_last_error()


def test_cpu_tensors_keep_the_module_path_with_every_switch():
    """The configurations of tests/test_tower_host.py, and the two switches this path now serves on the GPU: a CPU tensor says None."""
    from delora_amd.models.model import OdometryModel
    x = torch.zeros((1, 8, 16, 128))
    for over in (dict(), dict(factor_fewer_resnet_channels=8, resnet_outputs=64), dict(cnn_impl="modules"), dict(use_dropout=True),
                 dict(use_dropout=True, use_single_mlp_at_output=True), dict(use_single_mlp_at_output=True)):
        m = OdometryModel(util.repo_config(64, 720, pre_feature_extraction=True, **over))
        assert m.training and m.resnet.wide_path_dtype(x) is None and m.resnet.wide_path_dtype(x[:, :4], pair=True) is None
        assert not m._fused_heads_ok(x)
    assert OdometryModel(util.repo_config(64, 720)).resnet.wide_path_dtype(x) is None
    # the single MLP keeps the reference's parameter names
    names = set(OdometryModel(util.repo_config(64, 720, use_single_mlp_at_output=True)).state_dict())
    assert {f"fully_connected_rot_trans.{i}.{k}" for i in (1, 3, 5, 7, 9) for k in ("weight", "bias")} <= names
