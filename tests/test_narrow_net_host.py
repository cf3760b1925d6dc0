"""Narrow pose networks (``factor_fewer_resnet_channels`` 2 and 4) on the HIP path, the parts that need no GPU: the shape tests, the
routing decision of ``ring_conv._layer_plan`` against a literal list, the refusals of the ``dl_narrow_*`` entry points (all before any
launch: the pointers are host memory and never touched), and the torch-free inference that keeps refusing such networks."""
import ctypes

import pytest
import torch

from tests import util


def _model(f, H=64, W=720, **over):
    from delora_amd.models.model import OdometryModel
    return OdometryModel(util.repo_config(H, W, factor_fewer_resnet_channels=f, **over))


def test_shape_tests_take_factor_2_and_4_and_nothing_else_new():
    from delora_amd.models import ring_conv as rc
    for f in (2, 4):
        assert _model(f).resnet.hip_path_takes(64, 720) is True
        assert _model(f).resnet.hip_path_takes(64, 722) is False                          # a width that is not a multiple of 4
        assert _model(f, cnn_impl="modules").resnet.hip_path_takes(64, 720) is False
        assert _model(f).resnet.hip_path_takes(64, 720, in_channels=rc.TOWER_CHANNELS) is False      # behind the feature tower
    assert _model(8).resnet.hip_path_takes(64, 720) is False                              # factor 8 stays the module-path specimen
    assert _model(1).resnet.hip_path_takes(64, 720) is True
    # the stem: 16 and 32 outputs for the 8-channel planar input alone
    assert rc.stem_supported((1, 8, 64, 720), 16) and rc.planar_stem_supported((1, 8, 64, 720), 32)
    assert not rc.stem_supported((1, 8, 64, 720), 8) and not rc.stem_supported((1, 8, 64, 720), 48)
    assert not rc.stem_supported((1, rc.TOWER_CHANNELS, 64, 720), 32) and not rc.stem_supported((1, 24, 64, 720), 32)
    # the half-precision trunk does not widen
    for f in (2, 4):
        blocks = _model(f).resnet._trunk_blocks()[0]
        C0 = blocks[0][0]
        assert rc.supported((1, 64, 180, C0), blocks, narrow=True) and not rc.supported_h((1, 64, 180, C0), blocks)
        assert not rc.supported((1, 64, 180, C0), blocks)                 # asked for by the 8-channel pose network alone
    # outside the narrow domain: 8 channels, a narrow layer at stride (2,2), a jump from 32 to 128
    assert not rc.supported((1, 64, 180, 8), ((8, 8, (1, 1), False),), narrow=True)
    assert not rc.supported((1, 64, 180, 32), ((32, 64, (2, 2), True),), narrow=True)
    assert not rc.supported((1, 64, 180, 32), ((32, 128, (1, 2), True),), narrow=True)


WINO, PAIR, DIRECT, NARROW = "_WinoLayer", "_PairLayer", "_DirectLayer", "_NarrowLayer"
S11, S12, S22 = (1, 1), (1, 2), (2, 2)

# (kind, cin, cout, filter, stride, down) per weight, in weight order: conv1, conv2[, downsample] of layer1.0 .. layer4.1 at (1, 64, 180, C0)
PLAN_F2 = [
    (NARROW, 32, 32, 3, S11, False), (NARROW, 32, 32, 3, S11, False), (NARROW, 32, 32, 3, S11, False), (NARROW, 32, 32, 3, S11, False),      # layer1
    (NARROW, 32, 64, 3, S12, True), (WINO, 64, 64, 3, S11, False), (NARROW, 32, 64, 1, S12, True),                                            # layer2.0
    (WINO, 64, 64, 3, S11, False), (WINO, 64, 64, 3, S11, False),                                                                             # layer2.1
    (DIRECT, 64, 128, 3, S12, True), (WINO, 128, 128, 3, S11, False), (DIRECT, 64, 128, 1, S12, True),                                        # layer3.0
    (WINO, 128, 128, 3, S11, False), (WINO, 128, 128, 3, S11, False),                                                                         # layer3.1
    (DIRECT, 128, 256, 3, S22, True), (WINO, 256, 256, 3, S11, False), (DIRECT, 128, 256, 1, S22, True),                                      # layer4.0
    (WINO, 256, 256, 3, S11, False), (WINO, 256, 256, 3, S11, False),                                                                         # layer4.1
]
PLAN_F4 = [
    (NARROW, 16, 16, 3, S11, False), (NARROW, 16, 16, 3, S11, False), (NARROW, 16, 16, 3, S11, False), (NARROW, 16, 16, 3, S11, False),      # layer1
    (NARROW, 16, 32, 3, S12, True), (NARROW, 32, 32, 3, S11, False), (NARROW, 16, 32, 1, S12, True),                                          # layer2.0
    (NARROW, 32, 32, 3, S11, False), (NARROW, 32, 32, 3, S11, False),                                                                         # layer2.1
    (NARROW, 32, 64, 3, S12, True), (WINO, 64, 64, 3, S11, False), (NARROW, 32, 64, 1, S12, True),                                            # layer3.0
    (WINO, 64, 64, 3, S11, False), (WINO, 64, 64, 3, S11, False),                                                                             # layer3.1
    (DIRECT, 64, 128, 3, S22, True), (WINO, 128, 128, 3, S11, False), (DIRECT, 64, 128, 1, S22, True),                                        # layer4.0
    (WINO, 128, 128, 3, S11, False), (WINO, 128, 128, 3, S11, False),                                                                         # layer4.1
]
# the full-width network, as the parent commit routes it at this shape (batch 1: the pixel-pair kernel does not take layer2.0 / layer3.0)
PLAN_F1 = [
    (WINO, 64, 64, 3, S11, False), (WINO, 64, 64, 3, S11, False), (WINO, 64, 64, 3, S11, False), (WINO, 64, 64, 3, S11, False),
    (DIRECT, 64, 128, 3, S12, True), (WINO, 128, 128, 3, S11, False), (DIRECT, 64, 128, 1, S12, True),
    (WINO, 128, 128, 3, S11, False), (WINO, 128, 128, 3, S11, False),
    (DIRECT, 128, 256, 3, S12, True), (WINO, 256, 256, 3, S11, False), (DIRECT, 128, 256, 1, S12, True),
    (WINO, 256, 256, 3, S11, False), (WINO, 256, 256, 3, S11, False),
    (DIRECT, 256, 512, 3, S22, True), (WINO, 512, 512, 3, S11, False), (DIRECT, 256, 512, 1, S22, True),
    (WINO, 512, 512, 3, S11, False), (WINO, 512, 512, 3, S11, False),
]


@pytest.mark.parametrize("f,want", [(2, PLAN_F2), (4, PLAN_F4), (1, PLAN_F1)], ids=["factor2", "factor4", "factor1"])
def test_layer_plan_names_the_narrow_kind_exactly_where_the_channels_are_narrow(f, want):
    from delora_amd.models import ring_conv as rc
    blocks = _model(f).resnet._trunk_blocks()[0]
    plan = rc._layer_plan((1, 64, 180, blocks[0][0]), blocks, torch.float32)
    got = [(kind.__name__, cin, cout, ks, tuple(stride), bool(down)) for (kind, cin, cout, ks, stride, down) in plan]
    assert got == want
    # half precision has one family, narrow channel counts or not
    assert {kind.__name__ for (kind, *_) in rc._layer_plan((1, 64, 180, blocks[0][0]), blocks, torch.bfloat16)} == {"_HalfLayer"}


def test_entry_points_refuse_before_any_launch_and_name_the_argument():
    from delora_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))               # host memory: a refused call never touches it
    null = ctypes.c_void_p(0)
    N, H, W = 1, 3, 20
    UNSUPPORTED, INVALID = -3, -1

    def conv(C=16, K=16, ks=3, sh=1, sw=2, x=p, add=null, dsrc=null, transposed=0, act=0, epi=0):
        return lib.dl_narrow_conv2d_nhwc_f32(x, p, p, add, dsrc, N, H, W, C, K, ks, sh, sw, transposed, act, epi, null)

    def dgrad(C=16, K=16, ks=3, sh=1, sw=2, g=p, add=null, dsrc=null, dense=0, act=0, epi=0):
        return lib.dl_narrow_dgrad_strided_nhwc_f32(g, p, p, add, dsrc, N, H, W, K, C, ks, sh, sw, dense, act, epi, null)

    def wgrad(C=16, K=16, ks=3, sh=1, sw=2, x=p, ws=p):
        return lib.dl_narrow_wgrad_nhwc_f32(x, p, p, ws, N, H, W, C, K, ks, sh, sw, null)

    def wbytes(C=16, K=16, ks=3, sh=1, sw=2):
        return lib.dl_narrow_wgrad_workspace_bytes(N, H, W, C, K, ks, sh, sw)

    def refused(rc, code, who, word):
        err = lib.dl_last_error()
        assert rc == code, (rc, code, err)
        assert who.encode() in err and word.encode() in err, err

    names = {conv: "dl_narrow_conv2d_nhwc_f32", dgrad: "dl_narrow_dgrad_strided_nhwc_f32", wgrad: "dl_narrow_wgrad_nhwc_f32"}
    assert wbytes() > 0
    for over, word in ((dict(C=6), "C=6"), (dict(K=12), "K=12"), (dict(C=68), "C=68"), (dict(K=72), "K=72"), (dict(sh=2, sw=2), "stride (2,2)"),
                       (dict(sh=2, sw=1), "stride (2,1)"), (dict(ks=5), "ksize=5")):
        for fn, who in names.items():
            refused(fn(**over), UNSUPPORTED, who, word)
        assert wbytes(**over) == 0
    # null pointers
    refused(conv(x=null), INVALID, names[conv], "null")
    refused(dgrad(g=null), INVALID, names[dgrad], "null")
    refused(wgrad(x=null), INVALID, names[wgrad], "null")
    refused(wgrad(ws=null), INVALID, names[wgrad], "null")
    # epilogue: an unknown flag (ADD_GRID belongs to the strided input gradient, ADD and ACT do not), a flag without its operand, a bad act
    refused(conv(epi=8), INVALID, names[conv], "epilogue")
    refused(conv(epi=16), INVALID, names[conv], "epilogue")
    refused(dgrad(epi=1), INVALID, names[dgrad], "epilogue")
    refused(conv(epi=1), INVALID, names[conv], "DL_CONV_ADD without add")
    refused(conv(epi=4, act=1), INVALID, names[conv], "DL_CONV_DACT without dsrc")
    refused(dgrad(epi=8), INVALID, names[dgrad], "DL_CONV_ADD_GRID without add_grid")
    refused(conv(act=3), INVALID, names[conv], "act=3")
    # the transposed form is stride 1; the strided input gradient is stride (1,2); dense is the 1x1 layer's
    refused(conv(transposed=1), UNSUPPORTED, names[conv], "transposed")
    refused(dgrad(sw=1), UNSUPPORTED, names[dgrad], "stride (1,1)")
    refused(dgrad(dense=1), UNSUPPORTED, names[dgrad], "dense")


def test_torch_free_inference_still_refuses_narrow_networks():
    from delora_amd.deploy import native_infer
    for f in (2, 4):
        assert "narrow" in native_infer.why_unsupported(_model(f, 16, 128), 16, 128)
