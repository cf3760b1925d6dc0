"""What the dispatch of csrc/conv.hip selects for the strided layers of the benchmark's network (batch 8, 64 x 2048 scans), asked of
``dl_conv_plan_describe`` at 256 CUs -- no GPU needed.  The chunk depth chosen for the 1x1 layers is the one they had: 16 channels
for the forward and the dense input gradient (32-channel chunks were measured slower forward and cost waves per SIMD:
profiles/direct_addr_harness.txt), 32 pixels for the weight gradient; the strided 3x3 layers keep their instantiations too.  So every
name below is also the parent's: the test pins the dispatch against a drift of the chunk depth, it does not tell two versions apart."""
import re

from delora_amd import _lib as L

F32, B = 0, 8
# (H, W, C, K, stride) of the three down-sampling blocks: conv1 is the strided 3x3, ds the 1x1 shortcut
BLOCKS = [(64, 512, 64, 128, (1, 2)), (64, 256, 128, 256, (1, 2)), (64, 128, 256, 512, (2, 2))]


def _names(op, H, W, C, K, ks, st, mode=0):
    return [re.split(r" grid=", line)[0] for line in L.conv_plan(op, F32, B, H, W, C, K, ks, st[0], st[1], mode, 256) if line]


def test_every_1x1_launch_of_the_bench_runs_the_chosen_chunk_depth():
    lines = []
    for H, W, C, K, st in BLOCKS:
        lines += _names(L.PLAN_CONV, H, W, C, K, 1, st) + _names(L.PLAN_DGRAD_STRIDED, H, W, C, K, 1, st, 1) + _names(L.PLAN_WGRAD_BATCH, H, W, C, K, 1, st)
    main = [n for n in lines if not n.startswith("k_wgrad_reduce")]
    assert len(main) == 9, lines
    for n in main:
        m = re.match(r"k_conv_f32<128, 64, (\d+), \d+, Geom\w+<1, |k_wgrad_f32_batch<64, 64, (\d+), \d, 2, 1, true>", n)
        assert m and (m.group(1) == "16" or m.group(2) == "32"), n


def test_strided_3x3_launches_of_the_bench_keep_their_instantiations():
    fwd = [_names(L.PLAN_CONV, H, W, C, K, 3, st) for H, W, C, K, st in BLOCKS]
    assert fwd == [["k_conv_f32<256, 64, 8, 128, GeomConv<3, 1, 2>, false, 1>"]] * 2 + [["k_conv_f32<128, 64, 8, 64, GeomConv<3, 2, 2>, false, 2>"]]
    dg = [_names(L.PLAN_DGRAD_STRIDED, H, W, C, K, 3, st) for H, W, C, K, st in BLOCKS]
    s12 = [f"k_conv_f32<128, 64, 8, 128, GeomDgrad<3, 1, 2, 0, {pw}, true>, true, 2>" for pw in (0, 1)]
    assert dg[0] == s12 and dg[1] == s12
    assert dg[2] == [f"k_conv_f32<128, 64, 16, 64, GeomDgrad<3, 2, 2, {ph}, {pw}, true>, true, 2>" for ph in (0, 1) for pw in (0, 1)]
    wg = [[n for n in _names(L.PLAN_WGRAD_BATCH, H, W, C, K, 3, st) if not n.startswith("k_wgrad_reduce")] for H, W, C, K, st in BLOCKS]
    assert wg == [["k_wgrad_f32_batch<64, 64, 16, 1, 2, 3, true>"]] * 2 + [["k_wgrad_f32_batch<64, 64, 16, 2, 2, 3, true>"]]
