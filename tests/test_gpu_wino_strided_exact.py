"""The pixel-pair Winograd form of the stride-(1,2) 3x3 layers (csrc/wino.hip: k_wino_conv_strided) BIT FOR BIT against the float64
reference and against the direct entry points, on small-integer data in poisoned arenas (the method of tests/test_gpu_conv_exact.py).

Exactness is by construction: the rearranged kernel holds the layer's own integer weights and zeros, so U = G g G^T lives on the grid
1/4, V = B^T d B holds integers, every channel sum stays below 2^23 grid steps (``conv_ref.headroom`` asserts it for the pair view's 2C
reduction channels -- an upper bound: half of them carry one tap column instead of two), and the planes the kernel leaves out are exact
zeros.  tanh is the same ``dl_tanh`` on the same value in both paths, so a forward pass with tanh must equal the direct kernel's bit
for bit although neither equals float64.

Shapes are given as the pair view H' x W' the kernel tiles (the layer's image is H' x 2W'):
  4x64   one 2x32 tile group, wrapping onto itself        8x32   one 4x16 group
  4x128  two groups across the wrap                       8x64   two 4x16 groups side by side, zero rows at the image edge only
with 64 -> 128 and 128 -> 64 channels: the boundary between the even- and the odd-pixel channels then falls inside a workgroup's
chunk range, and the input gradient has one and two 64-channel output blocks per pixel phase (only the even-pixel blocks add the
down-sampling branch's gradient).  Stride (2,2) is not built: layer4.0 stays on the direct kernel.
"""
import numpy as np
import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util
from tests.test_gpu_conv_exact import ACT, ADD_GRID, DACT, RELU, TANH, Run, _dev, _guarded, _p, _stream

pytestmark = pytest.mark.gpu

XMAX, WMAX = 4, 3
VIEWS = [(4, 64), (8, 32), (4, 128), (8, 64)]
CHANNELS = [(64, 128), (128, 64)]
CASES = [cc.Case(2, h, 2 * w, c, k, 3, (1, 2), xmax=XMAX, wmax=WMAX) for (h, w) in VIEWS for (c, k) in CHANNELS]
FWD = [(0, 0), (ACT, RELU), (ACT, TANH)]
BWD = [(0, 0, None), (ADD_GRID, 0, None), (ADD_GRID | DACT, TANH, "tanh"), (ADD_GRID | DACT, RELU, "relu")]


def _strided_weights(r):
    c = r.c
    n = int(r.lib.dl_wino_strided_weights_floats(c.K, c.C, 1, 2))
    assert n == 16 * c.K * 2 * c.C
    uf, ub = r.out((n,), torch.float32, "u_fwd", 0), r.out((n,), torch.float32, "u_bwd", 0)
    r.ok(r.lib.dl_wino_strided_weights_f32(_p(r.w_d), _p(uf), _p(ub), c.K, c.C, 1, 2, _stream()), "dl_wino_strided_weights_f32")
    torch.cuda.synchronize()
    r.A.check(f"{c.id} weight preparation")
    for t in (uf, ub):
        r.A.check_output(t, f"{c.id} weight preparation")
        r.A.freeze(t)
    return uf, ub


def strided_groups(N, h, w, out_channels):
    """Tile groups of one k_wino_conv_strided launch on the pair view h x w: wn_strided_tiles / wn_strided_launch of csrc/wino.hip
    restated (no plan query describes these launches).  ``out_channels`` is K forward and 2C for the input gradient."""
    th, tw = h // 2, w // 2
    tc = 32 if (tw % 32 == 0 and th % 2 == 0) else 16
    tr = 64 // tc
    assert th % tr == 0 and tw % tc == 0 and out_channels % 64 == 0
    return N * (th // tr) * (tw // tc) * (out_channels // 64)


def run_strided(case, dev, skew=0, cap=None, below_two_rounds=True, block_must_change=False):
    """Forward and / or input gradient (``case.passes``) of one case.  ``cap``: the device's CU count -- every launch must then have
    more tile groups than that (several groups per workgroup) and, with ``below_two_rounds``, fewer than twice as many; with
    ``block_must_change`` some workgroup's consecutive groups must differ in their output block (forward) or lie on different
    sides of the even- / odd-pixel boundary k0 < K/2 (input gradient: ``grid_block`` changes), by the restated swizzle."""
    r = Run(case, dev, skew)
    c, lib = case, r.lib
    # the pair view's sums: 2C reduction channels forward, K backward, the grid operand (<= 3) and tanh' on top
    cr.headroom("wino_conv", 2 * c.C, c.xmax, c.wmax, add=3, dact_tanh=True)
    cr.headroom("wino_conv", c.K, c.xmax, c.wmax, add=3, dact_tanh=True)
    assert lib.dl_wino_strided_takes(c.N, c.H, c.W, c.C, c.K, 1, 2, 1 if cap is None else 0) == 1, "the case must be one the dispatch can take"
    if cap is not None:
        for what, outc in (("forward", c.K), ("dgrad", 2 * c.C)):
            if what in c.passes:
                groups = strided_groups(c.N, c.H, c.W // 2, outc)
                handovers, block, phase = cc.block_changes(groups, min(cap, groups), outc // 64)
                print(f"[persistent] {c.id} {what}: groups {groups}, grid {min(cap, groups)} ({cap} CUs); of {handovers} hand-overs {block} go to "
                      f"another channel block, {phase} across the even- / odd-pixel boundary")
                assert cap < groups and (groups < 2 * cap or not below_two_rounds), f"{c.id} {what}: {groups} groups on {cap} CUs is not the launch this test is about"
                assert not block_must_change or (block if what == "forward" else phase) > 0, f"{c.id} {what}: every workgroup keeps its channel block"
    uf, ub = _strided_weights(r)
    yshape, xshape = tuple(r.y0.shape), tuple(r.x.shape)
    for flags, act in (FWD if "forward" in c.passes else []):
        y_new, y_dir = r.out(yshape, name="y (pixel-pair Winograd)"), r.out(yshape, name="y (direct)")
        r.ok(lib.dl_wino_strided_conv3x3_nhwc_f32(_p(r.x_d), _p(uf), _p(y_new), c.N, c.H, c.W, c.C, c.K, 1, 2, act, flags, _stream()),
             "dl_wino_strided_conv3x3_nhwc_f32")
        r.ok(lib.dl_conv2d_nhwc_f32(_p(r.x_d), _p(r.w_d), _p(y_dir), None, None, c.N, c.H, c.W, c.C, c.K, 3, 1, 2, 0, act, flags, _stream()),
             "dl_conv2d_nhwc_f32")
        what = f"forward, tail {flags}/{act}"
        if act == TANH:                                  # not exact against float64; the two kernels must still agree to the bit
            torch.cuda.synchronize()
            r.A.check(f"{c.id} {what}")
            r.A.check_output(y_new, f"{c.id} {what}")
            r.A.check_output(y_dir, f"{c.id} {what}")
        else:
            ref = cr.epilogue(r.y0, flags, act)
            r.compare(y_new, ref, "pixel-pair Winograd " + what)
            r.compare(y_dir, ref, "direct " + what, (8, 64))
        r.bad += cr.mismatches(y_new, y_dir.detach().cpu(), f"{c.id} pixel-pair Winograd against direct, {what}")
    gshape = (c.N, c.Ho, c.Wo, c.C)
    for i, (flags, act, kind) in enumerate(BWD if c.dgrad_ok else []):
        _, sv, _, sv_d = r.tail_operands(xshape, flags, kind, 50 + 2 * i)
        addg = cr.ints(gshape, 3, c.seed(60 + i)) if flags & ADD_GRID else None
        addg_d = r.A.arena(gshape, r.dt, addg, "add_grid") if addg is not None else None
        ref = cr.epilogue(r.dx0, flags, act, None, sv, addg, c.stride)
        dx_new, dx_dir = r.out(xshape, name="dx (pixel-pair Winograd)"), r.out(xshape, name="dx (direct)")
        r.ok(lib.dl_wino_strided_dgrad3x3_nhwc_f32(_p(r.g_d), _p(ub), _p(dx_new), _p(addg_d), _p(sv_d), c.N, c.H, c.W, c.K, c.C, 1, 2, act, flags,
                                                   _stream()), "dl_wino_strided_dgrad3x3_nhwc_f32")
        r.ok(lib.dl_conv2d_dgrad_strided_nhwc_f32(_p(r.g_d), _p(r.w_d), _p(dx_dir), _p(addg_d), _p(sv_d), c.N, c.H, c.W, c.K, c.C, 3, 1, 2, 0, act,
                                                  flags, None, _stream()), "dl_conv2d_dgrad_strided_nhwc_f32")
        what = f"input gradient, tail {flags}/{act}"
        r.compare(dx_new, ref, "pixel-pair Winograd " + what)
        r.compare(dx_dir, ref, "direct " + what, (8, 64))
        assert torch.equal(dx_new, dx_dir), f"{c.id}: the two input gradients differ from each other ({what})"
    return r.bad


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_pixel_pair_winograd_equals_float64_and_the_direct_kernel(case):
    dev = _dev()
    bad = _guarded(run_strided, case, dev)
    util.measured(f"strided Winograd exact {case.id}: elements that differ", bad, bound=0)


# More tile groups than CUs (the persistent loop of csrc/wino_conv_body.h, as tests/test_gpu_wino_persistent_exact.py runs it for the
# stride-1 kernels): pair views 12x64 (2x32 groups) and 24x32 (4x16 groups) have three groups per image and 64-channel block.  The
# batch is the smallest that gives a pass more groups than the device has CUs; 64 -> 128 has six groups per image in both passes,
# 128 -> 64 three forward and twelve (2C = 256 output channels) in the input gradient, hence a case per pass.  The ADD_GRID | DACT
# tails read their operand offsets after the next group's set-up has run.
# The batch must be one ``dl_wino_strided_takes`` accepts, as the trunk asks before it uses these kernels: it refuses a layer either
# of whose passes the stride-1 dispatch would split.  The forward pass of 128 -> 64 (32 chunks, three groups per image) is split
# until 6 N exceeds the CU count, so its input gradient cannot run below 12 * (cu / 6) -- two rounds of the CUs: that ONE case
# (``raised``) has a few workgroups with three groups and the rest with two; every other case runs at the smallest batch.
# A workgroup steps through the groups by grid / 8 positions (wn_xcd_swizzle), 32 on 256 CUs, and the channel block is the fastest
# index: with 2 or 4 output blocks every group of a workgroup then has the SAME k0 and the same ``grid_block``.  The cases of
# ``test_..._changes_the_channel_block`` take 192 channels (3 blocks forward, 6 in the input gradient, or the next count that does
# not divide the step): there k0 changes from a workgroup's group to its next, and in the input gradient it crosses k0 < K/2 --
# ``grid_block`` (only the even-pixel blocks add the grid operand) differs between the group whose epilogue runs and the one
# whose set-up has just run.  The tests print the counts and assert them from the restated swizzle.
SEVERAL = [(view, ch, passes, raised) for view in ((12, 64), (24, 32))
           for ch, passes, raised in (((64, 128), ("forward", "dgrad"), False), ((128, 64), ("forward",), False), ((128, 64), ("dgrad",), True))]


def _smallest_batch(lib, cap, view, channels, passes):
    """(smallest batch that gives the passes more groups than CUs, that batch raised until the dispatch takes the layer)."""
    (h, w), (c, k) = view, channels
    per_image = max(strided_groups(1, h, w, k) if "forward" in passes else 0, strided_groups(1, h, w, 2 * c) if "dgrad" in passes else 0)
    first = N = cap // per_image + 1
    while lib.dl_wino_strided_takes(N, h, 2 * w, c, k, 1, 2, 0) != 1 and N < 8 * first:
        N += 1
    return first, N


@pytest.mark.parametrize("view,channels,passes,raised", SEVERAL, ids=[f"{v[0]}x{v[1]}-c{ch[0]}-k{ch[1]}-{'+'.join(p)}" for v, ch, p, _ in SEVERAL])
def test_pixel_pair_winograd_with_several_groups_per_workgroup(view, channels, passes, raised):
    from delora_amd import _lib
    dev = _dev()
    cap = torch.cuda.get_device_properties(dev).multi_processor_count
    first, N = _smallest_batch(_lib.load(), cap, view, channels, passes)
    assert raised or N == first, f"the dispatch takes this layer only from batch {N} on ({first} gives more groups than CUs)"
    case = cc.Case(N, view[0], 2 * view[1], channels[0], channels[1], 3, (1, 2), xmax=XMAX, wmax=WMAX, passes=passes)
    bad = _guarded(run_strided, case, dev, 0, cap, not raised)
    util.measured(f"strided Winograd exact {case.id}, {' and '.join(passes)}, more groups than CUs: elements that differ", bad, bound=0)


@pytest.mark.parametrize("which", ["forward", "dgrad"])
@pytest.mark.parametrize("view", [(12, 64), (24, 32)], ids=["12x64", "24x32"])
def test_pixel_pair_hand_over_changes_the_channel_block(view, which):
    """64 -> ch forward (ch / 64 output blocks) and ch -> ch input gradient (2 ch / 64 blocks, the even-pixel half adds the grid
    operand) with ch = 192, or the next count for which, on this device's CU count, a workgroup's consecutive groups differ in their
    block -- in the input gradient: lie on different sides of k0 < K/2.  Between one and two rounds of the CUs, at the smallest batch."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    cap = torch.cuda.get_device_properties(dev).multi_processor_count
    for ch in (192, 320, 448):
        channels = (64, ch) if which == "forward" else (ch, ch)
        first, N = _smallest_batch(lib, cap, view, channels, (which,))
        groups = strided_groups(N, view[0], view[1], ch if which == "forward" else 2 * ch)
        _, block, phase = cc.block_changes(groups, min(cap, groups), (ch if which == "forward" else 2 * ch) // 64)
        if N == first and (block if which == "forward" else phase) > 0:
            break
    else:
        pytest.fail(f"no channel count of 192, 320, 448 changes the block across a hand-over on {cap} CUs")
    case = cc.Case(N, view[0], 2 * view[1], channels[0], channels[1], 3, (1, 2), xmax=XMAX, wmax=WMAX, passes=(which,))
    bad = _guarded(run_strided, case, dev, 0, cap, True, True)
    util.measured(f"strided Winograd exact {case.id}, {which}, the channel block changes across a hand-over: elements that differ", bad, bound=0)


def test_minimum_documented_alignment_of_the_pixel_pair_kernels():
    """Forward and input gradient with every base pointer 16 bytes -- the documented minimum -- past a 256-byte boundary."""
    dev = _dev()
    case = cc.Case(2, 4, 2 * 64, 64, 128, 3, (1, 2), xmax=XMAX, wmax=WMAX, passes=("forward", "dgrad"))
    bad = _guarded(run_strided, case, dev, 16)
    util.measured(f"strided Winograd exact {case.id}, bases 16 bytes past a 256-byte boundary: elements that differ", bad, bound=0)


def test_all_ones_weights_against_numpy_box_sums():
    """With every weight 1 the layer is a box sum: rows h-1..h+1 inside the image, columns 2j-1..2j+1 around the wrap, all channels.
    The expected values come from numpy alone, so the comparison does not lean on the direct kernel or on torch's convolution."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    N, H, W, C, K = 2, 8, 128, 64, 64
    cr.headroom("wino_conv", 2 * C, XMAX, 1)
    x = cr.ints((N, H, W, C), XMAX, 4242)
    g = cr.ints((N, H, W // 2, K), XMAX, 4243)
    xs = x.numpy().sum(axis=3)                                                  # [N,H,W]
    cols = np.roll(xs, 1, axis=2) + xs + np.roll(xs, -1, axis=2)                # columns w-1..w+1 (wrapped)
    rows = cols.copy()
    rows[:, 1:] += cols[:, :-1]
    rows[:, :-1] += cols[:, 1:]
    y_ref = np.repeat(rows[:, :, 0::2, None], K, axis=3)                         # output column j sits on image column 2j
    gs = g.numpy().sum(axis=3)                                                  # [N,H,W/2]
    up = np.zeros((N, H, W))
    up[:, :, 0::2] = gs                                                         # g on the image grid, then the same box sum (the box is symmetric)
    cols = np.roll(up, 1, axis=2) + up + np.roll(up, -1, axis=2)
    rows = cols.copy()
    rows[:, 1:] += cols[:, :-1]
    rows[:, :-1] += cols[:, 1:]
    dx_ref = np.repeat(rows[:, :, :, None], C, axis=3)
    A = cr.Arenas(dev)
    x_d, g_d = A.arena(x.shape, torch.float32, x, "x"), A.arena(g.shape, torch.float32, g, "g")
    w_d = A.arena((K, 3, 3, C), torch.float32, torch.ones((K, 3, 3, C), dtype=torch.float64), "w", 0)
    n = int(lib.dl_wino_strided_weights_floats(K, C, 1, 2))
    uf, ub = A.arena((n,), torch.float32, None, "u_fwd", 0), A.arena((n,), torch.float32, None, "u_bwd", 0)
    y_d, dx_d = A.arena(y_ref.shape, torch.float32, None, "y"), A.arena(dx_ref.shape, torch.float32, None, "dx")
    _lib.check(lib.dl_wino_strided_weights_f32(_p(w_d), _p(uf), _p(ub), K, C, 1, 2, _stream()), "dl_wino_strided_weights_f32")
    _lib.check(lib.dl_wino_strided_conv3x3_nhwc_f32(_p(x_d), _p(uf), _p(y_d), N, H, W, C, K, 1, 2, 0, 0, _stream()), "dl_wino_strided_conv3x3_nhwc_f32")
    _lib.check(lib.dl_wino_strided_dgrad3x3_nhwc_f32(_p(g_d), _p(ub), _p(dx_d), None, None, N, H, W, K, C, 1, 2, 0, 0, _stream()),
               "dl_wino_strided_dgrad3x3_nhwc_f32")
    torch.cuda.synchronize()
    A.check("all-ones weights")
    for t in (uf, ub, y_d, dx_d):
        A.check_output(t, "all-ones weights")
    bad = cr.mismatches(y_d, torch.from_numpy(y_ref).float(), "all-ones weights, forward against numpy box sums")
    bad += cr.mismatches(dx_d, torch.from_numpy(dx_ref).float(), "all-ones weights, input gradient against numpy box sums")
    util.measured("strided Winograd exact, all-ones weights against numpy box sums: elements that differ", bad, bound=0)
