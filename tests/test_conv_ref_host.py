"""The exact convolution referee (tests/conv_ref.py) checked on the CPU: against plain nested loops, the two Winograd algebras in
float32 with shuffled accumulation orders against float64 direct sums, ``headroom`` for every GPU case, the coverage of the GPU
cases at 256 CUs, the dispatch query itself, and the arena / reporter helpers."""
import numpy as np
import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr

GEOMS = [(3, (1, 1)), (3, (1, 2)), (3, (2, 2)), (1, (1, 2)), (1, (2, 2))]


@pytest.mark.parametrize("ks,stride", GEOMS)
@pytest.mark.parametrize("hw", [(1, 2), (3, 5), (4, 6), (5, 3)])
def test_reference_equals_nested_loops(ks, stride, hw):
    H, W = hw
    x, w = cr.ints((2, H, W, 3), 3, 1), cr.ints((4, ks, ks, 3), 2, 2)
    y = cr.conv(x, w, stride)
    assert torch.equal(y, torch.from_numpy(cr.conv_loops(x.numpy(), w.numpy(), stride)))
    # the gradients are the adjoints of the (bilinear) forward: <g, conv(x', w)> = <dx, x'> and <g, conv(x, w')> = <dw, w'>, exactly
    g = cr.ints(tuple(y.shape), 3, 3)
    dx, dw = cr.conv_grads(x, w, g, stride)
    x2, w2 = cr.ints(tuple(x.shape), 3, 4), cr.ints(tuple(w.shape), 2, 5)
    assert float((g * torch.from_numpy(cr.conv_loops(x2.numpy(), w.numpy(), stride))).sum()) == float((dx * x2).sum())
    assert float((g * torch.from_numpy(cr.conv_loops(x.numpy(), w2.numpy(), stride))).sum()) == float((dw * w2).sum())


@pytest.mark.parametrize("ks,stride", GEOMS)
def test_input_gradient_without_autograd_through_the_weights(ks, stride):
    """``conv_dx`` (what a case without the weight-gradient pass uses) equals the dx of ``conv_grads``; the stride-1 3x3 branch is a
    second ``conv`` with flipped, transposed taps, on an odd and an even image, one row, two columns."""
    for H, W in ((1, 2), (3, 5), (4, 6)):
        x, w = cr.ints((2, H, W, 3), 3, 1), cr.ints((4, ks, ks, 3), 2, 2)
        g = cr.ints((2, cr.out_size(H, stride[0]), cr.out_size(W, stride[1]), 4), 3, 3)
        assert torch.equal(cr.conv_dx(x.shape, w, g, stride), cr.conv_grads(x, w, g, stride)[0])


def test_epilogue_order_and_saved_activations():
    v = torch.tensor([[-3.0, 2.0, 5.0, -1.0]], dtype=torch.float64)
    add = torch.tensor([[4.0, -4.0, 0.0, 1.0]], dtype=torch.float64)
    s = torch.tensor([[0.5, 0.0, -0.75, 2.0]], dtype=torch.float64)
    assert cr.epilogue(v, cr.EPI_ADD | cr.EPI_ACT, cr.ACT_RELU, add).tolist() == [[1.0, 0.0, 5.0, 0.0]]
    assert cr.epilogue(v, cr.EPI_ADD | cr.EPI_DACT, cr.ACT_TANH, add, s).tolist() == [[0.75, -2.0, 5.0 * (1 - 0.5625), 0.0 * -3.0]]
    assert cr.epilogue(v, cr.EPI_DACT, cr.ACT_RELU, None, s).tolist() == [[-3.0, 0.0, 0.0, -1.0]]
    t = cr.saved_tanh((1000,), 7)
    assert set((t * 4).tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0} and bool(((1 - t * t) * 16 == torch.round((1 - t * t) * 16)).all())
    assert set(cr.saved_relu((1000,), 7).tolist()) == {0.0, 1.0, 2.0, 3.0}
    assert torch.equal(cr.ints((5, 7), 3, 11), cr.ints((5, 7), 3, 11)) and float(cr.ints((4096,), 3, 1).abs().max()) == 3.0
    g = torch.zeros((1, 2, 3, 1), dtype=torch.float64)
    full = cr.epilogue(torch.zeros((1, 4, 5, 1), dtype=torch.float64), cr.EPI_ADD_GRID, 0, add_grid=g + 1, stride=(2, 2))
    assert float(full.sum()) == 6.0 and float(full[0, ::2, ::2].sum()) == 6.0


def test_pool_equals_nested_loops_with_ties_everywhere():
    a = torch.relu(cr.ints((1, 3, 6, 2), 2, 5))
    y = cr.pool3x3s12(a)
    H, W = 3, 6
    for h in range(H):
        for wo in range(W // 2):
            for ch in range(2):
                win = [float(a[0, hh, (2 * wo + s - 1) % W, ch]) for hh in range(max(0, h - 1), min(H, h + 2)) for s in range(3)]
                assert float(y[0, h, wo, ch]) == max(win)


# ---- the two Winograd algebras in float32, accumulated in a shuffled order, against float64 direct sums
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float32)
G3 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float32)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float32)
G2 = np.array([[1, 0], [.5, .5], [.5, -.5], [0, 1]], dtype=np.float32)
AT3 = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, -1]], dtype=np.float32)


def _input_tiles(x):
    """x [N,H,W,C] (H, W even) -> 4x4 input tiles [N,H/2,W/2,4,4,C] of the wrapped, zero-row-padded image."""
    N, H, W, C = x.shape
    xp = np.zeros((N, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    xp[:, 1:-1, 0], xp[:, 1:-1, -1] = x[:, :, -1], x[:, :, 0]
    return np.stack([np.stack([xp[:, i:i + H:2, j:j + W:2] for j in range(4)], axis=3) for i in range(4)], axis=3)


def _shuffled_sum(terms, axis_len, seed):
    """Sum over the LAST axis in float32 in a random order; every partial sum must be what float64 gives (nothing was rounded)."""
    perm = np.random.default_rng(seed).permutation(axis_len)
    t = terms[..., perm]
    c32 = np.cumsum(t, axis=-1, dtype=np.float32)
    c64 = np.cumsum(t.astype(np.float64), axis=-1)
    assert np.array_equal(c32.astype(np.float64), c64)
    return c32[..., -1], float(np.abs(c64).max())


def test_winograd_forward_algebra_is_exact_in_float32_for_512_channels():
    C, K = 512, 4
    x, w = cr.ints((1, 4, 8, C), 3, 1), cr.ints((K, 3, 3, C), 2, 2)
    cr.headroom("wino_conv", C, 3, 2)
    d = _input_tiles(x.numpy().astype(np.float32))                                     # [1,2,4,4,4,C]
    V = np.einsum("ai,nhwijc,bj->nhwabc", BT, d, BT).astype(np.float32)
    U = np.einsum("ar,krsc,bs->abkc", G3, w.numpy().astype(np.float32), G3).astype(np.float32)
    assert np.array_equal(U * 4, np.round(U * 4))                                       # the grid 1/4
    M, peak = _shuffled_sum(V[:, :, :, :, :, None, :] * U[None, None, None], C, 3)      # [1,2,4,4,4,K]
    Y = np.einsum("pa,nhwabk,qb->nhpwqk", AT2, M, AT2).astype(np.float32).reshape(1, 4, 8, K)
    assert np.array_equal(Y.astype(np.float64), cr.conv(x, w).numpy())
    assert peak < 2 ** 22


def test_winograd_weight_gradient_algebra_is_exact_in_float32_for_11520_tiles():
    """F(3x3,2x2) over 11 520 tiles of random integers (x in [-3,3], g in [-2,2]): the partial sums walk randomly and stay far inside
    fp32 (``headroom`` is the WORST case and bounds the GPU cases; this is the regime the network's images are in)."""
    N, H, W, C, K = 5, 48, 192, 2, 2
    x, g = cr.ints((N, H, W, C), 3, 1), cr.ints((N, H, W, K), 2, 2)
    d = _input_tiles(x.numpy().astype(np.float32))                                     # [N,24,96,4,4,C]
    gn = g.numpy().astype(np.float32)
    gt = np.stack([np.stack([gn[:, i::2, j::2] for j in range(2)], axis=3) for i in range(2)], axis=3)       # [N,24,96,2,2,K]
    V = np.einsum("ai,nhwijc,bj->abcnhw", BT, d, BT).astype(np.float32).reshape(4, 4, C, -1)
    Ug = np.einsum("ai,nhwijk,bj->abknhw", G2, gt, G2).astype(np.float32).reshape(4, 4, K, -1)
    assert V.shape[-1] == 11520
    M, peak = _shuffled_sum(Ug[:, :, :, None, :] * V[:, :, None, :, :], 11520, 5)     # [4,4,K,C]
    dw = np.einsum("ra,abkc,sb->krsc", AT3, M, AT3).astype(np.float32)
    ref = cr.conv_grads(x, torch.zeros((K, 3, 3, C), dtype=torch.float64), g)[1].numpy()
    assert np.array_equal(dw.astype(np.float64), ref)
    assert peak < 2 ** 20


# ---- headroom
def test_headroom_holds_for_every_gpu_case_and_refuses_what_is_not_exact():
    worst = max(c.headroom() for c in cc.ALL)
    assert worst < cr.LIMIT
    assert all(c.xmax >= 1 and c.wmax >= 1 for c in cc.ALL) and len({c.id for c in cc.ALL}) == len(cc.ALL)
    with pytest.raises(AssertionError):
        cr.headroom("wino_conv", 512, 16, 16)                  # 81 * 512 * 256 * 4 grid steps
    with pytest.raises(AssertionError):
        cr.headroom("wino_wgrad", 11520, 3, 2)                 # the worst case of the 11 520-tile image is NOT exact
    with pytest.raises(AssertionError):
        cr.headroom("direct", 512, 3, 6, storage=torch.float16)            # 82 944 does not fit fp16
    assert cr.headroom("direct", 64, 3, 2, add=3, dact_tanh=True) == (9 * 64 * 6 + 3) * 16


# ---- the dispatch query and the coverage of the GPU cases
def _lib():
    from delora_amd import _lib
    return _lib


def test_plan_query_runs_the_dispatch_without_a_gpu():
    L = _lib()
    assert L.conv_plan(L.PLAN_WINO_CONV, 0, 1, 4, 64, 128, 64, cu_count=256) == ["k_wino_conv<32, false, true> grid=4x1x1 block=512 splits=4",
                                                                                 "k_wino_split_sum grid=16x1x1 block=256"]
    assert L.conv_plan(L.PLAN_WINO_CONV, 0, 1, 4, 64, 128, 64, mode=1, cu_count=256) == ["k_wino_conv<32, false, false> grid=1x1x1 block=512"]
    assert L.conv_plan(L.PLAN_WINO_CONV, 0, 1, 4, 64, 512, 64, cu_count=8)[0].endswith("splits=8")      # the plan follows the CU count given
    assert L.conv_plan(L.PLAN_CONV, 2, 1, 64, 512, 160, 512)[0].startswith("k_convh<false, 512, 128, 4, 2, 64, GeomConv<3, 1, 1>, 3, 3, 0> grid=256x1x1")
    odd = L.conv_plan(L.PLAN_DGRAD_STRIDED, 0, 1, 7, 45, 256, 512, 3, 2, 2, 0, 256)
    assert odd[0].startswith("k_dgrad_oddw_seam grid=1x2x4") and len(odd) == 5                          # seam terms + four stride phases
    assert [l.split(" grid")[0] for l in L.conv_plan(L.PLAN_WGRAD, 0, 1, 8, 64, 64, 64)] == ["k_wgrad_f32<64, 64, 32, 1, 1, 3, true>", "k_wgrad_reduce"]
    assert L.conv_plan(L.PLAN_WGRAD, 0, 1, 8, 32, 64, 64)[0].startswith("k_wgrad_f32<64, 64, 32, 1, 1, 3, false>")        # 31 + 3 columns > W
    lib = L.load()
    with pytest.raises(L.DeloraHipError, match="does not tile"):
        L.conv_plan(L.PLAN_CONV, 0, 1, 4, 64, 64, 48)
    with pytest.raises(L.DeloraHipError, match="unknown op"):
        L.conv_plan(99, 0, 1, 4, 64, 64, 64)
    import ctypes
    small = ctypes.create_string_buffer(8)
    assert lib.dl_conv_plan_describe(L.PLAN_CONV, 0, 1, 4, 64, 64, 64, 3, 1, 1, 0, 256, small, 8) == -1 and b"needs" in lib.dl_last_error()
    # a query leaves no sink behind: the next real call reports through the usual path
    assert lib.dl_conv2d_nhwc_f32(None, None, None, None, None, 1, 4, 64, 64, 64, 3, 1, 1, 0, 0, 0, None) == -1


def test_the_gpu_cases_reach_every_instantiation_at_256_cus():
    reach = cc.reachable_labels(256)
    got = set()
    for c in cc.ALL:
        got |= c.labels(256)
    assert not (reach - got), f"instantiations no case reaches: {sorted(reach - got)}"
    written = cc.expected_wino_labels() | cc.expected_wgrad_labels()
    assert not (written - got), f"written down from the dispatch, reached by no case: {sorted(written - got)}"
    assert not (written - reach)
    # nothing of these families is selected that was not written down
    fam = {l for l in reach if l.startswith(("k_wino_conv", "k_wino_split", "k_wino_wgrad<", "k_wino_wgrad_batch<", "k_wgrad_f32<", "k_wgrad_f32_batch<", "k_wgradh<", "k_wgradh_batch<"))}
    extra = {l.replace(" one slab", "").replace(" slabs", "") for l in fam} - written
    assert not extra, sorted(extra)
    # the persistent loop's hand-over is reached by the persistent cases and by nothing else
    several = {l for l in written if l.endswith(cc.SEVERAL)}
    assert len(several) == 6
    fixed = set()
    for c in cc.FIXED:
        fixed |= c.labels(256)
    assert not (fixed & several), sorted(fixed & several)


PERSISTENT_KERNEL = {"<32,F>": "k_wino_conv<32, false, false>", "<16,F>": "k_wino_conv<16, false, false>", "<32,T>": "k_wino_conv<32, true, false>",
                     "<16,T>": "k_wino_conv<16, true, false>", "<8,T>": "k_wino_conv<8, true, false>", "<4,T>": "k_wino_conv<4, true, false>"}


@pytest.mark.parametrize("cu", [256, 304, 120])
def test_persistent_cases_are_persistent_on_the_instantiation_they_name(cu):
    """The geometries of ``persistent_cases`` were worked out by hand from wino_plan; the dispatch is the authority.  For several CU
    counts: each case launches the instantiation its name says, forward and input gradient, with the grid capped at the CU count
    and cu < groups < 2 cu (the "3x" ones at least 3 cu and no multiple of it)."""
    L = _lib()
    cases = cc.persistent_cases(cu)
    assert set(PERSISTENT_KERNEL) < set(cases) and len(cases) == 11
    for name, c in cases.items():
        kernel = PERSISTENT_KERNEL[name.split(" ")[0]]
        geom = cc.PERSISTENT_GEOMS[name if name.endswith("one image") else name.split(" ")[0]]
        for transposed in ((False, True) if c.dgrad_ok else (False,)):
            C, K = (c.K, c.C) if transposed else (c.C, c.K)
            lines = L.conv_plan(L.PLAN_WINO_CONV, 0, c.N, c.H, c.W, C, K, cu_count=cu)
            assert len(lines) == 1 and lines[0].startswith(kernel + " grid="), (name, lines)
            groups, grid = cc.wino_groups(lines[0], c.N, c.H, c.W, K)
            assert grid == cu and groups == c.N * geom[2] * (K // 64), (name, lines, groups)
            handovers, block, _ = cc.block_changes(groups, grid, K // 64)
            assert handovers == groups - grid and (block > 0) == name.endswith("several blocks"), (name, handovers, block)
            if name.endswith("3x"):
                assert groups >= 3 * cu and groups % cu, (name, groups)
            else:
                assert cu < groups < 2 * cu, (name, groups)
        assert f"{kernel} {cc.SEVERAL}" in c.labels(cu)
        assert (c.xmax, c.wmax) == (3, 2) and not c.wgrad_ok and c.headroom() < 2 ** 20
    assert cases["<32,F> 72 channels"].C == 72 and not cases["<32,F> 72 channels"].dgrad_ok


def test_persistent_cases_hand_over_inside_an_image_and_across_images():
    """At 256 CUs a workgroup's next group is 32 positions on (the XCD swizzle): another image where an image has 2 or 3 groups,
    the same image (other tile rows, the edge flag changing) in the 48-group geometry."""
    cases = cc.persistent_cases(256)
    assert cc.group_walk(cases["<32,F>"], 256) == (258, 256, 0, 2)
    assert cc.group_walk(cases["<32,F> 3x"], 256) == (771, 256, 0, 771 - 256)
    groups, grid, same, other = cc.group_walk(cases["<32,F> one image"], 256)
    assert (groups, grid) == (288, 256) and same > 0 and same + other == 32


def test_a_case_can_leave_the_weight_gradient_and_its_headroom_out():
    assert cc.Case(86, 12, 64, 64, 64).xmax == 1                                         # the Winograd-domain weight gradient narrows it
    with pytest.raises(AssertionError):
        cc.Case(257, 12, 64, 64, 64, xmax=1, wmax=1).headroom()                          # ... and refuses this one outright
    c = cc.Case(257, 12, 64, 64, 64, xmax=3, wmax=2, passes=("forward", "dgrad"))
    assert c.dgrad_ok and not c.wgrad_ok and c.headroom() == cr.headroom("wino_conv", 64, 3, 2, add=3, dact_tanh=True)
    L = _lib()
    assert not any(q[0] in (L.PLAN_WGRAD, L.PLAN_WGRAD_BATCH, L.PLAN_WINO_WGRAD, L.PLAN_WINO_WGRAD_BATCH) for q in c.plan_queries())
    fwd = cc.Case(1, 4, 64, 64, 64, passes=("forward",))
    assert not fwd.dgrad_ok and len(fwd.plan_queries()) == 2


def test_chunk_count_cases_and_their_split():
    """1, 2, 3 and 9 chunks run as one range; 160 channels are 20 chunks, cut into four ranges of five (odd) at 256 CUs."""
    L = _lib()
    chunk = [c for c in cc.FIXED if c.dtype == cc.F32 and c.s1 and c.C in cc.CHUNK_CHANNELS]
    assert sorted((c.H, c.W, c.C) for c in chunk) == sorted((h, w, ch) for h, w in ((4, 64), (7, 30)) for ch in cc.CHUNK_CHANNELS)
    for c in chunk:
        lines = L.conv_plan(L.PLAN_WINO_CONV, 0, c.N, c.H, c.W, c.C, c.K, cu_count=256)
        kernel = ("k_wino_conv<32, false, " if c.W == 64 else "k_wino_conv<16, true, ") + ("true>" if c.C == 160 else "false>")
        assert lines[0].startswith(kernel + " grid="), lines
        assert lines[0].endswith(" splits=4") == (c.C == 160) and len(lines) == (2 if c.C == 160 else 1), lines
        assert not c.dgrad_ok and not c.wgrad_ok
    # the direct kernel reduces the ragged image in chunks of 16 channels: three cases are the Winograd kernel's alone; every
    # case of 64-channel multiples has a direct forward by definition
    assert [(c.W, c.C) for c in chunk if not c.direct_ok] == [(30, 8), (30, 24), (30, 72)]
    assert all(c.direct_ok for c in cc.ALL if c not in chunk)


# ---- arenas and the reporter (on the CPU: the helpers are device-agnostic)
def test_arena_sees_a_write_beside_the_buffer_and_a_changed_input():
    A = cr.Arenas(torch.device("cpu"), skew=16)
    x = A.arena((1, 2, 3, 8), torch.float32, torch.ones((1, 2, 3, 8), dtype=torch.float64), "x")
    y = A.arena((1, 2, 3, 8), torch.bfloat16, None, "y")
    assert x.data_ptr() % 256 == 16 and y.data_ptr() % 256 == 16 and bool(torch.isnan(y).all())
    A.check("clean")
    with pytest.raises(AssertionError, match="never written"):
        A.check_output(y, "y")
    it = A.items[1]
    it["raw"][it["hi"]] = 0                                   # the first word behind y
    with pytest.raises(AssertionError, match="guard of y touched: 0 words below, 1 above"):
        A.check("overrun")
    it["raw"][it["hi"]] = it["word"]
    x[0, 1, 2, 3] = 5.0
    with pytest.raises(AssertionError, match="input x was modified"):
        A.check("input")
    assert it["lo"] * 4 >= cr.GUARD_MIN_BYTES and A.arena((1, 64, 720, 64), torch.float32, None, "big") is not None
    assert A.items[2]["lo"] * 4 >= 32 * 720 * 64 * 4                                  # 32 image rows where that is more than 256 KiB


def test_reporter_names_the_seam_column(capsys):
    ref = torch.zeros((2, 4, 6, 8))
    got = ref.clone()
    got[1, 2, 5, 3] = 1.0
    got[0, 0, 0, 0] = -1.0
    assert cr.mismatches(got, ref, "demo") == 2
    text = capsys.readouterr().out
    assert "2 of 384 elements differ" in text and "at (0, 0, 0, 0): got -1.0, expected 0.0" in text
    assert "1 at column 0" in text and "1 at column W-1 = 5" in text and "ALL mismatches lie on the wrap-around seam" in text
    assert cr.mismatches(ref, ref.clone(), "same") == 0
