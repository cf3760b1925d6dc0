"""The referee of tests/test_gpu_stem_exact.py checked without a GPU: the pooling reference against torch's max-pool (values and
positions, special values included) and against float64 autograd, the float32 emulation of the fused weight gradient against
the float64 reference bit for bit on every exact case and inside the derived bound on real-valued data, the plan table, and --
so that the suite is known to be able to fail -- every planted defect rejected by named cases.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as cr
from tests import stem_ref as sr
from tests import util

PIN_CASES = tuple((2, H, Wc, 8) for H in (1, 2, 3, 5) for Wc in (2, 4, 6, 10, 66)) + sr.POOL_CASES


def _same_bits64(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return int((~((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y)))).sum()) == 0


def _torch_pool(a):
    """(y, code) of torch's max-pool on the wrapped map; its flat index into the [H][Wc + 2] padded plane becomes the 0..8 code."""
    N, H, Wc, C = a.shape
    t = F.pad(torch.from_numpy(a).permute(0, 3, 1, 2), (1, 1, 0, 0), mode="circular")
    y, idx = F.max_pool2d(t, kernel_size=3, stride=(1, 2), padding=(1, 0), return_indices=True)
    ih, iw = idx // (Wc + 2), idx % (Wc + 2)
    r = torch.arange(H).view(1, 1, H, 1)
    q = torch.arange(Wc // 2).view(1, 1, 1, Wc // 2)
    code = (ih - r + 1) * 3 + (iw - 2 * q)
    return y.permute(0, 2, 3, 1).numpy(), code.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("case", PIN_CASES, ids=["x".join(map(str, c)) for c in PIN_CASES])
def test_pool_fwd_ref_is_torchs_max_pool(case):
    """Values (bit patterns: the +-0 rule) and positions (first strictly greater wins, the LAST NaN wins, the first in-range position
    for a window of -inf) on every generated map, specials included."""
    for act in sr.ACTS:
        for special in (False, True):
            a, _, _ = sr.pool_case_data(case, act, special)
            y, win = sr.pool_fwd_ref(a)
            ty, tcode = _torch_pool(a)
            what = f"{case} act {act} specials {special}"
            assert _same_bits64(y, ty), what
            assert np.array_equal(win, tcode), what
            assert win.min() >= 0 and win.max() <= 8 and (win[:, 0] >= 3).all() and (win[:, -1] <= 5).all(), what


def test_specials_plant_what_they_promise():
    """Over the pooling cases the planted maps produce -inf, +inf and NaN outputs, -0.0 and +0.0 from windows that hold both zeros,
    and a NaN that is not the window's first."""
    seen = {"-inf": 0, "+inf": 0, "nan": 0, "-0.0": 0, "+0.0 beside -0.0": 0, "nan not first": 0}
    for case in sr.POOL_CASES:
        a, _, _ = sr.pool_case_data(case, sr.NONE, True)
        y, win = sr.pool_fwd_ref(a)
        seen["-inf"] += int((y == -np.inf).sum())
        seen["+inf"] += int((y == np.inf).sum())
        seen["nan"] += int(np.isnan(y).sum())
        seen["-0.0"] += int(((y == 0) & np.signbit(y)).sum())
        N, H, Wc, C = a.shape
        neg_zero_in_a = bool(((a == 0) & np.signbit(a)).any())
        seen["+0.0 beside -0.0"] += int(((y == 0) & ~np.signbit(y)).sum()) if neg_zero_in_a else 0
        first = np.where(np.arange(H)[None, :, None, None] > 0, 0, 3)
        seen["nan not first"] += int((np.isnan(y) & (win > first)).sum())
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("case", PIN_CASES, ids=["x".join(map(str, c)) for c in PIN_CASES])
def test_pool_bwd_ref_is_autograd(case):
    """With the forward's own positions the scatter equals float64 autograd through max_pool2d(act(pre)), a = act(pre), for none and
    relu (relu'(0) = 0 in both); tanh multiplies the routed gradient by 1 - a^2.  The gather form in float32 (the kernel's order)
    equals the scatter bit for bit, with the forward's positions and with uniform ones."""
    N, H, Wc, C = case
    for act in sr.ACTS:
        pre, g, wu = sr.pool_case_data(case, sr.NONE if act == sr.RELU else act)
        pre_t = torch.from_numpy(pre).requires_grad_(True)
        a_t = torch.relu(pre_t) if act == sr.RELU else pre_t
        a = a_t.detach().numpy()
        win = sr.pool_fwd_ref(a)[1]
        got = sr.pool_bwd_ref(g, a, win, act)
        if act != sr.TANH:
            cr.pool3x3s12(a_t).backward(torch.from_numpy(g))
            assert np.array_equal(got, pre_t.grad.numpy()), (case, act)
        else:
            assert np.array_equal(got, sr.pool_bwd_ref(g, a, win, sr.NONE) * (1.0 - a * a)), case
        for w in (win, wu):
            ref = sr.pool_bwd_ref(g, a, w, act)
            assert sr.bits_differ(sr.pool_bwd_emul32(g, a, w, act), ref, f"gather form {case} act {act}") == 0
            assert not (np.signbit(ref) & (ref == 0)).any()


@pytest.mark.parametrize("case", sr.POOL_CASES, ids=["x".join(map(str, c)) for c in sr.POOL_CASES])
def test_seam_and_edge_rows_receive_gradient(case):
    """The counts the GPU file asserts per case hold for the committed seeds: with the forward's positions and with uniform ones a
    non-zero gradient crosses the wrap to column Wc - 1, reaches column 0, row 0 and row H - 1."""
    for act in sr.ACTS:
        a, g, wu = sr.pool_case_data(case, act)
        for w in (sr.pool_fwd_ref(a)[1], wu):
            counts = sr.seam_counts(g, w)
            assert all(v > 0 for v in counts.values()), (case, act, counts)
            # the garbage of the GPU file: some elements are free of it, and there the gather form does not see it
            g2, clean = sr.garbage(g, a.shape, w, 1 + act)
            e1, e2 = sr.pool_bwd_emul32(g, a, w, act), sr.pool_bwd_emul32(g2, a, w, act)
            assert np.array_equal(e1.view(np.int32)[clean], e2.view(np.int32)[clean])


# ---------------------------------------------------------------------------------------------------- fused weight gradient


@functools.lru_cache(maxsize=None)
def _wcase(case, act):
    c = sr.wgrad_case(*case, act)
    return c, sr.stem_wgrad_ref(c["g"], c["a"], c["win"], c["x8"], act)


@functools.lru_cache(maxsize=None)
def _partials(case, act, defect=None):
    c, _ = _wcase(case, act)
    return sr.slab_partials_emul32(c["g"], c["a"], c["win"], c["x8"], act, defect)


def _emul(case, act, defect=None):
    """(the defects of the reduction reuse the slab partials of the sound emulation)"""
    return sr.reduce_emul32(_partials(case, act, None if defect in sr.WGRAD_DEFECTS[1:3] + sr.WGRAD_DEFECTS[4:] else defect), defect)


def test_plan_table_and_coverage():
    """plan() at every case, literally -- a change of the slab cap shows up here -- and against the library's workspace size."""
    from delora_amd import _lib
    lib = _lib.load()
    for case, (chunks, cps, grid) in sr.WGRAD_PLAN.items():
        p = sr.plan(*case)
        assert (p[0], p[2], p[3]) == (chunks, cps, grid), (case, p)
        assert p[1] == min(chunks, 512) and (grid - 1) * cps < chunks <= grid * cps
        assert int(lib.dl_stem_wgrad_workspace_bytes(*case)) == sr.workspace_bytes(*case) == p[1] * 64 * 72 * 4, case
    for case in sr.REAL_SHAPES + ((8, 64, 2048),):
        assert int(lib.dl_stem_wgrad_workspace_bytes(*case)) == sr.workspace_bytes(*case), case
    assert sr.plan(8, 64, 2048) == (8192, 512, 16, 512)
    assert sr.plan(*sr.REAL_SHAPES[0])[2] == 1 and sr.plan(*sr.REAL_SHAPES[1]) == (216, 216, 1, 216) and sr.plan(*sr.REAL_SHAPES[2])[2] == 2
    for bad in ((1, 1, 6), (1, 1, 2), (0, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert int(lib.dl_stem_wgrad_workspace_bytes(*bad)) == sr.workspace_bytes(*bad) == 0
    assert sr.coverage() == []
    assert sr.coverage([c for c in sr.WGRAD_CASES if sr.plan(*c)[2] == 1]) != []


@pytest.mark.parametrize("case", sr.WGRAD_CASES, ids=["x".join(map(str, c)) for c in sr.WGRAD_CASES])
def test_emulation_equals_the_float64_reference(case):
    """The data are order-proof: the float32 emulation in the fused kernels' order of additions equals float64 autograd bit for bit,
    for every activation; the headroom of the case is asserted while it is generated."""
    for act in sr.ACTS:
        _, ref = _wcase(case, act)
        assert np.abs(ref).max() > 0
        assert sr.bits_differ(_emul(case, act), ref, f"emulation {case} act {act}") == 0


def test_headroom_narrows_instead_of_failing():
    assert sr.headroom(1, 3, 8, sr.TANH) == (3, 2) and sr.headroom(4, 43, 260, sr.RELU) == (3, 2)
    assert sr.headroom(4, 43, 260, sr.TANH) == (2, 1)            # 22 360 pixels on the grid 1/16: (3,2) and (2,2) exceed 2^23 steps


# ---------------------------------------------------------------------------------------------------- planted defects


def _fwd_rejecting(defect):
    out = set()
    for case in sr.POOL_CASES:
        for special in (False, True):
            a, _, _ = sr.pool_case_data(case, sr.NONE, special)
            y, w = sr.pool_fwd_ref(a)
            py, pw = sr.pool_fwd_planted(a, defect)
            if not (_same_bits64(y, py) and np.array_equal(w, pw)):
                out.add((case, special))
    return out


def test_planted_forward_defects_are_rejected():
    plain = {(c, False) for c in sr.POOL_CASES}
    special = {(c, True) for c in sr.POOL_CASES}
    assert _fwd_rejecting("tie_to_later") == plain | special                  # integer maps (and windows of -inf): ties in every case
    # only a window of -inf in row 0 never takes over from the start position: the specials alone show it
    got = _fwd_rejecting("start_0_at_row_0")
    assert got == special, got
    # the left neighbour matters wherever the map is not constant along the row; every case but none in particular
    # (with the specials the one window of (1,1,2,4) is -inf in every channel: no neighbour can change it)
    assert _fwd_rejecting("left_not_wrapped") == (plain | special) - {((1, 1, 2, 4), True)}


def _bwd_rejecting(defect):
    out = set()
    for case in sr.POOL_CASES:
        for act in sr.ACTS:
            a, g, wu = sr.pool_case_data(case, act)
            for name, w in (("fwd", sr.pool_fwd_ref(a)[1]), ("uniform", wu)):
                if sr.bits_differ(sr.pool_bwd_emul32(g, a, w, act, defect), sr.pool_bwd_ref(g, a, w, act), quiet=True):
                    out.add((case, act, name))
    return out


def test_planted_backward_defects_are_rejected():
    every = {(c, act, n) for c in sr.POOL_CASES for act in sr.ACTS for n in ("fwd", "uniform")}
    # the last pooled column's right neighbour: every case has one; in the map of ONE window the emulation clamps the unwrapped
    # neighbour to the end of the plane, which is that window (a kernel would read behind the plane)
    one_window = {e for e in every if e[0] == (1, 1, 2, 4)}
    got = _bwd_rejecting("q1_not_wrapped")
    assert got == every - one_window, (every - one_window) ^ got
    got = _bwd_rejecting("second_window_omitted")
    assert got == every, every - got
    # a missing row test shows where a neighbouring row's code can match: rows exist above / below (H > 1 or N > 1) -- with one row
    # and one image the clamped row is the row itself, compared with codes 0..2 / 6..8 that a single-row map never holds
    got = _bwd_rejecting("row_clamp_missing")
    single = {e for e in every if e[0][0] == 1 and e[0][1] == 1}
    assert got == every - single, (every - single) ^ got
    got = _bwd_rejecting("relu_ge")                              # only relu, and every relu case holds zeros
    assert got == {e for e in every if e[1] == sr.RELU}, got
    got = _bwd_rejecting("tanh_omitted")
    assert got == {e for e in every if e[1] == sr.TANH}, got


def _wgrad_rejecting(defect, act=sr.RELU):
    return {case for case in sr.WGRAD_CASES if sr.bits_differ(_emul(case, act, defect), _wcase(case, act)[1], quiet=True)}


def test_planted_weight_gradient_defects_are_rejected():
    plans = {c: sr.plan(*c) for c in sr.WGRAD_CASES}
    # the slab walk: only where a slab has more than one chunk
    assert _wgrad_rejecting("last_chunk_of_slab_skipped") == {c for c, p in plans.items() if p[2] > 1} == {(19, 27, 8), (25, 41, 8), (4, 43, 260)}
    # the reduction's tail loop: only where grid % 4 != 0
    assert _wgrad_rejecting("reduce_tail_skipped") == {c for c, p in plans.items() if p[3] % 4}
    # an unrolled loop that runs once: only above 32 slabs
    assert _wgrad_rejecting("slabs_32_skipped") == {c for c, p in plans.items() if p[3] > 32} == \
        {(3, 11, 8), (1, 61, 8), (1, 512, 8), (19, 27, 8), (25, 41, 8), (4, 43, 260)}
    # pixels behind a row's end: only where W/2 is no multiple of 64 and a following row exists
    got = _wgrad_rejecting("overhang_not_zeroed")
    ragged = {c for c in sr.WGRAD_CASES if (c[2] // 2) % 64 and c[0] * c[1] > 1}
    assert got == ragged, got ^ ragged
    assert {(1, 3, 132), (2, 5, 72), (4, 43, 260), (1, 2, 4)} <= got and (1, 3, 128) not in got and (1, 1, 8) not in got
    assert _wgrad_rejecting("dw_k_tap_c") == set(sr.WGRAD_CASES)
    for defect in sr.POOL_BWD_DEFECTS[:3]:                        # the fused kernel shares pool_bwd_value: the defects reach dw as well
        for case in ((2, 2, 8), (1, 3, 132), (2, 5, 72)):
            assert sr.bits_differ(_emul(case, sr.RELU, defect), _wcase(case, sr.RELU)[1], quiet=True), (defect, case)


# ---------------------------------------------------------------------------------------------------- float64 tier


@pytest.mark.parametrize("shape", sr.REAL_SHAPES, ids=["x".join(map(str, c)) for c in sr.REAL_SHAPES])
def test_emulation_passes_the_float64_bound(shape):
    """Real-valued data: the float32 emulation stays inside c 2^-24 S_abs per element; the planted slab-walk and layout defects do not."""
    N, H, W = shape
    x8, g, w = sr.real_inputs(N, H, W, 77 + W)
    for act in sr.ACTS:
        a = sr.conv1_host(x8, w, act)
        assert np.abs(a).max() < (0.995 if act == sr.TANH else 1e3)
        win = sr.pool_fwd_ref(a)[1]
        ref = sr.stem_wgrad_ref(g, a, win, x8, act)
        bound = sr.wgrad_bound(g, a, win, x8, act)
        assert bound.min() > 0
        ratio = float((np.abs(sr.stem_wgrad_emul32(g, a, win, x8, act).astype(np.float64) - ref) / bound).max())
        util.measured(f"stem wgrad emulation {shape} act {sr.ACT_NAME[act]}: worst error / bound (c = {sr.op_count(N, H, W, act)})", ratio, bound=1.0)
        bad = float((np.abs(sr.stem_wgrad_emul32(g, a, win, x8, act, "dw_k_tap_c").astype(np.float64) - ref) / bound).max())
        assert bad > 1.0, bad
        if sr.plan(N, H, W)[2] > 1:
            bad = float((np.abs(sr.stem_wgrad_emul32(g, a, win, x8, act, "last_chunk_of_slab_skipped").astype(np.float64) - ref) / bound).max())
            assert bad > 1.0, bad


def test_op_count_is_what_the_code_says():
    # relu at (2,16,256): 64 slabs of one chunk -- 5 + 1 + 16 + 3 + 16 + 3; tanh two more; (19,27,8): two chunks, 257 slabs
    assert sr.op_count(2, 16, 256, sr.RELU) == 44 and sr.op_count(2, 16, 256, sr.TANH) == 46 and sr.op_count(2, 16, 256, sr.NONE) == 44
    assert sr.op_count(8, 9, 264, sr.RELU) == 5 + 1 + 16 + 3 + 54 + 3
    assert sr.op_count(19, 27, 8, sr.RELU) == 5 + 1 + 32 + 3 + 65 + 3
