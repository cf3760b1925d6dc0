"""The half-precision stem kernels (csrc/stemh.hip) through the C ABI against the references of tests/stem_half_ref.py and
tests/stem_ref.py, in bf16 and fp16: the rounding input copy, conv1 on integers whose sums leave the exact-integer range of the type
(the final rounding, ties included, decides every bit), the pooling with its window plane and the fused weight gradient BIT FOR BIT;
conv1 and the weight gradient on real-valued data inside bounds that are derived, not tuned.  Everything runs in
tests/conv_ref.Arenas allocations: inputs frozen, outputs and the workspace -- exactly as long as promised -- poisoned, guards checked
after every launch; a device error ends the session.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import stem_half_ref as hr
from tests import stem_ref as sr
from tests import util

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3                       # DL_ERR_INVALID_ARGUMENT, DL_ERR_UNSUPPORTED
DT = pytest.mark.parametrize("dtype", hr.DTYPES, ids=[hr.NAME[d] for d in hr.DTYPES])


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _ids(cases):
    return ["x".join(map(str, c)) for c in cases]


def _poison_left(o):
    """Elements of an output that still hold the arena's poison (a 32-bit word for fp32 / int8 buffers, a 16-bit one for half)."""
    if o.dtype in hr.DTYPES:
        return int((o.view(torch.int16) == (cr.NAN_WORD[o.dtype] & 0xffff)).sum())
    words = o.reshape(-1).view(torch.int32) if o.dtype == torch.float32 else o.reshape(-1)[: o.numel() // 4 * 4].view(torch.int32)
    return int((words == cr._as_i32(cr.NAN_WORD[o.dtype])).sum())


class Bufs:
    def __init__(self, dev, skew=0):
        self.A, self.W = cr.Arenas(dev, skew), cr.Arenas(dev, 0)       # (the workspace is never skewed)

    def inp(self, arr, dtype=torch.float32, name=""):
        t = torch.from_numpy(np.ascontiguousarray(arr))
        return self.A.arena(tuple(t.shape), dtype, t, name, None if t.dim() == 4 else 0)

    def out(self, shape, dtype=torch.float32, name=""):
        return self.A.arena(shape, dtype, None, name, None if len(shape) == 4 else 0)

    def ws(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return self.W.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)

    def done(self, what, *outs):
        """After a launch: no device error, guards and inputs intact, every element of the outputs written (a half or fp32 output may
        legitimately BE NaN, but not the arena's NaN; int8 planes are checked by their value range)."""
        _sync()
        self.A.check(what)
        self.W.check(what)
        for o in outs:
            if o.dtype != torch.int8:
                left = _poison_left(o)
                assert left == 0, f"{what}: {left} elements were never written"

    def untouched(self, what, *outs):
        _sync()
        self.A.check(what)
        self.W.check(what)
        for o in outs:
            n = o.numel() if o.dtype in hr.DTYPES else o.numel() * o.element_size() // 4
            assert _poison_left(o) == n, f"{what}: a refused call wrote to an output"


# ====================================================================================================== 1. input copy


def _input_copy(case, dtype, skew):
    dev = _dev()
    L, lib = _lib()
    N, H, W = case
    x = hr.input_case(N, H, W, dtype)
    ties, over = hr.input_case_properties(x, dtype)
    assert ties > 0 and over > 0
    b = Bufs(dev, skew)
    x_d = b.A.arena(x.shape, torch.float32, torch.from_numpy(x), "x", H * W)
    o = b.out((N, H, W, 8), dtype, "x8h")
    L.check(lib.dl_stem_input_nhwc_h(_p(x_d), N, H, W, hr.CODE[dtype], _p(o), _stream()), "dl_stem_input_nhwc_h")
    b.done(f"input copy {case}", o)
    want = torch.from_numpy(x).permute(0, 2, 3, 1).contiguous().to(dtype)
    bad = int((o.cpu().view(torch.int16) != want.view(torch.int16)).sum())
    return bad + hr.bits_differ_h(o, hr.input_ref(x, dtype), dtype, f"x8h {case}")


@DT
@pytest.mark.parametrize("case", hr.INPUT_CASES, ids=_ids(hr.INPUT_CASES))
def test_input_copy(case, dtype):
    """x8h equals torch's .to(dtype) of the transposed image bit for bit: Gaussian values, exact ties in both directions, the largest
    finite number, values that overflow to infinity, subnormals and what underflows."""
    util.measured(f"half stem {hr.NAME[dtype]} input copy {case}: elements that differ", _input_copy(case, dtype, 0), bound=0)


@DT
def test_input_copy_minimum_documented_alignment(dtype):
    util.measured(f"half stem {hr.NAME[dtype]} input copy {hr.INPUT_SKEW_CASE}, bases 16 bytes past a 256-byte boundary: elements that differ",
                  _input_copy(hr.INPUT_SKEW_CASE, dtype, 16), bound=0)


# ====================================================================================================== 2. conv1 on integers


def _conv1(L, lib, b, x8, w, N, H, W, act, dtype, tag):
    x_d = b.inp(x8, dtype, "x8h")
    w_d = b.A.arena(w.shape, torch.float32, torch.from_numpy(np.ascontiguousarray(w)), "w1", 0)
    a_d = b.out((N, H, W // 2, 64), dtype, "a")
    L.check(lib.dl_stem_conv1_h(_p(x_d), _p(w_d), N, H, W, act, hr.CODE[dtype], _p(a_d), _stream()), "dl_stem_conv1_h")
    b.done(tag, a_d)
    return x_d, a_d


@DT
@pytest.mark.parametrize("act", [sr.NONE, sr.RELU], ids=["none", "relu"])
@pytest.mark.parametrize("case", hr.CONV1_CASES, ids=_ids(hr.CONV1_CASES))
def test_conv1_integers(case, act, dtype):
    """a = h(act(the exact integer sum)) bit for bit; the case asserts that sums lie beyond the exact-integer range of the type and on
    exact ties, and that the sum is exact in fp32 in any order."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = case
    c = hr.conv1_int_case(N, H, W, dtype, act)
    b = Bufs(dev)
    _, a_d = _conv1(L, lib, b, c["x8"], c["w"], N, H, W, act, dtype, f"conv1 {case}")
    for k, v in c["props"].items():
        util.measured(f"half stem {hr.NAME[dtype]} conv1 {case} act {sr.ACT_NAME[act]}: outputs [{k}]", v)
    util.measured(f"half stem {hr.NAME[dtype]} conv1 {case} act {sr.ACT_NAME[act]}: elements that differ",
                  hr.bits_differ_h(a_d, c["want"], dtype, f"conv1 {case}"), bound=0)


@DT
@pytest.mark.parametrize("act", [sr.NONE, sr.RELU], ids=["none", "relu"])
def test_conv1_minimum_documented_alignment(act, dtype):
    dev = _dev()
    L, lib = _lib()
    N, H, W = hr.CONV1_SKEW_CASE
    c = hr.conv1_int_case(N, H, W, dtype, act, seed=99)
    b = Bufs(dev, 16)
    _, a_d = _conv1(L, lib, b, c["x8"], c["w"], N, H, W, act, dtype, "conv1 skewed")
    util.measured(f"half stem {hr.NAME[dtype]} conv1 {hr.CONV1_SKEW_CASE} act {sr.ACT_NAME[act]}, bases 16 bytes past a 256-byte boundary: "
                  "elements that differ", hr.bits_differ_h(a_d, c["want"], dtype, "conv1 skewed"), bound=0)


@DT
@pytest.mark.parametrize("act", [sr.NONE, sr.RELU], ids=["none", "relu"])
def test_conv1_with_4608_different_weights(act, dtype):
    """Every weight differs from every other one and is converted by the kernel; every window holds one non-zero pixel."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = hr.CONV1_DISTINCT_CASE
    c = hr.conv1_distinct_case(dtype, act)
    b = Bufs(dev)
    _, a_d = _conv1(L, lib, b, c["x8"], c["w"], N, H, W, act, dtype, "conv1 distinct weights")
    util.measured(f"half stem {hr.NAME[dtype]} conv1 with pairwise different weights, act {sr.ACT_NAME[act]}: elements that differ",
                  hr.bits_differ_h(a_d, c["want"], dtype, "conv1 distinct weights"), bound=0)


# ====================================================================================================== 3. conv1 on real values

C1R = [(s, act) for s in hr.CONV1_REAL_SHAPES for act in sr.ACTS]


@DT
@pytest.mark.parametrize("shape,act", C1R, ids=[f"{'x'.join(map(str, s))}-{sr.ACT_NAME[a]}" for s, a in C1R])
def test_conv1_real_values(shape, act, dtype):
    """stem_ref.real_inputs rounded to the type; float64 on the rounded operands; the metric and the absolute terms of
    tests/test_gpu_convh.py (one rounding of the stored value)."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = shape
    x8, _, w = hr.real_case(N, H, W, dtype, 55 + W)
    b = Bufs(dev)
    _, a_d = _conv1(L, lib, b, x8, w, N, H, W, act, dtype, f"conv1 real {shape}")
    want = hr.conv1_ref64(x8, w, act)
    util.measured(f"half stem {hr.NAME[dtype]} conv1 {shape} act {sr.ACT_NAME[act]} vs float64 (units of one rounding)",
                  hr.worst(a_d.cpu().double().numpy(), want, hr.EPS[dtype], hr.conv1_abs_tol(act)), bound=1.0)


# ====================================================================================================== 4. pooling


@DT
@pytest.mark.parametrize("special", [False, True], ids=["plain", "specials"])
@pytest.mark.parametrize("case", hr.POOL_CASES, ids=_ids(hr.POOL_CASES))
def test_pool_forward(case, special, dtype):
    dev = _dev()
    L, lib = _lib()
    N, H, Wc, C = case
    bad = 0
    for act in sr.ACTS:
        a, _, _ = sr.pool_case_data(case, act, special)
        assert hr.representable(a, dtype)
        y_ref, win_ref = sr.pool_fwd_ref(a)
        b = Bufs(dev)
        a_d = b.inp(a, dtype, "a")
        y_d, win_d = b.out(y_ref.shape, dtype, "y"), b.out(y_ref.shape, torch.int8, "win")
        L.check(lib.dl_stem_pool_fwd_h(_p(a_d), N, H, Wc, C, hr.CODE[dtype], _p(y_d), _p(win_d), _stream()), "dl_stem_pool_fwd_h")
        b.done(f"pool forward {case}", y_d)
        win = win_d.cpu().numpy()
        assert win.min() >= 0 and win.max() <= 8, "a window position outside 0..8 (an element of win never written)"
        bad += hr.bits_differ_h(y_d, y_ref, dtype, f"pooled output {case} act {act}")
        nw = int((win != win_ref).sum())
        if nw:
            print(f"win {case} act {act}: {nw} positions differ, first at {np.argwhere(win != win_ref)[:8].tolist()}")
        bad += nw
    util.measured(f"half stem {hr.NAME[dtype]} pool forward {case}{' specials' if special else ''}: elements of y and win that differ", bad, bound=0)


# ====================================================================================================== 5. fused weight gradient on integers


def _wgrad_launch(L, lib, b, N, H, W, act, dtype, g_d, a_d, win_d, x_d):
    nbytes = int(lib.dl_stem_wgrad_h_workspace_bytes(N, H, W))
    assert nbytes == hr.workspace_bytes(N, H, W)
    ws, dw = b.ws(nbytes), b.A.arena((64, 8, 3, 3), torch.float32, None, "dw", 0)
    L.check(lib.dl_stem_wgrad_h(_p(g_d), _p(a_d), _p(win_d), _p(x_d), N, H, W, act, hr.CODE[dtype], _p(ws), _p(dw), _stream()), "dl_stem_wgrad_h")
    b.done(f"half stem wgrad {(N, H, W)} act {act}", dw)
    return dw, ws


def _run_wgrad_case(case, act, dtype, skew=0):
    dev = _dev()
    L, lib = _lib()
    N, H, W = case
    c = hr.wgrad_case(N, H, W, act, dtype)                  # (asserts the headroom and that half storage loses nothing)
    ref = sr.stem_wgrad_ref(c["g"], c["a"], c["win"], c["x8"], act)
    b = Bufs(dev, skew)
    g_d, a_d, win_d, x_d = b.inp(c["g"], dtype, "g pooled"), b.inp(c["a"], dtype, "a"), b.inp(c["win"], torch.int8, "win"), b.inp(c["x8"], dtype, "x8h")
    dw1, ws1 = _wgrad_launch(L, lib, b, N, H, W, act, dtype, g_d, a_d, win_d, x_d)
    dw2, ws2 = _wgrad_launch(L, lib, b, N, H, W, act, dtype, g_d, a_d, win_d, x_d)
    tag = f"half stem wgrad {case} act {sr.ACT_NAME[act]} {hr.NAME[dtype]}"
    # 8. determinism: dw and the partials (grid of them are written; the rest of the workspace keeps its poison in both runs)
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)), f"{tag}: two runs differ"
    assert torch.equal(ws1.view(torch.int32), ws2.view(torch.int32)), f"{tag}: the partials of two runs differ"
    grid = hr.plan(N, H, W)[3]
    assert _poison_left(ws1[: grid * 64 * 72]) == 0, f"{tag}: a partial was not written"
    return sr.bits_differ(dw1, ref, tag)


WGRAD_PARAMS = [(c, act) for c in hr.WGRAD_CASES for act in sr.ACTS]


@DT
@pytest.mark.parametrize("case,act", WGRAD_PARAMS, ids=[f"{'x'.join(map(str, c))}-{sr.ACT_NAME[a]}" for c, a in WGRAD_PARAMS])
def test_stem_wgrad_integers(case, act, dtype):
    """dw of the fused launch equals float64 autograd bit for bit, and two launches leave the same bits in dw and in the partials."""
    util.measured(f"half stem {hr.NAME[dtype]} wgrad {case} act {sr.ACT_NAME[act]}: elements that differ from float64",
                  _run_wgrad_case(case, act, dtype), bound=0)


@DT
@pytest.mark.parametrize("act", sr.ACTS, ids=[sr.ACT_NAME[a] for a in sr.ACTS])
def test_stem_wgrad_minimum_documented_alignment(act, dtype):
    util.measured(f"half stem {hr.NAME[dtype]} wgrad {hr.SKEW_CASE} act {sr.ACT_NAME[act]}, bases 16 bytes past a 256-byte boundary: "
                  "elements that differ", _run_wgrad_case(hr.SKEW_CASE, act, dtype, skew=16), bound=0)


def test_the_cases_cover_the_launch_plans():
    """The literal plan tables against the restated plans and the library's workspace sizes."""
    _dev()
    _, lib = _lib()
    for case, (chunks, cps, grid) in hr.WGRAD_PLAN.items():
        p = hr.plan(*case)
        assert (p[0], p[2], p[3]) == (chunks, cps, grid), (case, p)
        assert int(lib.dl_stem_wgrad_h_workspace_bytes(*case)) == p[1] * 64 * 72 * 4
    assert not hr.coverage() and not hr.conv1_coverage()
    for case, want in hr.CONV1_PLAN.items():
        assert hr.conv1_plan(*case) == want, case


# ====================================================================================================== 6. fused weight gradient on real values

REAL_PARAMS = [(s, act) for s in sr.REAL_SHAPES for act in sr.ACTS]


@DT
@pytest.mark.parametrize("shape,act", REAL_PARAMS, ids=[f"{'x'.join(map(str, c))}-{sr.ACT_NAME[a]}" for c, a in REAL_PARAMS])
def test_stem_wgrad_real_values(shape, act, dtype):
    """Real-valued data through the three forward entry points, then the fused weight gradient: per element |dw - float64| <=
    c 2^-24 sum |gc| |x| with gc rounded to the type exactly as the kernel must (stem_half_ref.gc_half) and c the count of rounded
    additions read from the launch plan.  On the way: a inside one rounding of float64, y and win equal to the pooling reference."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = shape
    x8, g, w = hr.real_case(N, H, W, dtype, 77 + W)
    b = Bufs(dev)
    g_d = b.inp(g, dtype, "g pooled")
    x_d, a_d = _conv1(L, lib, b, x8, w, N, H, W, act, dtype, f"conv1 {shape}")
    b.A.freeze(a_d)
    a = a_d.cpu().double().numpy()
    assert np.abs(a).max() < (0.995 if act == sr.TANH else 1e3)
    assert hr.worst(a, hr.conv1_ref64(x8, w, act), hr.EPS[dtype], hr.conv1_abs_tol(act)) <= 1.0
    y_d, win_d = b.out((N, H, W // 4, 64), dtype, "y"), b.out((N, H, W // 4, 64), torch.int8, "win")
    L.check(lib.dl_stem_pool_fwd_h(_p(a_d), N, H, W // 2, 64, hr.CODE[dtype], _p(y_d), _p(win_d), _stream()), "dl_stem_pool_fwd_h")
    b.done(f"pool forward {shape}", y_d)
    b.A.freeze(win_d)
    win = win_d.cpu().numpy()
    y_ref, win_ref = sr.pool_fwd_ref(a)
    assert hr.bits_differ_h(y_d, y_ref, dtype, f"pooled output {shape}") == 0 and np.array_equal(win, win_ref)
    dw, _ = _wgrad_launch(L, lib, b, N, H, W, act, dtype, g_d, a_d, win_d, x_d)
    ref, bound = hr.wgrad_ref_and_bound(hr.gc_half(g, a, win, act, dtype), x8, N, H, W)
    assert bound.min() > 0
    util.measured(f"half stem {hr.NAME[dtype]} wgrad float64 {shape} act {sr.ACT_NAME[act]}: worst error / bound (c = {hr.wgrad_op_count(N, H, W)})",
                  float((np.abs(dw.cpu().numpy().astype(np.float64) - ref) / bound).max()), bound=1.0)


# ====================================================================================================== 7. refusals


def _refused(lib, rc, code, *words):
    assert rc == code, (rc, code, lib.dl_last_error())
    text = lib.dl_last_error().decode()
    for wd in words:
        assert wd in text, (wd, text)


@DT
def test_refusals_leave_the_outputs_untouched(dtype):
    dev = _dev()
    _, lib = _lib()
    code, other = hr.CODE[dtype], 0                        # 0 = DL_DTYPE_F32: not a half type
    st = _stream()
    N, H, W = 1, 2, 8
    b = Bufs(dev)
    x = b.A.arena((N, 8, H, W), torch.float32, torch.ones((N, 8, H, W)), "x", H * W)
    x8 = b.inp(np.ones((N, H, W, 8)), dtype, "x8h")
    w1 = b.A.arena((64, 3, 3, 8), torch.float32, torch.ones((64, 3, 3, 8)), "w1", 0)
    a = b.inp(np.ones((N, H, W // 2, 64)), dtype, "a")
    g = b.inp(np.ones((N, H, W // 4, 64)), dtype, "g")
    win = b.inp(np.full((N, H, W // 4, 64), 4, dtype=np.int8), torch.int8, "win")
    o_x8, o_a = b.out((N, H, W, 8), dtype, "x8h out"), b.out((N, H, W // 2, 64), dtype, "a out")
    o_y, o_win = b.out((N, H, W // 4, 64), dtype, "y out"), b.out((N, H, W // 4, 64), torch.int8, "win out")
    ws, dw = b.ws(int(lib.dl_stem_wgrad_h_workspace_bytes(N, H, W))), b.A.arena((64, 8, 3, 3), torch.float32, None, "dw", 0)
    off = lambda t, nbytes: ctypes.c_void_p(t.data_ptr() + nbytes)       # a misaligned address inside the buffer
    big = (1, 1 << 15, 1 << 13)                            # N H W 8 = 2^31 elements

    f, name = lib.dl_stem_input_nhwc_h, "dl_stem_input_nhwc_h"
    _refused(lib, f(None, N, H, W, code, _p(o_x8), st), INVALID, name, "x_nchw")
    _refused(lib, f(_p(x), N, H, W, code, None, st), INVALID, name, "x8h")
    _refused(lib, f(_p(x), N, H, W, code, off(o_x8, 8), st), INVALID, name, "x8h", "aligned")
    _refused(lib, f(off(x, 2), N, H, W, code, _p(o_x8), st), INVALID, name, "x_nchw", "aligned")
    for bad in ((0, H, W), (N, -1, W), (N, H, 0)):
        _refused(lib, f(_p(x), *bad, code, _p(o_x8), st), INVALID, name, "positive")
    _refused(lib, f(_p(x), N, H, W, other, _p(o_x8), st), UNSUPPORTED, name, "dtype")
    _refused(lib, f(_p(x), N, H, 6, code, _p(o_x8), st), UNSUPPORTED, name, "W=6")
    _refused(lib, f(_p(x), *big, code, _p(o_x8), st), UNSUPPORTED, name, "2^31")

    f, name = lib.dl_stem_conv1_h, "dl_stem_conv1_h"
    args = [_p(x8), _p(w1), N, H, W, sr.RELU, code, _p(o_a), st]
    for i, field in ((0, "x8h"), (1, "w1"), (7, "a")):
        _refused(lib, f(*[None if k == i else v for k, v in enumerate(args)]), INVALID, name, field)
    for i, t, field in ((0, x8, "x8h"), (1, w1, "w1"), (7, o_a, "a")):
        _refused(lib, f(*[off(t, 8) if k == i else v for k, v in enumerate(args)]), INVALID, name, field, "aligned")
    for i in (2, 3, 4):
        _refused(lib, f(*[0 if k == i else v for k, v in enumerate(args)]), INVALID, name, "positive")
    for act in (-1, 3):
        _refused(lib, f(*[act if k == 5 else v for k, v in enumerate(args)]), INVALID, name, "act")
    _refused(lib, f(*[other if k == 6 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "dtype")
    _refused(lib, f(*[10 if k == 4 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "W=10")
    _refused(lib, f(_p(x8), _p(w1), 1, 1 << 13, 1 << 13, sr.RELU, code, _p(o_a), st), UNSUPPORTED, name, "2^31")

    f, name = lib.dl_stem_pool_fwd_h, "dl_stem_pool_fwd_h"
    args = [_p(a), N, H, W // 2, 64, code, _p(o_y), _p(o_win), st]
    for i, field in ((0, "a"), (6, "y"), (7, "win")):
        _refused(lib, f(*[None if k == i else v for k, v in enumerate(args)]), INVALID, name, field)
    for i, t, field, nb in ((0, a, "a", 8), (6, o_y, "y", 8), (7, o_win, "win", 4)):
        _refused(lib, f(*[off(t, nb) if k == i else v for k, v in enumerate(args)]), INVALID, name, field, "aligned")
    for i in (1, 2, 3, 4):
        _refused(lib, f(*[0 if k == i else v for k, v in enumerate(args)]), INVALID, name, "positive")
    _refused(lib, f(*[other if k == 5 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "dtype")
    _refused(lib, f(*[3 if k == 3 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "Wc=3")
    _refused(lib, f(*[12 if k == 4 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "C=12")
    _refused(lib, f(_p(a), 1, 1 << 12, 1 << 13, 64, code, _p(o_y), _p(o_win), st), UNSUPPORTED, name, "2^31")

    f, name = lib.dl_stem_wgrad_h, "dl_stem_wgrad_h"
    args = [_p(g), _p(a), _p(win), _p(x8), N, H, W, sr.RELU, code, _p(ws), _p(dw), st]
    for i, field in ((0, "g_pooled"), (1, "a"), (2, "win"), (3, "x8h"), (9, "workspace"), (10, "dw")):
        _refused(lib, f(*[None if k == i else v for k, v in enumerate(args)]), INVALID, name, field)
    for i, t, field, nb in ((0, g, "g_pooled", 8), (1, a, "a", 8), (2, win, "win", 4), (3, x8, "x8h", 8), (9, ws, "workspace", 8), (10, dw, "dw", 2)):
        _refused(lib, f(*[off(t, nb) if k == i else v for k, v in enumerate(args)]), INVALID, name, field, "aligned")
    for i in (4, 5, 6):
        _refused(lib, f(*[0 if k == i else v for k, v in enumerate(args)]), INVALID, name, "positive")
    for act in (-1, 3):
        _refused(lib, f(*[act if k == 7 else v for k, v in enumerate(args)]), INVALID, name, "act")
    _refused(lib, f(*[other if k == 8 else v for k, v in enumerate(args)]), UNSUPPORTED, name, "dtype")
    for Wb in (6, 10, 7):
        assert int(lib.dl_stem_wgrad_h_workspace_bytes(N, H, Wb)) == 0
        _refused(lib, f(*[Wb if k == 6 else v for k, v in enumerate(args)]), UNSUPPORTED, name, f"W={Wb}")
    assert int(lib.dl_stem_wgrad_h_workspace_bytes(1, 1 << 13, 1 << 13)) == 0 and int(lib.dl_stem_wgrad_h_workspace_bytes(0, H, W)) == 0
    _refused(lib, f(_p(g), _p(a), _p(win), _p(x8), 1, 1 << 13, 1 << 13, sr.RELU, code, _p(ws), _p(dw), st), UNSUPPORTED, name, "2^31")
    b.untouched("half stem refusals", o_x8, o_a, o_y, o_win, dw, ws)
