"""The stem kernels (csrc/stem.hip) against the references of tests/stem_ref.py: the wrapped max-pooling forward and backward and the
fused conv1 weight gradient BIT FOR BIT on small-integer data (every case's headroom is asserted while it is generated), the fused
weight gradient within a derived first-order rounding bound of float64 on real-valued data.  Everything goes through the C ABI in
tests/conv_ref.Arenas allocations: inputs frozen, outputs and the workspace -- exactly as long as promised -- poisoned, guards
checked after every launch.  Comparisons are equality of fp32 bit patterns (any NaN equals any NaN); a pooled output may
legitimately BE NaN, so "written" means: no element still holds the arena's poison word.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import stem_ref as sr
from tests import util

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3                       # DL_ERR_INVALID_ARGUMENT, DL_ERR_UNSUPPORTED
F32_POISON = cr._as_i32(cr.NAN_WORD[torch.float32])


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


class Bufs:
    def __init__(self, dev, skew=0):
        self.A, self.W = cr.Arenas(dev, skew), cr.Arenas(dev, 0)       # (the workspace is never skewed)

    def inp(self, arr, dtype=torch.float32, name=""):
        t = torch.from_numpy(np.ascontiguousarray(arr))
        return self.A.arena(tuple(t.shape), dtype, t, name)

    def out(self, shape, dtype=torch.float32, name=""):
        return self.A.arena(shape, dtype, None, name)

    def ws(self, nbytes):
        assert nbytes > 0 and nbytes % 4 == 0
        return self.W.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)

    def done(self, what, *outs):
        """After a launch: no device error, guards and inputs intact, every element of the outputs written."""
        _sync()
        self.A.check(what)
        self.W.check(what)
        for o in outs:
            if o.dtype == torch.float32:
                left = int((o.view(torch.int32) == F32_POISON).sum())
                assert left == 0, f"{what}: {left} elements were never written"

    def untouched(self, what, *outs):
        _sync()
        self.A.check(what)
        self.W.check(what)
        for o in outs:
            words = o.view(torch.int32) if o.dtype == torch.float32 else o.view(-1).view(torch.int32)
            assert int((words != F32_POISON).sum()) == 0, f"{what}: a refused call wrote to an output"


# ====================================================================================================== pooling forward


@pytest.mark.parametrize("special", [False, True], ids=["plain", "specials"])
@pytest.mark.parametrize("case", sr.POOL_CASES, ids=_ids(sr.POOL_CASES))
def test_pool_forward(case, special):
    """y and win of every map -- integers with ties everywhere, and with planted windows of -inf, +inf, both zeros in both orders and
    one to three NaNs at the seam columns and the edge rows -- equal the reference that tests/test_stem_ref_host.py pins to torch."""
    dev = _dev()
    L, lib = _lib()
    N, H, Wc, C = case
    bad = 0
    for act in sr.ACTS:
        a, _, _ = sr.pool_case_data(case, act, special)
        y_ref, win_ref = sr.pool_fwd_ref(a)
        b = Bufs(dev)
        a_d = b.inp(a, name="a")
        y_d, win_d = b.out(y_ref.shape, name="y"), b.out(y_ref.shape, torch.int8, "win")
        L.check(lib.dl_pool3x3s12_nhwc_fwd(_p(a_d), N, H, Wc, C, _p(y_d), _p(win_d), _stream()), "dl_pool3x3s12_nhwc_fwd")
        b.done(f"pool forward {case}", y_d)
        win = win_d.cpu().numpy()
        assert win.min() >= 0 and win.max() <= 8, "a window position outside 0..8 (an element of win never written)"
        bad += sr.bits_differ(y_d, y_ref, f"pooled output {case} act {act}")
        nw = int((win != win_ref).sum())
        if nw:
            print(f"win {case} act {act}: {nw} positions differ, first at {np.argwhere(win != win_ref)[:8].tolist()}")
        bad += nw
    util.measured(f"stem exact pool forward {case}{' specials' if special else ''}: elements of y and win that differ", bad, bound=0)


# ====================================================================================================== pooling backward


def _with_negative_zeros(a):
    """Every third zero of the map becomes -0.0: relu' (a > 0 in the header, a <= 0 ? 0 : 1 in the kernel) and 1 - a^2 do not
    see the sign.  Non-finite a is outside the backward's contract (include/delora_hip.h)."""
    a = a.copy()
    z = np.flatnonzero(a == 0)[::3]
    a.reshape(-1)[z] = -0.0
    return a


@pytest.mark.parametrize("case", sr.POOL_CASES, ids=_ids(sr.POOL_CASES))
def test_pool_backward(case):
    """dl_pool3x3s12_nhwc_bwd as a kernel, act none / tanh / relu, with the forward's positions and with positions drawn uniformly
    from the valid ones (the backward is a pure function of win): g_conv equals the float64 scatter; gradient crosses the wrap and
    reaches both edge rows (counted); garbage in g at windows that did not select an element changes no bit of it."""
    dev = _dev()
    L, lib = _lib()
    N, H, Wc, C = case
    bad, seam = 0, {}
    for act in sr.ACTS:
        a, g, wu = sr.pool_case_data(case, act)
        a = _with_negative_zeros(a)
        for wname, win in (("forward", sr.pool_fwd_ref(a)[1]), ("uniform", wu)):
            counts = sr.seam_counts(g, win)
            assert all(v > 0 for v in counts.values()), (case, act, wname, counts)
            for k, v in counts.items():
                seam[k] = seam.get(k, 0) + v
            ref = sr.pool_bwd_ref(g, a, win, act)
            # garbage at a quarter of the (window, channel) pairs; the elements none of those selected must not change
            g2, clean = sr.garbage(g, a.shape, win, 1 + act + 10 * len(wname))
            b = Bufs(dev)
            a_d, win_d = b.inp(a, name="a"), b.inp(win, torch.int8, "win")
            outs = []
            for gi, tag in ((g, "g"), (g2, "g with garbage")):
                g_d = b.inp(gi, name=tag)
                o = b.out(a.shape, name="g_conv")
                L.check(lib.dl_pool3x3s12_nhwc_bwd(_p(g_d), _p(a_d), _p(win_d), N, H, Wc, C, act, _p(o), _stream()), "dl_pool3x3s12_nhwc_bwd")
                b.done(f"pool backward {case} act {act} win {wname} {tag}", o)
                outs.append(o.cpu())
            bad += sr.bits_differ(outs[0], ref, f"pool backward {case} act {act} win {wname}")
            m = torch.from_numpy(clean)
            leaked = int((outs[0].view(torch.int32)[m] != outs[1].view(torch.int32)[m]).sum())
            if leaked:
                print(f"pool backward {case} act {act} win {wname}: garbage reached {leaked} elements that no garbage window selected")
            bad += leaked
    for k, v in seam.items():
        util.measured(f"stem exact pool backward {case}: gradients routed to [{k}]", v)
    util.measured(f"stem exact pool backward {case}: elements that differ", bad, bound=0)


# ====================================================================================================== fused weight gradient


def _wgrad_launch(L, lib, b, c, g_d, a_d, win_d, x8_d):
    nbytes = int(lib.dl_stem_wgrad_workspace_bytes(c["N"], c["H"], c["W"]))
    assert nbytes == sr.workspace_bytes(c["N"], c["H"], c["W"])
    ws, dw = b.ws(nbytes), b.A.arena((64, 8, 3, 3), torch.float32, None, "dw", 0)
    L.check(lib.dl_stem_wgrad_f32(_p(g_d), _p(a_d), _p(win_d), _p(x8_d), c["N"], c["H"], c["W"], c["act"], _p(ws), _p(dw), _stream()),
            "dl_stem_wgrad_f32")
    b.done(f"stem wgrad {(c['N'], c['H'], c['W'])} act {c['act']}", dw)
    return dw


def _run_wgrad_case(case, act, skew=0):
    dev = _dev()
    L, lib = _lib()
    c = sr.wgrad_case(*case, act)                           # (asserts the headroom)
    N, H, W = case
    ref = sr.stem_wgrad_ref(c["g"], c["a"], c["win"], c["x8"], act)
    b = Bufs(dev, skew)
    g_d, a_d, win_d, x8_d = b.inp(c["g"], name="g pooled"), b.inp(c["a"], name="a"), b.inp(c["win"], torch.int8, "win"), b.inp(c["x8"], name="x8")
    dw1 = _wgrad_launch(L, lib, b, c, g_d, a_d, win_d, x8_d)
    dw2 = _wgrad_launch(L, lib, b, c, g_d, a_d, win_d, x8_d)
    tag = f"stem wgrad {case} act {sr.ACT_NAME[act]}"
    bad = sr.bits_differ(dw1, ref, tag)
    assert torch.equal(dw1.view(torch.int32), dw2.view(torch.int32)), f"{tag}: two runs differ"
    # the unfused route: the pooling backward as a kernel, its map through float64 autograd of conv1
    gc = b.out(c["a"].shape, name="g_conv")
    L.check(lib.dl_pool3x3s12_nhwc_bwd(_p(g_d), _p(a_d), _p(win_d), N, H, W // 2, 64, act, _p(gc), _stream()), "dl_pool3x3s12_nhwc_bwd")
    b.done(tag + " unfused", gc)
    x8 = torch.from_numpy(c["x8"])
    unfused = cr.conv_grads(x8, torch.zeros((64, 3, 3, 8), dtype=torch.float64), gc.cpu().double(), (1, 2))[1].permute(0, 3, 1, 2).contiguous()
    bad += sr.bits_differ(dw1, unfused, tag + ": fused against unfused")
    return bad


WGRAD_PARAMS = [(c, act) for c in sr.WGRAD_CASES for act in sr.ACTS]


@pytest.mark.parametrize("case,act", WGRAD_PARAMS, ids=[f"{'x'.join(map(str, c))}-{sr.ACT_NAME[a]}" for c, a in WGRAD_PARAMS])
def test_stem_wgrad(case, act):
    """dw of the fused launch equals float64 autograd, twice the same bits, and equals the unfused route (dl_pool3x3s12_nhwc_bwd, then
    float64 autograd of conv1)."""
    bad = _run_wgrad_case(case, act)
    util.measured(f"stem exact wgrad {case} act {sr.ACT_NAME[act]}: elements that differ from float64", bad, bound=0)


@pytest.mark.parametrize("act", sr.ACTS, ids=[sr.ACT_NAME[a] for a in sr.ACTS])
def test_stem_wgrad_minimum_documented_alignment(act):
    """Every base 16 bytes past a 256-byte boundary."""
    bad = _run_wgrad_case(sr.SKEW_CASE, act, skew=16)
    util.measured(f"stem exact wgrad {sr.SKEW_CASE} act {sr.ACT_NAME[act]}, bases 16 bytes past a 256-byte boundary: elements that differ", bad, bound=0)


def test_the_cases_cover_the_slab_walk_and_both_reduction_loops():
    """plan() of every case: chunks per slab 1, 2 and 3, every grid % 4, a grid below 29, one in 29..32, one above 60, grid < nslabs,
    a short last slab -- and the table itself, literally, and the library's workspace size."""
    _dev()
    _, lib = _lib()
    for case, (chunks, cps, grid) in sr.WGRAD_PLAN.items():
        p = sr.plan(*case)
        assert (p[0], p[2], p[3]) == (chunks, cps, grid), (case, p)
        assert int(lib.dl_stem_wgrad_workspace_bytes(*case)) == p[1] * 64 * 72 * 4
    missing = sr.coverage()
    assert not missing, missing


def test_refusals_leave_the_outputs_untouched():
    dev = _dev()
    _, lib = _lib()
    N, H, Wc, C = 1, 2, 4, 8
    b = Bufs(dev)
    a, g, win = np.ones((N, H, Wc, C)), np.ones((N, H, Wc // 2, C)), np.full((N, H, Wc // 2, C), 4, dtype=np.int8)
    a_d, g_d, win_d = b.inp(a, name="a"), b.inp(g, name="g"), b.inp(win, torch.int8, "win")
    y_d, wo_d, gc_d = b.out(g.shape, name="y"), b.out(g.shape, torch.int8, "win out"), b.out(a.shape, name="g_conv")
    fwd, bwd = lib.dl_pool3x3s12_nhwc_fwd, lib.dl_pool3x3s12_nhwc_bwd
    st = _stream()
    assert fwd(_p(a_d), N, H, 3, C, _p(y_d), _p(wo_d), st) == UNSUPPORTED                       # odd width
    assert fwd(_p(a_d), N, H, Wc, 6, _p(y_d), _p(wo_d), st) == UNSUPPORTED                      # C % 4
    assert fwd(None, N, H, Wc, C, _p(y_d), _p(wo_d), st) == INVALID
    assert fwd(_p(a_d), N, H, Wc, C, None, _p(wo_d), st) == INVALID
    assert fwd(_p(a_d), N, H, Wc, C, _p(y_d), None, st) == INVALID
    assert fwd(_p(a_d), 0, H, Wc, C, _p(y_d), _p(wo_d), st) == INVALID
    assert bwd(_p(g_d), _p(a_d), _p(win_d), N, H, 3, C, 0, _p(gc_d), st) == UNSUPPORTED
    assert bwd(_p(g_d), _p(a_d), _p(win_d), N, H, Wc, 6, 0, _p(gc_d), st) == UNSUPPORTED
    assert bwd(_p(g_d), _p(a_d), _p(win_d), N, H, Wc, C, 3, _p(gc_d), st) == INVALID             # bad act
    assert bwd(_p(g_d), _p(a_d), _p(win_d), N, H, Wc, C, -1, _p(gc_d), st) == INVALID
    assert bwd(_p(g_d), _p(a_d), _p(win_d), N, H, Wc, C, 0, None, st) == INVALID
    assert bwd(None, _p(a_d), _p(win_d), N, H, Wc, C, 0, _p(gc_d), st) == INVALID
    b.untouched("pooling refusals", y_d, wo_d, gc_d)
    # the fused weight gradient: W % 4 != 0 has no workspace size and is refused; NULL pointers and a bad act are invalid arguments
    c = sr.wgrad_case(1, 2, 8, sr.RELU)
    g_d, a_d, win_d, x8_d = b.inp(c["g"], name="g pooled"), b.inp(c["a"], name="a"), b.inp(c["win"], torch.int8, "win"), b.inp(c["x8"], name="x8")
    ws, dw = b.ws(int(lib.dl_stem_wgrad_workspace_bytes(1, 2, 8))), b.A.arena((64, 8, 3, 3), torch.float32, None, "dw", 0)
    wg = lib.dl_stem_wgrad_f32
    for W in (6, 10, 7):
        assert int(lib.dl_stem_wgrad_workspace_bytes(1, 2, W)) == 0
        assert wg(_p(g_d), _p(a_d), _p(win_d), _p(x8_d), 1, 2, W, sr.RELU, _p(ws), _p(dw), st) == UNSUPPORTED
    args = [_p(g_d), _p(a_d), _p(win_d), _p(x8_d), 1, 2, 8, sr.RELU, _p(ws), _p(dw), st]
    for i in (0, 1, 2, 3, 8, 9):
        assert wg(*[None if k == i else v for k, v in enumerate(args)]) == INVALID, i
    for act in (-1, 3):
        assert wg(*[act if k == 7 else v for k, v in enumerate(args)]) == INVALID
    assert wg(*[0 if k == 4 else v for k, v in enumerate(args)]) == INVALID
    b.untouched("weight-gradient refusals", dw, ws)


# ====================================================================================================== float64 tier

REAL_PARAMS = [(s, act) for s in sr.REAL_SHAPES for act in sr.ACTS]


@pytest.mark.parametrize("shape,act", REAL_PARAMS, ids=[f"{'x'.join(map(str, c))}-{sr.ACT_NAME[a]}" for c, a in REAL_PARAMS])
def test_stem_wgrad_float64(shape, act):
    """Real-valued data: Gaussian x8 * 3 and g, a from the library's own conv1 with the activation, win from its pooling.  Per element
    |dw - float64| <= c 2^-24 S_abs, S_abs the float64 sum of |g_c| |x| and c the count of rounded operations read from the code
    (stem_ref.op_count; the host emulation passes it at about 0.01).  The pooled map of the real data equals the reference too."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = shape
    x8, g, w = sr.real_inputs(N, H, W, 77 + W)
    b = Bufs(dev)
    x8_d, g_d, w_d = b.inp(x8, name="x8"), b.inp(g, name="g pooled"), b.A.arena(w.shape, torch.float32, torch.from_numpy(w), "w", 0)
    a_d = b.out((N, H, W // 2, 64), name="a")
    L.check(lib.dl_conv2d_nhwc_f32(_p(x8_d), _p(w_d), _p(a_d), None, None, N, H, W, 8, 64, 3, 1, 2, 0, act, cr.EPI_ACT if act else 0, _stream()),
            "dl_conv2d_nhwc_f32")
    b.done(f"conv1 {shape}", a_d)
    b.A.freeze(a_d)
    y_d, win_d = b.out((N, H, W // 4, 64), name="y"), b.out((N, H, W // 4, 64), torch.int8, "win")
    L.check(lib.dl_pool3x3s12_nhwc_fwd(_p(a_d), N, H, W // 2, 64, _p(y_d), _p(win_d), _stream()), "dl_pool3x3s12_nhwc_fwd")
    b.done(f"pool forward {shape}", y_d)
    b.A.freeze(win_d)
    a, win = a_d.cpu().numpy(), win_d.cpu().numpy()
    assert np.abs(a).max() < (0.995 if act == sr.TANH else 1e3)
    y_ref, win_ref = sr.pool_fwd_ref(a)
    assert sr.bits_differ(y_d, y_ref, f"pooled output {shape}") == 0 and np.array_equal(win, win_ref)
    c = {"N": N, "H": H, "W": W, "act": act}
    dw = _wgrad_launch(L, lib, b, c, g_d, a_d, win_d, x8_d).cpu().numpy().astype(np.float64)
    ref, bound = sr.stem_wgrad_ref(g, a, win, x8, act), sr.wgrad_bound(g, a, win, x8, act)
    assert bound.min() > 0
    util.measured(f"stem wgrad float64 {shape} act {sr.ACT_NAME[act]}: worst error / bound (c = {sr.op_count(N, H, W, act)})",
                  float((np.abs(dw - ref) / bound).max()), bound=1.0)
