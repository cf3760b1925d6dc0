"""The ring ops (csrc/ringops.hip) through the C ABI against the references of tests/ring_ref.py, BIT FOR BIT: [residual add] +
activation + wrap-around padding forward and backward in fp32 / fp16 / bf16 for every residual layout (a foreign pitch and offset
among them), the stem's activation + wrapped max-pooling + padding forward (``out`` AND ``win``) and backward in the three storage
types, the even-width fast path against the general kernels on the same data (the pointer the dispatch looks at is 8-byte aligned
in one run and 4 bytes off in the other), the adversarial near-tie windows of ``ring_ref.near_ties``, the rounding specials, and the
argument checks.

Every buffer is a view inside a tests/conv_ref.Arenas allocation: inputs frozen, outputs poisoned and exactly as long as promised,
guards checked after every launch; a device error ends the session.  Comparisons are equality of bit patterns (any NaN equals any
NaN, -0.0 differs from +0.0).  tanh itself is the device's ``tanhf``: its distance to float64 is measured against the bound of
tests/test_gpu_ringops.py (2e-7 absolute), and everything downstream of it is compared on the device's own activation values.

Not executed here: the ``uint64_t`` index instantiations of ``k_ring_act_pad_fwd`` / ``_bwd``.  The smallest tensor that reaches them
has 2^31 elements (4 GiB per buffer in half precision); the largest activation of the bench workload has 2^26.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import ring_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

OK, INVALID = 0, -1
TANH_ATOL = 2e-7                                    # tests/test_gpu_ringops.py


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


def _poison_left(v):
    """Elements of an output view that still hold the arena's poison pattern (the view starts on a 4-byte boundary)."""
    word = cr.NAN_WORD[v.dtype]
    flat = v.reshape(-1)
    if flat.element_size() == 4:
        return int((flat.view(torch.int32) == cr._as_i32(word)).sum())
    if flat.element_size() == 2:
        half = word & 0xFFFF
        return int((flat.view(torch.int16) == (half - (1 << 16) if half >= (1 << 15) else half)).sum())
    pat = torch.tensor([((word >> (8 * k)) & 0xFF) for k in range(4)], dtype=torch.uint8, device=v.device)
    return int((flat.view(torch.uint8) == pat.repeat(flat.numel() // 4 + 1)[:flat.numel()]).sum())


class Bufs:
    """Two arenas: ``K`` holds the pointer the stem's dispatch looks at (x of a forward, grad_x of a backward) with the skew under test,
    ``A`` everything else, never skewed."""

    def __init__(self, dev, skew=0):
        self.K, self.A = cr.Arenas(dev, skew), cr.Arenas(dev, 0)

    def inp(self, arr, storage=torch.float32, name="", key=False):
        t = arr if isinstance(arr, torch.Tensor) else (torch.from_numpy(np.ascontiguousarray(arr)) if storage == torch.int8 else rr.to_storage(arr, storage))
        return (self.K if key else self.A).arena(tuple(t.shape), storage, t, name, row_elems=0)

    def out(self, shape, storage=torch.float32, name="", key=False):
        return (self.K if key else self.A).arena(shape, storage, None, name, row_elems=0)

    def done(self, what, *outs):
        """After a launch: no device error, guards and inputs intact, every element of the outputs written."""
        _sync()
        self.K.check(what)
        self.A.check(what)
        for o in outs:
            left = _poison_left(o)
            assert left == 0, f"{what}: {left} elements were never written"

    def untouched(self, what, *outs):
        _sync()
        self.K.check(what)
        self.A.check(what)
        for o in outs:
            assert _poison_left(o) == o.numel(), f"{what}: a call that must not launch wrote to an output"


def _f32(t):
    return t.detach().float().cpu().numpy()


# ====================================================================================================== act + pad


def _res_buffer(r2d, lay):
    """Flat residual memory of a layout: row r's W values at r * pitch + off, NaN everywhere else; exactly as long as the last row needs."""
    rows, W = r2d.shape
    pitch, off = lay
    flat = np.full((rows - 1) * pitch + off + W, np.nan, dtype=np.float32)
    for r in range(rows):
        flat[r * pitch + off:r * pitch + off + W] = r2d[r]
    return flat


def _act_pad_fwd(L, lib, b, x, flat, lay, rows, W, pad, act, storage, what):
    x_d = b.inp(x, storage, "x")
    r_d = b.inp(flat, storage, "res") if flat is not None else None
    o_d = b.out((rows, W + 2 * pad), storage, "out")
    pitch, off = lay or (0, 0)
    L.check(lib.dl_ring_act_pad_fwd_t(_p(x_d), _p(r_d), pitch, off, rows, W, pad, act, cr.DTYPE_CODE[storage], _p(o_d), _stream()), "dl_ring_act_pad_fwd_t")
    b.done(what, o_d)
    return _f32(o_d)


@pytest.mark.parametrize("storage", rr.STORAGES, ids=[rr.ST_NAME[s] for s in rr.STORAGES])
@pytest.mark.parametrize("shape", rr.PAD_SHAPES, ids=_ids(rr.PAD_SHAPES))
def test_act_pad_forward(shape, storage):
    """none and relu on integers: out equals the reference bit for bit for every residual layout and pad.  tanh on multiples of 1/8:
    the fp32 interior IS the device's tanhf (measured against float64, bound 2e-7), its wrap columns are copies, and the half-precision
    output is that fp32 value rounded once."""
    dev = _dev()
    L, lib = _lib()
    rows, W = shape
    bad, worst = 0, 0.0
    for kind in rr.RES_KINDS:
        lay = rr.res_layout(kind, W)
        for pad in (0, 1):
            for act in rr.ACTS:
                sd = 9000 + 100 * rows + W + 7 * act + pad + 31 * len(kind)
                scale = 0.125 if act == rr.TANH else 1.0
                x = (rr.ints((rows, W), 3 if act != rr.TANH else 24, sd).numpy() * scale).astype(np.float32)
                flat = None
                if lay is not None:
                    flat = _res_buffer((rr.ints((rows, W), 3 if act != rr.TANH else 24, sd + 1).numpy() * scale).astype(np.float32), lay)
                what = f"act_pad forward {shape} {rr.ST_NAME[storage]} res {kind} pad {pad} act {rr.ACT_NAME[act]}"
                activated = None
                if act == rr.TANH:
                    a_dev = _act_pad_fwd(L, lib, Bufs(dev), x, flat, lay, rows, W, 0, act, torch.float32, what + " (fp32 activations)")
                    host = rr.act_pad_fwd(x, flat, *(lay or (0, 0)), W, 0, act, torch.float32)
                    worst = max(worst, float(np.abs(a_dev.astype(np.float64) - host.astype(np.float64)).max()))
                    activated = a_dev
                got = _act_pad_fwd(L, lib, Bufs(dev), x, flat, lay, rows, W, pad, act, storage, what)
                bad += rr.bits_differ(got, rr.act_pad_fwd(x, flat, *(lay or (0, 0)), W, pad, act, storage, activated=activated), what)
    util.measured(f"ring exact act_pad forward {shape} {rr.ST_NAME[storage]}: device tanhf against float64 tanh rounded to fp32 (absolute)", worst, bound=TANH_ATOL)
    util.measured(f"ring exact act_pad forward {shape} {rr.ST_NAME[storage]}: elements that differ", bad, bound=0)


@pytest.mark.parametrize("storage", rr.STORAGES, ids=[rr.ST_NAME[s] for s in rr.STORAGES])
@pytest.mark.parametrize("shape", rr.PAD_SHAPES, ids=_ids(rr.PAD_SHAPES))
def test_act_pad_backward(shape, storage):
    """grad_x for every activation and pad on integer gradients and grid-valued saved outputs (1 - y^2 exact), with and without
    grad_res_padded: the same grad_x both times, grad_res_padded = grad_x between two columns of +0.0.  Under relu a dead unit (y <= 0)
    gives +0.0 for any gradient, infinite and NaN ones included."""
    dev = _dev()
    L, lib = _lib()
    rows, W = shape
    gmax = rr.GMAX[storage]
    bad = 0
    for pad in (0, 1):
        for act in rr.ACTS:
            rr.headroom(gmax, act, windows=1)
            sd = 9500 + 100 * rows + W + 7 * act + pad
            g, y = rr.ints((rows, W + 2 * pad), gmax, sd).numpy(), rr.saved((rows, W + 2 * pad), act, sd + 1)
            if act == rr.RELU:                              # infinite and NaN gradients at dead units: +0.0 comes out
                g = rr.dead_garbage(g, y, pad + 1, pad + W - 1)
            ref_gx, ref_gr = rr.act_pad_bwd(g, y, W, pad, act, storage, with_res=True)
            for with_res in (False, True):
                what = f"act_pad backward {shape} {rr.ST_NAME[storage]} pad {pad} act {rr.ACT_NAME[act]} grad_res {with_res}"
                b = Bufs(dev)
                g_d, y_d = b.inp(g, storage, "grad_out"), b.inp(y, storage, "y")
                gx_d = b.out((rows, W), storage, "grad_x")
                gr_d = b.out((rows, W + 2), storage, "grad_res_padded") if with_res else None
                L.check(lib.dl_ring_act_pad_bwd_t(_p(g_d), _p(y_d), rows, W, pad, act, cr.DTYPE_CODE[storage], _p(gx_d), _p(gr_d), _stream()), "dl_ring_act_pad_bwd_t")
                b.done(what, *([gx_d, gr_d] if with_res else [gx_d]))
                bad += rr.bits_differ(_f32(gx_d), ref_gx, what)
                if with_res:
                    bad += rr.bits_differ(_f32(gr_d), ref_gr, what + ": grad_res_padded")
    util.measured(f"ring exact act_pad backward {shape} {rr.ST_NAME[storage]}: elements that differ", bad, bound=0)


def test_fp32_entry_points_are_the_typed_ones_with_dtype_0():
    dev = _dev()
    L, lib = _lib()
    rows, W = 5, 7
    x, r2d = rr.ints((rows, W), 3, 1).numpy().astype(np.float32), rr.ints((rows, W), 3, 2).numpy().astype(np.float32)
    lay = rr.res_layout("foreign", W)
    flat = _res_buffer(r2d, lay)
    b = Bufs(dev)
    x_d, r_d, o_d = b.inp(x, name="x"), b.inp(flat, name="res"), b.out((rows, W + 2), name="out")
    L.check(lib.dl_ring_act_pad_fwd(_p(x_d), _p(r_d), lay[0], lay[1], rows, W, 1, rr.RELU, _p(o_d), _stream()), "dl_ring_act_pad_fwd")
    b.done("dl_ring_act_pad_fwd", o_d)
    out = _f32(o_d)
    assert rr.bits_differ(out, rr.act_pad_fwd(x, flat, *lay, W, 1, rr.RELU, torch.float32), "dl_ring_act_pad_fwd") == 0
    g = rr.ints((rows, W + 2), 3, 3).numpy()
    g_d, y_d, gx_d, gr_d = b.inp(g, name="grad_out"), b.inp(out, name="y"), b.out((rows, W), name="grad_x"), b.out((rows, W + 2), name="grad_res_padded")
    L.check(lib.dl_ring_act_pad_bwd(_p(g_d), _p(y_d), rows, W, 1, rr.RELU, _p(gx_d), _p(gr_d), _stream()), "dl_ring_act_pad_bwd")
    b.done("dl_ring_act_pad_bwd", gx_d, gr_d)
    ref_gx, ref_gr = rr.act_pad_bwd(g, out, W, 1, rr.RELU, torch.float32, with_res=True)
    assert rr.bits_differ(_f32(gx_d), ref_gx, "dl_ring_act_pad_bwd") == 0 and rr.bits_differ(_f32(gr_d), ref_gr, "grad_res_padded") == 0


@pytest.mark.parametrize("storage", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_rounding_specials_through_the_residual_add(storage):
    """act none, x + res in fp32, ONE rounding to the storage type: half-way sums to the even neighbour in both directions, just above
    and below half-way, overflow to either infinity, NaN, inf - inf, every pairing of the zeros, subnormal sums."""
    dev = _dev()
    L, lib = _lib()
    x, res = rr.specials(storage)
    n = len(x)
    bad = 0
    for rows, W in ((1, n), (n, 1)):
        lay = (W + 5, 3)
        flat = _res_buffer(res.reshape(rows, W), lay)
        for pad in (0, 1):
            what = f"specials {rr.ST_NAME[storage]} as {rows}x{W} pad {pad}"
            got = _act_pad_fwd(L, lib, Bufs(dev), x.reshape(rows, W), flat, lay, rows, W, pad, rr.NONE, storage, what)
            bad += rr.bits_differ(got, rr.act_pad_fwd(x.reshape(rows, W), flat, *lay, W, pad, rr.NONE, storage), what)
    util.measured(f"ring exact rounding specials {rr.ST_NAME[storage]}: elements that differ", bad, bound=0)


# ====================================================================================================== stem


def _window(x, H, W, r, wo):
    h = r % H
    return [float(x[r + dh, (2 * wo + dw) % W]) if 0 <= h + dh < H else None for dh in (-1, 0, 1) for dw in (-1, 0, 1)]


def _report_win(tag, win, ref, x, a, H, W):
    bad = np.argwhere(win != ref)
    if len(bad):
        print(f"{tag}: {len(bad)} positions of win differ")
        for r, wo in bad[:6].tolist():
            print(f"    row {r} (h = {r % H}) pooled column {wo}: got {int(win[r, wo])}, expected {int(ref[r, wo])}\n"
                  f"        window x = {[None if v is None else float(v).hex() for v in _window(x, H, W, r, wo)]}\n"
                  f"        activated = {[None if v is None else float(v).hex() for v in _window(a, H, W, r, wo)]}")
    return len(bad)


def _stem_fwd(L, lib, b, x, planes, H, W, act, storage, what):
    Wo = rr.out_width(W)
    x_d = b.inp(x, storage, "x", key=True)
    o_d, w_d = b.out((planes * H, Wo + 2), storage, "out"), b.out((planes * H, Wo), torch.int8, "win")
    if storage == torch.float32:
        rc = lib.dl_ring_act_pool_pad_fwd(_p(x_d), planes, H, W, act, _p(o_d), _p(w_d), _stream())
    else:
        rc = lib.dl_ring_act_pool_pad_fwd_t(_p(x_d), planes, H, W, act, cr.DTYPE_CODE[storage], _p(o_d), _p(w_d), _stream())
    L.check(rc, "dl_ring_act_pool_pad_fwd")
    b.done(what, o_d, w_d)
    win = w_d.cpu().numpy()
    assert win.min() >= 0 and win.max() <= 8, f"{what}: a window position outside 0..8"
    return _f32(o_d), win


def _stem_bwd(L, lib, b, g, y, win, planes, H, W, act, storage, what):
    g_d, y_d, w_d = b.inp(g, storage, "grad_out"), b.inp(y, storage, "y"), b.inp(win.astype(np.int8), torch.int8, "win")
    gx_d = b.out((planes * H, W), storage, "grad_x", key=True)
    if storage == torch.float32:
        rc = lib.dl_ring_act_pool_pad_bwd(_p(g_d), _p(y_d), _p(w_d), planes, H, W, act, _p(gx_d), _stream())
    else:
        rc = lib.dl_ring_act_pool_pad_bwd_t(_p(g_d), _p(y_d), _p(w_d), planes, H, W, act, cr.DTYPE_CODE[storage], _p(gx_d), _stream())
    L.check(rc, "dl_ring_act_pool_pad_bwd")
    b.done(what, gx_d)
    return _f32(gx_d)


def _device_activations(L, lib, dev, x, rows, W, act, storage):
    """act(x) as the library's own element-wise kernel stores it (pad 0, no residual): the values the stem's arg-max compares."""
    return _act_pad_fwd(L, lib, Bufs(dev), x, None, None, rows, W, 0, act, storage, f"activations {rows}x{W} act {act}")


STEM_DATA = (("ints", rr.NONE, rr.NONE), ("ints", rr.TANH, rr.TANH), ("ints", rr.RELU, rr.RELU),
             ("near", rr.NONE, rr.TANH), ("near", rr.TANH, rr.TANH), ("near", rr.RELU, rr.RELU))     # (kind, act, whose near_ties)
ALL_STEM = rr.STEM_EVEN + rr.STEM_ODD


@pytest.mark.parametrize("case", ALL_STEM, ids=_ids(ALL_STEM))
def test_stem_fp32_fast_and_general_kernels(case):
    """Per data set (integers with ties everywhere under each activation; the near-tie windows under none, tanh and relu):
      1. out and win of the run with x 8-byte aligned (even W: the fast kernel) equal those of the run with x 4 bytes off (the general
         kernel), bit for bit;
      2. both equal ring_ref.pool_fwd of the device's own activations, which for none and relu equal the host's;
      3. the backward with the reference's win, grid-valued y and integer g equals ring_ref.pool_bwd on both dispatches (selected by
         grad_x), and again with the forward's own win."""
    dev = _dev()
    L, lib = _lib()
    planes, H, W = case
    rows, Wo = planes * H, rr.out_width(W)
    skews = (0, 4) if W % 2 == 0 else (0,)
    bad_fwd, bad_pair, bad_bwd, bad_act = 0, 0, 0, 0
    for kind, act, whose in STEM_DATA:
        x, _ = rr.stem_inputs(planes, H, W, whose if kind == "near" else act, kind)
        tag = f"stem {case} {kind} act {rr.ACT_NAME[act]}"
        a_dev = _device_activations(L, lib, dev, x, rows, W, act, torch.float32)
        if act != rr.TANH:
            bad_act += rr.bits_differ(a_dev, rr.act_host(x, act).astype(np.float32), tag + ": device activations against the host's")
        ref_out, ref_win = rr.pool_fwd(a_dev, H, W)
        runs = []
        for skew in skews:
            what = f"{tag} x {'aligned' if skew == 0 else 'skewed by 4 bytes'}"
            out, win = _stem_fwd(L, lib, Bufs(dev, skew), x, planes, H, W, act, torch.float32, what)
            bad_fwd += rr.bits_differ(out, ref_out, what + ": out") + _report_win(what, win, ref_win, x, a_dev, H, W)
            runs.append((out, win))
        if len(runs) == 2:
            n = rr.bits_differ(runs[0][0], runs[1][0], tag + ": out, aligned against skewed") + _report_win(tag + ": aligned (got) against skewed (expected)", runs[0][1], runs[1][1], x, a_dev, H, W)
            if kind == "near":
                util.measured(f"ring exact {tag}: elements of out and win on which the fast and the general kernel disagree", n)
            bad_pair += n
        # backward
        rr.headroom(2, act)
        sd = rr.stem_case_seed(planes, H, W, act) + (5 if kind == "near" else 0)
        g, y = rr.ints((rows, Wo + 2), 2, sd + 2).numpy(), rr.saved((rows, Wo + 2), act, sd + 3)
        if act == rr.RELU:                                  # infinite and NaN gradients at windows whose pooled value is <= 0: nothing arrives
            g = rr.dead_garbage(g, y, 2, Wo)
        wins = [("reference win", ref_win)]
        if not np.array_equal(runs[0][1], ref_win):
            wins.append(("the forward's own win", runs[0][1]))      # (equal otherwise: the loop is closed by the first entry)
        for wname, win in wins:
            ref_gx = rr.pool_bwd(g, y, win, H, W, act)
            for skew in skews:
                what = f"{tag} backward, {wname}, grad_x {'aligned' if skew == 0 else 'skewed by 4 bytes'}"
                bad_bwd += rr.bits_differ(_stem_bwd(L, lib, Bufs(dev, skew), g, y, win, planes, H, W, act, torch.float32, what), ref_gx, what)
    util.measured(f"ring exact stem {case}: device activations that differ from the host's (none, relu)", bad_act, bound=0)
    util.measured(f"ring exact stem {case}: elements of out and win that differ from the reference", bad_fwd, bound=0)
    util.measured(f"ring exact stem {case}: elements on which the aligned and the skewed run differ", bad_pair, bound=0)
    util.measured(f"ring exact stem {case}: elements of grad_x that differ", bad_bwd, bound=0)


def test_stem_backward_closes_the_loop_with_the_forwards_own_win():
    """Forward on the device, its win handed to the backward untouched (device to device), y = its own out: equals the reference chain."""
    dev = _dev()
    L, lib = _lib()
    planes, H, W = 2, 7, 34
    rows, Wo = planes * H, rr.out_width(W)
    bad = 0
    for act in (rr.NONE, rr.RELU):
        x, _ = rr.stem_inputs(planes, H, W, act, "ints")
        for skew in (0, 4):
            b = Bufs(dev, skew)
            x_d = b.inp(x, name="x", key=True)
            o_d, w_d = b.out((rows, Wo + 2), name="out"), b.out((rows, Wo), torch.int8, "win")
            L.check(lib.dl_ring_act_pool_pad_fwd(_p(x_d), planes, H, W, act, _p(o_d), _p(w_d), _stream()), "dl_ring_act_pool_pad_fwd")
            b.done("loop forward", o_d, w_d)
            b.A.freeze(o_d), b.A.freeze(w_d)
            g = rr.ints((rows, Wo + 2), 2, 77 + act).numpy()
            g_d, gx_d = b.inp(g, name="grad_out"), b.out((rows, W), name="grad_x", key=True)
            L.check(lib.dl_ring_act_pool_pad_bwd(_p(g_d), _p(o_d), _p(w_d), planes, H, W, act, _p(gx_d), _stream()), "dl_ring_act_pool_pad_bwd")
            b.done("loop backward", gx_d)
            out, win = rr.pool_fwd(rr.act_host(x, act), H, W)
            bad += rr.bits_differ(_f32(gx_d), rr.pool_bwd(g, out, win, H, W, act), f"loop act {act} skew {skew}")
    util.measured("ring exact stem loop (forward's win and out into the backward): elements that differ", bad, bound=0)


HALF_PARAMS = [(c, s) for c in rr.STEM_HALF for s in (torch.float16, torch.bfloat16)]


@pytest.mark.parametrize("case,storage", HALF_PARAMS, ids=[f"{'x'.join(map(str, c))}-{rr.ST_NAME[s]}" for c, s in HALF_PARAMS])
def test_stem_half_storage(case, storage):
    """fp16 / bf16: the arg-max runs on activations ROUNDED to the storage type, so distinct inputs tie (tanh of multiples of 1/8 up
    to 6).  out and win equal ring_ref.pool_fwd of the device's own stored activations; none and relu equal the host's as well; NaN
    inputs propagate; the backward is exact with one rounding."""
    dev = _dev()
    L, lib = _lib()
    planes, H, W = case
    rows, Wo = planes * H, rr.out_width(W)
    bad = 0
    for act in rr.ACTS:
        sd = rr.stem_case_seed(planes, H, W, act) + 11
        x = rr.half_stem_input(planes, H, W, act, sd)
        tag = f"stem {case} {rr.ST_NAME[storage]} act {rr.ACT_NAME[act]}"
        a_dev = _device_activations(L, lib, dev, x, rows, W, act, storage)
        if act != rr.TANH:
            bad += rr.bits_differ(a_dev, rr.act_host(x, act).astype(np.float32), tag + ": device activations")
        else:
            a32 = _device_activations(L, lib, dev, x, rows, W, act, torch.float32)
            bad += rr.bits_differ(a_dev, rr.round_to(a32, storage), tag + ": stored activation = the fp32 one rounded once")
        ref_out, ref_win = rr.pool_fwd(a_dev, H, W)
        out, win = _stem_fwd(L, lib, Bufs(dev), x, planes, H, W, act, storage, tag)
        bad += rr.bits_differ(out, ref_out, tag + ": out") + _report_win(tag, win, ref_win, x, a_dev, H, W)
        gmax = rr.GMAX[storage]
        rr.headroom(gmax, act)
        g, y = rr.ints((rows, Wo + 2), gmax, sd + 2).numpy(), rr.saved((rows, Wo + 2), act, sd + 3)
        what = tag + " backward"
        bad += rr.bits_differ(_stem_bwd(L, lib, Bufs(dev), g, y, ref_win, planes, H, W, act, storage, what), rr.pool_bwd(g, y, ref_win, H, W, act, storage), what)
    util.measured(f"ring exact stem {case} {rr.ST_NAME[storage]}: elements of out, win and grad_x that differ", bad, bound=0)


# ====================================================================================================== argument checks


def test_refusals_and_empty_tensors_write_nothing():
    """Null pointers, rows < 0, W <= 0 (W < 2 for the stem), pad 2, act 3 and -1, dtype 3 and -1, tensors past 2^40 / at 2^31 elements:
    the invalid-argument code, nothing launched.  rows = 0 and planes = 0: OK, nothing written."""
    dev = _dev()
    _, lib = _lib()
    rows, W = 3, 4
    st = _stream()
    b = Bufs(dev)
    ones = np.ones((rows, W + 2), dtype=np.float32)
    x_d, r_d, g_d = b.inp(ones[:, :W], name="x"), b.inp(ones[:, :W], name="res"), b.inp(ones, name="grad_out / y")
    o_d, gx_d, gr_d = b.out((rows, W + 2), name="out"), b.out((rows, W), name="grad_x"), b.out((rows, W + 2), name="grad_res_padded")
    fwd, bwd = lib.dl_ring_act_pad_fwd_t, lib.dl_ring_act_pad_bwd_t
    good_f = [_p(x_d), _p(r_d), W, 0, rows, W, 1, rr.RELU, 0, _p(o_d), st]
    for i, v in ((0, None), (9, None), (4, -1), (5, 0), (5, -3), (6, 2), (6, -1), (7, 3), (7, -1), (8, 3), (8, -1), (4, (1 << 40) + 1)):
        assert fwd(*[v if k == i else a for k, a in enumerate(good_f)]) == INVALID, ("forward", i, v)
    assert fwd(*[0 if k == 4 else a for k, a in enumerate(good_f)]) == OK
    good_b = [_p(g_d), _p(g_d), rows, W, 1, rr.RELU, 0, _p(gx_d), _p(gr_d), st]
    for i, v in ((0, None), (1, None), (7, None), (2, -1), (3, 0), (3, -3), (4, 2), (4, -1), (5, 3), (5, -1), (6, 3), (6, -1), (2, (1 << 40) + 1)):
        assert bwd(*[v if k == i else a for k, a in enumerate(good_b)]) == INVALID, ("backward", i, v)
    assert bwd(*[0 if k == 2 else a for k, a in enumerate(good_b)]) == OK
    assert lib.dl_ring_act_pad_fwd(None, None, 0, 0, rows, W, 1, 0, _p(o_d), st) == INVALID
    assert lib.dl_ring_act_pad_bwd(_p(g_d), _p(g_d), rows, W, 1, 0, None, None, st) == INVALID
    b.untouched("act_pad refusals", o_d, gx_d, gr_d)
    # the stem
    planes, H, W = 2, 3, 4
    Wo = rr.out_width(W)
    b = Bufs(dev)
    x_d = b.inp(np.ones((planes * H, W), dtype=np.float32), name="x", key=True)
    g_d = b.inp(np.ones((planes * H, Wo + 2), dtype=np.float32), name="grad_out / y")
    wi_d = b.inp(np.full((planes * H, Wo), 4, dtype=np.int8), torch.int8, "win")
    o_d, w_d, gx_d = b.out((planes * H, Wo + 2), name="out"), b.out((planes * H, Wo), torch.int8, "win out"), b.out((planes * H, W), name="grad_x", key=True)
    big = (1 << 31) // (H * (W + 2)) + 1                       # planes * H * (W + 2) >= 2^31
    for dtype in (0, 1, 2):
        good_f = [_p(x_d), planes, H, W, rr.TANH, dtype, _p(o_d), _p(w_d), st]
        for i, v in ((0, None), (6, None), (7, None), (1, -1), (2, 0), (3, 1), (3, 0), (4, 3), (4, -1), (1, big)):
            assert lib.dl_ring_act_pool_pad_fwd_t(*[v if k == i else a for k, a in enumerate(good_f)]) == INVALID, ("stem forward", dtype, i, v)
        assert lib.dl_ring_act_pool_pad_fwd_t(*[0 if k == 1 else a for k, a in enumerate(good_f)]) == OK
        good_b = [_p(g_d), _p(g_d), _p(wi_d), planes, H, W, rr.TANH, dtype, _p(gx_d), st]
        for i, v in ((0, None), (1, None), (2, None), (8, None), (3, -1), (4, 0), (5, 1), (5, 0), (6, 3), (6, -1), (3, big)):
            assert lib.dl_ring_act_pool_pad_bwd_t(*[v if k == i else a for k, a in enumerate(good_b)]) == INVALID, ("stem backward", dtype, i, v)
        assert lib.dl_ring_act_pool_pad_bwd_t(*[0 if k == 3 else a for k, a in enumerate(good_b)]) == OK
    for dtype in (3, -1):
        assert lib.dl_ring_act_pool_pad_fwd_t(_p(x_d), planes, H, W, rr.TANH, dtype, _p(o_d), _p(w_d), st) == INVALID
        assert lib.dl_ring_act_pool_pad_bwd_t(_p(g_d), _p(g_d), _p(wi_d), planes, H, W, rr.TANH, dtype, _p(gx_d), st) == INVALID
    assert lib.dl_ring_act_pool_pad_fwd(_p(x_d), planes, H, 1, rr.TANH, _p(o_d), _p(w_d), st) == INVALID
    assert lib.dl_ring_act_pool_pad_bwd(_p(g_d), _p(g_d), _p(wi_d), planes, H, 1, rr.TANH, _p(gx_d), st) == INVALID
    assert lib.dl_ring_act_pool_pad_fwd(_p(x_d), 0, H, W, rr.TANH, _p(o_d), _p(w_d), st) == OK
    assert lib.dl_ring_act_pool_pad_bwd(_p(g_d), _p(g_d), _p(wi_d), 0, H, W, rr.TANH, _p(gx_d), st) == OK
    b.untouched("stem refusals", o_d, w_d, gx_d)
