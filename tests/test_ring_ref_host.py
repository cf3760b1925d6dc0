"""The referee of tests/test_gpu_ringops_exact.py checked without a GPU: tests/ring_ref.py against torch's CPU ops in float64
(F.pad circular, tanh / relu, the add, max_pool2d with its indices, autograd) on every shape and data set of the GPU suite, the
rounding helpers against torch's conversions, every planted defect rejected, and the case tables shown to reach what they claim.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as cr
from tests import ring_ref as rr

ALL_STEM = rr.STEM_EVEN + rr.STEM_ODD


def _same64(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return int((~((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y)))).sum())


def _wrap(t):
    return F.pad(t, (1, 1, 0, 0), mode="circular")


def _act_t(v, act):
    return torch.tanh(v) if act == rr.TANH else torch.relu(v) if act == rr.RELU else v


def _ids(cases):
    return ["x".join(map(str, c)) for c in cases]


# ---------------------------------------------------------------------------------------------------- rounding


@pytest.mark.parametrize("storage", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_round_to_is_torchs_conversion(storage):
    """On the fp32 sums of the specials and on 2^16 random bit patterns (NaNs, infinities and subnormals among them)."""
    x, res = rr.specials(storage)
    with np.errstate(over="ignore", invalid="ignore"):
        sums = (x.astype(np.float64) + res.astype(np.float64)).astype(np.float32)
    bits = cr._rng(5).integers(0, 2 ** 32, size=2 ** 16, dtype=np.uint64).astype(np.uint32).view(np.float32)
    near = (np.float32(1.0) + cr._rng(6).integers(-2 ** 14, 2 ** 14, size=4096).astype(np.float32) * np.float32(2.0 ** -23))
    for v in (sums, bits, near, np.array([65519.99, 65520.0, 65520.01, 6e-8, 2.0 ** -25, 2.0 ** -25 * 1.0001, 2.0 ** -24 * 1.5, 2.0 ** -24 * 2.5, 3.4e38], dtype=np.float32)):
        want = torch.from_numpy(v.copy()).to(storage).float().numpy()
        assert rr.bits_differ(rr.round_to(v, storage), want, f"round_to {storage}") == 0
    assert rr.bits_differ(rr.round_to(bits, torch.float32), bits) == 0


@pytest.mark.parametrize("storage", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_the_specials_hold_what_they_promise(storage):
    """Every (x, res) is a number of the storage type; the rounded sums contain ties in both directions (the chopped value differs
    from / equals the rounded one on a half-way sum), an overflow to each infinity, NaN, both zeros and subnormals."""
    x, res = rr.specials(storage)
    for v in (x, res):
        rr.to_storage(v, storage)
    with np.errstate(over="ignore", invalid="ignore"):
        s = (x.astype(np.float64) + res.astype(np.float64)).astype(np.float32)
    r, t = rr.round_to(s, storage), rr.round_to(s, storage, "truncate")
    ulp = 2.0 ** -10 if storage == torch.float16 else 2.0 ** -7          # of the storage type, beside 1
    # the first four pairs: 1 + ulp/2 (half-way, down to the even 1), 1 + ulp + ulp/2 (half-way, up to the even 1 + 2 ulp), just above
    # and just below half-way; all four sums are exact in fp32
    assert s[:4].astype(np.float64).tolist() == (x[:4].astype(np.float64) + res[:4].astype(np.float64)).tolist()
    assert r[:4].tolist() == [1.0, 1.0 + 2 * ulp, 1.0 + ulp, 1.0] and t[:4].tolist() == [1.0, 1.0 + ulp, 1.0, 1.0]
    assert (np.isposinf(r) & np.isfinite(x) & np.isfinite(res)).any() and (np.isneginf(r) & np.isfinite(x) & np.isfinite(res)).any()
    assert np.isnan(r).any() and ((r == 0) & np.signbit(r)).any() and ((r == 0) & ~np.signbit(r)).any()
    tiny = 2.0 ** -14 if storage == torch.float16 else 2.0 ** -126
    assert ((r != 0) & (np.abs(r) < tiny)).any()
    assert rr.bits_differ(r, t, quiet=True) > 0


# ---------------------------------------------------------------------------------------------------- act + pad


@pytest.mark.parametrize("shape", rr.PAD_SHAPES, ids=_ids(rr.PAD_SHAPES))
def test_act_pad_is_the_separate_torch_ops(shape):
    """Forward and backward for every residual layout, pad and activation against float64 torch on integer data; the foreign layouts
    are views into a larger flat buffer whose other elements are NaN."""
    rows, W = shape
    for kind in rr.RES_KINDS:
        for pad in (0, 1):
            for act in rr.ACTS:
                sd = 100 * rows + W + 7 * act + pad
                x = rr.ints((rows, W), 3, sd).numpy()
                lay = rr.res_layout(kind, W)
                flat, r2d = None, None
                if lay is not None:
                    pitch, off = lay
                    flat = np.full(rows * pitch + off + W, np.nan)
                    r2d = rr.ints((rows, W), 3, sd + 1).numpy()
                    for r in range(rows):
                        flat[r * pitch + off:r * pitch + off + W] = r2d[r]
                out = rr.act_pad_fwd(x, flat, *(lay or (0, 0)), W, pad, act, torch.float32)
                xt = torch.from_numpy(x).view(1, 1, rows, W).requires_grad_(True)
                v = xt if r2d is None else xt + torch.from_numpy(r2d).view(1, 1, rows, W)
                a = _act_t(v, act)
                want = _wrap(a) if pad else a
                assert rr.bits_differ(out, want.detach().float().view(rows, -1), f"act_pad_fwd {shape} {kind} pad {pad} act {act}") == 0
                # backward: the fold of the wrap columns is autograd of F.pad, act' comes from a saved y on the grid
                g = rr.ints((rows, W + 2 * pad), 3, sd + 2).numpy()
                y = rr.saved((rows, W + 2 * pad), act, sd + 3)
                lt = torch.from_numpy(x).view(1, 1, rows, W).requires_grad_(True)
                (_wrap(lt) if pad else lt * 1.0).backward(torch.from_numpy(g).view(1, 1, rows, -1))
                folded, yi = lt.grad.view(rows, W).numpy(), y[:, pad:pad + W]
                want_gx = np.where(yi <= 0, 0.0, folded) if act == rr.RELU else folded * rr.dact(yi, act)
                gx, gr = rr.act_pad_bwd(g, y, W, pad, act, torch.float32, with_res=True)
                assert _same64(gx, want_gx) == 0
                assert _same64(gr[:, 1:-1], want_gx) == 0 and not gr[:, 0].any() and not gr[:, -1].any() and not np.signbit(gr[:, [0, -1]]).any()
                if act != rr.TANH:                                   # the whole chain under autograd, y = the forward's own output
                    want.backward(torch.from_numpy(g).view(1, 1, rows, -1))
                    assert _same64(rr.act_pad_bwd(g, out, W, pad, act, torch.float32), xt.grad.view(rows, W).numpy()) == 0       # (+0.0 at dead units)


# ---------------------------------------------------------------------------------------------------- stem


def _torch_pool(a, H, W):
    """(out, code) of torch's max-pool on the wrapped planes; its flat index into the [H][W + 2] padded plane becomes the 0..8 code."""
    planes, Wo = a.shape[0] // H, rr.out_width(W)
    t = _wrap(torch.from_numpy(np.asarray(a, dtype=np.float64)).view(1, planes, H, W))
    y, idx = F.max_pool2d(t, kernel_size=3, stride=(1, 2), padding=(1, 0), return_indices=True)
    ih, iw = idx // (W + 2), idx % (W + 2)
    code = (ih - torch.arange(H).view(1, 1, H, 1) + 1) * 3 + (iw - 2 * torch.arange(Wo).view(1, 1, 1, Wo))
    return _wrap(y).view(planes * H, Wo + 2).numpy(), code.view(planes * H, Wo).numpy()


def _stem_maps(case):
    """(act, activated float64 map) of every data set of a case: integers under each activation, near_ties("tanh") under none and
    tanh, near_ties("relu") under relu."""
    planes, H, W = case
    for act in rr.ACTS:
        yield act, "ints", rr.act_host(rr.stem_inputs(planes, H, W, act, "ints")[0], act)
    for act, data in ((rr.NONE, rr.TANH), (rr.TANH, rr.TANH), (rr.RELU, rr.RELU)):
        yield act, "near", rr.act_host(rr.stem_inputs(planes, H, W, data, "near")[0], act).astype(np.float32)


@pytest.mark.parametrize("case", ALL_STEM, ids=_ids(ALL_STEM))
def test_pool_fwd_is_torchs_max_pool(case):
    """Values (bit patterns) and positions on the integer maps and on the near-tie and NaN windows: the first strictly greater value
    wins, the last NaN wins, a window of -inf keeps the first in-range position."""
    planes, H, W = case
    for act, kind, a in _stem_maps(case):
        out, win = rr.pool_fwd(a, H, W)
        t_out, t_code = _torch_pool(a, H, W)
        what = f"{case} act {act} {kind}"
        assert _same64(out, t_out) == 0, what
        assert np.array_equal(win, t_code), what
        rows_h = np.arange(planes * H) % H
        assert win.min() >= 0 and win.max() <= 8 and (win[rows_h == 0] >= 3).all() and (win[rows_h == H - 1] <= 5).all(), what


@pytest.mark.parametrize("case", ALL_STEM, ids=_ids(ALL_STEM))
def test_pool_bwd_is_autograd(case):
    """Scatter against float64 autograd through wrap, max_pool2d, wrap; under tanh the incoming gradient is multiplied by 1 - y^2 of
    the (wrapped) pooled map, which is the same number in its copies."""
    planes, H, W = case
    Wo = rr.out_width(W)
    for act in rr.ACTS:
        sd = rr.stem_case_seed(planes, H, W, act)
        rr.headroom(2, act)
        a = rr.saved((planes * H, W), act, sd + 1)
        g = rr.ints((planes * H, Wo + 2), 2, sd + 2).numpy()
        y, win = rr.pool_fwd(a, H, W)
        at = torch.from_numpy(a).view(1, planes, H, W).requires_grad_(True)
        yt = _wrap(F.max_pool2d(_wrap(at), kernel_size=3, stride=(1, 2), padding=(1, 0)))
        gt = torch.from_numpy(g).view(1, planes, H, Wo + 2)
        yt.backward(gt * torch.from_numpy(rr.dact(yt.detach().numpy(), act)))
        got = rr.pool_bwd(g, y, win, H, W, act)
        assert rr.bits_differ(got, at.grad.view(planes * H, W).float().numpy(), f"pool_bwd {case} act {act}") == 0
        assert _same64(got, at.grad.view(planes * H, W).numpy()) == 0            # (nothing was rounded)


# ---------------------------------------------------------------------------------------------------- planted defects


def test_every_planted_defect_is_caught_on_the_committed_cases():
    """The comparator of the GPU suite (bits_differ / inequality of win) counts mismatches for each defect over the case lists."""
    caught = dict.fromkeys(rr.DEFECTS, 0)
    for case in ALL_STEM:
        planes, H, W = case
        Wo = rr.out_width(W)
        for act, kind, a in _stem_maps(case):
            out, win = rr.pool_fwd(a, H, W)
            for d in ("start_0_at_row_0", "tie_to_later"):
                o2, w2 = rr.pool_fwd(a, H, W, defect=d)
                caught[d] += rr.bits_differ(o2, out, quiet=True) + int((w2 != win).sum())
        for act in rr.ACTS:
            sd = rr.stem_case_seed(planes, H, W, act)
            a, g = rr.saved((planes * H, W), act, sd + 1), rr.ints((planes * H, Wo + 2), 2, sd + 2).numpy()
            y, win = rr.pool_fwd(a, H, W)
            caught["no_wrap"] += rr.bits_differ(rr.pool_bwd(g, y, win, H, W, act, defect="no_wrap"), rr.pool_bwd(g, y, win, H, W, act), quiet=True)
    for storage in (torch.float16, torch.bfloat16):
        x, res = rr.specials(storage)
        n = len(x)
        flat = np.concatenate([np.zeros(3, dtype=np.float32), res])
        caught["truncate"] += rr.bits_differ(rr.act_pad_fwd(x.reshape(1, n), flat, n, 3, n, 1, rr.NONE, storage, defect="truncate"),
                                             rr.act_pad_fwd(x.reshape(1, n), flat, n, 3, n, 1, rr.NONE, storage), quiet=True)
    for storage in (torch.float16, torch.bfloat16):
        chopped = 0
        for rows, W in rr.PAD_SHAPES:
            rr.headroom(rr.GMAX[storage], rr.TANH, windows=1)
            g, y = rr.ints((rows, W + 2), rr.GMAX[storage], rows + W).numpy(), rr.saved((rows, W + 2), rr.TANH, rows)
            good = rr.act_pad_bwd(g, y, W, 1, rr.TANH, storage)
            assert rr.bits_differ(rr.act_pad_bwd(g, y, W, 1, rr.TANH, storage, defect="no_wrap"), good, quiet=True) > 0
            chopped += rr.bits_differ(rr.act_pad_bwd(g, y, W, 1, rr.TANH, storage, defect="truncate"), good, quiet=True)
        assert chopped > 0, storage
    assert all(v > 0 for v in caught.values()), caught


# ---------------------------------------------------------------------------------------------------- what the cases reach


def test_the_stem_cases_reach_every_dispatch_and_every_edge_of_the_even_kernels():
    """Dispatch (even / general, the general kernels at even W through a 4-byte skew), a wave whose lane 0 lies mid-row, idle lanes
    in the last wave, a strip that ends below the plane, a strip whose row h0 - 1 would be the previous plane's, several blocks."""
    seen = set()
    for run in rr.STEM_RUNS:
        seen |= rr.stem_props(*run)
    assert seen == set(rr.STEM_PROPS), set(rr.STEM_PROPS) - seen
    for p, h, w in rr.STEM_EVEN:
        assert "even" in rr.stem_props(p, h, w, 0) and "general at even W" in rr.stem_props(p, h, w, 4)
    for c in rr.STEM_HALF:
        assert c in ALL_STEM


@pytest.mark.parametrize("act", [rr.TANH, rr.RELU], ids=["tanh", "relu"])
def test_the_near_tie_windows_all_land_somewhere_and_on_the_edges(act):
    """Over the stem cases every window of near_ties is placed intact at least once; windows land on lane 0 of a wave of the even
    kernel, on both seam columns and in a last partial wave."""
    wins = rr.near_ties(act)
    placed_all, where = set(), set()
    for planes, H, W in ALL_STEM:
        x, placed = rr.stem_inputs(planes, H, W, act, "near")
        Wo, S = rr.out_width(W), (H + rr.STEM_RH - 1) // rr.STEM_RH
        total = planes * S * Wo
        for n, row, wo in placed:
            placed_all.add(n)
            got = np.array([x[row + dh, (2 * wo + dw) % W] for dh in (-1, 0, 1) for dw in (-1, 0, 1)], dtype=np.float32)
            assert rr.bits_differ(got, wins[n][1].reshape(-1)) == 0
            where.add("wo = 0" if wo == 0 else "wo = Wo - 1" if wo == Wo - 1 else "inside")
            if W % 2 == 0:
                i = ((row // H) * S + (row % H) // rr.STEM_RH) * Wo + wo
                if i % rr.WAVE == 0:
                    where.add("lane 0")
                if total % rr.WAVE and i >= total - total % rr.WAVE:
                    where.add("last partial wave")
    assert placed_all == set(range(len(wins))), sorted(set(range(len(wins))) - placed_all)[:20]
    assert where >= {"wo = 0", "wo = Wo - 1", "inside", "lane 0", "last partial wave"}, where
    # the single-row and two-row cases start from the windows of -inf, where only the start code says which position "won"
    x, _ = rr.stem_inputs(2, 1, 8, act, "near")
    assert np.isneginf(x).any()


def test_a_dead_relu_unit_gives_zero_whatever_its_gradient():
    """+inf, -inf and NaN gradients at elements whose saved output is <= 0 (torch's threshold_backward selects): the result is the one
    without them, bit for bit, in both backward references."""
    rows, W, pad = 5, 7, 1
    g, y = rr.ints((rows, W + 2), 3, 1).numpy(), rr.saved((rows, W + 2), rr.RELU, 2)
    g2 = rr.dead_garbage(g, y, pad + 1, pad + W - 1)
    assert (~np.isfinite(g2)).sum() == 3
    assert rr.bits_differ(rr.act_pad_bwd(g2, y, W, pad, rr.RELU, torch.float32), rr.act_pad_bwd(g, y, W, pad, rr.RELU, torch.float32)) == 0
    assert np.isnan(rr.act_pad_bwd(g2, y, W, pad, rr.NONE, torch.float32)).any()
    planes, H, W = 2, 5, 10
    Wo = rr.out_width(W)
    a = rr.saved((planes * H, W), rr.RELU, 3)
    a[:H] = 0.0                                         # (the first plane pools to zeros: every window there is dead)
    out, win = rr.pool_fwd(a, H, W)
    g = rr.ints((planes * H, Wo + 2), 2, 4).numpy()
    g2 = rr.dead_garbage(g, out, 2, Wo)
    assert (~np.isfinite(g2)).sum() > 0
    assert rr.bits_differ(rr.pool_bwd(g2, out, win, H, W, rr.RELU), rr.pool_bwd(g, out, win, H, W, rr.RELU)) == 0


def test_near_ties_hold_candidates_on_both_sides_of_the_threshold_band():
    """For a maximum in the unsaturated range the window holds candidates inside 24 ulp(a) / (1 - a^2) of it and outside, equal to it,
    and one ulp below; maxima on both sides of the switch 1 - a^2 < 1e-4 occur."""
    for xm in (0.5, 2.0, 4.0, 5.2):
        c = np.array(rr._candidates(np.float32(xm)), dtype=np.float64)
        a = np.tanh(xm)
        band = 24.0 * 6e-8 * a / (1 - a * a)
        assert ((xm - c > 0) & (xm - c < band)).any() and (xm - c > band).any() and (c == np.float32(xm)).any()
    d = [1.0 - float(np.tanh(np.float32(m))) ** 2 for m in rr.TIE_MAGNITUDES]
    assert any(0 < v < 1e-4 for v in d) and any(1e-4 < v < 1e-3 for v in d) and any(v == 0 for v in d)
    assert float(np.tanh(np.float32(5.2))) ** 2 < 1 - 1e-4 < float(np.tanh(np.float32(5.4))) ** 2


def test_half_stem_inputs_are_storage_numbers_whose_activations_collide_after_rounding():
    for storage in (torch.float16, torch.bfloat16):
        for case in rr.STEM_HALF:
            for act in rr.ACTS:
                rr.to_storage(rr.half_stem_input(*case, act, 3), storage)
        x = rr.half_stem_input(2, 4, 128, rr.TANH, 3)
        a = np.tanh(x.astype(np.float64)).astype(np.float32)
        r = rr.round_to(a, storage)
        fin = ~np.isnan(x)
        assert len(np.unique(r[fin])) < len(np.unique(a[fin])) and np.isnan(x).sum() == 5
