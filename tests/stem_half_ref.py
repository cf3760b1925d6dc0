"""Referee of the half-precision stem (csrc/stemh.hip: ``dl_stem_input_nhwc_h``, ``dl_stem_conv1_h``, ``dl_stem_pool_fwd_h``,
``dl_stem_wgrad_h``), written from the text of include/delora_hip.h:

  * ``h`` = torch's round-to-nearest-even conversion, and ``h_f64``, the same rounding restated in float64 arithmetic (the host tier
    holds one against the other on hand-made values),
  * the generated cases of tests/test_gpu_stem_half_exact.py -- input copies with planted ties and values beyond the half range,
    integer conv1 cases whose sums leave the exact-integer range of the storage type (so the final rounding, ties included, is what
    the comparison sees), a delta image under 4608 pairwise different weights, real-valued cases -- each asserting its own headroom,
  * the launch plans of the new kernels restated, with literal tables and coverage lists,
  * the first-order bounds of the real-valued tiers.

The pooling and the integer weight-gradient cases are those of tests/stem_ref.py: their values (small integers, quarters, zeros, infinities)
are half-precision numbers, which ``representable`` asserts.  No GPU is needed to import this module."""
import numpy as np
import torch

from tests import conv_ref as cr
from tests import stem_ref as sr

DTYPES = (torch.bfloat16, torch.float16)
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
CODE = {torch.float16: 1, torch.bfloat16: 2}
EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}        # half an ulp, relative (tests/test_gpu_convh.py)
BITS = {torch.bfloat16: 8, torch.float16: 11}                       # significant bits
EXACT_INT = {torch.bfloat16: 256.0, torch.float16: 2048.0}          # every integer up to here is a number of the type
f32 = np.float32


def h(v, dtype):
    """Round-to-nearest-even conversion of fp32 values to ``dtype`` (torch's), returned as float64 numpy.  ``v`` must hold fp32 numbers."""
    v = np.asarray(v, dtype=np.float64)
    v32 = v.astype(f32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(v32.astype(np.float64), v, equal_nan=True), "h() is defined on fp32 values"
    return torch.from_numpy(np.ascontiguousarray(v32)).to(dtype).double().numpy()


def h_f64(v, dtype):
    """The same rounding from its definition, in float64: p significant bits, ties to even, gradual underflow below the smallest
    normal exponent, overflow to infinity from max + half an ulp on."""
    v = np.asarray(v, dtype=np.float64)
    p = BITS[dtype]
    emin, emax = (-14, 15) if dtype == torch.float16 else (-126, 127)
    _, e = np.frexp(np.where(np.isfinite(v) & (v != 0), v, 1.0))            # |v| in [2^(e-1), 2^e)
    quantum = np.exp2((np.maximum(e - 1, emin) - (p - 1)).astype(np.float64))
    q = np.rint(v / quantum) * quantum                                      # np.rint: half to even
    top = (2.0 - 2.0 ** (1 - p)) * 2.0 ** emax
    with np.errstate(invalid="ignore"):
        q = np.where(np.abs(q) > top, np.sign(v) * np.inf, q)
    return np.where(np.isfinite(v), q, v)


def representable(v, dtype):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.array_equal(h(v, dtype), v, equal_nan=True))


def bits_differ_h(got, ref, dtype, name="", quiet=False):
    """Number of elements whose 16-bit patterns differ (any NaN equals any NaN; -0.0 and +0.0 differ).  ``got``: a tensor of ``dtype``;
    ``ref``: float64 values that ARE numbers of the type."""
    got = got.detach().cpu().contiguous()
    assert got.dtype == dtype
    ref_t = torch.from_numpy(np.ascontiguousarray(np.asarray(ref, dtype=np.float64))).to(dtype)
    assert got.shape == ref_t.shape, (name, got.shape, ref_t.shape)
    bad = ~((got.view(torch.int16) == ref_t.view(torch.int16)) | (torch.isnan(got) & torch.isnan(ref_t)))
    n = int(bad.sum())
    if n and not quiet:
        print(cr.describe(bad, got.float(), ref_t.float(), name))
    return n


# ---------------------------------------------------------------------------------------------------- input copy

INPUT_CASES = ((1, 1, 4), (2, 3, 8), (1, 2, 132))
INPUT_SKEW_CASE = (2, 3, 8)


def planted(dtype):
    """fp32 values whose conversion is decided by the rounding rule: exact ties (an odd multiple of half an ulp: both directions of
    ties-to-even), their fp32 neighbours, the largest finite number, the tie above it (-> inf), values beyond it, the smallest
    subnormal's tie and what lies below."""
    p = BITS[dtype]
    u = 2.0 ** (1 - p)                                                      # ulp at 1
    top = (2.0 - u) * (2.0 ** 15 if dtype == torch.float16 else 2.0 ** 127)
    tiny = 2.0 ** (-14 - (p - 1)) if dtype == torch.float16 else 2.0 ** (-126 - (p - 1))
    vals = [1 + u / 2, 1 + 3 * u / 2, 1 + 5 * u / 2, -(1 + u / 2), -(1 + 3 * u / 2), 60 * (1 + u / 2), 60 * (1 + 3 * u / 2),
            float(np.nextafter(f32(1 + u / 2), f32(2))), float(np.nextafter(f32(1 + u / 2), f32(0))),
            top, -top, top * (1 + u / 4), float(np.nextafter(f32(top * (1 + u / 4)), f32(0))), -top * (1 + u / 4),
            tiny, tiny / 2, 3 * tiny / 2, float(np.nextafter(f32(tiny / 2), f32(1))), tiny / 4, -tiny / 2, 0.0, -0.0]
    if dtype == torch.float16:
        vals += [1e5, -1e5, 70000.0, 3e38]
    else:
        vals += [float(np.finfo(f32).max), -float(np.finfo(f32).max), 3.4e38]
    return np.array(vals, dtype=f32)


def input_case(N, H, W, dtype, seed=None):
    """Planar fp32 image [N][8][H][W]: Gaussian * 30 (a range image's magnitudes) with ``planted`` spread over it."""
    r = cr._rng(seed if seed is not None else 4100 + 17 * N + 5 * H + W)
    x = (r.standard_normal((N, 8, H, W)) * 30.0).astype(f32)
    pv = planted(dtype)
    pos = r.choice(x.size, size=min(len(pv), x.size), replace=False)
    x.reshape(-1)[pos] = pv[:len(pos)]
    return x


def input_ref(x, dtype):
    """x8h [N][H][W][8] as float64."""
    return h(np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1))), dtype)


def input_case_properties(x, dtype):
    """(exact ties, values that overflow to infinity) in the case."""
    v = x.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        q = h_f64(v, dtype)
        lo, hi = np.minimum(q, v), np.maximum(q, v)
        fin = np.isfinite(q) & (q != v)
        # a tie: the value is as far from its rounded neighbour as from the other one
        p = BITS[dtype]
        _, e = np.frexp(np.where(v != 0, v, 1.0))
        emin = -14 if dtype == torch.float16 else -126
        quantum = np.exp2((np.maximum(e - 1, emin) - (p - 1)).astype(np.float64))
        ties = fin & (np.abs(hi - lo) == quantum / 2)
    return int(ties.sum()), int((np.isinf(q) & np.isfinite(v)).sum())


# ---------------------------------------------------------------------------------------------------- conv1

SH_TILE, SH_WAVES, SH_MAX_GRID = 32, 4, 1024


def conv1_plan(N, H, W):
    """(pixels, tiles, grid, iterations) of dl_stem_conv1_h: the N H W/2 output pixels as one flat list, 32 per tile, one tile per wave
    and iteration, four waves per workgroup, at most 1024 workgroups."""
    pixels = N * H * (W // 2)
    tiles = -(-pixels // SH_TILE)
    grid = min(-(-tiles // SH_WAVES), SH_MAX_GRID)
    return pixels, tiles, grid, -(-tiles // (grid * SH_WAVES))


# (N, H, W) -> (pixels, tiles, grid, iterations), asserted literally against conv1_plan()
CONV1_PLAN = {
    (1, 1, 4): (2, 1, 1, 1), (1, 2, 4): (4, 1, 1, 1), (2, 3, 8): (24, 1, 1, 1), (1, 5, 12): (30, 1, 1, 1), (1, 3, 128): (192, 6, 2, 1),
    (1, 3, 132): (198, 7, 2, 1), (2, 5, 72): (360, 12, 3, 1), (3, 2, 260): (780, 25, 7, 1), (1, 129, 2036): (131322, 4104, 1024, 2),
}
CONV1_CASES = tuple(CONV1_PLAN)
CONV1_SKEW_CASE = (2, 5, 72)
CONV1_DISTINCT_CASE = (2, 5, 72)
CONV1_RANGES = {torch.bfloat16: (15, 15), torch.float16: (30, 30)}      # (|x|, |w|): integers of the type; 72 * 30 * 30 < 65504


def conv1_coverage(cases=CONV1_CASES):
    plans = {c: conv1_plan(*c) for c in cases}
    missing = []
    for what, ok in (
            ("a pixel count that is no multiple of the tile", any(p[0] % SH_TILE for p in plans.values())),
            ("a pixel count that is a multiple of the tile", any(p[0] % SH_TILE == 0 for p in plans.values())),
            ("fewer pixels than one tile", any(p[0] < SH_TILE for p in plans.values())),
            ("more than one workgroup", any(p[2] > 1 for p in plans.values())),
            ("idle waves in the last workgroup", any(p[1] % SH_WAVES and p[3] == 1 for p in plans.values())),
            ("a tile that crosses a row's end", any((c[2] // 2) % SH_TILE and p[1] > 1 for c, p in plans.items())),
            ("a tile that crosses an image's end", any(c[0] > 1 and (c[1] * (c[2] // 2)) % SH_TILE and p[1] > 1 for c, p in plans.items())),
            ("a map that wraps onto itself (W = 4)", any(c[2] == 4 for c in plans)),
            ("two iterations, the second one ragged", any(p[3] == 2 and p[1] % (p[2] * SH_WAVES) for p in plans.values()))):
        if not ok:
            missing.append(what)
    return missing


def conv1_ref64(x8, w, act):
    """act(conv1) in float64 on the given operands: x8 [N][H][W][8], w [64][3][3][8] -> [N][H][W/2][64] (numpy)."""
    pre = cr.conv(torch.from_numpy(np.asarray(x8, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64)), (1, 2))
    a = torch.tanh(pre) if act == sr.TANH else torch.relu(pre) if act == sr.RELU else pre
    return a.numpy()


def conv1_int_case(N, H, W, dtype, act, seed=None):
    """Integer operands (numbers of the type) and the expected map h(act(exact sum)).  Asserts: the sum is exact in fp32 in any order
    (conv_ref.headroom; finite in fp16), outputs lie beyond the type's exact-integer range, and exact ties are among them."""
    assert act in (sr.NONE, sr.RELU)
    xmax, wmax = CONV1_RANGES[dtype]
    cr.headroom("direct", 8, xmax, wmax, taps=9, storage=dtype)
    sd = (seed if seed is not None else 6100 + 131 * N + 17 * H + W) * 4 + act + (1000003 if dtype == torch.float16 else 0)
    x8, w = cr.ints((N, H, W, 8), xmax, sd * 2 + 1).numpy(), cr.ints((64, 3, 3, 8), wmax, sd * 2 + 2).numpy()
    assert representable(x8, dtype) and representable(w, dtype)
    exact = conv1_ref64(x8, w, act)
    assert np.array_equal(exact, np.rint(exact)), "integer sums"
    want = h(exact, dtype)
    props = {"beyond the exact-integer range": int((np.abs(exact) > EXACT_INT[dtype]).sum()), "rounded": int((want != exact).sum()),
             "ties": int(_is_tie(exact, dtype).sum())}
    assert all(v > 0 for v in props.values()), ((N, H, W), NAME[dtype], act, props)
    return {"x8": x8, "w": w, "want": want, "exact": exact, "props": props}


def _is_tie(v, dtype):
    """Finite values that lie exactly between two neighbouring numbers of the type."""
    v = np.asarray(v, dtype=np.float64)
    p = BITS[dtype]
    _, e = np.frexp(np.where(v != 0, v, 1.0))
    emin = -14 if dtype == torch.float16 else -126
    quantum = np.exp2((np.maximum(e - 1, emin) - (p - 1)).astype(np.float64))
    r = np.abs(v) / quantum
    return np.isfinite(v) & (r - np.floor(r) == 0.5)


def conv1_distinct_case(dtype, act, seed=77):
    """4608 pairwise different weights -- different after the conversion too, and NOT numbers of the type: the kernel's own conversion
    of the parameter is part of the result -- under an image of isolated +-1 / +-2 pixels: every 3x3 window holds at most one non-zero
    element, so every output is h(act(+-h(w) * 2^j)) whatever the order of the sum, and a permuted operand cannot pass.  Asserts that
    every (r, s, c) is reached."""
    N, H, W = CONV1_DISTINCT_CASE
    r = cr._rng(seed)
    # 2304 consecutive bit patterns of the type (18 binades of bf16 from 2^-16, 2.25 of fp16 from 2^-3), both signs, each moved off
    # the type's grid by an eighth of an ulp, in a random order
    base = torch.tensor([2.0 ** -16 if dtype == torch.bfloat16 else 2.0 ** -3]).to(dtype).view(torch.int16)
    mag = (base + torch.arange(2304, dtype=torch.int16)).view(dtype).double().numpy()
    w = (np.concatenate([mag, -mag]) * (1.0 + 2.0 ** -(BITS[dtype] + 3))).astype(f32)[r.permutation(4608)].reshape(64, 3, 3, 8)
    wh = h(w, dtype)
    assert np.array_equal(np.sort(np.abs(wh).reshape(-1)), np.sort(np.concatenate([mag, mag])))
    assert len(np.unique(wh)) == w.size and not representable(w, dtype)
    x8 = np.zeros((N, H, W, 8), dtype=np.float64)
    i = 0
    for n in range(N):
        for y in (1, 4):
            for col in range(0, W, 3):
                x8[n, y, col, (i // 2) % 8] = (1.0, -2.0, 2.0, -1.0)[(i // 16) % 4]      # (column parity, channel): all 16 pairs
                i += 1
    # every window of three rows and three (wrapped) columns holds at most one non-zero element
    cnt = conv1_ref64((x8 != 0).astype(np.float64), np.ones((64, 3, 3, 8)), sr.NONE)
    assert cnt.max() == 1.0
    hit = np.zeros((3, 3, 8), dtype=bool)
    for rr in range(3):
        for s in range(3):
            for c in range(8):
                one = np.zeros((64, 3, 3, 8))
                one[:, rr, s, c] = 1.0
                hit[rr, s, c] = bool(np.abs(conv1_ref64(x8, one, sr.NONE)).max() > 0)
    assert hit.all(), "a tap or channel no output reads"
    exact = conv1_ref64(x8, wh, act)                                        # (one term per sum: float64 is exact)
    return {"x8": x8, "w": w, "want": h(exact.astype(f32).astype(np.float64), dtype)}


CONV1_REAL_SHAPES = ((2, 16, 256), (1, 7, 132))


def conv1_abs_tol(act):
    """The absolute term of tests/test_gpu_convh.py for a 3x3 layer's activated outputs: 3e-5 behind tanh, 2e-5 sqrt(9 max(C, K))
    otherwise (C = 8, K = 64)."""
    return 3e-5 if act == sr.TANH else 2e-5 * np.sqrt(9 * 64)


def worst(got, want, eps, abs_tol):
    """tests/test_gpu_convh.py::_worst: max |got - want| / (eps |want| + abs_tol)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float((np.abs(got - want) / (eps * np.abs(want) + abs_tol)).max())


def real_case(N, H, W, dtype, seed):
    """stem_ref.real_inputs rounded to the type: x8, g, w (float64 numpy holding numbers of the type)."""
    x8, g, w = sr.real_inputs(N, H, W, seed)
    return h(x8, dtype), h(g, dtype), h(w, dtype)


# ---------------------------------------------------------------------------------------------------- pooling

POOL_CASES = tuple(c for c in sr.POOL_CASES if c[3] % 8 == 0) + ((1, 1, 2, 8), (1, 19, 54, 8))      # the last: 513 threads


def pool_threads(case):
    N, H, Wc, C = case
    return N * H * (Wc // 2) * (C // 8)


# ---------------------------------------------------------------------------------------------------- fused weight gradient

# The launch plan of dl_stem_wgrad_h is that of dl_stem_wgrad_f32 (64-pixel chunks, at most 512 slabs): stem_ref.plan, WGRAD_PLAN and
# coverage() apply as they are.
plan, WGRAD_PLAN, WGRAD_CASES, SKEW_CASE, coverage = sr.plan, sr.WGRAD_PLAN, sr.WGRAD_CASES, sr.SKEW_CASE, sr.coverage


def workspace_bytes(N, H, W):
    return 0 if (N <= 0 or H <= 0 or W <= 0 or W % 4 or N * H * W * 32 >= 2 ** 31) else plan(N, H, W)[1] * 64 * 72 * 4


def wgrad_case(N, H, W, act, dtype):
    """stem_ref.wgrad_case, with the assertion that g, a, x8 and the intermediate gc are numbers of the type: half storage loses
    nothing, and stem_ref.stem_wgrad_ref is the exact answer."""
    c = sr.wgrad_case(N, H, W, act)
    gc = sr.pool_bwd_ref(c["g"], c["a"], c["win"], act)
    for k, v in (("g", c["g"]), ("a", c["a"]), ("x8", c["x8"]), ("gc", gc)):
        assert representable(v, dtype), (k, (N, H, W), act, NAME[dtype])
    return c


def gc_half(g, a, win, act, dtype):
    """gc as the kernel must form it: the six candidates added in fp32 in the order of the header's gather (pooled rows r - 1, r, r + 1;
    the window of column j / 2, then the wrapped neighbour's), times act'(a) in fp32 (tanh: 1 - a * a, every operation rounded; relu
    selects), rounded ONCE to the type.  stem_ref.pool_bwd_emul32 is that fp32 arithmetic."""
    return h(sr.pool_bwd_emul32(g, a, win, act).astype(np.float64), dtype)


def wgrad_op_count(N, H, W):
    """Rounded fp32 additions behind one element of dw: 16 products per MFMA and chunk of a wave's chain (the products of two half
    numbers are exact; each is counted as one rounded addition, whatever the order inside the instruction), 3 for the four waves,
    ceil(grid / 4) slab additions of a reduction wave, 3 for its waves."""
    _, _, cps, grid = plan(N, H, W)
    return 16 * cps + 3 + (grid + 3) // 4 + 3


def wgrad_ref_and_bound(gc, x8, N, H, W):
    """(dw [64][8][3][3] float64 of the ROUNDED gc and x8, per-element bound c 2^-24 sum |gc| |x|)."""
    z = torch.zeros((64, 3, 3, 8), dtype=torch.float64)
    x = torch.from_numpy(np.asarray(x8, dtype=np.float64))
    gct = torch.from_numpy(np.asarray(gc, dtype=np.float64))
    dw = cr.conv_grads(x, z, gct, (1, 2))[1].permute(0, 3, 1, 2).contiguous().numpy()
    s_abs = cr.conv_grads(x.abs(), z, gct.abs(), (1, 2))[1].permute(0, 3, 1, 2).contiguous().numpy()
    return dw, wgrad_op_count(N, H, W) * 2.0 ** -24 * s_abs
