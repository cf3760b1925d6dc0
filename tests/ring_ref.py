"""Exact referee of the ring ops (csrc/ringops.hip): [residual add] + activation + wrap-around padding, and the stem's activation +
wrapped 3x3 / stride-(1,2) max-pooling + padding, forward and backward, in the three storage types.

Written from the contract in the header of ringops.hip, per output element, in float64 numpy:

  * ``act_pad_fwd`` / ``act_pad_bwd``, ``pool_fwd`` / ``pool_bwd`` (plain loops over windows, torch's scan rule),
  * ``round_to``: one round-to-nearest-even from fp32 to the storage type, as bit arithmetic,
  * data makers: small integers, saved activations on a coarse grid (``headroom`` asserts that a six-window sum stays exact),
    ``near_ties`` (single adversarial windows around the tanh arg-max shortcuts) with ``tile`` (windows laid into a map without
    overlapping), ``bf16_specials`` / ``fp16_specials`` (rounding ties, overflow, NaN, signed zeros, subnormals),
  * planted defects (``defect=``), so that the suite is known to be able to fail,
  * the case tables of tests/test_gpu_ringops_exact.py and what each stem case reaches in the kernels (``stem_props``).

No GPU is needed to import it.
"""
import numpy as np
import torch

from tests import conv_ref as cr

NONE, TANH, RELU = cr.ACT_NONE, cr.ACT_TANH, cr.ACT_RELU
ACTS = (NONE, TANH, RELU)
ACT_NAME = {NONE: "none", TANH: "tanh", RELU: "relu"}
STORAGES = (torch.float32, torch.float16, torch.bfloat16)
ST_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
DEFECTS = ("start_0_at_row_0", "tie_to_later", "no_wrap", "truncate")
f32 = np.float32
ints = cr.ints

DL_BLOCK, RING_UN, STEM_RH, WAVE = 256, 4, 4, 64


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---------------------------------------------------------------------------------------------------- rounding


def round_to(v, storage, defect=None):
    """float32 array -> float32 array holding v rounded ONCE to ``storage``, round-to-nearest-even (ties to the even significand,
    overflow to infinity, NaN stays NaN, the sign of zero kept).  ``defect`` "truncate" chops instead."""
    v = np.ascontiguousarray(v, dtype=f32)
    if storage == torch.float32:
        return v.copy()
    u = v.view(np.uint32).astype(np.uint64)
    if storage == torch.bfloat16:
        r = u if defect == "truncate" else u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))
        r = np.where(np.isnan(v), np.uint64(0x7FC00000), r & np.uint64(0xFFFF0000))
        return r.astype(np.uint32).view(f32).reshape(v.shape)
    assert storage == torch.float16
    # fp16: 11 significant bits down to 2^-14, below that the fixed grid 2^-24; spelled out with integers on the fp32 bit pattern
    sign, mag = u & np.uint64(0x80000000), u & np.uint64(0x7FFFFFFF)
    e = (mag >> np.uint64(23)).astype(np.int64)                       # biased fp32 exponent
    # bits to drop: 13 for a normal fp16 result, more below 2^-14 (fp32 exponent 113), everything below 2^-25
    drop = np.clip(13 + (113 - e), 13, 25).astype(np.uint64)
    sig = np.where(e > 0, (mag & np.uint64(0x7FFFFF)) | np.uint64(0x800000), mag & np.uint64(0x7FFFFF))      # 24-bit significand
    sh = np.where(e > 0, drop, np.uint64(25))
    q = sig >> sh
    rem = sig & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
    if defect != "truncate":
        q = q + up.astype(np.uint64)
    # value = q * 2^(E - 23 + sh), E = unbiased exponent (e - 127, or -126 for fp32 subnormals)
    scale = np.where(e > 0, e - 127, -126) - 23 + sh.astype(np.int64)
    val = np.ldexp(q.astype(np.float64), scale.astype(np.int32))
    val = np.where(val > 65504.0, np.inf if defect != "truncate" else 65504.0, val)
    val = np.where(mag == np.uint64(0x7F800000), np.inf, val)
    out = np.where(sign != 0, -val, val).astype(f32)
    return np.where(np.isnan(v), f32(np.nan), out).reshape(v.shape)


def to_storage(v, storage):
    """torch tensor of ``storage`` holding the float values of v, which must be representable (asserted)."""
    t = torch.from_numpy(np.ascontiguousarray(_np(v), dtype=f32))
    s = t.to(storage)
    back = s.float()
    assert bool(((back.view(torch.int32) == t.view(torch.int32)) | (torch.isnan(back) & torch.isnan(t))).all()), "data not representable in " + ST_NAME[storage]
    return s


def bits_differ(got, ref, name="", quiet=False):
    """Number of elements whose fp32 bit patterns differ (any NaN equals any NaN); -0.0 and +0.0 differ."""
    got = torch.as_tensor(_np(got)).float().contiguous()
    ref = torch.as_tensor(np.ascontiguousarray(_np(ref), dtype=f32)).contiguous()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = ~((got.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(got) & torch.isnan(ref)))
    n = int(bad.sum())
    if n and not quiet:
        print(cr.describe(bad, got, ref, name))
    return n


# ---------------------------------------------------------------------------------------------------- references


def act_host(v, act):
    """Activation of float64 values as the kernels define it: relu keeps NaN and -0.0 (v < 0 ? 0 : v); tanh is the float64 one."""
    v = np.asarray(v, dtype=np.float64)
    if act == TANH:
        return np.tanh(v)
    if act == RELU:
        with np.errstate(invalid="ignore"):
            return np.where(v < 0, 0.0, v)
    return v.copy()


def dact(y, act):
    """act' from the saved OUTPUT: 1 - y^2, [y > 0] (y <= 0 ? 0 : 1), 1."""
    y = np.asarray(y, dtype=np.float64)
    if act == TANH:
        return 1.0 - y * y
    if act == RELU:
        return np.where(y <= 0, 0.0, 1.0)
    return np.ones_like(y)


def dact_mul(g, y, act):
    """g * act'(y) as the contract forms it: a product under tanh; under relu a SELECTION, torch's threshold_backward -- y <= 0 gives
    +0.0 whatever g is (its sign, an infinity, a NaN), anything else (a NaN y too) passes g unchanged."""
    if act == TANH:
        return g * (1.0 - y * y)
    if act == RELU:
        return 0.0 if y <= 0 else g
    return g


def act_pad_fwd(x, res, res_pitch, res_off, W, pad, act, storage, activated=None, defect=None):
    """x [rows][W]; res flat memory (or None), row r's element w at r * res_pitch + res_off + w -> out [rows][W + 2 pad] float32:
    out[r][pad + w] = act(x + res) formed in fp32 and rounded once to ``storage``; with pad, out[r][0] = out[r][W] and
    out[r][W + 1] = out[r][1] (copies).  ``activated`` [rows][W] fp32 replaces act(x + res) (the device's own tanhf values)."""
    x = _np(x).astype(np.float64)
    rows = x.shape[0]
    assert x.shape == (rows, W)
    out = np.zeros((rows, W + 2 * pad), dtype=f32)
    if activated is not None:
        a = np.asarray(activated, dtype=f32)
    else:
        v = x
        if res is not None:
            flat = _np(res).astype(np.float64).reshape(-1)
            idx = np.arange(rows)[:, None] * res_pitch + res_off + np.arange(W)[None, :]
            with np.errstate(invalid="ignore"):                           # (inf - inf among the specials)
                v = x + flat[idx]
        with np.errstate(over="ignore"):
            a = act_host(v.astype(f32), act).astype(f32)                 # the fp32 sum, then the activation rounded to fp32
    a = round_to(a, storage, defect)
    for r in range(rows):
        for w in range(W):
            out[r, pad + w] = a[r, w]
        if pad:
            out[r, 0] = out[r, W]
            out[r, W + 1] = out[r, 1]
    return out


def act_pad_bwd(g, y, W, pad, act, storage, with_res=False, defect=None):
    """g, y [rows][W + 2 pad] -> grad_x [rows][W] (and grad_res_padded [rows][W + 2]: grad_x between two columns of +0.0):
    (g[pad + w] + g[0] if w = W - 1 + g[W + 1] if w = 0) * act'(y[pad + w]) (``dact_mul``: relu selects), float64, rounded once."""
    g, y = _np(g).astype(np.float64), _np(y).astype(np.float64)
    rows = g.shape[0]
    assert g.shape == y.shape == (rows, W + 2 * pad)
    d = np.zeros((rows, W))
    for r in range(rows):
        for w in range(W):
            s = g[r, pad + w]
            if pad and defect != "no_wrap":
                if w == W - 1:
                    s = s + g[r, 0]
                if w == 0:
                    s = s + g[r, W + 1]
            d[r, w] = dact_mul(s, y[r, pad + w], act)
    gx = round_to(d.astype(f32), storage, defect)
    if not with_res:
        return gx
    gr = np.zeros((rows, W + 2), dtype=f32)
    gr[:, 1:W + 1] = gx
    return gx, gr


def out_width(W):
    return (W - 1) // 2 + 1


def pool_fwd(a_act, H, W, defect=None):
    """a_act [planes * H][W] ALREADY ACTIVATED values -> (out [rows][Wo + 2], win [rows][Wo] int8).  Window wo of row h holds the
    columns 2 wo - 1, 2 wo, 2 wo + 1 (mod W) of the rows h - 1 .. h + 1 that exist, scanned row-major; a candidate takes over if
    a > best or isnan(a); win = its position 0..8, starting from the first in-range position (3 when h == 0)."""
    a = _np(a_act).astype(np.float64).reshape(-1, W)
    rows, Wo = a.shape[0], out_width(W)
    assert rows % H == 0 and W >= 2
    out = np.zeros((rows, Wo + 2))
    win = np.zeros((rows, Wo), dtype=np.int8)
    for r in range(rows):
        h = r % H
        for wo in range(Wo):
            best = -np.inf
            k = 0 if (h > 0 or defect == "start_0_at_row_0") else 3
            for dh in (-1, 0, 1):
                if h + dh < 0 or h + dh >= H:
                    continue
                for dw in (-1, 0, 1):
                    v = a[r + dh, (2 * wo + dw) % W]
                    if (v >= best if defect == "tie_to_later" else v > best) or v != v:
                        best, k = v, (dh + 1) * 3 + dw + 1
            out[r, 1 + wo] = best
            win[r, wo] = k
        out[r, 0] = out[r, Wo]
        out[r, Wo + 1] = out[r, 1]
    return out, win


def pool_bwd(g, y, win, H, W, act, storage=torch.float32, defect=None):
    """Scatter form.  g, y [rows][Wo + 2] (y = the saved forward output), win [rows][Wo] -> grad_x [rows][W]: window (r, wo) adds
    (g[1 + wo] + g[0] if wo = Wo - 1 + g[Wo + 1] if wo = 0) * act'(y[1 + wo]) to the element it selected; float64 sums, one rounding."""
    g, y, win = _np(g).astype(np.float64), _np(y).astype(np.float64), _np(win).astype(np.int64)
    rows, Wo = win.shape
    assert Wo == out_width(W) and g.shape == y.shape == (rows, Wo + 2) and rows % H == 0
    gx = np.zeros((rows, W))
    for r in range(rows):
        h = r % H
        for wo in range(Wo):
            k = int(win[r, wo])
            rr, ww = r + k // 3 - 1, (2 * wo + k % 3 - 1) % W
            assert 0 <= k <= 8 and 0 <= h + k // 3 - 1 < H, "a window position outside the plane"
            s = g[r, 1 + wo]
            if defect != "no_wrap":
                if wo == Wo - 1:
                    s = s + g[r, 0]
                if wo == 0:
                    s = s + g[r, Wo + 1]
            gx[rr, ww] += dact_mul(s, y[r, 1 + wo], act)
    return round_to((gx + 0.0).astype(f32), storage, defect)


# ---------------------------------------------------------------------------------------------------- data makers


def saved(shape, act, seed):
    """Saved activations on a coarse grid: multiples of 1/4 up to 3/4 (tanh: 1 - y^2 is a multiple of 1/16), {0,1,2,3} (relu),
    integers in [-3, 3] (none)."""
    if act == TANH:
        return cr.saved_tanh(shape, seed).numpy()
    if act == RELU:
        return cr.saved_relu(shape, seed).numpy()
    return cr.ints(shape, 3, seed).numpy()


# largest gradient magnitude per storage type: integers that the type holds exactly, large enough that (sum of three) * k / 16 needs
# more significant bits than the type has, so that the ONE rounding of a half-precision backward is exercised
GMAX = {torch.float32: 3, torch.float16: 500, torch.bfloat16: 40}


def dead_garbage(g, y, lo, hi):
    """A copy of g with +inf, -inf and NaN at up to three elements (r, c), lo <= c < hi, whose saved output y[r, c] is <= 0: under relu
    such a unit is dead and its gradient is +0.0 whatever arrives (returns g itself if there is no such element)."""
    g = np.array(_np(g), dtype=np.float64)
    dead = np.argwhere(np.asarray(y)[:, lo:hi] <= 0)
    for (r, c), v in zip(dead[::max(1, len(dead) // 3)][:3].tolist(), (np.inf, -np.inf, np.nan)):
        g[r, lo + c] = v
    return g


def headroom(gmax, act, windows=6):
    """A window's gradient is a sum of up to three values of at most gmax; up to ``windows`` windows select one element; times
    act' on the grid 1/16: every partial sum, in any order, is below 2^23 grid steps -- exact in fp32."""
    steps = windows * 3 * float(gmax) * (16.0 if act == TANH else 1.0)
    assert steps < cr.LIMIT, f"headroom: {steps} grid steps"
    assert windows * 3 * float(gmax) < cr.FP16_MAX
    return steps


def _ord(v):
    """float32 -> integers whose order is the order of the floats (-0.0 and +0.0 both 0)."""
    b = np.asarray(v, dtype=f32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _from_ord(o):
    o = np.clip(np.asarray(o, dtype=np.int64), -0x7F800000, 0x7F800000)
    b = np.where(o < 0, (-o) | 0x80000000, o).astype(np.uint32)
    return b.view(f32)


def below(xm, k):
    """The float32 k representable steps below xm (never past -inf)."""
    return f32(_from_ord(_ord(f32(xm)) - int(k)))


TIE_MAGNITUDES = (1e-41, 1e-30, 1e-3, 0.5, 2.0, 4.0, 5.2, 5.3, 5.4, 7.0, 9.1, 20.0, np.inf, 0.0)
TIE_ULPS = (0, 1, 2, 3, 8, 64, 4096)
TIE_BAND = (0.5, 0.99, 1.01, 2.0)
FILLER = f32(-30.0)


def _candidates(xm):
    """The other candidates of a window whose maximum is xm: xm - k ulp, and the edge of the even kernel's threshold band
    xm - c * 24 * 6e-8 |a| / (1 - a^2), a = tanh(xm) (where that is finite)."""
    out = [below(xm, k) for k in TIE_ULPS]
    a = np.tanh(np.float64(xm))
    d = 1.0 - a * a
    for c in TIE_BAND:
        if np.isfinite(xm) and d > 0:
            v = f32(np.float64(xm) - c * 24.0 * max(6e-8 * abs(a), 1e-37) / d)
            out.append(v if np.isfinite(v) else below(xm, 5))
        else:
            out.append(below(xm, 5 + int(c * 100)))
    return out


def near_ties(act, seed=0):
    """List of (label, 3x3 float32 window): one window per case.  Maxima of every magnitude in TIE_MAGNITUDES with both signs, the
    maximum at each of the nine positions in turn, the other eight positions filled from ``_candidates`` (rotating with the seed, so
    runners-up come before and after the maximum in scan order); NaN first, in the middle, last and twice; for relu all-negative
    windows, -0.0 against +0.0 and a repeated positive maximum."""
    wins = []
    n = 0
    for m in TIE_MAGNITUDES:
        for sgn in (1.0, -1.0):
            xm = f32(sgn * m)
            cand = _candidates(xm)
            for pos in range(9):
                w = np.empty(9, dtype=f32)
                for j in range(9):
                    w[j] = cand[(j + pos + n + seed) % len(cand)]
                w[pos] = xm
                n += 1
                wins.append((f"max {float(xm)!r} at {pos}", w.reshape(3, 3)))
    base = np.array([0.5, -1.0, 0.25, 2.0, 0.5, -3.0, 2.0, 1.0, 0.0], dtype=f32)
    for label, where in (("first", (0,)), ("first of the middle row", (3,)), ("middle", (4,)), ("last", (8,)), ("last of the middle row", (5,)),
                         ("twice", (1, 7)), ("twice in the middle row", (3, 5)), ("before the maximum", (2,))):
        w = base.copy()
        for p in where:
            w[p] = np.nan
        wins.append((f"NaN {label}", w.reshape(3, 3)))
    if act == RELU:
        neg = -np.arange(1, 10, dtype=f32)
        wins.append(("all negative", neg.reshape(3, 3).copy()))
        for pos in range(9):
            for z0, z1 in ((-0.0, 0.0), (0.0, -0.0)):
                w = neg.copy()
                w[pos] = z0
                w[(pos + 4) % 9] = z1
                wins.append((f"zeros {z0!r} at {pos}, {z1!r} at {(pos + 4) % 9}", w.reshape(3, 3)))
            w = neg.copy()
            w[pos] = -0.0
            wins.append((f"-0.0 alone at {pos}", w.reshape(3, 3)))
            w = neg.copy()
            w[pos] = w[(pos + 5) % 9] = 3.0
            wins.append((f"positive maximum at {pos} and {(pos + 5) % 9}", w.reshape(3, 3)))
    return wins


def tile(windows, planes, H, W, start=0):
    """Lay windows into a [planes * H][W] float32 map without overlap, cycling through the list from ``start``: bands of three rows
    (the rows that exist when H < 3), pooled columns two apart, alternating between even and odd columns from band to band so that
    column 0 (the seam: its left neighbour is column W - 1) and the last pooled column are both reached.  Everything else is FILLER.
    Returns (map, placed) with placed = [(window index, row, pooled column)]."""
    Wo = out_width(W)
    x = np.full((planes * H, W), FILLER, dtype=f32)
    used = np.zeros((planes * H, W), dtype=bool)
    placed, n, band = [], int(start), 0
    centres = [0] if H < 3 else list(range(1, H - 1, 3))
    for p in range(planes):
        for hc in centres:
            phase = band % 2
            band += 1
            cols = list(range(phase, Wo, 2))
            if phase == 0 and Wo - 1 not in cols:
                cols.append(Wo - 1)
            for wo in cols:
                cells = [(p * H + hc + dh, (2 * wo + dw) % W, (dh + 1) * 3 + dw + 1) for dh in (-1, 0, 1) if 0 <= hc + dh < H for dw in (-1, 0, 1)]
                if any(used[r, c] for r, c, _ in cells):
                    continue
                w = windows[n % len(windows)][1].reshape(-1)
                for r, c, k in cells:                               # (W = 2: columns 2 wo - 1 and 2 wo + 1 coincide, the later one stays)
                    x[r, c] = w[k]
                    used[r, c] = True
                if len({(r, c) for r, c, _ in cells}) == 9:          # the whole window, intact
                    placed.append((n % len(windows), p * H + hc, wo))
                n += 1
    return x, placed


def bf16_specials():
    """(x, res) float32 arrays of bf16 numbers: the fp32 sum is a tie that rounds down to even, a tie that rounds up to even, just
    above and just below a tie (both signs); largest finite + largest finite; NaN; both zeros in every pairing; subnormal sums."""
    big = np.array([0x7F7F0000], dtype=np.uint32).view(f32)[0]
    sub = f32(2.0 ** -133)
    pairs = [(1.0, 2.0 ** -8), (1.0 + 2.0 ** -7, 2.0 ** -8), (1.0, 2.0 ** -8 + 2.0 ** -15), (1.0, 2.0 ** -8 - 2.0 ** -16),
             (3.0, 2.0 ** -7), (3.0 + 2.0 ** -6, 2.0 ** -7), (big, big), (big, 2.0 ** 119), (big, 2.0 ** 118), (np.nan, 1.0), (1.0, np.nan), (np.inf, -np.inf),
             (np.inf, 1.0), (sub, sub), (sub * 3, -sub), (2.0 ** -126, -(2.0 ** -126 - 2.0 ** -133)), (sub, -sub)]
    pairs += [(-a, -b) for a, b in pairs]
    pairs += [(-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0), (0.0, 0.0), (1.0, -1.0)]
    return np.array([p[0] for p in pairs], dtype=f32), np.array([p[1] for p in pairs], dtype=f32)


def fp16_specials():
    """The same for fp16 (11 significant bits): ties at 2^-11 beside 1, 65504 + 16 = 65520 (the tie that rounds to infinity)."""
    sub = f32(2.0 ** -24)
    pairs = [(1.0, 2.0 ** -11), (1.0 + 2.0 ** -10, 2.0 ** -11), (1.0, 2.0 ** -11 + 2.0 ** -21), (1.0, 2.0 ** -11 - 2.0 ** -22),
             (3.0, 2.0 ** -10), (3.0 + 2.0 ** -9, 2.0 ** -10), (65504.0, 65504.0), (65504.0, 16.0), (65504.0, 8.0), (65504.0, 24.0), (np.nan, 1.0), (1.0, np.nan),
             (np.inf, -np.inf), (np.inf, 1.0), (sub, sub), (sub * 3, -sub), (2.0 ** -14, -(2.0 ** -14 - 2.0 ** -24)), (sub, -sub)]
    pairs += [(-a, -b) for a, b in pairs]
    pairs += [(-0.0, -0.0), (-0.0, 0.0), (0.0, -0.0), (0.0, 0.0), (1.0, -1.0)]
    return np.array([p[0] for p in pairs], dtype=f32), np.array([p[1] for p in pairs], dtype=f32)


def specials(storage):
    return bf16_specials() if storage == torch.bfloat16 else fp16_specials()


def half_stem_input(planes, H, W, act, seed):
    """Input map of a half-precision stem case, every value a number of fp16 AND bf16.  tanh: integers in [-48, 48] / 8 -- the
    activations of DISTINCT inputs beyond 3.5 (bf16) / 4.5 (fp16) round to the SAME stored value, ties that only rnd<T> creates;
    otherwise integers in [-2, 2].  NaN at the first and the last element, in the middle and at two neighbours."""
    x = (ints((planes * H, W), 48, seed).numpy() / 8.0 if act == TANH else ints((planes * H, W), 2, seed).numpy()).astype(f32)
    flat = x.reshape(-1)
    if flat.size >= 16:
        for i in (0, flat.size - 1, flat.size // 2, flat.size // 3, flat.size // 3 + 1):
            flat[i] = np.nan
    return x


# ---------------------------------------------------------------------------------------------------- case tables

PAD_SHAPES = ((1, 1), (3, 2), (5, 7), (2, 64), (7, 130), (9, 255))                 # (rows, W); the last: three blocks of 1024, ragged tail
RES_KINDS = ("none", "dense", "padded", "foreign")


def res_layout(kind, W):
    """(res_pitch, res_off) of a residual variant; None without a residual."""
    return {"none": None, "dense": (W, 0), "padded": (W + 2, 1), "foreign": (W + 5, 3)}[kind]


# (planes, H, W).  The last even one is there for the even kernels alone: they run one thread per pooled column and FOUR rows, so none
# of the others gives them a second block (2 * 3 * 48 = 288 threads)
STEM_EVEN = ((1, 1, 2), (2, 1, 8), (1, 2, 2), (3, 3, 4), (2, 5, 6), (2, 4, 128), (1, 9, 130), (1, 6, 126), (2, 7, 34), (3, 8, 64), (2, 12, 96))
STEM_ODD = ((1, 1, 3), (2, 3, 3), (2, 2, 9), (1, 5, 131))
STEM_HALF = ((1, 1, 2), (2, 1, 8), (2, 5, 6), (2, 4, 128), (2, 2, 9), (1, 5, 131))
# (planes, H, W, skew in bytes of the pointer the dispatch looks at)
STEM_RUNS = tuple((p, h, w, s) for (p, h, w) in STEM_EVEN for s in (0, 4)) + tuple((p, h, w, 0) for (p, h, w) in STEM_ODD)


def stem_props(planes, H, W, skew):
    """What a stem case reaches in dl_ring_act_pool_pad_fwd / _bwd, from the dispatch rule (W even and the pointer 8-byte aligned ->
    the even kernels: one thread per pooled column and strip of STEM_RH rows, threads numbered strip-major)."""
    even = W % 2 == 0 and skew % 8 == 0
    props = {"even" if even else "general"}
    if W % 2 == 0 and not even:
        props.add("general at even W")
    if even:
        Wo, S = W // 2, (H + STEM_RH - 1) // STEM_RH
        total = planes * S * Wo
        if any((i % Wo) != 0 for i in range(0, total, WAVE)):
            props.add("lane 0 mid-row")
        if total % WAVE:
            props.add("idle lanes in the last wave")
        if H % STEM_RH:
            props.add("strip with h0 + 4 > H")
        if planes > 1:
            props.add("row h0 - 1 in the previous plane")
        if total > DL_BLOCK:
            props.add("more than one block")
    return props


STEM_PROPS = ("even", "general", "general at even W", "lane 0 mid-row", "idle lanes in the last wave", "strip with h0 + 4 > H",
              "row h0 - 1 in the previous plane", "more than one block")


def stem_case_seed(planes, H, W, act):
    return 71000 + 1009 * planes + 101 * H + 7 * W + 100000 * act


def stem_inputs(planes, H, W, act, kind):
    """The input map [planes * H][W] float32 of a stem case: "ints" (integers in [-2, 2]: ties everywhere) or "near" (near_ties of
    the activation, tiled from a case-dependent start so that the union of the cases places every window)."""
    if kind == "ints":
        return ints((planes * H, W), 2, stem_case_seed(planes, H, W, act)).numpy().astype(f32), None
    wins = near_ties(act)
    if H < 3:           # rows 0 and H - 1 only: begin with the windows of -inf, where nothing but the start code names a position
        return tile(wins, planes, H, W, [label for label, _ in wins].index("max -inf at 3"))
    start = 0           # the taller cases share the list out in table order: each begins where the one before it stopped
    for c in STEM_EVEN + STEM_ODD:
        if c == (planes, H, W):
            break
        if c[1] >= 3:
            start += len(tile(wins, *c, start)[1])
    return tile(wins, planes, H, W, start)
