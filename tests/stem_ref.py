"""Exact referee of the stem kernels (csrc/stem.hip): the wrapped 3x3 / stride-(1,2) max-pooling, its backward and the weight
gradient of conv1 fused with both (``dl_pool3x3s12_nhwc_fwd`` / ``_bwd``, ``dl_stem_wgrad_f32``, ``dl_stem_wgrad_workspace_bytes``).

Written from the text of include/delora_hip.h, not from the kernels:

  * references in float64 numpy / torch-CPU (``pool_fwd_ref``, ``pool_bwd_ref``, ``stem_wgrad_ref``) and ``plan``, the slab
    arithmetic of the fused launch restated,
  * seeded small-integer generators on which every product and partial sum of the weight gradient is an fp32 number
    (``headroom`` narrows the ranges of a case until ``conv_ref.headroom`` holds), synthetic ``win`` planes and special values,
  * a float32 emulation that follows the kernels' order of operations (gather form of the backward; pixel pairs per wave, waves
    0 + 1 + 2 + 3, slabs w, w + 4, ..., waves in order) -- it must equal the float64 reference bit for bit on the exact data and
    stay inside the derived bound on real-valued data,
  * planted defects: the emulation / the references with one change each, so that the suite is known to be able to fail,
  * the case tables of tests/test_gpu_stem_exact.py.

No GPU is needed to import it.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_ref as cr

NONE, TANH, RELU = cr.ACT_NONE, cr.ACT_TANH, cr.ACT_RELU
ACTS = (NONE, TANH, RELU)
ACT_NAME = {NONE: "none", TANH: "tanh", RELU: "relu"}
SG_PX = 64                       # conv1-output pixels per chunk of the fused weight gradient
SLAB_CAP = 512                   # stem_wgrad_slabs


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# ---------------------------------------------------------------------------------------------------- references


def _pool_fwd(a, defect=None):
    a = _np(a).astype(np.float64)
    N, H, Wc, C = a.shape
    assert Wc % 2 == 0 and Wc >= 2
    Wp = Wc // 2
    flat = a.reshape(N * H * Wc, C)
    nr = np.arange(N * H)[:, None]
    r = nr % H
    q = np.arange(Wp)[None, :]
    best = np.full((N * H, Wp, C), -np.inf)
    first = 0 if defect == "start_0_at_row_0" else 3
    k = np.broadcast_to(np.where(r > 0, 0, first)[:, :, None], best.shape).astype(np.int8).copy()
    for dh in (-1, 0, 1):                                       # rows first ...
        ok = ((r + dh >= 0) & (r + dh < H))[:, :, None]
        for dw in (-1, 0, 1):                                   # ... then columns
            j = 2 * q + dw
            if defect == "left_not_wrapped":                    # the element before (row, 0) in memory: the previous row's last one
                idx = np.clip((nr + dh) * Wc + j, 0, N * H * Wc - 1)
            else:
                idx = np.clip(nr + dh, 0, N * H - 1) * Wc + j % Wc     # the column left of column 0 is Wc - 1
            v = flat[idx]
            with np.errstate(invalid="ignore"):
                take = ((v >= best) if defect == "tie_to_later" else (v > best)) | np.isnan(v)
            take &= ok
            best = np.where(take, v, best)
            k = np.where(take, np.int8((dh + 1) * 3 + dw + 1), k)
    return best.reshape(N, H, Wp, C), k.reshape(N, H, Wp, C)


def pool_fwd_ref(a):
    """a [N][H][Wc][C] -> (y [N][H][Wc/2][C] float64, win int8 = position 0..8, row-major in the window).  The window of pooled
    column q holds the columns 2q - 1 (Wc - 1 for q = 0), 2q, 2q + 1 of the rows r - 1 .. r + 1 that exist; it is scanned rows
    first from the first in-range position (0 for r > 0, else 3), a strictly greater value or any NaN takes over."""
    return _pool_fwd(a)


def pool_bwd_ref(g, a, win, act):
    """g [N][H][Wp][C], a [N][H][Wc][C], win -> g_conv [N][H][Wc][C] float64: g scattered to the element each window selected,
    times act'(a) (conv_ref.dact).  The kernel SELECTS under relu (a <= 0 gives +0.0) where this multiplies (-g * 0 = -0.0), so a
    final + 0.0 makes every zero positive: no kernel path can produce -0.0 here (its sums start from +0.0)."""
    g, a, win = _np(g).astype(np.float64), _np(a).astype(np.float64), _np(win).astype(np.int64)
    N, H, Wc, C = a.shape
    Wp = Wc // 2
    assert g.shape == (N, H, Wp, C) and win.shape == g.shape and win.min() >= 0 and win.max() <= 8
    n, r, q, c = np.meshgrid(np.arange(N), np.arange(H), np.arange(Wp), np.arange(C), indexing="ij")
    rr, jj = r + win // 3 - 1, (2 * q + win % 3 - 1) % Wc
    assert rr.min() >= 0 and rr.max() < H, "a window position outside the image"
    out = np.zeros((N, H, Wc, C))
    np.add.at(out, (n, rr, jj, c), g)
    return out * cr.dact(torch.from_numpy(a), act).numpy() + 0.0


def stem_wgrad_ref(g, a, win, x8, act):
    """dw [64][8][3][3] float64 of conv1 (3x3, stride (1,2), wrap-around width) for the output gradient pool_bwd_ref(g, a, win, act):
    torch autograd (conv_ref.conv_grads)."""
    gc = torch.from_numpy(pool_bwd_ref(g, a, win, act))
    x8 = torch.from_numpy(_np(x8).astype(np.float64))
    dw = cr.conv_grads(x8, torch.zeros((gc.shape[3], 3, 3, x8.shape[3]), dtype=torch.float64), gc, (1, 2))[1]
    return dw.permute(0, 3, 1, 2).contiguous().numpy()


def plan(N, H, W):
    """(chunks, nslabs, chunks per slab, grid) of dl_stem_wgrad_f32 for an [N][H][W][8] input: 64-pixel chunks of the W/2-wide
    conv1 rows, at most 512 slabs; the workspace holds nslabs partials of [64][72] floats."""
    Wc = W // 2
    chunks = N * H * ((Wc + SG_PX - 1) // SG_PX)
    nslabs = min(chunks, SLAB_CAP)
    cps = (chunks + nslabs - 1) // nslabs
    return chunks, nslabs, cps, (chunks + cps - 1) // cps


def workspace_bytes(N, H, W):
    return 0 if (N <= 0 or H <= 0 or W <= 0 or W % 4) else plan(N, H, W)[1] * 64 * 72 * 4


# ---------------------------------------------------------------------------------------------------- generators


def gen_a(shape, act, seed):
    """Activated conv1 outputs (float64 numpy): integers in [-3, 3] without activation, {0, 1, 2, 3} for relu, multiples of 1/4 up
    to 3/4 for tanh.  Ties are everywhere, at the seam too."""
    if act == RELU:
        return cr.saved_relu(shape, seed).numpy()
    if act == TANH:
        return cr.saved_tanh(shape, seed).numpy()
    return cr.ints(shape, 3, seed).numpy()


def win_uniform(N, H, Wp, C, seed):
    """Window positions drawn uniformly from those valid at the row: 3..8 at row 0, 0..5 at row H - 1, 3..5 when H = 1."""
    r = np.arange(H)[None, :, None, None]
    lo, hi = np.where(r == 0, 3, 0), np.where(r == H - 1, 5, 8)
    u = cr._rng(seed).random(size=(N, H, Wp, C))
    return (lo + np.floor(u * (hi - lo + 1))).astype(np.int8)


SPECIAL_KINDS = ("pos_inf", "zeros_pm", "zeros_mp", "nan1", "nan2", "nan3", "neg_inf")      # the last one survives every overlap


def specials(a, seed=1):
    """A copy of ``a`` with planted windows: all -inf, one +inf, +0.0 before -0.0 and -0.0 before +0.0 among negative values, and
    one, two or three NaNs -- each at pooled column 0 and at the last one, in row 0 and in row H - 1 (images and channels rotate;
    in a narrow map the windows overlap, the reference decides what comes out)."""
    a = np.array(_np(a), dtype=np.float64)
    N, H, Wc, C = a.shape
    Wp = Wc // 2
    rng = cr._rng(seed)
    i = 0
    for kind in SPECIAL_KINDS:
        for r in (0, H - 1):
            for q in (0, Wp - 1):
                n, c = i % N, i % C
                i += 1
                pos = [(rr, (2 * q + dw) % Wc) for rr in (r - 1, r, r + 1) if 0 <= rr < H for dw in (-1, 0, 1)]      # scan order
                if kind == "neg_inf":
                    for (rr, j) in pos:
                        a[n, rr, j, c] = -np.inf
                elif kind == "pos_inf":
                    rr, j = pos[int(rng.integers(len(pos)))]
                    a[n, rr, j, c] = np.inf
                elif kind in ("zeros_pm", "zeros_mp"):
                    for (rr, j) in pos:
                        a[n, rr, j, c] = -float(rng.integers(1, 4))
                    i0, i1 = sorted(rng.choice(len(pos), size=2, replace=False).tolist()) if len(set(pos)) > 2 else (0, 1)
                    z = (0.0, -0.0) if kind == "zeros_pm" else (-0.0, 0.0)
                    a[n, pos[i1][0], pos[i1][1], c] = z[1]            # (the later one first: at Wc = 2 the positions coincide)
                    a[n, pos[i0][0], pos[i0][1], c] = z[0]
                else:
                    cnt = int(kind[3])
                    for p in rng.choice(len(pos), size=min(cnt, len(pos)), replace=False).tolist():
                        a[n, pos[p][0], pos[p][1], c] = np.nan
    return a


def garbage(g, a_shape, win, seed):
    """(g with 1e30, inf and NaN at about a quarter of its (window, channel) pairs -- at least one --, mask of the conv1 elements that
    none of those pairs selected): such an element must come out of the backward unchanged to the bit."""
    rng = cr._rng(seed)
    hit = rng.random(size=g.shape) < 0.25
    hit.reshape(-1)[int(rng.integers(hit.size))] = True
    g2 = np.where(hit, rng.choice(np.array([1e30, -1e30, np.inf, -np.inf, np.nan]), size=g.shape), g)
    clean = pool_bwd_ref(hit.astype(np.float64), np.ones(a_shape), win, NONE) == 0
    assert clean.any() and not clean.all()
    return g2, clean


def bits_differ(got, ref, name="", quiet=False):
    """Number of elements whose fp32 bit patterns differ (any NaN equals any NaN); -0.0 and +0.0 differ."""
    got = torch.as_tensor(_np(got)).float().contiguous()
    ref = torch.as_tensor(_np(ref)).float().contiguous()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = ~((got.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(got) & torch.isnan(ref)))
    n = int(bad.sum())
    if n and not quiet:
        print(cr.describe(bad, got, ref, name))
    return n


# ---------------------------------------------------------------------------------------------------- headroom

RANGES = ((3, 2), (2, 2), (2, 1), (1, 1))


def headroom(N, H, W, act):
    """(xmax, gmax) of a weight-gradient case: the widest of (3,2), (2,2), (2,1), (1,1) for which ``conv_ref.headroom`` holds over
    the N H W/2 pixels of conv1's output.  An element is selected by at most 3 x 2 windows, so |g_c| <= 6 gmax; under tanh the
    products g_c x live on the grid 1/16."""
    pixels = N * H * (W // 2)
    for xmax, gmax in RANGES:
        try:
            cr.headroom("wgrad", pixels, xmax, 6 * gmax, dact_tanh=(act == TANH))
            return xmax, gmax
        except AssertionError:
            continue
    raise AssertionError(f"no exact ranges for {(N, H, W)} with act {act}")


def wgrad_case(N, H, W, act, seed=None):
    """The operands of one exact weight-gradient case: g [N][H][W/4][64], a [N][H][W/2][64], win (pool_fwd_ref's own), x8."""
    xmax, gmax = headroom(N, H, W, act)
    sd = (seed if seed is not None else 31000 + 97 * N + 13 * H + W) * 4 + act
    a = gen_a((N, H, W // 2, 64), act, sd * 8 + 1)
    return {"N": N, "H": H, "W": W, "act": act, "a": a, "win": pool_fwd_ref(a)[1],
            "g": cr.ints((N, H, W // 4, 64), gmax, sd * 8 + 2).numpy(), "x8": cr.ints((N, H, W, 8), xmax, sd * 8 + 3).numpy()}


# ---------------------------------------------------------------------------------------------------- float32 emulation

f32 = np.float32


def pool_bwd_emul32(g, a, win, act, defect=None):
    """The backward in the kernel's GATHER form and order, in float32: every conv1 output looks up the windows that contain it --
    pooled rows r - 1, r, r + 1 (seen at window rows 2, 1, 0), pooled column j / 2 at window column 1 (j even) or 2 (j odd) and,
    for odd j, column j / 2 + 1 (0 after the last) at window column 0 -- and adds the gradients of those that selected it, then
    multiplies by act'(a) (relu: 0 where a <= 0)."""
    g, a, win = _np(g).astype(f32), _np(a).astype(f32), _np(win).astype(np.int64)
    N, H, Wc, C = a.shape
    Wp = Wc // 2
    gf, wf = g.reshape(N * H * Wp, C), win.reshape(N * H * Wp, C)
    nr = np.arange(N * H)[:, None]
    r = nr % H
    j = np.arange(Wc)[None, :]
    q0, col0, two = j >> 1, 1 + (j & 1), (j & 1) != 0
    q1 = q0 + 1 if defect == "q1_not_wrapped" else np.where(q0 + 1 == Wp, 0, q0 + 1)
    acc = np.zeros((N * H, Wc, C), dtype=f32)
    for d in (-1, 0, 1):
        row_ok = (r + d >= 0) & (r + d < H)
        if defect == "row_clamp_missing":                       # the neighbouring image's row (or the map's end) is compared
            rows, row_ok = np.clip(nr + d, 0, N * H - 1), np.ones_like(row_ok)
        else:
            rows = nr + np.where(row_ok, d, 0)
        for t in (0, 1):
            if t == 1 and defect == "second_window_omitted":
                continue
            valid = row_ok & ((t == 0) | two)
            code = np.where(valid, (1 - d) * 3 + (0 if t else col0), 255)
            idx = np.clip(rows * Wp + np.where(two & (t == 1), q1, q0), 0, N * H * Wp - 1)
            with np.errstate(invalid="ignore"):                  # (inf - inf where a test plants garbage in g)
                acc = acc + np.where(wf[idx] == code[:, :, None], gf[idx], f32(0))
    acc = acc.reshape(a.shape)
    if act == TANH:
        return acc if defect == "tanh_omitted" else acc * (f32(1) - a * a)
    if act == RELU:
        return np.where(a >= 0, acc, f32(0)) if defect == "relu_ge" else np.where(a <= 0, f32(0), acc)
    return acc


def _patches(x8, N, H, W):
    """[N*H][Wc][72] float32: column (tap, c) of conv1-output pixel (nr, j) = x8[row + tap / 3 - 1][(2 j + tap % 3 - 1) mod W][c],
    zero above and below the image."""
    x = _np(x8).astype(f32).reshape(N, H, W, 8)
    Wc = W // 2
    xp = np.zeros((N, H + 2, W, 8), dtype=f32)
    xp[:, 1:H + 1] = x
    out = np.zeros((N, H, Wc, 9, 8), dtype=f32)
    cols = 2 * np.arange(Wc)
    for r in range(3):
        for s in range(3):
            out[:, :, :, r * 3 + s] = xp[:, r:r + H][:, :, (cols + s - 1) % W]
    return out.reshape(N * H, Wc, 72)


def stem_wgrad_emul32(g, a, win, x8, act, defect=None):
    """dw [64][8][3][3] float32 in the fused kernels' order of additions: ``slab_partials_emul32`` then ``reduce_emul32``."""
    return reduce_emul32(slab_partials_emul32(g, a, win, x8, act, defect), defect)


def slab_partials_emul32(g, a, win, x8, act, defect=None):
    """part [grid][64][72] float32, the partial sums k_stem_wgrad leaves in the workspace.  A slab is ``cps`` consecutive 64-pixel
    chunks (chunk = (image row, 64-pixel piece), pixels past the row's end contribute zero); in a chunk wave w multiplies the
    pixels 16 w .. 16 w + 15, one fused multiply-add per pixel and accumulator element in pixel order (a 32x32x2 MFMA takes a
    pair); a slab's partial is ((wave 0 + wave 1) + wave 2) + wave 3.  Each fused multiply-add is a float64 product and sum
    rounded to float32."""
    N, H, Wc, K = _np(a).shape
    W = 2 * Wc
    assert K == 64 and _np(x8).shape == (N, H, W, 8)
    chunks, nslabs, cps, grid = plan(N, H, W)
    cpr = (Wc + SG_PX - 1) // SG_PX
    pool_defect = defect if defect in POOL_BWD_DEFECTS else None
    gc = pool_bwd_emul32(g, a, win, act, pool_defect).reshape(N * H, Wc, K)
    X = _patches(x8, N, H, W)
    pad = cpr * SG_PX - Wc
    if pad:
        if defect == "overhang_not_zeroed":                     # the pixels behind a row's end are the next row's first ones
            gflat = np.concatenate([gc.reshape(-1, K), np.zeros((SG_PX, K), dtype=f32)])
            idx = np.arange(N * H)[:, None] * Wc + np.arange(cpr * SG_PX)[None, :]
            gc = gflat[np.minimum(idx, gflat.shape[0] - 1)]
            X = X[:, np.arange(cpr * SG_PX) % Wc]                # (2 j + s - 1) mod W with j = Wc + j': the row's own first columns
        else:
            gc = np.concatenate([gc, np.zeros((N * H, pad, K), dtype=f32)], axis=1)
            X = np.concatenate([X, np.zeros((N * H, pad, 72), dtype=f32)], axis=1)
    gch = gc.reshape(chunks, SG_PX, K)
    Xch = X.reshape(chunks, SG_PX, 72)
    full = grid * cps
    if full > chunks:                                           # the short last slab: chunks that do not exist add nothing
        gch = np.concatenate([gch, np.zeros((full - chunks, SG_PX, K), dtype=f32)])
        Xch = np.concatenate([Xch, np.zeros((full - chunks, SG_PX, 72), dtype=f32)])
    gch = gch.reshape(grid, cps, 4, 16, K)                      # [slab][chunk of the slab][wave][pixel of the wave][k]
    Xch = Xch.reshape(grid, cps, 4, 16, 72)
    acc = np.zeros((grid, 4, K, 72), dtype=f32)
    for p in range(cps - 1 if (defect == "last_chunk_of_slab_skipped" and cps > 1) else cps):
        for t in range(16):
            if not gch[:, p, :, t].any():                       # (adding exact zeros changes no bit: the sums start from +0.0)
                continue
            prod = gch[:, p, :, t, :, None].astype(np.float64) * Xch[:, p, :, t, None, :].astype(np.float64)
            acc = (acc.astype(np.float64) + prod).astype(f32)
    return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]    # [slab][k][72]


def reduce_emul32(part, defect=None):
    """k_stem_wgrad_reduce: wave w adds the slabs w, w + 4, ... in order, the four sums are added in wave order; dw [64][8][3][3]."""
    grid, K = part.shape[0], part.shape[1]
    n_red = grid
    if defect == "reduce_tail_skipped":
        n_red = grid // 4 * 4
    elif defect == "slabs_32_skipped":
        n_red = min(grid, 32)
    red = np.zeros((4, K, 72), dtype=f32)
    for w in range(4):
        for sl in range(w, n_red, 4):
            red[w] = red[w] + part[sl]
    tot = ((red[0] + red[1]) + red[2]) + red[3]                 # [k][tap * 8 + c]
    if defect == "dw_k_tap_c":
        return tot.reshape(K, 8, 3, 3).copy()
    return tot.reshape(K, 9, 8).transpose(0, 2, 1).reshape(K, 8, 3, 3).copy()


# ---------------------------------------------------------------------------------------------------- planted defects

POOL_FWD_DEFECTS = ("tie_to_later", "start_0_at_row_0", "left_not_wrapped")
POOL_BWD_DEFECTS = ("q1_not_wrapped", "second_window_omitted", "row_clamp_missing", "relu_ge", "tanh_omitted")
WGRAD_DEFECTS = ("last_chunk_of_slab_skipped", "reduce_tail_skipped", "slabs_32_skipped", "overhang_not_zeroed", "dw_k_tap_c")


def pool_fwd_planted(a, defect):
    assert defect in POOL_FWD_DEFECTS
    return _pool_fwd(a, defect)


# ---------------------------------------------------------------------------------------------------- float64 tier


def op_count(N, H, W, act):
    """Rounded fp32 operations behind one element of dw, from csrc/stem.hip: 5 additions in pool_bwd_value's ``acc`` (six candidates,
    the first added to zero), the multiplication by act' (tanh: also a * a and 1 - ...; relu selects but counts as one), one fused
    multiply-add per pixel of a lane's chain in a slab (16 pixels of a wave per chunk, ``cps`` chunks), 3 additions of the four
    waves, the ceil(grid / 4) slab additions of a reduction wave (the first is added to zero; counted) and 3 more for the waves."""
    _, _, cps, grid = plan(N, H, W)
    return 5 + (3 if act == TANH else 1) + 16 * cps + 3 + (grid + 3) // 4 + 3


def wgrad_bound(g, a, win, x8, act):
    """Per element of dw [64][8][3][3]: c 2^-24 S_abs with S_abs the float64 sum over the pixels of |g_c| |x| (the weight gradient
    of |g_c| and |x|)."""
    N, H, W, _ = _np(x8).shape
    gc = torch.from_numpy(np.abs(pool_bwd_ref(g, a, win, act)))
    x = torch.from_numpy(np.abs(_np(x8).astype(np.float64)))
    s_abs = cr.conv_grads(x, torch.zeros((64, 3, 3, 8), dtype=torch.float64), gc, (1, 2))[1].permute(0, 3, 1, 2).contiguous().numpy()
    return op_count(N, H, W, act) * 2.0 ** -24 * s_abs


REAL_SHAPES = ((2, 16, 256), (8, 9, 264), (19, 27, 8))          # the last one: two chunks per slab on real-valued data
REAL_PREACT_STD = 0.5


def real_inputs(N, H, W, seed):
    """Gaussian x8 * 3, g, and conv1 weights [64][3][3][8] scaled so that the pre-activation has a standard deviation of about 0.5:
    the count of tanh's two extra operations holds while a^2 <= 1 - a^2; next to saturation the rounding of a * a is amplified by
    a^2 / (1 - a^2), and at this scale |a| > 0.99 (pre-activation beyond 5 standard deviations) does not occur in a sum's bulk."""
    r = cr._rng(seed)
    x8 = (r.standard_normal((N, H, W, 8)) * 3.0).astype(f32)
    g = r.standard_normal((N, H, W // 4, 64)).astype(f32)
    w = (r.standard_normal((64, 3, 3, 8)) * (REAL_PREACT_STD / (3.0 * np.sqrt(72.0)))).astype(f32)
    return x8, g, w


def conv1_host(x8, w, act):
    """conv1 + activation on the CPU in float64 rounded to float32 (the host tier's stand-in for the library's conv1)."""
    pre = cr.conv(torch.from_numpy(x8.astype(np.float64)), torch.from_numpy(w.astype(np.float64)), (1, 2))
    a = torch.tanh(pre) if act == TANH else torch.relu(pre) if act == RELU else pre
    return a.numpy().astype(f32)


# ---------------------------------------------------------------------------------------------------- case tables

# pooling: (N, H, Wc, C); the last one launches 513 = 2 * 256 + 1 forward threads (one thread = one pooled pixel x 4 channels)
POOL_CASES = ((1, 1, 2, 4), (1, 2, 2, 16), (2, 3, 4, 32), (1, 5, 6, 64), (3, 2, 10, 80), (1, 3, 66, 16), (2, 4, 130, 64), (1, 1, 64, 4),
              (1, 19, 54, 4))

# fused weight gradient: (N, H, W) of the network input -> (chunks, cps, grid), asserted literally against plan()
WGRAD_PLAN = {
    (1, 1, 8): (1, 1, 1), (1, 2, 8): (2, 1, 2), (1, 3, 8): (3, 1, 3), (2, 2, 8): (4, 1, 4), (1, 5, 8): (5, 1, 5),
    (1, 29, 8): (29, 1, 29), (2, 16, 8): (32, 1, 32), (3, 11, 8): (33, 1, 33), (1, 61, 8): (61, 1, 61), (1, 512, 8): (512, 1, 512),
    (19, 27, 8): (513, 2, 257), (25, 41, 8): (1025, 3, 342), (4, 43, 260): (516, 2, 258), (1, 2, 4): (2, 1, 2),
    (1, 3, 128): (3, 1, 3), (1, 3, 132): (6, 1, 6), (2, 5, 72): (10, 1, 10),
}
WGRAD_CASES = tuple(WGRAD_PLAN)
SKEW_CASE = (2, 5, 72)


def coverage(cases=WGRAD_CASES):
    """What the union of the cases must contain; returns the list of what is missing."""
    plans = [plan(*c) for c in cases]
    missing = []
    if not {1, 2, 3} <= {p[2] for p in plans}:
        missing.append("cps in {1, 2, 3}")
    if {p[3] % 4 for p in plans} != {0, 1, 2, 3}:
        missing.append("grid % 4 in {0, 1, 2, 3}")
    grids = [p[3] for p in plans]
    for what, ok in (("a grid below 29", any(x < 29 for x in grids)), ("a grid in 29..32", any(29 <= x <= 32 for x in grids)),
                     ("a grid above 60", any(x > 60 for x in grids)), ("grid < nslabs", any(p[3] < p[1] for p in plans)),
                     ("a short last slab", any(p[0] % p[2] for p in plans))):
        if not ok:
            missing.append(what)
    return missing


def seam_counts(g, win):
    """How many (window, channel) pairs with a non-zero gradient route it across a seam or onto an edge row: to column Wc - 1 from
    pooled column 0 (window column 0, the wrap), to column 0 (pooled column 0, window column 1), into row 0, into row H - 1."""
    g, win = _np(g), _np(win).astype(np.int64)
    H = win.shape[1]
    nz = g != 0
    rr = np.arange(H)[None, :, None, None] + win // 3 - 1
    return {"wrap to column Wc-1": int((nz[:, :, 0] & (win[:, :, 0] % 3 == 0)).sum()), "column 0": int((nz[:, :, 0] & (win[:, :, 0] % 3 == 1)).sum()),
            "row 0": int((nz & (rr == 0)).sum()), "row H-1": int((nz & (rr == H - 1)).sum())}


def pool_case_data(case, act, special=False):
    """(a, g, win_uniform) of a pooling case.  The seed is the first of a fixed sequence per (case, act) with which ``seam_counts`` is
    positive everywhere for the forward's positions and for the uniform ones (a map of four windows needs a second or third draw)."""
    N, H, Wc, C = case
    for salt in range(64):
        sd = 52000 + 1009 * N + 101 * H + 7 * Wc + C + 100000 * act + 1000000 * salt
        a = gen_a((N, H, Wc, C), act, sd)
        g, wu = cr.ints((N, H, Wc // 2, C), 2, sd + 2).numpy(), win_uniform(N, H, Wc // 2, C, sd + 3)
        if all(v > 0 for w in (pool_fwd_ref(a)[1], wu) for v in seam_counts(g, w).values()):
            return (specials(a, sd + 1) if special else a), g, wu
    raise AssertionError(f"no seed routes gradient across every seam of {case}")
