"""Exact referee of the convolution families (csrc/conv.hip, wino.hip, convh.hip, wgradh.hip, stem.hip).

On small-integer data every product and every partial sum of a convolution is exactly representable in fp32, in the Winograd
domain too (G, B^T, A^T of F(2x2,3x3) and of F(3x3,2x2) have only entries 0, +-1, +-1/2), so the summation order of a kernel
cannot matter: every fp32 kernel must equal a float64 CPU evaluation BIT FOR BIT, element by element, and every half-precision
kernel that value rounded once to nearest-even.  This module holds

  * the reference operators in torch-CPU float64 (channels-last in and out, autograd for the gradients),
  * seeded, portable integer generators,
  * ``headroom``: the proof obligation that a test's data stay exact (worst-case magnitude of any partial sum in any order, on
    the finest dyadic grid that occurs, below 2^23 grid steps),
  * arenas: every device buffer a test hands to the library is a view inside a larger allocation whose guard zones (and whose
    interior, for outputs and workspaces) hold a quiet-NaN pattern -- a write beside a buffer, an element never written and a
    workspace assumed to be zero all become visible,
  * a mismatch reporter that names where the wrong elements lie (seam column, last tile row / column, last image).

No GPU is needed to import it; the arena helpers take the device as an argument.
"""
import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_TANH, ACT_RELU = 0, 1, 2
EPI_ADD, EPI_ACT, EPI_DACT, EPI_ADD_GRID = 1, 2, 4, 8
DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

# ---------------------------------------------------------------------------------------------------- reference operators


def out_size(n, s):
    return -(-int(n) // int(s))


def _nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2)


def conv(x, w, stride=(1, 1)):
    """x [N,H,W,C], w [K,ks,ks,C] (float64, CPU) -> [N,Ho,Wo,K]: 3x3 with circular padding on W and zero padding on H, or 1x1
    unpadded; the reference network's layer."""
    assert x.dtype == torch.float64 and w.dtype == torch.float64
    ks = w.shape[1]
    xn, wn = _nchw(x), _nchw(w)
    if ks == 3:
        y = F.conv2d(F.pad(xn, (1, 1, 0, 0), mode="circular"), wn, stride=stride, padding=(1, 0))
    else:
        y = F.conv2d(xn, wn, stride=stride)
    return y.permute(0, 2, 3, 1).contiguous()


def dact(s, act):
    """act'(.) from the SAVED OUTPUT s of the activation, as the kernels' DACT epilogue forms it."""
    if act == ACT_TANH:
        return 1.0 - s * s
    if act == ACT_RELU:
        return (s > 0).to(s.dtype)
    return torch.ones_like(s)


def epilogue(v, flags=0, act=ACT_NONE, add=None, dsrc=None, add_grid=None, stride=(1, 1)):
    """The fused tail in the order of include/delora_hip.h: ADD, ACT (relu only: tanh cannot be exact), DACT; ADD_GRID adds a
    gradient that lives on the stride-phase (0,0) pixels."""
    if flags & EPI_ADD:
        v = v + add
    if flags & EPI_ADD_GRID:
        full = torch.zeros_like(v)
        full[:, ::stride[0], ::stride[1]] = add_grid
        v = v + full
    if flags & EPI_ACT:
        assert act == ACT_RELU, "only relu is exact"
        v = torch.relu(v)
    if flags & EPI_DACT:
        v = v * dact(dsrc, act)
    return v


def conv_grads(x, w, g, stride=(1, 1)):
    """(dx [N,H,W,C], dw [K,ks,ks,C]) of ``conv`` under torch autograd in float64."""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    conv(xr, wr, stride).backward(g)
    return xr.grad.contiguous(), wr.grad.contiguous()


def conv_dx(x_shape, w, g, stride=(1, 1)):
    """dx [N,H,W,C] of ``conv`` alone.  A stride-1 3x3 layer's is the same convolution of g with the taps flipped and the channel
    roles swapped (the padding is symmetric: wrap-around in W, zero rows in H) -- no autograd graph, no dw; any other layer's comes
    from autograd with respect to x only."""
    if w.shape[1] == 3 and tuple(stride) == (1, 1):
        return conv(g, w.flip(1, 2).permute(3, 1, 2, 0).contiguous())
    xr = torch.zeros(tuple(x_shape), dtype=torch.float64, requires_grad=True)      # (the map is linear: dx does not depend on x)
    return torch.autograd.grad(conv(xr, w, stride), xr, g)[0].contiguous()


def pool3x3s12(a):
    """Wrapped 3x3 max-pool of the stem: circular padding on W, -inf padding on H, stride (1,2).  a [N,H,W,C] -> [N,H,W/2,C]."""
    an = F.pad(_nchw(a), (1, 1, 0, 0), mode="circular")
    return F.max_pool2d(an, kernel_size=3, stride=(1, 2), padding=(1, 0)).permute(0, 2, 3, 1).contiguous()


def stem(x, w, act=ACT_RELU):
    """conv1 (3x3, stride (1,2)) + relu + wrapped 3x3/(1,2) max-pool: x [N,H,W,8], w [64,3,3,8] -> (a, pooled)."""
    assert act == ACT_RELU
    a = torch.relu(conv(x, w, (1, 2)))
    return a, pool3x3s12(a)


def basic_block(x, w1, w2, wd, stride, act_last=True):
    """BasicBlock with relu: relu(conv2(relu(conv1(x))) + shortcut), shortcut = x or the 1x1 strided convolution wd of x;
    ``act_last`` False leaves the final activation to the caller (the last block of a segment)."""
    h = torch.relu(conv(x, w1, stride))
    y = conv(h, w2) + (x if wd is None else conv(x, wd, stride))
    return torch.relu(y) if act_last else y


def conv_loops(x, w, stride=(1, 1)):
    """The same convolution as plain nested loops in numpy float64 (tiny shapes only): the referee's referee."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    N, H, W, C = x.shape
    K, ks = w.shape[0], w.shape[1]
    Ho, Wo = out_size(H, stride[0]), out_size(W, stride[1])
    y = np.zeros((N, Ho, Wo, K))
    p = 1 if ks == 3 else 0
    for n in range(N):
        for ho in range(Ho):
            for wo in range(Wo):
                for r in range(ks):
                    h = ho * stride[0] + r - p
                    if h < 0 or h >= H:
                        continue                                   # zero rows above and below
                    for s in range(ks):
                        ww = (wo * stride[1] + s - p) % W           # the image wraps around in W
                        for k in range(K):
                            y[n, ho, wo, k] += float(np.dot(w[k, r, s], x[n, h, ww]))
    return y


# ---------------------------------------------------------------------------------------------------- integer generators


def _rng(seed):
    return np.random.default_rng(int(seed))      # PCG64: the same stream on every platform


def ints(shape, amax, seed, density=1.0):
    """float64 tensor of integers uniform in [-amax, amax]; ``density`` < 1 zeroes the rest at random."""
    r = _rng(seed)
    v = r.integers(-amax, amax + 1, size=shape).astype(np.float64)
    if density < 1.0:
        v *= r.random(size=shape) < density
    return torch.from_numpy(v)


def saved_tanh(shape, seed):
    """Saved activations for DACT in tanh style: {0, +-1/4, +-1/2, +-3/4}, so that 1 - s^2 is an exact multiple of 1/16."""
    return torch.from_numpy(_rng(seed).integers(-3, 4, size=shape).astype(np.float64) * 0.25)


def saved_relu(shape, seed):
    """Saved relu outputs: {0, 1, 2, 3}, zeros about half of the time."""
    r = _rng(seed)
    return torch.from_numpy((r.integers(1, 4, size=shape) * (r.random(size=shape) < 0.5)).astype(np.float64))


# ---------------------------------------------------------------------------------------------------- headroom

LIMIT = 2.0 ** 23          # grid steps: every integer multiple of the grid below this is an fp32 number with a bit to spare
FP16_MAX = 65504.0


def headroom(kind, terms, amax, bmax, taps=9, add=0.0, dact_tanh=False, storage=torch.float32):
    """Assert that a convolution-like sum stays exact in fp32 whatever order a kernel adds it up in, and return the worst case in
    grid steps.  ``terms`` = reduction positions with a non-zero contribution (input channels of a forward / input-gradient
    pass, output pixels of a direct weight gradient, 2x2 tiles of a Winograd-domain one); ``amax``, ``bmax`` = the largest
    magnitudes of the two operands; ``taps`` = filter taps per position (9 or 1; forward kinds only).

      direct       every partial sum is an integer of at most  taps * terms * amax * bmax
      wino_conv    F(2x2,3x3): |B^T d B| <= 4 amax (integers), |G g G^T| <= (3/2)^2 bmax on the grid 1/4, their channel sums
                   <= 9 terms amax bmax, the output transform adds up to 9 of those: 81 * terms * amax * bmax on the grid 1/4
      wgrad        direct weight gradient: terms * amax * bmax, integers
      wino_wgrad   F(3x3,2x2): |B^T d B| <= 4 amax, the 2x2 gradient tile transforms to <= 4 bmax (integers; the halves of G
                   may also sit in the output transform), tile sums <= 16 terms amax bmax, the output transform (rows of
                   absolute sum 2, both ways) 64 * terms * amax * bmax on the grid 1/4
    The tail adds ``add`` (an integer magnitude) and, with ``dact_tanh``, multiplies by 1 - s^2, a multiple of 1/16 of at most 1:
    the final value then lives on the grid 1/16.  Half-precision storage: the stored magnitude must also stay finite in fp16
    (the rounding itself is what the tests pin, so it need not be exact)."""
    ab = float(amax) * float(bmax) * float(terms)
    if kind == "direct":
        worst, grid, final = taps * ab, 1.0, taps * ab
    elif kind == "wino_conv":
        worst, grid, final = 81.0 * ab, 0.25, 9.0 * ab
    elif kind == "wgrad":
        worst, grid, final = ab, 1.0, ab
    elif kind == "wino_wgrad":
        worst, grid, final = 64.0 * ab, 0.25, ab
    else:
        raise ValueError(kind)
    steps = worst / grid
    final = final + float(add)
    steps = max(steps, final / (1.0 / 16.0 if dact_tanh else 1.0))
    assert steps < LIMIT, f"headroom({kind}): worst case {steps:.0f} grid steps is not below 2^23 -- the test would no longer be exact"
    if storage == torch.float16:
        assert final < FP16_MAX, f"headroom({kind}): |value| up to {final:.0f} overflows fp16"
    return steps


# ---------------------------------------------------------------------------------------------------- arenas

GUARD_MIN_BYTES = 256 * 1024
GUARD_ROWS = 32                      # the tallest tile group: the 4-column Winograd groups have 16 tile rows = 32 image rows
NAN_WORD = {torch.float32: 0x7FC0DEAD, torch.float16: 0x7E017E01, torch.bfloat16: 0x7FC17FC1,      # quiet NaNs in every lane
            torch.int8: 0x7FC0DEAD, torch.int32: 0x7FC0DEAD, torch.int64: 0x7FC0DEAD}


def _as_i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


class Arenas:
    """The device buffers of one test.  ``arena`` returns a contiguous view inside a larger 1-D allocation; ``check`` proves that
    no guard word changed, no input changed and no NaN is left in an output."""

    def __init__(self, device, skew=0):
        self.device, self.skew, self.items = device, int(skew), []

    def arena(self, shape, dtype, fill=None, name="", row_elems=None):
        """``fill`` None: an output / workspace (interior = NaN pattern); a CPU tensor: an input (copied in, must stay unchanged).
        Guard on each side: the larger of 32 image rows of this tensor (``row_elems`` elements per row; default W*C of an NHWC
        shape) and 256 KiB.  The view starts ``skew`` bytes past a 256-byte boundary."""
        shape = tuple(int(s) for s in shape)
        esz = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape)) if shape else 1
        if row_elems is None:
            row_elems = shape[-2] * shape[-1] if len(shape) == 4 else 0
        guard = max(GUARD_MIN_BYTES, GUARD_ROWS * row_elems * esz)
        guard = (guard + 255) // 256 * 256
        body = (n * esz + 3) // 4 * 4
        total = guard + self.skew + body + guard + 512
        raw = torch.empty((total // 4 + 1,), dtype=torch.int32, device=self.device)
        raw.fill_(_as_i32(NAN_WORD[dtype]))
        pad = (-raw.data_ptr()) % 256                       # (the allocator's blocks are 512-byte aligned; do not rely on it)
        start = pad + guard + self.skew
        assert start % 4 == 0
        view = raw.view(torch.uint8)[start:start + n * esz].view(dtype).view(shape)
        assert view.data_ptr() % 256 == self.skew % 256 and view.is_contiguous()
        item = {"raw": raw, "view": view, "name": name, "lo": start // 4, "hi": (start + body) // 4, "dtype": dtype, "input": None,
                "word": _as_i32(NAN_WORD[dtype]), "tail_bytes": body - n * esz}
        if fill is not None:
            view.copy_(fill.to(dtype))
            item["input"] = view.clone()
        self.items.append(item)
        return view

    def freeze(self, view):
        """An output (prepared weights) becomes an input of what follows."""
        for it in self.items:
            if it["view"] is view:
                it["input"] = view.clone()
                return view
        raise KeyError("not an arena view")

    def check(self, what=""):
        """One device round trip: per arena the number of changed guard words below and above, and of changed input bytes."""
        counts = []
        for it in self.items:
            raw, w = it["raw"], it["word"]
            counts += [(raw[:it["lo"]] != w).sum(), (raw[it["hi"]:] != w).sum(),
                       (it["view"].view(torch.uint8) != it["input"].view(torch.uint8)).sum() if it["input"] is not None else torch.zeros((), dtype=torch.int64, device=raw.device)]
        counts = torch.stack(counts).cpu().view(-1, 3).tolist() if counts else []
        for it, (lo_bad, hi_bad, in_bad) in zip(self.items, counts):
            raw, w = it["raw"], it["word"]
            assert lo_bad == 0 and hi_bad == 0, (f"{what}: guard of {it['name']} touched: {lo_bad} words below, {hi_bad} above the buffer; "
                                                 f"first above at word +{int(torch.nonzero(raw[it['hi']:] != w)[0]) if hi_bad else -1}, "
                                                 f"last below at word -{it['lo'] - int(torch.nonzero(raw[:it['lo']] != w)[-1]) if lo_bad else -1}")
            assert in_bad == 0, f"{what}: input {it['name']} was modified ({in_bad} bytes)"

    def check_output(self, view, what=""):
        if view.dtype.is_floating_point:
            n = int(torch.isnan(view).sum())
            assert n == 0, f"{what}: {n} elements were never written (NaN left in the output)"


# ---------------------------------------------------------------------------------------------------- mismatch reporter


def mismatches(got, ref, name, tile=(2, 2)):
    """Count of elements of ``got`` (device or CPU, [N,H,W,K]-like or anything) that differ from ``ref`` in value; a non-zero count
    is printed with its first coordinates and where the wrong elements lie."""
    got = got.detach().cpu()
    ref = ref.to(got.dtype)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = ~((got == ref) | (torch.isnan(got) & torch.isnan(ref)))
    n = int(bad.sum())
    if n:
        print(describe(bad, got, ref, name, tile))
    return n


def describe(bad, got, ref, name, tile=(2, 2)):
    idx = torch.nonzero(bad)
    n = idx.shape[0]
    lines = [f"{name}: {n} of {bad.numel()} elements differ"]
    for row in idx[:8].tolist():
        t = tuple(row)
        lines.append(f"    at {t}: got {float(got[t])!r}, expected {float(ref[t])!r}")
    if bad.dim() == 4:
        N, H, W, K = bad.shape
        nn, hh, ww = idx[:, 0], idx[:, 1], idx[:, 2]
        th, tw = tile
        last_row0, last_col0 = (H - 1) // th * th, (W - 1) // tw * tw
        where = {"in the last image": int((nn == N - 1).sum()), "at column 0": int((ww == 0).sum()), f"at column W-1 = {W - 1}": int((ww == W - 1).sum()),
                 f"in the last tile row (h >= {last_row0})": int((hh >= last_row0).sum()),
                 f"in the last tile column (w >= {last_col0})": int((ww >= last_col0).sum())}
        lines.append("    of these: " + "; ".join(f"{v} {k}" for k, v in where.items()))
        if int(((ww == 0) | (ww == W - 1)).sum()) == n:
            lines.append("    ALL mismatches lie on the wrap-around seam (columns 0 / W-1)")
        lines.append(f"    columns: {sorted(set(ww.tolist()))[:16]}  rows: {sorted(set(hh.tolist()))[:16]}  images: {sorted(set(nn.tolist()))[:8]}")
    return "\n".join(lines)
