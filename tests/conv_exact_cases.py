"""Shapes of the bit-exact convolution tests (tests/test_gpu_conv_exact.py) and the bookkeeping that proves their coverage:
which kernel instantiations every case reaches (asked of the dispatch itself through ``dl_conv_plan_describe``), which
instantiations the dispatch can select at all, and the value ranges that keep every case exact (``conv_ref.headroom``).
``persistent_cases`` sizes the launches with more Winograd tile groups than CUs (tests/test_gpu_wino_persistent_exact.py) from a CU
count; ``ALL`` holds those of 256 CUs, ``FIXED`` everything else.

Host only: the GPU tests and tests/test_conv_ref_host.py import it.
"""
import re

import torch

from tests import conv_ref as cr

F32, F16, BF16 = 0, 1, 2
TORCH_DTYPE = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
STRIDED_GEOMS = [(3, (1, 2)), (3, (2, 2)), (1, (1, 2)), (1, (2, 2))]          # every strided layer kind the network has


class Case:
    """One layer shape: x [N,H,W,C] -> K channels, kernel ks, stride; dtype code; ``xmax`` / ``wmax`` the integer ranges.
    ``passes`` names what a test may run of it, out of "forward", "dgrad", "wgrad": a pass left out is neither computed by the
    reference nor counted in ``headroom`` (the weight gradient of a large batch is what narrows the ranges, or refuses the case)."""

    def __init__(self, N, H, W, C, K, ks=3, stride=(1, 1), dtype=F32, xmax=None, wmax=None, why="", passes=("forward", "dgrad", "wgrad")):
        self.N, self.H, self.W, self.C, self.K, self.ks, self.stride, self.dtype = N, H, W, C, K, ks, tuple(stride), dtype
        self.why, self.passes = why, tuple(passes)
        assert set(self.passes) <= {"forward", "dgrad", "wgrad"} and self.passes
        self.Ho, self.Wo = cr.out_size(H, stride[0]), cr.out_size(W, stride[1])
        # value ranges: x, g, shortcut in [-xmax, xmax], weights in [-wmax, wmax] -- the widest of (3,2), (2,2), (2,1), (1,1) that
        # ``headroom`` accepts for every sum of the case (the weight gradient of a large image is the one that narrows them)
        for self.xmax, self.wmax in ([(xmax, wmax)] if xmax else [(3, 2), (2, 2), (2, 1), (1, 1)]):
            try:
                self.headroom()
                break
            except AssertionError:
                continue

    @property
    def id(self):
        return f"{['f32', 'f16', 'bf16'][self.dtype]}-{self.N}x{self.H}x{self.W}-c{self.C}-k{self.K}-{self.ks}x{self.ks}s{self.stride[0]}{self.stride[1]}"

    @property
    def s1(self):
        return self.ks == 3 and self.stride == (1, 1)

    @property
    def dgrad_ok(self):
        return "dgrad" in self.passes and self.C % 64 == 0           # (the input gradient's output channels must tile)

    @property
    def wgrad_ok(self):
        return "wgrad" in self.passes and self.C % 64 == 0 and self.K % 64 == 0

    @property
    def direct_ok(self):
        """Whether the direct entry point takes the forward pass.  Asked of the dispatch for channel counts that are no multiple of
        64 (a stride-1 3x3 image that does not divide into 256-pixel tiles reduces in chunks of 16 channels: C = 8, 24, 72 are then
        refused and the Winograd kernel, which takes any C % 8 == 0, is compared with the reference alone); a refusal of any
        other case stays an error."""
        if self.C % 64 == 0:
            return True
        from delora_amd import _lib as L
        try:
            L.conv_plan(L.PLAN_CONV, self.dtype, self.N, self.H, self.W, self.C, self.K, self.ks, self.stride[0], self.stride[1], 0, 256)
            return True
        except L.DeloraHipError as e:
            assert "does not tile" in str(e), e
            return False

    def seed(self, salt=0):
        return (self.N * 1000003 + self.H * 10007 + self.W * 101 + self.C * 7 + self.K * 3 + self.ks + 10 * self.stride[0] + 100 * self.stride[1]
                + 1000 * self.dtype) * 16 + salt

    # ---- what the GPU test runs for this case, as (op, dtype, N, H, W, C, K, ks, sh, sw, mode) of dl_conv_plan_describe
    def plan_queries(self):
        from delora_amd import _lib as L
        N, H, W, C, K, ks, (sh, sw), dt = self.N, self.H, self.W, self.C, self.K, self.ks, self.stride, self.dtype
        q = [(L.PLAN_CONV, dt, N, H, W, C, K, ks, sh, sw, 0)] if self.direct_ok else []
        if self.s1:
            if self.dgrad_ok:
                q.append((L.PLAN_CONV, dt, N, H, W, K, C, 3, 1, 1, 1))                     # input gradient: the transposed pass
            if dt == F32:
                q.append((L.PLAN_WINO_CONV, F32, N, H, W, C, K, 3, 1, 1, 0))
                if self.dgrad_ok:
                    q.append((L.PLAN_WINO_CONV, F32, N, H, W, K, C, 3, 1, 1, 0))
                if W >= 2 and self.wgrad_ok:
                    q += [(L.PLAN_WINO_WGRAD, F32, N, H, W, C, K, 3, 1, 1, 0), (L.PLAN_WINO_WGRAD_BATCH, F32, N, H, W, C, K, 3, 1, 1, 0)]
        elif self.dgrad_ok:
            q.append((L.PLAN_DGRAD_STRIDED, dt, N, H, W, C, K, ks, sh, sw, 1 if ks == 1 else 0))
        if self.wgrad_ok:
            q += [(L.PLAN_WGRAD, dt, N, H, W, C, K, ks, sh, sw, 0), (L.PLAN_WGRAD_BATCH, dt, N, H, W, C, K, ks, sh, sw, 0)]
        return q

    def labels(self, cu_count=0):
        out = set()
        for q in self.plan_queries():
            out |= labels_of(q, cu_count)
        return out

    # ---- exactness: every sum the case's kernels form, in any order
    def headroom(self):
        st = TORCH_DTYPE[self.dtype]
        taps = self.ks * self.ks
        add = max(self.xmax, 3)
        worst = [cr.headroom("direct", self.C, self.xmax, self.wmax, taps=taps, add=add, dact_tanh=True, storage=st),        # forward
                 cr.headroom("direct", self.K, self.xmax, self.wmax, taps=taps, add=add, dact_tanh=True, storage=st)]        # input gradient
        if self.s1 and self.dtype == F32:
            worst += [cr.headroom("wino_conv", self.C, self.xmax, self.wmax, add=add, dact_tanh=True),
                      cr.headroom("wino_conv", self.K, self.xmax, self.wmax, add=add, dact_tanh=True)]
        if self.wgrad_ok:
            worst.append(cr.headroom("wgrad", self.N * self.Ho * self.Wo, self.xmax, self.xmax))
            if self.s1 and self.dtype == F32 and self.W >= 2:
                worst.append(cr.headroom("wino_wgrad", self.N * cr.out_size(self.H, 2) * cr.out_size(self.W, 2), self.xmax, self.xmax))
        return max(worst)


_TAIL = re.compile(r" grid=(\d+)x\d+x\d+ block=\d+")
_WINO = re.compile(r"k_wino_conv<(\d+), (true|false), (true|false)>$")
SEVERAL = "several groups per workgroup"


def wino_groups(line, N, H, W, K):
    """(tile groups, grid) of a ``k_wino_conv<TC, RAG, SPLIT>`` plan line for an N x H x W image with K output channels, or None
    for any other line: N * ceil(th / TR) * ceil(tw / TC) * K / 64 groups of TR x TC tiles (TR = 64 / TC), times the channel ranges
    of a split launch -- the ``ngroups`` of csrc/wino_conv_body.h, restated from the line's own TC / RAG."""
    s = wino_shape(line, H, W)
    if not s:
        return None
    tr, tc, tiles_h, tiles_w, splits, grid = s
    return N * tiles_h * tiles_w * (K // 64) * splits, grid


def wino_shape(line, H, W):
    """(TR, TC, tile-group rows, tile-group columns per image, channel ranges, grid) of a ``k_wino_conv`` plan line, else None."""
    m = _TAIL.search(line)
    w = _WINO.match(line[:m.start()])
    if not w:
        return None
    tc, rag = int(w.group(1)), w.group(2) == "true"
    tr = 64 // tc
    th, tw = (H + 1) // 2, (W + 1) // 2
    assert rag or (H % 2 == 0 and W % 2 == 0 and th % tr == 0 and tw % tc == 0), line
    splits = [int(n[7:]) for n in line[m.end():].split() if n.startswith("splits=")]
    return tr, tc, -(-th // tr), -(-tw // tc), (splits[0] if splits else 1), int(m.group(1))


def labels_of(query, cu_count=0):
    """Labels of one dispatch query: the kernel instantiation of every launch; a Winograd split adds "<kernel> splits=<n>", a
    merged weight-gradient launch "<kernel> one slab" (it writes dW directly) or "<kernel> slabs" (partials + reduction), a
    Winograd launch with fewer workgroups than tile groups "<kernel> several groups per workgroup" (the persistent loop's
    hand-over from one group to the next runs)."""
    from delora_amd import _lib as L
    op, dt, N, H, W, C, K, ks, sh, sw, mode = query
    out = set()
    for line in L.conv_plan(op, dt, N, H, W, C, K, ks, sh, sw, mode, cu_count):
        m = _TAIL.search(line)
        name, notes = line[:m.start()], line[m.end():].split()
        out.add(name)
        for n in notes:
            if n.startswith("splits="):
                out.add(f"{name.split('<')[0]} {n}")
            elif n.startswith("slabs=") and "_batch" in name:
                out.add(f"{name} {'one slab' if n == 'slabs=1' else 'slabs'}")
        gg = wino_groups(line, N, H, W, K) if op == L.PLAN_WINO_CONV else None
        if gg and gg[1] < gg[0]:
            out.add(f"{name} {SEVERAL}")
    return out


def queries_of_shape(N, H, W, C, K, dtypes=(F32, F16, BF16)):
    """Every dispatch query a layer shape admits (all kernel sizes, strides and passes)."""
    out = []
    for dt in dtypes:
        for ks, st in [(3, (1, 1))] + STRIDED_GEOMS:
            out += Case(N, H, W, C, K, ks, st, dt).plan_queries()
    return out


def reachable_labels(cu_count, dtypes=(F32, F16, BF16)):
    """What the dispatch can select for channel counts 64..512 (160 and 192 where a rule needs C > 128 or K % 128 != 0) over a grid
    of image sizes wide enough for every rule: sizes that divide into every tile shape and sizes that divide into none, one to 64 rows,
    2 to 1024 columns, batch 1 and 8 (the half-precision tiles of layer3 / layer4 need up to 131 072 pixels)."""
    from delora_amd import _lib as L
    out = set()
    for N in (1, 8):
        for H in (1, 4, 7, 8, 15, 31, 32, 64):
            for W in (2, 7, 14, 16, 30, 32, 45, 62, 64, 128, 256, 512):
                for C in (64, 128, 160, 192, 256, 512):
                    for K in (64, 128, 192, 256, 512):
                        for q in queries_of_shape(N, H, W, C, K, dtypes):
                            try:
                                out |= labels_of(q, cu_count)
                            except L.DeloraHipError:
                                pass                       # (a channel count the entry point rejects)
    # one rule wants more work than batch 8 gives the narrowest images: the cap of a Winograd grid at the CU count (a 64 x 7 image
    # has two groups of 16 x 4 tiles per 64-channel block)
    for W in (7, 14, 30, 62, 64):
        for q in Case(64, 64, W, 64, 512, passes=("forward",)).plan_queries():
            if q[0] == L.PLAN_WINO_CONV and F32 in dtypes:
                out |= labels_of(q, cu_count)
    return out


# ---------------------------------------------------------------------------------------------------- the cases
def _s1(N, H, W, C, K, **kw):
    return Case(N, H, W, C, K, 3, (1, 1), **kw)


# fp32, stride-1 3x3: direct and Winograd forward / input gradient, direct and Winograd-domain weight gradients (single and merged)
S1_F32 = [
    # the twelve (TC, RAG, SPLIT) instantiations of k_wino_conv and split counts 2..16 (at 256 CUs)
    _s1(1, 4, 64, 64, 64, why="<32,F,F>; direct 256x64 CK8 TW64"), _s1(1, 4, 64, 128, 64, why="<32,F,T> 4 splits"),
    _s1(1, 8, 32, 64, 64, why="<16,F,F>"), _s1(1, 8, 32, 128, 128, why="<16,F,T>"),
    _s1(1, 3, 62, 64, 64, why="<32,T,F>"), _s1(1, 3, 62, 128, 64, why="<32,T,T>"),
    _s1(1, 7, 30, 64, 64, why="<16,T,F>"), _s1(1, 7, 30, 128, 64, why="<16,T,T>"),
    _s1(1, 15, 14, 64, 64, why="<8,T,F>"), _s1(1, 15, 14, 128, 64, why="<8,T,T>"),
    _s1(1, 31, 7, 64, 64, why="<4,T,F>"), _s1(1, 31, 7, 128, 64, why="<4,T,T>"),
    _s1(1, 4, 64, 512, 64, why="16 splits"), _s1(1, 4, 64, 256, 64, why="8 splits; direct CK16 TW64"),
    _s1(2, 4, 64, 128, 128, why="2 splits"),
    # direct tiles: 256-pixel tiles need Wo % 128 == 0 and even Ho, or Wo % 64 == 0 and Ho % 4 == 0; everything else 128 pixels
    _s1(1, 2, 128, 64, 64, why="direct 256x64 CK8 TW128"), _s1(1, 2, 128, 256, 64, why="direct 256x64 CK16 TW128"),
    _s1(1, 1, 128, 64, 64, why="H = 1; direct 128 TW128"),
    # the sizes that matter: the shipped 64x720 image's feature maps, odd heights, W = 2
    _s1(2, 5, 180, 64, 64, why="width 180"), _s1(1, 6, 90, 64, 128, why="width 90"), _s1(2, 5, 45, 64, 64, why="width 45, odd"),
    _s1(1, 7, 23, 128, 64, why="width 23"), _s1(1, 3, 2, 64, 64, why="W = 2"), _s1(1, 1, 2, 64, 64, why="W = 2, H = 1"),
    _s1(3, 18, 16, 64, 192, why="more than one tile group per image, last one overhanging; K = 192"),
]
# chunk counts a workgroup of k_wino_conv walks (C / 8, forward only: the input gradient would have C output channels): 1 -- only the
# tail body runs, raw(0) is fetched twice; 2 -- first chunk body and tail, the steady loop empty; 3 and 9 -- odd, the last chunk sits in
# the upper buffer; 20 -- split four ways at 256 CUs, ranges of 5 chunks.  On an even image (<32,F>) and a ragged one (<16,T>).
CHUNK_CHANNELS = {8: 1, 16: 2, 24: 3, 72: 9, 160: 20}
for _H, _W in ((4, 64), (7, 30)):
    S1_F32 += [_s1(1, _H, _W, _C, 64, why=f"{_n} chunks of 8 input channels") for _C, _n in CHUNK_CHANNELS.items()]

# fp32, strided layers: forward, stride-phase input gradient (seam terms on odd widths), dense 1x1, weight gradients
STRIDED_F32 = []
for _ks, _st in STRIDED_GEOMS:
    for _C in (64, 512):
        # output widths 128 / 64 / 32 / 16 pick the four tile widths of the 128-pixel tiles; C <= 256 / C = 512 the 8- / 16-channel chunks
        for _Wo in (128, 64, 32, 16):
            STRIDED_F32.append(Case(1, 8 * _st[0], _Wo * _st[1], _C, 64, _ks, _st, why=f"tile width {_Wo}"))
STRIDED_F32 += [
    Case(1, 4, 256, 64, 64, 3, (1, 2), why="stride (1,2) forward on 256-pixel tiles"),
    # odd widths: the seam path, H not a multiple of 16, both row strides; the shipped widths 180 / 90 / 45 / 23
    Case(2, 7, 45, 64, 128, 3, (1, 2), why="odd width, seam, H % 16 != 0"), Case(2, 19, 45, 64, 64, 3, (2, 2), why="odd width, seam, two row tiles"),
    Case(1, 5, 23, 128, 64, 3, (2, 2), why="width 23, odd height"), Case(1, 8, 180, 64, 128, 3, (1, 2)), Case(1, 6, 90, 128, 64, 3, (2, 2)),
    Case(2, 8, 45, 64, 128, 1, (2, 2), why="1x1 on an odd width"), Case(1, 5, 90, 64, 64, 1, (1, 2)), Case(1, 3, 3, 64, 64, 3, (2, 2), why="W = 3"),
    Case(1, 1, 2, 64, 64, 3, (1, 2), why="W = 2, H = 1"),
]

# half precision (both storage types): stride-1 tiles by pixel count, the strided tiles, odd sizes
HALF = []
for _dt in (F16, BF16):
    HALF += [
        _s1(1, 8, 64, 64, 64, dtype=_dt, why="256x64 (C <= 128)"), _s1(1, 64, 512, 160, 512, dtype=_dt, why="512x128 WS=3: 32 768 pixels"),
        _s1(1, 8, 64, 160, 128, dtype=_dt, why="256x128 WS=3"), _s1(8, 32, 512, 160, 64, dtype=_dt, why="512x64: 131 072 pixels"),
        _s1(1, 8, 64, 160, 64, dtype=_dt, why="256x64 (C > 128)"), _s1(1, 4, 32, 160, 128, dtype=_dt, why="128x128 TW32"),
        _s1(1, 4, 32, 160, 64, dtype=_dt, why="128x64 TW32"), _s1(2, 5, 45, 64, 64, dtype=_dt, why="odd width"), _s1(1, 7, 23, 128, 128, dtype=_dt),
        _s1(1, 1, 2, 64, 64, dtype=_dt, why="W = 2, H = 1"),
        Case(1, 64, 512, 64, 512, 3, (1, 2), dtype=_dt, why="strided 256x128 TW32: 16 384 output pixels"),
        Case(2, 7, 45, 64, 128, 3, (1, 2), dtype=_dt, why="odd width, seam"), Case(2, 19, 45, 64, 64, 3, (2, 2), dtype=_dt, why="odd width, seam, (2,2)"),
        Case(1, 8, 128, 64, 64, 3, (2, 2), dtype=_dt), Case(2, 8, 128, 64, 128, 1, (1, 2), dtype=_dt), Case(2, 8, 45, 64, 128, 1, (2, 2), dtype=_dt),
    ]

# The rest of what the dispatch can select (reachable_labels), each by the cheapest shape of the scan grid that reaches it -- chosen
# with the query (greedy cover, cost = multiply-adds of the layer): (N, H, W, C, K, ks, stride, dtype).  The two-column images are
# the smallest on which every wide tile wastes more than 10 % more than the narrowest one, which is what sends a layer to the
# fall-back tiles; the 131 072-pixel ones the only way to the tiles that want 256 workgroups of 512 pixels.
COVER = [
    (1, 1, 2, 64, 64, 1, (1, 2), 0),
    (1, 1, 64, 64, 64, 1, (1, 2), 0),
    (1, 1, 2, 64, 64, 1, (2, 2), 0),
    (1, 1, 64, 64, 64, 1, (2, 2), 0),
    (1, 1, 45, 128, 512, 3, (1, 1), 0),
    (1, 4, 16, 128, 512, 3, (1, 1), 0),
    (1, 4, 64, 64, 256, 3, (1, 1), 0),
    (1, 4, 128, 64, 256, 3, (1, 1), 0),
    (8, 1, 256, 128, 192, 3, (1, 1), 0),
    (1, 4, 2, 64, 512, 3, (1, 2), 0),
    (1, 7, 2, 64, 512, 3, (1, 2), 0),
    (1, 1, 45, 128, 512, 3, (1, 2), 0),
    (1, 4, 128, 64, 512, 3, (1, 2), 0),
    (1, 1, 2, 64, 512, 3, (2, 2), 0),
    (1, 4, 2, 64, 512, 3, (2, 2), 0),
    (1, 7, 2, 64, 512, 3, (2, 2), 0),
    (1, 15, 2, 64, 512, 3, (2, 2), 0),
    (1, 1, 45, 128, 512, 3, (2, 2), 0),
    (1, 1, 2, 128, 64, 1, (1, 2), 1),
    (1, 4, 2, 64, 64, 1, (1, 2), 1),
    (1, 4, 2, 256, 512, 1, (1, 2), 1),
    (8, 64, 512, 64, 64, 1, (1, 2), 1),
    (8, 64, 512, 128, 128, 1, (1, 2), 1),
    (1, 1, 2, 64, 64, 1, (2, 2), 1),
    (1, 1, 2, 128, 128, 1, (2, 2), 1),
    (1, 7, 2, 128, 64, 1, (2, 2), 1),
    (8, 64, 512, 64, 192, 1, (2, 2), 1),
    (8, 64, 512, 192, 64, 1, (2, 2), 1),
    (8, 31, 512, 64, 512, 1, (2, 2), 1),
    (8, 31, 512, 512, 64, 1, (2, 2), 1),
    (1, 1, 2, 64, 128, 3, (1, 1), 1),
    (1, 1, 128, 64, 128, 3, (1, 1), 1),
    (1, 1, 45, 128, 256, 3, (1, 1), 1),
    (8, 32, 512, 64, 192, 3, (1, 1), 1),
    (1, 64, 512, 512, 192, 3, (1, 1), 1),
    (1, 1, 2, 128, 64, 3, (1, 2), 1),
    (1, 1, 2, 64, 128, 3, (1, 2), 1),
    (1, 4, 2, 128, 64, 3, (1, 2), 1),
    (8, 32, 512, 64, 64, 3, (1, 2), 1),
    (1, 64, 512, 512, 64, 3, (1, 2), 1),
    (1, 1, 2, 64, 64, 3, (2, 2), 1),
    (1, 1, 2, 128, 128, 3, (2, 2), 1),
    (1, 7, 2, 128, 128, 3, (2, 2), 1),
    (8, 64, 512, 64, 64, 3, (2, 2), 1),
    (8, 15, 512, 512, 64, 3, (2, 2), 1),
    (8, 64, 512, 192, 64, 3, (2, 2), 1),
    (8, 31, 512, 512, 64, 3, (2, 2), 1),
    (1, 1, 2, 128, 64, 1, (1, 2), 2),
    (1, 4, 2, 64, 64, 1, (1, 2), 2),
    (1, 4, 2, 256, 512, 1, (1, 2), 2),
    (8, 64, 512, 64, 64, 1, (1, 2), 2),
    (8, 64, 512, 128, 128, 1, (1, 2), 2),
    (1, 1, 2, 64, 64, 1, (2, 2), 2),
    (1, 1, 2, 128, 128, 1, (2, 2), 2),
    (1, 7, 2, 128, 64, 1, (2, 2), 2),
    (8, 64, 512, 64, 192, 1, (2, 2), 2),
    (8, 64, 512, 192, 64, 1, (2, 2), 2),
    (8, 31, 512, 64, 512, 1, (2, 2), 2),
    (8, 31, 512, 512, 64, 1, (2, 2), 2),
    (1, 1, 2, 64, 128, 3, (1, 1), 2),
    (1, 1, 128, 64, 128, 3, (1, 1), 2),
    (1, 1, 45, 128, 256, 3, (1, 1), 2),
    (8, 32, 512, 64, 192, 3, (1, 1), 2),
    (1, 64, 512, 512, 192, 3, (1, 1), 2),
    (1, 1, 2, 128, 64, 3, (1, 2), 2),
    (1, 1, 2, 64, 128, 3, (1, 2), 2),
    (1, 4, 2, 128, 64, 3, (1, 2), 2),
    (8, 32, 512, 64, 64, 3, (1, 2), 2),
    (1, 64, 512, 512, 64, 3, (1, 2), 2),
    (1, 1, 2, 64, 64, 3, (2, 2), 2),
    (1, 1, 2, 128, 128, 3, (2, 2), 2),
    (1, 7, 2, 128, 128, 3, (2, 2), 2),
    (8, 64, 512, 64, 64, 3, (2, 2), 2),
    (8, 15, 512, 512, 64, 3, (2, 2), 2),
    (8, 64, 512, 192, 64, 3, (2, 2), 2),
    (8, 31, 512, 512, 64, 3, (2, 2), 2),
]

# More tile groups than CUs: k_wino_conv's grid is capped at the CU count and a workgroup walks grp, grp + grid, ...; between two
# groups it fetches the next group's first operands under the epilogue of the one in hand (csrc/wino_conv_body.h).  One image
# geometry per non-split instantiation, (H, W, tile groups per image at K = 64) -- wino_plan's rules by hand, confirmed by the plan
# query in tests/test_conv_ref_host.py; the batch follows from the CU count.  64 -> 64 channels keep the input gradient on the same
# instantiation.  The last geometry has more groups per image than one round of the grid advances a workgroup (CUs / 8, the XCD
# swizzle of wn_xcd_swizzle), so a workgroup's consecutive groups lie in the SAME image; in the small ones they never do.
PERSISTENT_GEOMS = {"<32,F>": (12, 64, 3), "<16,F>": (24, 32, 3), "<32,T>": (11, 62, 3), "<16,T>": (15, 30, 2), "<8,T>": (31, 14, 2),
                    "<4,T>": (63, 7, 2), "<32,F> one image": (64, 192, 48)}
PERSISTENT_RANGES = dict(xmax=3, wmax=2, passes=("forward", "dgrad"))     # headroom("wino_conv", 64, 3, 2, add=3, dact_tanh=True): ~1.2e5 steps


def persistent_cases(cu_count):
    """{name: Case} for a device with ``cu_count`` CUs.  Per geometry cu_count < groups < 2 cu_count: some workgroups walk two groups,
    some one.  "3x": at least 3 cu_count groups and no multiple of it -- a middle group, which follows one and prefetches one, and
    workgroups with different numbers of groups.  "72 channels": 9 chunks -- the last chunk of a group sits in the upper buffer, where
    the next group's U(0) arrives (forward only).  "several blocks": 64 -> 192 channels (or the next count whose blocks do not
    divide a workgroup's step) -- k0 changes from a workgroup's group to its next (forward only).  Weight gradients stay out: they are not persistent kernels, and the batch of
    these cases leaves their sums no headroom."""
    assert cu_count > 48
    out = {}
    for name, (H, W, per_image) in PERSISTENT_GEOMS.items():
        N = cu_count // per_image + 1
        out[name] = _s1(N, H, W, 64, 64, why=f"{name}: {N * per_image} groups on {cu_count} CUs", **PERSISTENT_RANGES)
    for name in ("<32,F>", "<32,T>"):
        H, W, per_image = PERSISTENT_GEOMS[name]
        N = -(-3 * cu_count // per_image)
        while (N * per_image) % cu_count == 0:
            N += 1
        out[name + " 3x"] = _s1(N, H, W, 64, 64, why=f"{name}: {N * per_image} groups on {cu_count} CUs", **PERSISTENT_RANGES)
    H, W, per_image = PERSISTENT_GEOMS["<32,F>"]
    N = cu_count // per_image + 1
    out["<32,F> 72 channels"] = _s1(N, H, W, 72, 64, why=f"<32,F>, 9 chunks: {N * per_image} groups on {cu_count} CUs", xmax=3, wmax=2,
                                    passes=("forward",))
    # several 64-channel output blocks whose number does not divide a workgroup's step through the groups: its consecutive groups
    # then differ in k0 (with one block, or a step that is a multiple of the blocks, every group of a workgroup has the same k0)
    for K in (192, 320, 448):
        N = cu_count // (per_image * (K // 64)) + 1
        if block_changes(N * per_image * (K // 64), cu_count, K // 64)[1]:
            break
    out["<32,F> several blocks"] = _s1(N, H, W, 64, K, why=f"<32,F>, {K // 64} output blocks: {N * per_image * (K // 64)} groups on {cu_count} CUs",
                                       xmax=3, wmax=2, passes=("forward",))
    return out


def xcd_swizzle(g, groups):
    """wn_xcd_swizzle of csrc/wino.hip: the position in (image, group row, group column, channel block) order of launch id g."""
    q, r = divmod(groups, 8)
    xcd, k = g % 8, g // 8
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + k


def block_changes(groups, grid, kt):
    """(hand-overs of the launch, those whose two groups differ in their 64-channel output block, those whose two groups lie on
    different sides of kt / 2 -- the even- / odd-pixel halves of a pixel-pair input gradient): the channel block is the fastest
    index of WN_SETUP, t % kt."""
    pairs = [(xcd_swizzle(g - grid, groups) % kt, xcd_swizzle(g, groups) % kt) for g in range(grid, groups)]
    return len(pairs), sum(a != b for a, b in pairs), sum((2 * a < kt) != (2 * b < kt) for a, b in pairs)


def group_table(case, cu_count, transposed=False):
    """(grid, TR, TC, [(image, group row, group column, channel block) of group id 0, 1, ...]) of the case's non-split Winograd launch:
    wn_xcd_swizzle and WN_SETUP of csrc/wino_conv_body.h restated -- bookkeeping for what a test prints (which groups follow another
    group of their workgroup, and where a mismatch lies); the launch itself is asked of the dispatch.  Workgroup b walks the ids
    b, b + grid, ..."""
    from delora_amd import _lib as L
    c = case
    C, K = (c.K, c.C) if transposed else (c.C, c.K)
    line = L.conv_plan(L.PLAN_WINO_CONV, F32, c.N, c.H, c.W, C, K, 3, 1, 1, 0, cu_count)[0]
    tr, tc, tiles_h, tiles_w, splits, grid = wino_shape(line, c.H, c.W)
    assert splits == 1, line
    kt = K // 64
    groups = c.N * tiles_h * tiles_w * kt
    table = []
    for g in range(groups):
        t = xcd_swizzle(g, groups)
        table.append((t // (kt * tiles_w * tiles_h), t // (kt * tiles_w) % tiles_h, t // kt % tiles_w, t % kt))
    assert len(set(table)) == groups
    return grid, tr, tc, table


def group_walk(case, cu_count, transposed=False):
    """(groups, grid, same, other): over all workgroups, how many hand-overs go to a group of the SAME image, how many to another."""
    grid, _, _, table = group_table(case, cu_count, transposed)
    same = sum(table[g][0] == table[g - grid][0] for g in range(grid, len(table)))
    return len(table), grid, same, max(len(table) - grid, 0) - same


PERSISTENT_256 = list(persistent_cases(256).values())

ALL, _seen = [], set()
for _c in S1_F32 + STRIDED_F32 + HALF + [Case(*t, why="cover") for t in COVER] + PERSISTENT_256:
    if _c.id not in _seen:
        _seen.add(_c.id)
        ALL.append(_c)
# what tests/test_gpu_conv_exact.py runs one by one; the persistent cases run in tests/test_gpu_wino_persistent_exact.py, with the
# batch the device's own CU count asks for
FIXED = [c for c in ALL if c not in PERSISTENT_256]


def cases_for(cu_count):
    """The cases a device with ``cu_count`` CUs runs: the fixed ones and the persistent ones of its CU count."""
    return FIXED + list(persistent_cases(cu_count).values())


# ---------------------------------------------------------------------------------------------------- written down from the dispatch
def expected_wino_labels():
    """wino_plan (csrc/wino.hip): even images whose tile grid divides take <32,F> or <16,F>; everything else the ragged shape that
    wastes the fewest tiles, <32|16|8|4,T>; each with and without the split over input channels, whose count doubles from 2 up to 16
    (a range keeps at least 4 of the C / 8 chunks: 16 needs C = 512).  The grid of a launch without a split is capped at the CU
    count: every such instantiation also runs with several tile groups per workgroup (a split launch never does: its ranges fit
    one round of the CUs by construction)."""
    shapes = ((32, "false"), (16, "false"), (32, "true"), (16, "true"), (8, "true"), (4, "true"))
    out = {f"k_wino_conv<{tc}, {rag}, {sp}>" for tc, rag in shapes for sp in ("false", "true")}
    out |= {f"k_wino_conv splits={n}" for n in (2, 4, 8, 16)} | {"k_wino_split_sum"}
    out |= {f"k_wino_conv<{tc}, {rag}, false> {SEVERAL}" for tc, rag in shapes}
    return out


def expected_wgrad_labels():
    """Both bodies of every weight-gradient family.  Direct fp32 (csrc/conv.hip): PK = 16 for the 3x3 layers with stride 2 in W, else 32;
    FAST when a chunk's staged window is at most one image width, (PK - 1) * SW + KS <= W.  Winograd domain (wino.hip): RAG unless H and
    W are even and W / 2 divides into chunks of 8 tiles.  Half precision (wgradh.hip): 128- or 64-channel tiles by K % 128, chunks of 64
    pixels for stride-1 layers whose rows waste no more that way, else 32.  The merged launches: with one slab (writes dW) and several."""
    out = set()
    for sh, sw, ks in ((1, 1, 3), (1, 2, 3), (2, 2, 3), (1, 2, 1), (2, 2, 1)):
        pk = 16 if (sw == 2 and ks == 3) else 32
        for fast in ("false", "true"):
            out.add(f"k_wgrad_f32<64, 64, {pk}, {sh}, {sw}, {ks}, {fast}>")
            out.add(f"k_wgrad_f32_batch<64, 64, {pk}, {sh}, {sw}, {ks}, {fast}>")
        for f16 in ("true", "false"):
            tiles = [(128, 32), (64, 32)] + ([(128, 64)] if (sh, sw) == (1, 1) else [])
            for bmk, pk_h in tiles:
                out.add(f"k_wgradh<{f16}, {bmk}, {pk_h}, 2, {sh}, {sw}, {ks}>")
                out.add(f"k_wgradh_batch<{f16}, {bmk}, {pk_h}, 2, {sh}, {sw}, {ks}>")
    for rag in ("false", "true"):
        out |= {f"k_wino_wgrad<{rag}>", f"k_wino_wgrad_batch<{rag}>"}
    return out
