"""Shapes of the bit-exact convolution tests (tests/test_gpu_conv_exact.py) and the bookkeeping that proves their coverage:
which kernel instantiations every case reaches (asked of the dispatch itself through ``dl_conv_plan_describe``), which
instantiations the dispatch can select at all, and the value ranges that keep every case exact (``conv_ref.headroom``).

Host only: the GPU test and tests/test_conv_ref_host.py both import it.
"""
import re

import torch

from tests import conv_ref as cr

F32, F16, BF16 = 0, 1, 2
TORCH_DTYPE = {F32: torch.float32, F16: torch.float16, BF16: torch.bfloat16}
STRIDED_GEOMS = [(3, (1, 2)), (3, (2, 2)), (1, (1, 2)), (1, (2, 2))]          # every strided layer kind the network has


class Case:
    """One layer shape: x [N,H,W,C] -> K channels, kernel ks, stride; dtype code; ``xmax`` / ``wmax`` the integer ranges."""

    def __init__(self, N, H, W, C, K, ks=3, stride=(1, 1), dtype=F32, xmax=None, wmax=None, why=""):
        self.N, self.H, self.W, self.C, self.K, self.ks, self.stride, self.dtype = N, H, W, C, K, ks, tuple(stride), dtype
        self.why = why
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
        return self.C % 64 == 0           # (the input gradient's output channels must tile)

    @property
    def wgrad_ok(self):
        return self.C % 64 == 0 and self.K % 64 == 0

    def seed(self, salt=0):
        return (self.N * 1000003 + self.H * 10007 + self.W * 101 + self.C * 7 + self.K * 3 + self.ks + 10 * self.stride[0] + 100 * self.stride[1]
                + 1000 * self.dtype) * 16 + salt

    # ---- what the GPU test runs for this case, as (op, dtype, N, H, W, C, K, ks, sh, sw, mode) of dl_conv_plan_describe
    def plan_queries(self):
        from delora_amd import _lib as L
        N, H, W, C, K, ks, (sh, sw), dt = self.N, self.H, self.W, self.C, self.K, self.ks, self.stride, self.dtype
        q = [(L.PLAN_CONV, dt, N, H, W, C, K, ks, sh, sw, 0)]
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


_TAIL = re.compile(r" grid=\d+x\d+x\d+ block=\d+")


def labels_of(query, cu_count=0):
    """Labels of one dispatch query: the kernel instantiation of every launch; a Winograd split adds "<kernel> splits=<n>", a
    merged weight-gradient launch "<kernel> one slab" (it writes dW directly) or "<kernel> slabs" (partials + reduction)."""
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

ALL, _seen = [], set()
for _c in S1_F32 + STRIDED_F32 + HALF + [Case(*t, why="cover") for t in COVER]:
    if _c.id not in _seen:
        _seen.add(_c.id)
        ALL.append(_c)


# ---------------------------------------------------------------------------------------------------- written down from the dispatch
def expected_wino_labels():
    """wino_plan (csrc/wino.hip): even images whose tile grid divides take <32,F> or <16,F>; everything else the ragged shape that
    wastes the fewest tiles, <32|16|8|4,T>; each with and without the split over input channels, whose count doubles from 2 up to 16
    (a range keeps at least 4 of the C / 8 chunks: 16 needs C = 512)."""
    out = {f"k_wino_conv<{tc}, {rag}, {sp}>" for tc, rag in ((32, "false"), (16, "false"), (32, "true"), (16, "true"), (8, "true"), (4, "true"))
           for sp in ("false", "true")}
    out |= {f"k_wino_conv splits={n}" for n in (2, 4, 8, 16)} | {"k_wino_split_sum"}
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
