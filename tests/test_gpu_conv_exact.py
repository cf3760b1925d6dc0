"""Every convolution kernel against a float64 CPU reference, BIT FOR BIT, on small-integer data in poisoned arenas.

On the data of tests/conv_ref.py every product and every partial sum is an fp32 number (``headroom`` proves it per case), so no
summation order, tile shape, split or slab plan may change a single bit: the fp32 kernels (direct, Winograd, both weight-gradient
families, single and merged) must EQUAL the float64 reference, the half-precision kernels that value rounded once to nearest-even
(signed zeros compare equal).  Every pointer handed to the library is a view inside a larger allocation whose surroundings -- and
whose interior, for outputs and workspaces -- hold a quiet-NaN pattern: a write beside a buffer, an element never written, a
workspace assumed to be zero and a ``*_workspace_bytes`` that is too small all fail.  The cases (tests/conv_exact_cases.py) are
chosen with ``dl_conv_plan_describe`` so that together they reach every kernel instantiation the dispatch can select; a test
asserts that.  Forward tanh stays with tests/test_gpu_conv.py: it cannot be exact.
"""
import ctypes

import pytest
import torch

from tests import conv_exact_cases as cc
from tests import conv_ref as cr
from tests import util

pytestmark = pytest.mark.gpu

ADD, ACT, DACT, ADD_GRID = cr.EPI_ADD, cr.EPI_ACT, cr.EPI_DACT, cr.EPI_ADD_GRID
RELU, TANH = cr.ACT_RELU, cr.ACT_TANH
# (flags, act, kind of saved activation) -- forward tails, and the tails of an input gradient
FWD_TAILS = [(0, 0, None), (ADD, 0, None), (ADD | ACT, RELU, None)]
BWD_TAILS = [(0, 0, None), (DACT, RELU, "relu"), (DACT, TANH, "tanh"), (ADD | DACT, TANH, "tanh"), (ADD | DACT, RELU, "relu")]
GRID_TAILS = [(0, 0, None), (DACT, RELU, "relu"), (ADD_GRID, 0, None), (ADD_GRID | DACT, TANH, "tanh")]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _guarded(fn, *args, **kw):
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        return fn(*args, **kw)
    except RuntimeError as e:
        if "hip" in str(e).lower() and "error" in str(e).lower():
            pytest.exit(f"device error, stopping: {e}", returncode=3)
        raise


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Run:
    """One case on the device: its data (CPU float64 and arena copies), its references, and the calls."""

    def __init__(self, case, dev, skew=0):
        from delora_amd import _lib
        self.L, self.lib, self.c, self.dev = _lib, _lib.load(), case, dev
        self.A = cr.Arenas(dev, skew)
        self.dt = cc.TORCH_DTYPE[case.dtype]
        self.bad = 0
        c = case
        c.headroom()
        sd = c.seed
        self.x = cr.ints((c.N, c.H, c.W, c.C), c.xmax, sd(1))
        self.w = cr.ints((c.K, c.ks, c.ks, c.C), c.wmax, sd(2))
        self.g = cr.ints((c.N, c.Ho, c.Wo, c.K), c.xmax, sd(3))
        self.y0 = cr.conv(self.x, self.w, c.stride)
        self.dx0 = self.dw0 = None
        if c.wgrad_ok:
            self.dx0, self.dw0 = cr.conv_grads(self.x, self.w, self.g, c.stride)
        elif c.dgrad_ok:                                      # (a case that leaves the weight gradient out: no autograd through w)
            self.dx0 = cr.conv_dx(self.x.shape, self.w, self.g, c.stride)
        a = self.A.arena
        self.x_d = a(self.x.shape, self.dt, self.x, "x")
        self.g_d = a(self.g.shape, self.dt, self.g, "g")
        self.w_d = a(self.w.shape, torch.float32, self.w, "w", row_elems=0)

    # ---- helpers
    def out(self, shape, dtype=None, name="out", row_elems=None):
        return self.A.arena(shape, dtype or self.dt, None, name, row_elems)

    def ws(self, nbytes, name="workspace"):
        """Exactly ``nbytes`` of NaN-filled scratch: the guard begins at the first byte behind what the size function promised."""
        assert nbytes % 4 == 0
        return self.A.arena((max(nbytes // 4, 1),), torch.float32, None, name, row_elems=0) if nbytes else None

    def ok(self, rc, what):
        self.L.check(rc, what)

    def compare(self, got, ref, what, tile=(2, 2)):
        torch.cuda.synchronize()
        self.A.check(f"{self.c.id} {what}")
        self.A.check_output(got, f"{self.c.id} {what}")
        n = cr.mismatches(got, ref.to(got.dtype) if got.dtype != torch.float32 else ref.float(), f"{self.c.id} {what}", tile)
        self.bad += n
        return n

    def tail_operands(self, shape, flags, kind, salt):
        """(add, dsrc) as CPU float64 + arena copies for one tail."""
        add = cr.ints(shape, 3, self.c.seed(salt)) if flags & ADD else None
        sv = None
        if flags & DACT:
            sv = cr.saved_tanh(shape, self.c.seed(salt + 1)) if kind == "tanh" else cr.saved_relu(shape, self.c.seed(salt + 1))
        return add, sv, (self.A.arena(shape, self.dt, add, "add") if add is not None else None), \
            (self.A.arena(shape, self.dt, sv, "dsrc") if sv is not None else None)


def _conv_call(r, x_d, w_d, y_d, add_d, sv_d, C, K, ks, st, transposed, act, flags):
    c = r.c
    if c.dtype == cc.F32:
        r.ok(r.lib.dl_conv2d_nhwc_f32(_p(x_d), _p(w_d), _p(y_d), _p(add_d), _p(sv_d), c.N, c.H, c.W, C, K, ks, st[0], st[1], transposed, act, flags,
                                      _stream()), "dl_conv2d_nhwc_f32")
    else:
        r.ok(r.lib.dl_conv2d_nhwc_h(_p(x_d), _p(w_d), _p(y_d), _p(add_d), _p(sv_d), c.N, c.H, c.W, C, K, ks, st[0], st[1], transposed, c.dtype, act,
                                    flags, _stream()), "dl_conv2d_nhwc_h")


def _wino_call(r, x_d, u_d, y_d, add_d, sv_d, C, K, act, flags):
    c = r.c
    nbytes = int(r.lib.dl_wino_conv3x3_workspace_bytes(c.N, c.H, c.W, C, K))
    ws = r.ws(nbytes, "wino split workspace")
    r.ok(r.lib.dl_wino_conv3x3_nhwc_f32(_p(x_d), _p(u_d), _p(y_d), _p(add_d), _p(sv_d), c.N, c.H, c.W, C, K, act, flags, _p(ws), _stream()),
         "dl_wino_conv3x3_nhwc_f32")


def _prepared_weights(r):
    """(forward operand, backward operand) of the direct / half kernels and (u_fwd, u_bwd) of the Winograd kernels, in arenas."""
    c = r.c
    wf = wb = uf = ub = None
    if c.dtype == cc.F32:
        wf = wb = r.w_d                                   # the transposed pass reads the forward weight itself
        if c.s1:
            n = int(r.lib.dl_wino_weights_floats(c.K, c.C))
            uf, ub = r.out((n,), torch.float32, "u_fwd", 0), r.out((n,), torch.float32, "u_bwd", 0)
            r.ok(r.lib.dl_wino_weights_f32(_p(r.w_d), _p(uf), _p(ub), c.K, c.C, _stream()), "dl_wino_weights_f32")
    else:
        taps = c.ks * c.ks
        wf, wb = r.out((taps, c.K, c.C), r.dt, "w_fwd", 0), r.out((taps, c.C, c.K), r.dt, "w_bwd", 0)
        r.ok(r.lib.dl_conv_weights_h(_p(r.w_d), _p(wf), _p(wb), c.K, taps, c.C, c.dtype, _stream()), "dl_conv_weights_h")
    torch.cuda.synchronize()
    r.A.check(f"{c.id} weight preparation")
    for t in (wf, wb, uf, ub):
        if t is not None and t is not r.w_d:
            r.A.check_output(t, f"{c.id} weight preparation")
            r.A.freeze(t)
    return wf, wb, uf, ub


def _wgrad_layer(r, dw_d):
    c = r.c
    arr = (r.L.WgradLayer * 1)()
    arr[0].x, arr[0].g, arr[0].dw = r.x_d.data_ptr(), r.g_d.data_ptr(), dw_d.data_ptr()
    arr[0].N, arr[0].H, arr[0].W, arr[0].C, arr[0].K, arr[0].ksize, arr[0].stride_h, arr[0].stride_w = c.N, c.H, c.W, c.C, c.K, c.ks, c.stride[0], c.stride[1]
    return arr


def run_case(case, dev, skew=0):
    """Every entry point the case admits; returns the number of mismatching elements (guards, inputs and NaN survivors assert)."""
    r = Run(case, dev, skew)
    c, lib = case, r.lib
    wf, wb, uf, ub = _prepared_weights(r)
    yshape, xshape = tuple(r.y0.shape), tuple(r.x.shape)
    # ---- forward
    direct = c.direct_ok                     # (false only for the chunk-count cases the direct dispatch refuses: Winograd alone)
    assert direct or uf is not None
    for i, (flags, act, kind) in enumerate(FWD_TAILS):
        add, sv, add_d, sv_d = r.tail_operands(yshape, flags, kind, 10 + 2 * i)
        ref = cr.epilogue(r.y0, flags, act, add, sv)
        y_d = None
        if direct:
            y_d = r.out(yshape, name="y")
            _conv_call(r, r.x_d, wf, y_d, add_d, sv_d, c.C, c.K, c.ks, c.stride, 0, act, flags)
            r.compare(y_d, ref, f"forward, tail {flags}/{act}", (8, 64))
        if uf is not None:
            y2 = r.out(yshape, name="y (Winograd)")
            _wino_call(r, r.x_d, uf, y2, add_d, sv_d, c.C, c.K, act, flags)
            r.compare(y2, ref, f"Winograd forward, tail {flags}/{act}")
            assert y_d is None or torch.equal(y_d, y2), f"{c.id}: Winograd and direct forward differ from each other (tail {flags}/{act})"
    # ---- input gradient
    if c.dgrad_ok and c.s1:
        for i, (flags, act, kind) in enumerate(BWD_TAILS):
            add, sv, add_d, sv_d = r.tail_operands(xshape, flags, kind, 30 + 2 * i)
            ref = cr.epilogue(r.dx0, flags, act, add, sv)
            dx_d = r.out(xshape, name="dx")
            _conv_call(r, r.g_d, wb, dx_d, add_d, sv_d, c.K, c.C, 3, (1, 1), 1, act, flags)
            r.compare(dx_d, ref, f"input gradient, tail {flags}/{act}", (8, 64))
            if ub is not None:
                dx2 = r.out(xshape, name="dx (Winograd)")
                _wino_call(r, r.g_d, ub, dx2, add_d, sv_d, c.K, c.C, act, flags)
                r.compare(dx2, ref, f"Winograd input gradient, tail {flags}/{act}")
                assert torch.equal(dx_d, dx2), f"{c.id}: Winograd and direct input gradient differ from each other (tail {flags}/{act})"
    elif c.dgrad_ok:
        dense = c.ks == 1
        odd_w = c.ks == 3 and c.stride[1] == 2 and c.W % 2 == 1 and c.W >= 3
        gshape = (c.N, c.Ho, c.Wo, c.C)
        for i, (flags, act, kind) in enumerate(GRID_TAILS[:1] if dense else GRID_TAILS):
            _, sv, _, sv_d = r.tail_operands(xshape, flags, kind, 50 + 2 * i)
            addg = cr.ints(gshape, 3, c.seed(60 + i)) if flags & ADD_GRID else None
            addg_d = r.A.arena(gshape, r.dt, addg, "add_grid") if addg is not None else None
            ref = cr.epilogue(r.dx0, flags, act, None, sv, addg, c.stride)
            if dense:
                ref = ref[:, ::c.stride[0], ::c.stride[1]].contiguous()
            dx_d = r.out(tuple(ref.shape), name="dx")
            seam = r.out((c.N, c.H, 2, c.C), torch.float32, "seam_ws", 0) if odd_w else None
            args = (_p(r.g_d), _p(wb), _p(dx_d), _p(addg_d), _p(sv_d), c.N, c.H, c.W, c.K, c.C, c.ks, c.stride[0], c.stride[1], int(dense))
            if c.dtype == cc.F32:
                r.ok(lib.dl_conv2d_dgrad_strided_nhwc_f32(*args, act, flags, _p(seam), _stream()), "dl_conv2d_dgrad_strided_nhwc_f32")
            else:
                r.ok(lib.dl_conv2d_dgrad_strided_nhwc_h(*args, c.dtype, act, flags, _p(seam), _stream()), "dl_conv2d_dgrad_strided_nhwc_h")
            r.compare(dx_d, ref, f"strided input gradient{' (dense)' if dense else ''}, tail {flags}/{act}", (8, 64))
    # ---- weight gradients: single-layer and merged entry points of every family
    if c.wgrad_ok:
        dshape = tuple(r.dw0.shape)
        st = c.stride

        def dw_out(name):
            return r.out(dshape, torch.float32, name, 0)

        if c.dtype == cc.F32:
            dw = dw_out("dw")
            ws = r.ws(int(lib.dl_conv2d_wgrad_workspace_bytes(c.N, c.H, c.W, c.C, c.K, c.ks, st[0], st[1])))
            r.ok(lib.dl_conv2d_wgrad_nhwc_f32(_p(r.x_d), _p(r.g_d), _p(dw), _p(ws), c.N, c.H, c.W, c.C, c.K, c.ks, st[0], st[1], _stream()), "dl_conv2d_wgrad_nhwc_f32")
            r.compare(dw, r.dw0, "weight gradient")
            dw = dw_out("dw (merged)")
            arr = _wgrad_layer(r, dw)
            ws = r.ws(int(lib.dl_conv2d_wgrad_batch_workspace_bytes(ctypes.cast(arr, ctypes.c_void_p), 1)))
            r.ok(lib.dl_conv2d_wgrad_batch_nhwc_f32(ctypes.cast(arr, ctypes.c_void_p), 1, _p(ws), _stream()), "dl_conv2d_wgrad_batch_nhwc_f32")
            r.compare(dw, r.dw0, "weight gradient, merged entry point")
            if c.s1 and c.W >= 2:
                dw = dw_out("dw (Winograd)")
                ws = r.ws(int(lib.dl_wino_wgrad_workspace_bytes(c.N, c.H, c.W, c.C, c.K)))
                r.ok(lib.dl_wino_wgrad3x3_nhwc_f32(_p(r.x_d), _p(r.g_d), _p(dw), _p(ws), c.N, c.H, c.W, c.C, c.K, _stream()), "dl_wino_wgrad3x3_nhwc_f32")
                r.compare(dw, r.dw0, "Winograd-domain weight gradient")
                dw = dw_out("dw (Winograd, merged)")
                arr = _wgrad_layer(r, dw)
                ws = r.ws(int(lib.dl_wino_wgrad3x3_batch_workspace_bytes(ctypes.cast(arr, ctypes.c_void_p), 1)))
                r.ok(lib.dl_wino_wgrad3x3_batch_nhwc_f32(ctypes.cast(arr, ctypes.c_void_p), 1, _p(ws), _stream()), "dl_wino_wgrad3x3_batch_nhwc_f32")
                r.compare(dw, r.dw0, "Winograd-domain weight gradient, merged entry point")
        else:
            dw = dw_out("dw")
            ws = r.ws(int(lib.dl_conv2d_wgrad_h_workspace_bytes(c.N, c.H, c.W, c.C, c.K, c.ks, st[0], st[1])))
            r.ok(lib.dl_conv2d_wgrad_nhwc_h(_p(r.x_d), _p(r.g_d), _p(dw), _p(ws), c.N, c.H, c.W, c.C, c.K, c.ks, st[0], st[1], c.dtype, _stream()),
                 "dl_conv2d_wgrad_nhwc_h")
            r.compare(dw, r.dw0, "weight gradient")
            dw = dw_out("dw (merged)")
            arr = _wgrad_layer(r, dw)
            ws = r.ws(int(lib.dl_conv2d_wgrad_batch_h_workspace_bytes(ctypes.cast(arr, ctypes.c_void_p), 1)))
            r.ok(lib.dl_conv2d_wgrad_batch_nhwc_h(ctypes.cast(arr, ctypes.c_void_p), 1, _p(ws), c.dtype, _stream()), "dl_conv2d_wgrad_batch_nhwc_h")
            r.compare(dw, r.dw0, "weight gradient, merged entry point")
    return r.bad


def wino_plan_line(case, transposed=False):
    """The Winograd launch the dispatch of THIS device selects for the case's forward pass (or its input gradient), printed."""
    from delora_amd import _lib as L
    c = case
    C, K = (c.K, c.C) if transposed else (c.C, c.K)
    lines = L.conv_plan(L.PLAN_WINO_CONV, cc.F32, c.N, c.H, c.W, C, K, 3, 1, 1, 0, 0)
    print(f"[plan] {c.id}{' input gradient' if transposed else ''}: {'; '.join(lines)}")
    return lines[0]


# (the persistent cases of conv_exact_cases.ALL run in tests/test_gpu_wino_persistent_exact.py, sized by the device's CU count)
@pytest.mark.parametrize("case", cc.FIXED, ids=[c.id for c in cc.FIXED])
def test_every_kernel_equals_the_float64_reference(case):
    dev = _dev()
    if case.C in cc.CHUNK_CHANNELS and case.s1 and case.dtype == cc.F32:
        # a chunk-count case: its plan line, and the split that gives ranges of five chunks (one tile group: four ranges fit any device)
        line = wino_plan_line(case)
        assert ("splits=4" in line.split()) == (case.C == 160), line
    bad = _guarded(run_case, case, dev)
    util.measured(f"conv exact {case.id}: elements that differ from float64", bad, bound=0)


# one shape per family with every base pointer 16 bytes -- the documented minimum alignment -- past a 256-byte boundary
SKEWED = [cc.Case(1, 7, 30, 128, 64), cc.Case(2, 7, 45, 64, 128, 3, (1, 2)), cc.Case(2, 8, 45, 64, 128, 1, (2, 2)),
          cc.Case(1, 7, 23, 128, 128, dtype=cc.F16), cc.Case(2, 7, 45, 64, 128, 3, (1, 2), dtype=cc.BF16)]


@pytest.mark.parametrize("case", SKEWED, ids=[c.id for c in SKEWED])
def test_minimum_documented_alignment(case):
    dev = _dev()
    bad = _guarded(run_case, case, dev, skew=16)
    util.measured(f"conv exact {case.id}, bases 16 bytes past a 256-byte boundary: elements that differ", bad, bound=0)


def test_merged_weight_gradients_of_several_layers():
    """The merged entry points with SEVERAL layers per launch (the trunk's use): layers of different shapes share a launch, some with
    one slab (written straight to dW), some with partials -- each must still be exact."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    shapes = [(1, 7, 30, 64, 64), (2, 8, 32, 128, 64), (1, 4, 64, 64, 128), (1, 31, 7, 128, 128), (8, 16, 64, 64, 64)]
    for fam, dtype in (("direct", cc.F32), ("wino", cc.F32), ("half", cc.BF16), ("half", cc.F16)):
        A = cr.Arenas(dev)
        dt = cc.TORCH_DTYPE[dtype]
        arr = (_lib.WgradLayer * len(shapes))()
        refs, dws = [], []
        for j, (N, H, W, C, K) in enumerate(shapes):
            c = cc.Case(N, H, W, C, K, dtype=dtype)
            x, g = cr.ints((N, H, W, C), c.xmax, c.seed(1)), cr.ints((N, H, W, K), c.xmax, c.seed(3))
            refs.append(cr.conv_grads(x, torch.zeros((K, 3, 3, C), dtype=torch.float64), g)[1])
            x_d, g_d = A.arena(x.shape, dt, x, f"x{j}"), A.arena(g.shape, dt, g, f"g{j}")
            dws.append(A.arena((K, 3, 3, C), torch.float32, None, f"dw{j}", 0))
            arr[j].x, arr[j].g, arr[j].dw = x_d.data_ptr(), g_d.data_ptr(), dws[j].data_ptr()
            arr[j].N, arr[j].H, arr[j].W, arr[j].C, arr[j].K, arr[j].ksize, arr[j].stride_h, arr[j].stride_w = N, H, W, C, K, 3, 1, 1
        ap = ctypes.cast(arr, ctypes.c_void_p)
        size_fn, run_fn = {"direct": (lib.dl_conv2d_wgrad_batch_workspace_bytes, lib.dl_conv2d_wgrad_batch_nhwc_f32),
                           "wino": (lib.dl_wino_wgrad3x3_batch_workspace_bytes, lib.dl_wino_wgrad3x3_batch_nhwc_f32),
                           "half": (lib.dl_conv2d_wgrad_batch_h_workspace_bytes, lib.dl_conv2d_wgrad_batch_nhwc_h)}[fam]
        nbytes = int(size_fn(ap, len(shapes)))
        assert nbytes > 0 and nbytes % 4 == 0
        ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", 0)
        extra = (dtype,) if fam == "half" else ()
        _lib.check(run_fn(ap, len(shapes), _p(ws), *extra, _stream()), "merged weight gradient")
        torch.cuda.synchronize()
        A.check(f"merged {fam}")
        bad = 0
        for j, (dw, ref) in enumerate(zip(dws, refs)):
            A.check_output(dw, f"merged {fam} layer {j}")
            bad += cr.mismatches(dw, ref.float(), f"merged {fam} weight gradient, layer {j} {shapes[j]}")
        util.measured(f"conv exact merged weight gradients [{fam}, dtype {dtype}], {len(shapes)} layers: elements that differ", bad, bound=0)


# ---------------------------------------------------------------------------------------------------- one block per class, and the stem
BLOCKS = [("identity", (1, 8, 32, 64), 64, (1, 1)), ("down (1,2)", (1, 8, 32, 64), 128, (1, 2)), ("down (2,2)", (1, 8, 32, 64), 128, (2, 2)),
          ("down (2,2), odd width", (2, 7, 45, 64), 128, (2, 2))]


def _nnz(w, dim):
    """Largest number of non-zero entries of w [K,ks,ks,C] per output channel (dim 0) or per input channel (dim 3)."""
    other = tuple(d for d in range(4) if d != dim)
    return int((w != 0).sum(dim=other).max())


@pytest.mark.parametrize("first", [True, False], ids=["first", "inner"])
@pytest.mark.parametrize("last", [True, False], ids=["last", "notlast"])
@pytest.mark.parametrize("block", BLOCKS, ids=[b[0].replace(" ", "") for b in BLOCKS])
def test_one_block_segment_with_relu_equals_float64_autograd(block, first, last):
    """``RingSegment`` of one BasicBlock (Winograd and direct kernels with their fused tails, strided phases, dense 1x1, seam terms,
    merged weight gradients) on integer activations and sparse +-1 weights: output, returned gradient and every weight gradient equal
    float64 autograd under the segment's gradient convention -- ``last``: the incoming gradient is dL/dy and the segment applies
    relu'; otherwise it already is the gradient of the pre-activation; ``first``: the returned gradient is dL/dx, otherwise
    dL/dx * relu'(x)."""
    from delora_amd.models import ring_conv as rc
    dev = _dev()
    name, (N, H, W, C), K, stride = block
    has_ds = stride != (1, 1) or C != K
    sd = 7000 + 100 * BLOCKS.index(block)
    x = torch.relu(cr.ints((N, H, W, C), 2, sd + 1))                                   # an activated map: zeros, ones and twos
    w1, w2 = cr.ints((K, 3, 3, C), 1, sd + 2, density=4.0 / (9 * C)), cr.ints((K, 3, 3, K), 1, sd + 3, density=4.0 / (9 * K))
    wd = cr.ints((K, 1, 1, C), 1, sd + 4, density=2.0 / C) if has_ds else None
    Ho, Wo = cr.out_size(H, stride[0]), cr.out_size(W, stride[1])
    dy = cr.ints((N, Ho, Wo, K), 2, sd + 5)
    # headroom from the data's own sparsity: forward through conv1 -> conv2 (+ shortcut), backward through conv2^T -> conv1^T (+ branch)
    r1, r2, c1, c2 = _nnz(w1, 0), _nnz(w2, 0), _nnz(w1, 3), _nnz(w2, 3)
    rd, cd = (_nnz(wd, 0), _nnz(wd, 3)) if has_ds else (1, 1)
    hmax = r1 * 2
    cr.headroom("wino_conv", r1, 2, 1)
    ymax = r2 * hmax + max(2, rd * 2)
    cr.headroom("wino_conv", r2, hmax, 1, add=max(2, rd * 2))
    g1max = c2 * 2
    cr.headroom("wino_conv", c2, 2, 1)
    gxmax = c1 * g1max + max(2, cd * 2)
    cr.headroom("wino_conv", c1, g1max, 1, add=max(2, cd * 2))
    tiles = N * cr.out_size(Ho, 2) * cr.out_size(Wo, 2)
    cr.headroom("wino_wgrad", tiles, hmax, 2)                                          # conv2: h x dy
    cr.headroom("wgrad", N * Ho * Wo, 2, g1max)                                        # conv1 (direct when strided): x x g1
    cr.headroom("wino_wgrad", N * cr.out_size(H, 2) * cr.out_size(W, 2), 2, g1max)     # conv1 on the Winograd path
    assert ymax < 2 ** 20 and gxmax < 2 ** 20
    # float64 autograd
    xr = x.clone().requires_grad_(True)
    ws = [t.clone().requires_grad_(True) for t in (w1, w2) + ((wd,) if has_ds else ())]
    pre = cr.basic_block(xr, ws[0], ws[1], ws[2] if has_ds else None, stride, act_last=False)
    y_ref = torch.relu(pre)
    ((y_ref if last else pre) * dy).sum().backward()
    gx_ref = xr.grad if first else xr.grad * (x > 0)
    # the segment (parameters in their [K,C,k,k] shape, channels_last storage)
    params = [t.float().permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last).to(dev).requires_grad_(True) for t in (w1, w2) + ((wd,) if has_ds else ())]
    x_d = x.float().to(dev).requires_grad_(True)
    y = rc.RingSegment.apply(x_d, rc.ACT["relu"], ((C, K, stride, has_ds),), first, last, *params)
    y.backward(dy.float().to(dev))
    torch.cuda.synchronize()
    tag = f"block [{name}, {'first' if first else 'inner'}, {'last' if last else 'not last'}]"
    bad = cr.mismatches(y.detach(), y_ref.detach().float(), f"{tag} output") + cr.mismatches(x_d.grad, gx_ref.float(), f"{tag} returned gradient")
    for p, wr, nm in zip(params, ws, ("conv1", "conv2", "downsample")):
        bad += cr.mismatches(p.grad.permute(0, 2, 3, 1), wr.grad.float(), f"{tag} {nm} weight gradient")
    util.measured(f"conv exact {tag}: elements that differ from float64 autograd", bad, bound=0)


@pytest.mark.parametrize("shape", [(2, 5, 72), (1, 8, 256), (1, 3, 8)], ids=["2x5x72", "1x8x256", "1x3x8"])
def test_stem_with_relu_on_integer_images(shape):
    """The stem through the C ABI in arenas: the transposing input copy, conv1 + relu, the wrapped max-pool and the fused backward
    (pool backward + relu' + conv1's weight gradient).  Integer images make pooling ties ubiquitous, at the wrap seam too: the
    arg-max rule (rows first, the first strictly greater value wins) is pinned against torch's on every window."""
    from delora_amd import _lib
    dev = _dev()
    lib = _lib.load()
    N, H, W = shape
    sd = 9000 + W
    x_nchw = cr.ints((N, 8, H, W), 3, sd + 1)
    w = cr.ints((64, 3, 3, 8), 2, sd + 2)
    gp = cr.ints((N, H, W // 4, 64), 2, sd + 3)
    cr.headroom("direct", 8, 3, 2)
    cr.headroom("wgrad", N * H * (W // 2), 3, 6 * 2)          # an element of conv1's map is selected by at most 3 x 2 windows
    x8 = x_nchw.permute(0, 2, 3, 1).contiguous()
    xr, wr = x8.clone(), w.clone().requires_grad_(True)
    a_ref, y_ref = cr.stem(xr, wr)
    (y_ref * gp).sum().backward()
    A = cr.Arenas(dev)
    x_d = A.arena(x_nchw.shape, torch.float32, x_nchw, "x planar", row_elems=W)
    seed = A.arena((1,), torch.int64, torch.tensor([12345], dtype=torch.int64), "seed", 0)
    w_d = A.arena(w.shape, torch.float32, w, "w", 0)
    gp_d = A.arena(gp.shape, torch.float32, gp, "g pooled")
    x8_d = A.arena(x8.shape, torch.float32, None, "x channels-last")
    _lib.check(lib.dl_stem_input_nhwc_drop_f32(_p(x_d), N, 8, H, W, _p(seed), 0.0, _p(x8_d), _stream()), "dl_stem_input_nhwc_drop_f32")
    a_d = A.arena(a_ref.shape, torch.float32, None, "conv1 + relu")
    _lib.check(lib.dl_conv2d_nhwc_f32(_p(x8_d), _p(w_d), _p(a_d), None, None, N, H, W, 8, 64, 3, 1, 2, 0, cr.ACT_RELU, cr.EPI_ACT, _stream()), "dl_conv2d_nhwc_f32")
    y_d = A.arena(y_ref.shape, torch.float32, None, "pooled")
    win_d = A.arena(y_ref.shape, torch.int8, None, "win")
    _lib.check(lib.dl_pool3x3s12_nhwc_fwd(_p(a_d), N, H, W // 2, 64, _p(y_d), _p(win_d), _stream()), "dl_pool3x3s12_nhwc_fwd")
    torch.cuda.synchronize()
    A.check("stem forward")
    for t in (x8_d, a_d, y_d):
        A.check_output(t, "stem forward")
        A.freeze(t)
    assert int(((win_d < 0) | (win_d > 8)).sum()) == 0, "a window position outside 0..8 (an element of win never written)"
    A.freeze(win_d)
    tag = f"stem {N}x{H}x{W}"
    bad = cr.mismatches(x8_d, x8.float(), f"{tag} channels-last input") + cr.mismatches(a_d, a_ref.detach().float(), f"{tag} conv1 + relu", (1, 128))
    bad += cr.mismatches(y_d, y_ref.detach().float(), f"{tag} pooled output")
    nbytes = int(lib.dl_stem_wgrad_workspace_bytes(N, H, W))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = A.arena((nbytes // 4,), torch.float32, None, "workspace", 0)
    dw_d = A.arena((64, 8, 3, 3), torch.float32, None, "dw", 0)
    _lib.check(lib.dl_stem_wgrad_f32(_p(gp_d), _p(a_d), _p(win_d), _p(x8_d), N, H, W, cr.ACT_RELU, _p(ws), _p(dw_d), _stream()), "dl_stem_wgrad_f32")
    torch.cuda.synchronize()
    A.check("stem backward")
    A.check_output(dw_d, "stem backward")
    bad += cr.mismatches(dw_d, wr.grad.permute(0, 3, 1, 2).contiguous().float(), f"{tag} conv1 weight gradient")
    util.measured(f"conv exact {tag}: elements that differ from float64", bad, bound=0)


def test_the_cases_reach_every_instantiation_on_this_device():
    """The union of the labels the cases reach on THIS device (its CU count decides the Winograd splits) is everything its dispatch
    can select, and contains the sets written down from the dispatch code.  The persistent cases are built from the device's own
    CU count, as tests/test_gpu_wino_persistent_exact.py runs them."""
    dev = _dev()
    reach = cc.reachable_labels(0)
    table = {c.id: sorted(c.labels(0)) for c in cc.cases_for(torch.cuda.get_device_properties(dev).multi_processor_count)}
    got = set().union(*[set(v) for v in table.values()])
    for cid in sorted(table):
        print(f"[labels] {cid}: {'; '.join(table[cid])}")
    util.measured("conv exact coverage: kernel instantiations the cases reach on this device", len(got))
    assert not (reach - got), f"instantiations no case reaches: {sorted(reach - got)}"
    missing = (cc.expected_wino_labels() | cc.expected_wgrad_labels()) - got
    assert not missing, f"instantiations written down from the dispatch that no case reaches: {sorted(missing)}"
