"""The kernels between the trunk's last convolution and the scalar that is minimised -- global average pooling (fp32, half, fused
backward), the fp32 -> half cast, the fused pose heads, quaternion -> T and the ICP loss with its gradient moments -- against the
references of tests/tail_ref.py: BIT FOR BIT on small-integer data (every case's headroom is asserted), within a derived
first-order rounding bound of float64 on real-valued data.  Every device buffer lives in a tests/conv_ref.Arenas allocation (guard
zones, NaN-patterned outputs and workspaces of exactly the promised size, inputs that must stay unchanged), and the C ABI is called
directly so that strides and pointer skews are the test's.  An output may legitimately BE NaN here (a mean over an empty set), so
"written" means: no element still holds the arena's poison word.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import tail_ref as tr
from tests import util

pytestmark = pytest.mark.gpu

INVALID = -1                                           # DL_ERR_INVALID_ARGUMENT


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def _p(t, offset_elems=0):
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


class Bufs:
    """Arenas plus outputs that can be poisoned again between calls and checked for elements never written."""

    def __init__(self, dev, skew=0):
        self.A, self.W, self.dev, self.outs = cr.Arenas(dev, skew), cr.Arenas(dev, 0), dev, []

    def inp(self, t, dtype=torch.float32, name=""):
        return self.A.arena(tuple(t.shape), dtype, t, name, row_elems=0)

    def out(self, shape, dtype=torch.float32, name=""):
        v = self.A.arena(shape, dtype, None, name, row_elems=0)
        self.outs.append((v, name))
        return v

    def ws(self, nbytes, name="workspace"):
        """Exactly ``nbytes`` of poisoned scratch: the guard begins at the first byte behind what the size function promised.  Never
        skewed: the entry points ask for 16-byte aligned workspaces."""
        assert nbytes % 4 == 0 and nbytes > 0
        return self.W.arena((nbytes // 4,), torch.float32, None, name, row_elems=0)

    @staticmethod
    def _words(v):
        return v.view(torch.int32) if v.element_size() == 4 else v.view(torch.int16)

    def _word(self, v):
        w = cr.NAN_WORD[v.dtype]
        return cr._as_i32(w) if v.element_size() == 4 else int(np.int16(np.uint16(w & 0xFFFF)))

    def poison(self):
        for v, _ in self.outs:
            self._words(v).fill_(self._word(v))

    def written(self, what, only=None):
        _sync()
        self.A.check(what)
        self.W.check(what)
        for v, name in self.outs:
            if only is not None and not any(v is o for o in only):
                continue
            left = int((self._words(v) == self._word(v)).sum())
            assert left == 0, f"{what}: {left} elements of {name} were never written"


# ====================================================================================================================== ICP loss


class LossRun:
    """One generated case on the device.  The source is channels 0-2 of a [B,4,HW] image (channel 3 holds NaN: it is not an operand),
    normals and match are views into wider buffers (NaN between the samples); where HW % 4 != 0 their sample strides are not
    multiples of 4 and every plane pointer is skewed by 4 bytes, which the entry point allows (the workspace stays 16-byte aligned)."""

    def __init__(self, case, dev):
        self.L, self.lib = _lib()
        B, _, HW = case["p"].shape
        self.B, self.HW, self.vec = B, HW, HW % 4 == 0
        self.b = Bufs(dev, 0 if self.vec else 4)
        padn, padm = (8, 12) if self.vec else (3, 5)
        self.ss = (4 * HW, 3 * HW + padn, 6 * HW + padm)
        nan = float("nan")
        src = torch.full((B, self.ss[0]), nan, dtype=torch.float64)
        srcn = torch.full((B, self.ss[1]), nan, dtype=torch.float64)
        match = torch.full((B, self.ss[2]), nan, dtype=torch.float64)
        src[:, :3 * HW] = torch.from_numpy(case["p"]).reshape(B, -1)
        srcn[:, :3 * HW] = torch.from_numpy(case["n"]).reshape(B, -1)
        match[:, :3 * HW] = torch.from_numpy(case["pt"]).reshape(B, -1)
        match[:, 3 * HW:6 * HW] = torch.from_numpy(case["nt"]).reshape(B, -1)
        self.src, self.srcn, self.match = self.b.inp(src, name="src"), self.b.inp(srcn, name="src normals"), self.b.inp(match, name="match")
        self.nn = self.b.inp(torch.from_numpy(case["nn"]), torch.int32, "nn_pix")
        self.T = self.b.inp(torch.from_numpy(case["T"]).reshape(B, 16), name="T")
        self.lt, self.pc, self.gt = self.b.out((B, 3), name="loss_terms"), self.b.out((B, 2), torch.int32, "pair_counts"), self.b.out((B, 36), name="grad_terms")
        self.gT = self.b.out((B, 16), name="grad_T")
        nbytes = int(self.lib.dl_icp_loss_workspace_bytes(B, 1, HW))
        assert nbytes == B * tr.loss_blocks(HW) * 40 * 4
        self.wsp = self.b.ws(nbytes)

    def args(self, first=0, B=None):
        s = self
        return (_p(s.src, first * s.ss[0]), s.ss[0], _p(s.srcn, first * s.ss[1]), s.ss[1], _p(s.match, first * s.ss[2]), s.ss[2],
                _p(s.nn, first * s.HW), _p(s.T, first * 16), s.B if B is None else B, 1, s.HW)

    def fwd(self, flags, split=False, first=0, B=None):
        """loss_terms, pair_counts, grad_terms (numpy) of samples [first, first + B)."""
        s, lib = self, self.lib
        s.b.poison()
        a = s.args(first, B)
        if split:
            s.L.check(lib.dl_icp_loss_partial(*a, flags, _p(s.wsp), _stream()), "dl_icp_loss_partial")
            s.L.check(lib.dl_icp_loss_reduce(_p(s.wsp), a[8], 1, s.HW, flags, _p(s.lt), _p(s.pc), _p(s.gt), _stream()), "dl_icp_loss_reduce")
        else:
            s.L.check(lib.dl_icp_loss_fwd(*a, flags, _p(s.lt), _p(s.pc), _p(s.gt), _p(s.wsp), _stream()), "dl_icp_loss_fwd")
        n = a[8]
        if n == s.B:
            s.b.written(f"loss HW={s.HW} flags={flags}", only=(s.lt, s.pc, s.gt))
        _sync()
        return {"loss_terms": s.lt[:n].cpu().numpy(), "pair_counts": s.pc[:n].cpu().numpy(), "grad_terms": s.gt[:n].cpu().numpy().reshape(n, 3, 12)}

    def bwd(self, w):
        """grad_T [B,4,4] from the grad_terms the last full forward left on the device."""
        s = self
        w_d = s.b.inp(torch.from_numpy(w), name="grad_loss_terms")
        s.L.check(s.lib.dl_icp_loss_bwd(_p(s.gt), _p(w_d), s.B, _p(s.gT), _stream()), "dl_icp_loss_bwd")
        s.b.written(f"loss bwd HW={s.HW}", only=(s.gT,))
        return s.gT.cpu().numpy().reshape(s.B, 4, 4)


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def _loss_weights(B):
    """grad_loss_terms: not dyadic, so that an fma in the backward would show; one sample with zeros."""
    w = (np.arange(B * 3, dtype=np.float32).reshape(B, 3) % 7 - 3) * np.float32(0.3) + np.float32(0.1)
    w[B // 2] = 0
    return w


def _loss_exact(case, flag_words, neighbours=True):
    dev = _dev()
    run = LossRun(case, dev)
    bad = []
    for i, flags in enumerate(flag_words):
        tr.loss_headroom(case, flags)
        ref = tr.icp_loss(case, flags)
        got = run.fwd(flags)
        mism = tr.compare_loss_exact(got, ref)
        if any(mism.values()):
            bad.append((flags, mism))
            for b in range(run.B):
                for k in mism:
                    if tr.same_bits(got[k][b], ref[k][b]):
                        print(f"HW={run.HW} flags={flags} sample {b} {k}:\n  got      {got[k][b].reshape(-1)}\n  expected {ref[k][b].reshape(-1)}")
        w = _loss_weights(run.B)
        gT = run.bwd(w)
        nb = tr.same_bits(gT, tr.icp_loss_bwd(got["grad_terms"], w))
        if nb:
            bad.append((flags, {"grad_T": nb}))
        assert _same(got, run.fwd(flags, split=True)), f"flags {flags}: dl_icp_loss_fwd and partial + reduce differ"
        if i == 0:
            assert _same(got, run.fwd(flags)), "two runs differ"
            if neighbours and run.B > 1:
                b = run.B - 2
                alone = run.fwd(flags, first=b, B=1)
                assert _same(alone, {k: v[b:b + 1] for k, v in got.items()}), "a sample's result depends on its neighbours in the batch"
    run.b.written(f"loss HW={run.HW}", only=())
    assert not bad, f"HW={run.HW}: mismatching elements per flag word: {bad}"


@pytest.mark.parametrize("HW", [hw for hw, _ in tr.LOSS_HW])
def test_loss_exact(HW):
    """loss_terms, pair_counts, the 36 grad_terms per sample and grad_T equal the float64 reference bit for bit on integer data, for
    the four kernel instantiations (all 18 flag words at 260 and 1028); fwd == partial + reduce; two runs agree; a sample does not
    see its neighbours; guards, inputs and the workspace's end are untouched."""
    _loss_exact(tr.loss_case_exact(HW), tr.LOSS_FLAG_WORDS if HW in tr.LOSS_ALL_FLAGS_HW else tr.LOSS_INSTANCES)


def test_loss_exact_batch_of_17():
    """B = 17: dl_icp_loss_bwd crosses its 256-thread block (272 threads)."""
    _loss_exact(tr.loss_case_exact(tr.LOSS_B17_HW, B=17, seed=3), tr.LOSS_INSTANCES)


@pytest.mark.parametrize("HW", [260, 1021])
def test_loss_empty_and_all_normal_samples(HW):
    """Sample 0 has no valid pixel: counts 0, NaN for enabled terms and their gradients, 0 for disabled ones.  Every pair of sample
    1 has normals on both sides: NaN for point-to-point only."""
    case = tr.loss_case_exact(HW, seed=5)
    case["nn"][0][:] = -1
    case["pt"][0][:] = 0
    case["nt"][0][:] = 0
    v = case["nn"][1] >= 0
    for k in ("n", "nt"):
        z = v & ~tr._has(case[k][1])
        case[k][1][0, z] = 1
    _loss_exact(case, tr.LOSS_FLAG_WORDS, neighbours=False)
    run = LossRun(case, _dev())
    for flags in (tr.P2P | tr.PO2PL, tr.P2P | tr.PO2PL | tr.PL2PL | tr.LINEAR):
        got = run.fwd(flags)
        on = np.array([True, True, bool(flags & tr.PL2PL)])
        assert got["pair_counts"][0].tolist() == [0, 0] and got["pair_counts"][1][1] == 0 and got["pair_counts"][1][0] == int(v.sum())
        assert np.isnan(got["loss_terms"][0][on]).all() and (got["loss_terms"][0][~on] == 0).all()
        assert np.isnan(got["grad_terms"][0][on]).all() and (got["grad_terms"][0][~on] == 0).all()
        assert np.isnan(got["loss_terms"][1][0]) and np.isnan(got["grad_terms"][1][0]).all()
        assert np.isfinite(got["loss_terms"][1][1:]).all() and np.isfinite(got["grad_terms"][1][1:]).all()
        assert np.isfinite(got["loss_terms"][2]).all() and np.isfinite(got["grad_terms"][2]).all()
    run.b.written("special samples", only=())


@pytest.mark.parametrize("HW", [260, 1021, 26000])
def test_loss_ignores_finite_garbage_at_pixels_that_do_not_count(HW):
    """Non-zero integer garbage in all thirteen planes where nn_pix < 0, and other non-zero normals where the partner has none,
    change no bit: the masking is multiplicative (include/delora_hip.h), so finite operands contribute exact zeros."""
    case = tr.loss_case_exact(HW, seed=7)
    clean, dirty = LossRun(case, _dev()), LossRun(tr.loss_garbage(case), _dev())
    for flags in tr.LOSS_INSTANCES + [tr.ALONE | tr.P2P]:
        a, b = clean.fwd(flags), dirty.fwd(flags)
        assert not any(tr.compare_loss_exact(a, tr.icp_loss(case, flags)).values())
        assert _same(a, b), f"flags {flags}: garbage at masked pixels changed the result"
    clean.b.written("clean", only=())
    dirty.b.written("garbage", only=())


def test_loss_refusals():
    """Null pointers, misaligned planes with H*W % 4 == 0, a misaligned workspace and ALONE with a normal-based term are refused
    before any launch."""
    run = LossRun(tr.loss_case_exact(256, seed=9), _dev())
    lib, a = run.lib, list(run.args())
    run.b.poison()
    tail = (_p(run.lt), _p(run.pc), _p(run.gt), _p(run.wsp), _stream())
    assert lib.dl_icp_loss_fwd(*a, 6, *tail) == 0
    for i in (0, 2, 4, 6, 7):
        bad = list(a)
        bad[i] = ctypes.c_void_p(0)
        assert lib.dl_icp_loss_fwd(*bad, 6, *tail) == INVALID, f"null argument {i}"
    for i in range(4):
        bad = list(tail)
        bad[i] = ctypes.c_void_p(0)
        assert lib.dl_icp_loss_fwd(*a, 6, *bad) == INVALID, f"null output {i}"
    for i in (0, 2, 4, 6):                                          # a plane 4 bytes off a 16-byte boundary
        bad = list(a)
        bad[i] = ctypes.c_void_p(bad[i].value + 4)
        assert lib.dl_icp_loss_fwd(*bad, 6, *tail) == INVALID, f"misaligned argument {i}"
    for i in (1, 3, 5):                                             # a sample stride that is no multiple of 4
        bad = list(a)
        bad[i] = bad[i] + 1
        assert lib.dl_icp_loss_fwd(*bad, 6, *tail) == INVALID, f"stride {i}"
    for flags in (tr.ALONE | tr.PO2PL, tr.ALONE | tr.PL2PL | tr.P2P, tr.ALONE | 15):
        assert lib.dl_icp_loss_fwd(*a, flags, *tail) == INVALID, f"flags {flags}"
    off = ctypes.c_void_p(run.wsp.data_ptr() + 4)                   # a workspace 4 bytes off a 16-byte boundary
    assert lib.dl_icp_loss_fwd(*a, 6, _p(run.lt), _p(run.pc), _p(run.gt), off, _stream()) == INVALID
    assert lib.dl_icp_loss_partial(*a, 6, off, _stream()) == INVALID
    assert lib.dl_icp_loss_reduce(off, run.B, 1, run.HW, 6, _p(run.lt), _p(run.pc), _p(run.gt), _stream()) == INVALID
    assert lib.dl_icp_loss_bwd(_p(None), _p(run.lt), run.B, _p(run.gT), _stream()) == INVALID
    assert lib.dl_icp_loss_bwd(_p(run.gt), _p(run.lt), 0, _p(run.gT), _stream()) == INVALID
    assert lib.dl_icp_loss_reduce(_p(None), run.B, 1, run.HW, 6, _p(run.lt), _p(run.pc), _p(run.gt), _stream()) == INVALID
    run.b.written("refusals", only=(run.lt, run.pc, run.gt))


@pytest.mark.parametrize("HW", [260, 1021])
def test_loss_non_finite_pose_stays_in_its_sample(HW):
    """NaN, inf and 1e30 in one sample's T (include/delora_hip.h: T may be anything): the other samples' outputs do not change by a bit."""
    case = tr.loss_case_exact(HW, seed=13)
    clean = LossRun(case, _dev())
    for val in (float("nan"), float("inf"), -1e30):
        bad = {k: v.copy() for k, v in case.items() if not k.startswith("_")}
        bad["T"][1, 0, 3], bad["T"][1, 1, 1], bad["T"][1, 2, :3] = val, val, val
        dirty = LossRun(bad, _dev())
        for flags in tr.LOSS_INSTANCES:
            a, b = clean.fwd(flags), dirty.fwd(flags)
            assert _same({k: v[[0, 2]] for k, v in a.items()}, {k: v[[0, 2]] for k, v in b.items()}), f"T = {val}, flags {flags}: the neighbours changed"
            assert not np.isfinite(b["loss_terms"][1, 1:]).all(), f"T = {val}: sample 1 is untouched by its own pose"
        dirty.b.written("non-finite pose", only=())
    clean.b.written("non-finite pose, clean", only=())


LOSS_REAL = [("random", 1.0, 1028), ("converged", 1.0, 1028), ("random", 1e-2, 1021), ("converged", 1e-2, 1028), ("random", 1e2, 1028),
             ("converged", 1e2, 1021), ("random", 1.0, 26000), ("converged", 1.0, 131076), ("random", 1.0, 131333)]


@pytest.mark.parametrize("kind,scale,HW", LOSS_REAL)
def test_loss_float64(kind, scale, HW):
    """Real-valued scenes: every loss term and gradient moment within (c_term + c_sum) 2^-24 S_abs + 1 ulp of float64
    (tests/tail_ref.py derives c_term per accumulator, at most 16, and c_sum = 2 ceil(chunks / waves) + 20 from the kernel's code)."""
    case = tr.loss_case_real(HW, kind, scale=scale, seed=11)
    run = LossRun(case, _dev())
    worst = {"loss_terms": 0.0, "grad_terms": 0.0}
    for flags in tr.LOSS_INSTANCES + ([tr.ALONE | tr.P2P] if HW < 5000 else []):
        ref = tr.icp_loss(case, flags, majorant=True)
        got = run.fwd(flags)
        ratio = tr.compare_loss_real(got, ref, flags, HW)
        print(f"{kind} scale {scale} HW {HW} flags {flags}: error / bound {ratio}")
        worst = {k: max(worst[k], ratio[k]) for k in worst}
    run.b.written("loss float64", only=())
    for k, v in worst.items():
        util.measured(f"icp loss vs float64, {kind} scene, scale {scale:g}, HW {HW}: {k} error / bound", v, bound=1.0)


# ====================================================================================================================== pose heads


class HeadsRun:
    def __init__(self, x, P, scale, dev):
        self.L, self.lib = _lib()
        self.B, self.F = x.shape
        self.R, self.Hd = P["fc_w"].shape[0], P["r1_w"].shape[0]
        B, F, R, Hd = self.B, self.F, self.R, self.Hd
        self.b = b = Bufs(dev)
        self.x = b.inp(x, name="x")
        self.P = {k: b.inp(v, name=k) for k, v in P.items()}
        self.scale = b.inp(scale, name="fc_scale")
        self.params = self.struct(self.P)
        self.fo = {"a1": b.out((B, R), name="a1"), "a2": b.out((B, 2, Hd), name="a2"), "rot_raw": b.out((B, 4), name="rot_raw"),
                   "translation": b.out((B, 3), name="translation"), "rotation": b.out((B, 4), name="rotation"), "norm": b.out((1,), name="norm")}
        self.G = {k: b.out(tuple(v.shape), name="d_" + k) for k, v in P.items()}
        self.grads = self.struct(self.G)
        self.gx = b.out((B, F), name="grad_x")
        nbytes = int(self.lib.dl_heads_bwd_workspace_bytes(B, F, R, Hd))
        assert nbytes == 4 * (B * 2 * Hd + B * R + -(-R // 40) * B * F)
        self.wsp = b.ws(nbytes)

    def struct(self, d):
        s = self.L.HeadsParams()
        for k in tr.HEAD_PARAMS:
            setattr(s, k, d[k].data_ptr())
        return s

    def fwd(self, act, use_scale):
        s, o = self, self.fo
        s.b.poison()
        a = (_p(s.x), ctypes.byref(s.params), s.B, s.F, s.R, s.Hd, act)
        outs = (_p(o["a1"]), _p(o["a2"]), _p(o["rot_raw"]), _p(o["translation"]), _p(o["rotation"]), _p(o["norm"]), _stream())
        if use_scale:
            s.L.check(s.lib.dl_heads_fwd_drop(*a, _p(s.scale), *outs), "dl_heads_fwd_drop")
        else:
            s.L.check(s.lib.dl_heads_fwd(*a, *outs), "dl_heads_fwd")
        s.b.written(f"heads fwd {(s.B, s.F, s.R, s.Hd)} act {act}", only=tuple(o.values()))
        return {k: v.cpu() for k, v in o.items()}

    def bwd(self, act, use_scale, saved, g_t, g_r):
        s = self
        s.b.poison()
        sv = {k: s.b.inp(v, name="saved " + k) for k, v in saved.items()}
        gt_d, gr_d = s.b.inp(g_t, name="grad_translation"), s.b.inp(g_r, name="grad_rotation")
        a = (_p(s.x), ctypes.byref(s.params), s.B, s.F, s.R, s.Hd, act)
        rest = (_p(sv["a1"]), _p(sv["a2"]), _p(sv["rot_raw"]), _p(sv["norm"]), _p(gt_d), _p(gr_d), ctypes.byref(s.grads), _p(s.gx), _p(s.wsp), _stream())
        if use_scale:
            s.L.check(s.lib.dl_heads_bwd_drop(*a, _p(s.scale), *rest), "dl_heads_bwd_drop")
        else:
            s.L.check(s.lib.dl_heads_bwd(*a, *rest), "dl_heads_bwd")
        s.b.written(f"heads bwd {(s.B, s.F, s.R, s.Hd)} act {act}", only=tuple(s.G.values()) + (s.gx,))
        out = {"d_" + k: v.cpu() for k, v in s.G.items()}
        out["grad_x"] = s.gx.cpu()
        return out


@pytest.mark.parametrize("shape", tr.HEADS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_heads_exact(shape):
    """Integer inputs and weights, act none and relu, with and without a 0 / 1.25 mask: a1, a2, rot_raw, translation bit for bit,
    norm = fp32 sqrt of the exact sum, rotation = the fp32 quotient; with grad_rotation = 0 every rotation-head gradient is exactly
    zero and the other seven gradients equal the reference bit for bit."""
    x, P, scale, g_t = tr.heads_case_exact(*shape)
    run = HeadsRun(x, P, scale, _dev())
    zero = torch.zeros(shape[0], 4, dtype=torch.float64)
    bad = []
    for act in (0, 2):
        for use in (False, True):
            sc = scale if use else None
            tr.heads_headroom(x, P, sc, g_t, act)
            ref = tr.heads(x, P, act, sc, g_t, zero)
            exp = tr.heads_exact_expect(ref)
            got = run.fwd(act, use)
            for k in tr.HEADS_FWD_OUT:
                n = cr.mismatches(got[k], exp[k], f"heads {shape} act {act} mask {use}: {k}")
                if n:
                    bad.append((act, use, k, n))
            gb = run.bwd(act, use, tr.heads_saved(ref), g_t, zero)
            for k in tr.HEADS_BWD_OUT:
                want = torch.zeros_like(exp[k]) if k[2:4] in ("r1", "r3") else exp[k]
                n = cr.mismatches(gb[k], want, f"heads {shape} act {act} mask {use}: {k}")
                if n:
                    bad.append((act, use, k, n))
    run.b.written("heads exact", only=())
    assert not bad, f"heads {shape}: mismatching elements (act, mask, output, count): {bad}"


@pytest.mark.parametrize("shape", tr.HEADS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_heads_float64(shape):
    """All three activations, general gradients, with and without the mask: every output within the first-order rounding bound of
    tests/tail_ref.heads_bounds of the float64 autograd reference."""
    x, P, scale, g_t, g_r = tr.heads_case_real(*shape)
    run = HeadsRun(x, P, scale, _dev())
    worst = {}
    for act in (0, 1, 2):
        for use in (False, True):
            sc = scale if use else None
            ref, bnd = tr.heads_bounds(x, P, act, sc, g_t, g_r)
            got = run.fwd(act, use)
            got.update(run.bwd(act, use, tr.heads_saved(ref), g_t, g_r))
            for k in bnd:
                r = tr.worst_ratio(got[k].numpy(), ref[k].numpy(), bnd[k].numpy())
                worst[k] = max(worst.get(k, 0.0), r)
    run.b.written("heads float64", only=())
    name = "x".join(map(str, shape))
    fwd, bwd = max(worst[k] for k in tr.HEADS_FWD_OUT), max(worst[k] for k in tr.HEADS_BWD_OUT)
    print(f"heads {name}: forward {fwd:.4g}, gradients {bwd:.4g}")
    for k in tr.HEADS_FWD_OUT + tr.HEADS_BWD_OUT:
        util.measured(f"heads {name} vs float64: {k} error / bound", worst[k], bound=1.0)


def test_heads_refusals():
    x, P, scale, g_t = tr.heads_case_exact(3, 70, 41, 5)
    run = HeadsRun(x, P, scale, _dev())
    lib, o = run.lib, run.fo
    run.b.poison()
    outs = (_p(o["a1"]), _p(o["a2"]), _p(o["rot_raw"]), _p(o["translation"]), _p(o["rotation"]), _p(o["norm"]), _stream())
    for B in (17, 0):
        assert lib.dl_heads_fwd(_p(run.x), ctypes.byref(run.params), B, run.F, run.R, run.Hd, 2, *outs) == INVALID
        assert lib.dl_heads_bwd_workspace_bytes(B, run.F, run.R, run.Hd) == 0
        assert lib.dl_heads_bwd(_p(run.x), ctypes.byref(run.params), B, run.F, run.R, run.Hd, 2, _p(o["a1"]), _p(o["a2"]), _p(o["rot_raw"]), _p(o["norm"]),
                                _p(o["translation"]), _p(o["rotation"]), ctypes.byref(run.grads), _p(run.gx), _p(run.wsp), _stream()) == INVALID
    for k in tr.HEAD_PARAMS:
        broken = run.struct(run.P)
        setattr(broken, k, None)
        assert lib.dl_heads_fwd(_p(run.x), ctypes.byref(broken), run.B, run.F, run.R, run.Hd, 2, *outs) == INVALID, k
        assert lib.dl_heads_bwd(_p(run.x), ctypes.byref(run.params), run.B, run.F, run.R, run.Hd, 2, _p(o["a1"]), _p(o["a2"]), _p(o["rot_raw"]), _p(o["norm"]),
                                _p(o["translation"]), _p(o["rotation"]), ctypes.byref(broken), _p(run.gx), _p(run.wsp), _stream()) == INVALID, k
    assert lib.dl_heads_fwd(_p(run.x), ctypes.byref(run.params), run.B, run.F, run.R, run.Hd, 3, *outs) == INVALID
    _sync()
    run.b.A.check("heads refusals")
    for v, name in run.b.outs:                                     # nothing was launched: every output still holds the poison
        assert int((v.view(torch.int32) != cr._as_i32(cr.NAN_WORD[v.dtype])).sum()) == 0, name


# ====================================================================================================================== pooling, cast


MEAN_CASES = [("f32", torch.float32, 0)] + [("half", tr.HALF[c], c) for c in (1, 2)]


def _mean_call(lib, L, x_d, N, P, C, code, y_d):
    if code == 0:
        return lib.dl_mean_hw_nhwc_f32(_p(x_d), N, P, C, _p(y_d), _stream())
    return lib.dl_mean_hw_nhwc_h(_p(x_d), N, P, C, code, _p(y_d), _stream())


@pytest.mark.parametrize("kind,dtype,code", MEAN_CASES, ids=["f32", "f16", "bf16"])
def test_mean_exact_and_float64(kind, dtype, code):
    """Integer data: float32 sum * (1.0f / P) bit for bit.  Real data: within (adds + 1) 2^-24 sum|x| / P of float64, adds = ceil(P / lanes) +
    log2(lanes) (tests/tail_ref.mean_bound)."""
    dev = _dev()
    L, lib = _lib()
    lanes = 64 if code == 0 else 128
    bad, worst = [], 0.0
    for N in tr.MEAN_N:
        for C in tr.MEAN_C[kind]:
            b = Bufs(dev)
            for P in tr.MEAN_P:
                for exact in (True, False):
                    x = tr.mean_case(N, P, C, dtype, seed=P + C, exact=exact)
                    x_d, y_d = b.inp(x, dtype, "x"), b.out((N, C), name="y")
                    L.check(_mean_call(lib, L, x_d, N, P, C, code, y_d), "dl_mean_hw")
                    _sync()
                    if exact:
                        tr.pool_headroom(x)
                        n = cr.mismatches(y_d, tr.mean_exact(x), f"mean {kind} N{N} P{P} C{C}")
                        if n:
                            bad.append((N, P, C, n))
                    else:
                        ref, bnd = tr.mean_bound(x, lanes)
                        worst = max(worst, tr.worst_ratio(y_d.cpu().numpy(), ref.numpy(), bnd.numpy()))
            b.written(f"mean {kind} N{N} C{C}")
    assert not bad, f"mean {kind}: (N, P, C, mismatches) {bad}"
    util.measured(f"global average pooling ({'fp32' if code == 0 else str(dtype)}) vs float64: error / bound", worst, bound=1.0)


def test_mean_refusals():
    dev = _dev()
    L, lib = _lib()
    b = Bufs(dev)
    x_d, y_d = b.inp(torch.zeros(1, 4, 24), name="x"), b.out((1, 24), name="y")
    assert lib.dl_mean_hw_nhwc_f32(_p(x_d), 1, 16, 6, _p(y_d), _stream()) != 0            # C % 4
    assert lib.dl_mean_hw_nhwc_f32(_p(None), 1, 4, 24, _p(y_d), _stream()) == INVALID
    for code in (1, 2):
        assert lib.dl_mean_hw_nhwc_h(_p(x_d), 1, 4, 12, code, _p(y_d), _stream()) == INVALID   # C % 8
        assert lib.dl_mean_hw_bwd_act_h(_p(y_d), _p(x_d), 1, 4, 12, 1, code, _p(y_d), _stream()) == INVALID
        assert lib.dl_cast_f32_to_h(_p(x_d), _p(y_d), 12, code, _stream()) == INVALID       # n % 8
    assert lib.dl_mean_hw_nhwc_h(_p(x_d), 1, 4, 24, 0, _p(y_d), _stream()) == INVALID        # dtype
    assert lib.dl_mean_hw_bwd_act_h(_p(y_d), _p(x_d), 1, 4, 24, 3, 1, _p(y_d), _stream()) == INVALID   # act
    _sync()
    b.A.check("mean refusals")
    assert int((y_d.view(torch.int32) != cr._as_i32(cr.NAN_WORD[torch.float32])).sum()) == 0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _half_equal(got, want, what):
    """Bit equality of two half tensors, any NaN matching any NaN."""
    got, want = got.cpu(), want.cpu()
    badm = (_bits(got) != _bits(want)) & ~(torch.isnan(got) & torch.isnan(want))
    n = int(badm.sum())
    if n:
        i = torch.nonzero(badm.reshape(-1))[:8, 0].tolist()
        print(f"{what}: {n} differ; first at {i}: got {[float(got.reshape(-1)[j]) for j in i]} expected {[float(want.reshape(-1)[j]) for j in i]}")
    return n


@pytest.mark.parametrize("code", [1, 2], ids=["f16", "bf16"])
def test_cast_and_mean_backward_are_bit_exact(code):
    """dl_cast_f32_to_h equals torch's round-to-nearest-even conversion, and dl_mean_hw_bwd_act_h an op-by-op fp32 emulation followed
    by it, bit for bit, on +-0, subnormals of the half type, ties, values that round to infinity, +-inf, NaN and the largest finite
    values; sizes cross a 256-thread block of 8-element groups and n = 8; the backward runs the three activations."""
    dev = _dev()
    L, lib = _lib()
    dtype = tr.HALF[code]
    b = Bufs(dev)
    bad = 0
    for n in tr.ELEMENTWISE_N:
        src = tr.special_values(dtype, n, seed=n)
        s_d, d_d = b.inp(src, name="src"), b.out((n,), dtype, "dst")
        L.check(lib.dl_cast_f32_to_h(_p(s_d), _p(d_d), n, code, _stream()), "dl_cast_f32_to_h")
        _sync()
        bad += _half_equal(d_d, tr.cast_ref(src, dtype), f"cast n={n}")
        # backward on the same number of elements: C = 8 channels, two images where n allows it
        N, C = (2 if n % 16 == 0 else 1), 8
        P = n // (N * C)
        x = tr.special_values(dtype, n, seed=n + 1).to(dtype).view(N, P, C)
        gy = tr.special_values(dtype, N * C, seed=n + 2).view(N, C)
        gy[0, 0], gy[0, 1] = 3.0, -0.37
        x_d, gy_d = b.inp(x, dtype, "x"), b.inp(gy, name="grad_y")
        for act in (0, 1, 2):
            g_d = b.out((N, P, C), dtype, f"grad_pre act {act}")
            L.check(lib.dl_mean_hw_bwd_act_h(_p(gy_d), _p(x_d), N, P, C, act, code, _p(g_d), _stream()), "dl_mean_hw_bwd_act_h")
            _sync()
            bad += _half_equal(g_d, tr.mean_bwd_act(gy, x, P, act, dtype), f"mean backward n={n} act={act}")
    b.written("cast / mean backward")                               # any NaN matches any NaN above: the poison must be gone as well
    assert bad == 0


# ====================================================================================================================== quaternion -> T


@pytest.mark.parametrize("B", tr.QUAT_B)
def test_quat_to_T_float64(B):
    """Per-element float64 reference: 1e-6 absolute forward, 2e-5 of the row's largest component backward (the project's bounds, now
    against float64); grad_translation is a bit-exact copy.  Unnormalised, tiny on both sides of eps, exactly eps, up to 1e18."""
    dev = _dev()
    L, lib = _lib()
    eps = 1e-12
    q, t, G = tr.quat_case(B, eps, seed=B)
    b = Bufs(dev)
    q_d, t_d, G_d = b.inp(q, name="q"), b.inp(t, name="t"), b.inp(G.reshape(B, 16), name="grad_T")
    T_d, gt_d, gq_d = b.out((B, 16), name="T"), b.out((B, 3), name="grad_t"), b.out((B, 4), name="grad_q")
    L.check(lib.dl_quat_to_T_fwd(_p(t_d), _p(q_d), B, eps, _p(T_d), _stream()), "dl_quat_to_T_fwd")
    L.check(lib.dl_quat_to_T_bwd(_p(q_d), _p(G_d), B, eps, _p(gt_d), _p(gq_d), _stream()), "dl_quat_to_T_bwd")
    b.written(f"quat B={B}")
    T_ref, gt_ref, gq_ref = tr.quat_to_T(q, t, np.float32(eps), G)
    T = T_d.cpu().double().view(B, 4, 4)
    assert torch.equal(T[:, :3, 3], t.double()) and torch.equal(T[:, 3], torch.tensor([0.0, 0, 0, 1]).double().expand(B, 4))
    assert torch.equal(gt_d.cpu(), G[:, :3, 3]), "grad_translation is not a bit-exact copy"
    util.measured(f"quaternion -> T vs float64, B={B} (absolute)", float((T - T_ref).abs().max()), bound=1e-6)
    scale = gq_ref.abs().amax(dim=1, keepdim=True).clamp_min(1e-30)
    util.measured(f"quaternion -> T: dL/dq vs float64 autograd, B={B} (relative to the row's largest component)",
                  float(((gq_d.cpu().double() - gq_ref).abs() / scale).max()), bound=2e-5)
    assert lib.dl_quat_to_T_fwd(_p(None), _p(q_d), B, eps, _p(T_d), _stream()) == INVALID
    assert lib.dl_quat_to_T_bwd(_p(q_d), _p(G_d), 0, eps, _p(gt_d), _p(gq_d), _stream()) == INVALID
