"""The stem pooling that writes half precision (dl_pool3x3s12_nhwc_fwd_h, csrc/stem.hip) alone, BIT FOR BIT against the pooling reference
(tests/stem_ref.py: pool_fwd_ref, pinned to torch by tests/test_stem_ref_host.py) cast on the CPU with ``.to(dtype)``: the kernel promises
dl_pool3x3s12_nhwc_fwd followed by dl_cast_f32_to_h, i.e. the fp32 maximum of every window rounded to nearest even once.  The 16-bit
patterns are compared; where the reference is a NaN any NaN passes.  Outputs live in an arena of 0xFF bytes between guard bands."""
import numpy as np
import pytest
import torch

from delora_amd import _lib as L
from tests import stem_ref as sr

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -3, -1
DTYPES = {1: torch.float16, 2: torch.bfloat16}                   # DL_DTYPE_F16 / DL_DTYPE_BF16
GUARD = 4096

# (N, H, Wc, C), Wc = conv1's output width: a single row and a single pooled column (the left neighbour wraps onto the only other
# column, no rows above or below); every row touching an image edge; batch stride and the real channel count; C / 8 not a power of two
SHAPES = ((1, 1, 2, 8), (1, 2, 6, 8), (2, 3, 10, 64), (1, 5, 18, 72))

# magnitudes around the largest finite values of the two types: 65504 is fp16's largest, 65520 the first fp32 value that rounds to inf
# there; 3.3895e38 is bf16's largest and fp32's largest rounds to inf in bf16
BIG = np.array([65504.0, 65519.996, 65520.0, 70000.3, 1e30, 3.0e38, 3.3961775e38, 3.4028235e38], dtype=np.float32)


def _dev():
    return torch.device("cuda:0")


def _inputs(shape):
    """Three fp32 maps per shape: (a) stem_ref.gen_a (small multiples of 1/4: ties everywhere); (b) the same with stem_ref.specials planted
    (NaN, +-inf, -0.0 against +0.0, windows of -inf); (c) values that need rounding in both types, with magnitudes beyond the largest
    finite fp16 / bf16 of either sign planted where they win their window or lose it, plus the planted windows of (b)."""
    N, H, Wc, C = shape
    seed = 91000 + 1009 * N + 101 * H + 7 * Wc + C
    a = sr.gen_a(shape, sr.TANH, seed)
    rng = np.random.default_rng(seed)
    c = sr.gen_a(shape, sr.NONE, seed + 1) * 1.2345678 + rng.uniform(-0.4, 0.4, size=shape)
    hit = rng.random(size=shape) < 0.15
    hit.reshape(-1)[:: max(1, hit.size // 7)] = True
    big = rng.choice(BIG.astype(np.float64), size=shape) * rng.choice([-1.0, 1.0], size=shape)
    c = np.where(hit, big, c)
    if C >= 40:                                                      # (channels the planted windows of specials never touch)
        c[0, 0, 0, 32:40] = BIG
    return [("gen_a", a.astype(np.float32)), ("specials", sr.specials(a, seed + 2).astype(np.float32)),
            ("rounding and overflow", sr.specials(c, seed + 3).astype(np.float32))]


def _run(lib, a32, code):
    """The kernel on ``a32`` with its output carved from a 0xFF arena between two guard bands: (output as int16 on the CPU, guards intact)."""
    N, H, Wc, C = a32.shape
    nbytes = N * H * (Wc // 2) * C * 2
    arena = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=_dev())
    assert arena.data_ptr() % 16 == 0
    y = arena[GUARD:GUARD + nbytes]
    a_d = torch.from_numpy(a32).to(_dev())
    L.check(lib.dl_pool3x3s12_nhwc_fwd_h(a_d.data_ptr(), N, H, Wc, C, code, y.data_ptr(), torch.cuda.current_stream().cuda_stream),
            "dl_pool3x3s12_nhwc_fwd_h")
    torch.cuda.synchronize()
    intact = bool((arena[:GUARD] == 0xFF).all()) and bool((arena[GUARD + nbytes:] == 0xFF).all())
    return y.cpu().view(torch.int16).view(N, H, Wc // 2, C), intact


@pytest.mark.parametrize("code", (1, 2), ids=("fp16", "bf16"))
@pytest.mark.parametrize("shape", SHAPES)
def test_pooled_half_output_equals_the_reference_cast_bit_for_bit(shape, code):
    lib = L.load()
    dtype = DTYPES[code]
    for name, a32 in _inputs(shape):
        ref64 = sr.pool_fwd_ref(a32)[0]                              # every maximum is an element of a32: exact in fp32
        ref32 = torch.from_numpy(ref64.astype(np.float32))
        assert np.array_equal(ref32.double().numpy(), ref64, equal_nan=True)
        ref = ref32.to(dtype)
        if name != "gen_a":
            assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any())
        if name == "rounding and overflow" and shape[3] >= 40:
            assert bool((torch.isinf(ref) & torch.isfinite(ref32)).any()), "no finite maximum rounds to inf"
            assert bool((ref.float() != ref32)[torch.isfinite(ref32)].any()), "nothing needs rounding"
        got, intact = _run(lib, a32, code)
        assert intact, f"{name} {shape}: a guard band was written"
        nan = torch.isnan(ref)
        got_t = got.view(dtype)
        assert bool(torch.isnan(got_t[nan]).all()), f"{name} {shape}: a NaN of the reference is not a NaN"
        bad = (got != ref.view(torch.int16)) & ~nan
        assert not bool(bad.any()), (name, shape, int(bad.sum()), got_t[bad][:4], ref[bad][:4])


def test_refusals_return_their_codes_and_launch_nothing():
    lib = L.load()
    N, H, Wc, C = 1, 2, 4, 16
    a = torch.ones((N, H, Wc, C), device=_dev())
    y = torch.full((N * H * (Wc // 2) * C * 2 + 64,), 0xFF, dtype=torch.uint8, device=_dev())
    fn, st = lib.dl_pool3x3s12_nhwc_fwd_h, torch.cuda.current_stream().cuda_stream
    assert fn(a.data_ptr(), N, H, Wc, 12, 2, y.data_ptr(), st) == UNSUPPORTED and b"dl_pool3x3s12_nhwc_fwd_h" in lib.dl_last_error()      # C % 8
    assert fn(a.data_ptr(), N, H, 3, C, 2, y.data_ptr(), st) == UNSUPPORTED                                                              # odd width
    for code in (0, 3):
        assert fn(a.data_ptr(), N, H, Wc, C, code, y.data_ptr(), st) == UNSUPPORTED and f"dtype={code}".encode() in lib.dl_last_error()
    assert fn(None, N, H, Wc, C, 2, y.data_ptr(), st) == INVALID
    assert fn(a.data_ptr(), N, H, Wc, C, 2, None, st) == INVALID
    assert fn(a.data_ptr(), 0, H, Wc, C, 2, y.data_ptr(), st) == INVALID
    torch.cuda.synchronize()
    assert bool((y == 0xFF).all())
