"""The four stream kernels of csrc/dropout.hip that tests/test_gpu_tower_dropout.py does not cover -- ``dl_dropout_scale_f32``,
``dl_stem_input_nhwc_drop_f32``, ``dl_channel_scale_nhwc_t``, ``dl_channel_scale_bwd_act_nhwc_t`` -- through the C ABI in
tests/conv_ref.Arenas allocations (inputs frozen, outputs poisoned and exactly as long as promised, guards checked after every
launch), bit for bit against the host replica of the random stream (tests/test_dropout_host.site_scales) and plain numpy products on
integer and grid data.  A device error ends the session."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import ring_ref as rr
from tests import util
from tests.test_dropout_host import SITE_CHANNELS, SITE_FC, SITE_INPUT, site_scales

pytestmark = pytest.mark.gpu

SEEDS = [1234, (7 << 32) | 1234]
# integers the storage type holds exactly, large enough that x * k / 4 needs more significant bits than a half type has
XMAX = {torch.float32: 8, torch.float16: 2000, torch.bfloat16: 200}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _lib():
    from delora_amd import _lib
    return _lib, _lib.load()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _seed_arena(A, seed):
    return A.arena((2,), torch.int32, torch.tensor([int(seed)], dtype=torch.int64).view(torch.int32), "seed", row_elems=0)


def _done(A, what, out):
    _sync()
    A.check(what)
    A.check_output(out, what)


@pytest.mark.parametrize("p", [0.2, 0.5, 0.0])
@pytest.mark.parametrize("seed", SEEDS, ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("n", [1, 3, 5, 1023, 1025])
def test_dropout_scale_writes_n_decisions_and_nothing_past_them(n, seed, p):
    """The last thread owns a partial quad for n = 1, 3, 5, 1023 and 1025 (a second block): the buffer is n floats long, its guards stay."""
    dev = _dev()
    L, lib = _lib()
    bad = 0
    for site in (SITE_CHANNELS, SITE_FC):
        A = cr.Arenas(dev)
        sd, s_d = _seed_arena(A, seed), A.arena((n,), torch.float32, None, "scale", row_elems=0)
        L.check(lib.dl_dropout_scale_f32(_p(sd), site, p, n, _p(s_d), _stream()), "dl_dropout_scale_f32")
        _done(A, f"dropout scale n {n} site {site}", s_d)
        bad += rr.bits_differ(s_d.cpu().numpy(), site_scales(seed, site, n, p), f"dropout scale n {n} site {site} p {p}")
    util.measured(f"dropout exact scale n {n} seed {seed:#x} p {p}: elements that differ", bad, bound=0)


@pytest.mark.parametrize("C", [4, 8, 12])
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 20), (1, 5, 257)], ids=lambda s: "x".join(map(str, s)))
def test_stem_input_transpose_with_the_site_1_mask(shape, C):
    """x [N][C][H][W] integers -> [N][H][W][C] times the mask whose decision index is the flat index of the OUTPUT element; the product
    with 0 or 1.25 is exact.  C / 4 generator calls per pixel: one, two and three."""
    dev = _dev()
    L, lib = _lib()
    N, H, W = shape
    bad = 0
    for seed in SEEDS:
        for p in (0.2, 0.0):
            x = rr.ints((N, C, H, W), 8, 100 * C + W).numpy().astype(np.float32)
            A = cr.Arenas(dev)
            x_d, sd = A.arena(x.shape, torch.float32, torch.from_numpy(x), "x_nchw", row_elems=0), _seed_arena(A, seed)
            y_d = A.arena((N, H, W, C), torch.float32, None, "x_nhwc", row_elems=0)
            L.check(lib.dl_stem_input_nhwc_drop_f32(_p(x_d), N, C, H, W, _p(sd), p, _p(y_d), _stream()), "dl_stem_input_nhwc_drop_f32")
            _done(A, f"stem input {shape} C {C}", y_d)
            s = site_scales(seed, SITE_INPUT, N * H * W * C, p).reshape(N, H, W, C)
            want = np.ascontiguousarray(x.transpose(0, 2, 3, 1)) * s                     # one fp32 product per element
            assert want.dtype == np.float32
            bad += rr.bits_differ(y_d.cpu().numpy(), want, f"stem input {shape} C {C} seed {seed:#x} p {p}")
    util.measured(f"dropout exact stem input {shape} C {C}: elements that differ", bad, bound=0)


def _scale_vector(N, C):
    """[N][C] multiples of 1/4 in [-1, 1.25], a different pattern per sample and no period that divides a vector width."""
    n, c = np.arange(N)[:, None], np.arange(C)[None, :]
    return (((7 * n + 3 * c + (c // 8)) % 10) - 4).astype(np.float32) * np.float32(0.25)


CH_PARAMS = [(st, C) for st in rr.STORAGES for C in ((4 if st == torch.float32 else 8), 24, 256)]


@pytest.mark.parametrize("storage,C", CH_PARAMS, ids=[f"{rr.ST_NAME[s]}-C{c}" for s, c in CH_PARAMS])
def test_channel_scale_forward_and_backward(storage, C):
    """y = x * scale[n][c] and g_pre = (g * scale[n][c]) * act'(x) for P in 1, 23 and N in 1, 3, every activation: integer x and g,
    scales on the grid 1/4, saved activations on the grid 1/4 -- every fp32 intermediate is exact and the result is rounded once."""
    dev = _dev()
    L, lib = _lib()
    code = cr.DTYPE_CODE[storage]
    xmax = XMAX[storage]
    assert xmax * 5 * 16 < cr.LIMIT                     # |g s| <= 1.25 xmax on the grid 1/4, times 1 - y^2 on the grid 1/16
    bad = 0
    for N in (1, 3):
        for P in (1, 23):
            s = _scale_vector(N, C)
            assert N == 1 or not np.array_equal(s[0], s[1])
            sd = 1000 * N + 10 * P + C
            x = rr.ints((N, P, C), xmax, sd).numpy().astype(np.float32)
            A = cr.Arenas(dev)
            x_d, s_d = A.arena(x.shape, storage, rr.to_storage(x, storage), "x", row_elems=0), A.arena(s.shape, torch.float32, torch.from_numpy(s), "scale", row_elems=0)
            y_d = A.arena(x.shape, storage, None, "y", row_elems=0)
            L.check(lib.dl_channel_scale_nhwc_t(_p(x_d), _p(s_d), N, P, C, code, _p(y_d), _stream()), "dl_channel_scale_nhwc_t")
            what = f"channel scale {rr.ST_NAME[storage]} N {N} P {P} C {C}"
            _done(A, what, y_d)
            bad += rr.bits_differ(y_d.float().cpu().numpy(), rr.round_to(x * s[:, None, :], storage), what)
            for act in rr.ACTS:
                g, a = rr.ints((N, P, C), xmax, sd + 1 + act).numpy().astype(np.float32), rr.saved((N, P, C), act, sd + 5 + act).astype(np.float32)
                A = cr.Arenas(dev)
                g_d, a_d = A.arena(g.shape, storage, rr.to_storage(g, storage), "g", row_elems=0), A.arena(a.shape, storage, rr.to_storage(a, storage), "x", row_elems=0)
                s_d, o_d = A.arena(s.shape, torch.float32, torch.from_numpy(s), "scale", row_elems=0), A.arena(g.shape, storage, None, "g_pre", row_elems=0)
                L.check(lib.dl_channel_scale_bwd_act_nhwc_t(_p(g_d), _p(a_d), _p(s_d), N, P, C, act, code, _p(o_d), _stream()), "dl_channel_scale_bwd_act_nhwc_t")
                what = f"channel scale backward {rr.ST_NAME[storage]} N {N} P {P} C {C} act {rr.ACT_NAME[act]}"
                _done(A, what, o_d)
                want = (g * s[:, None, :]) * rr.dact(a, act).astype(np.float32)
                assert want.dtype == np.float32
                bad += rr.bits_differ(o_d.float().cpu().numpy(), rr.round_to(want, storage), what)
    util.measured(f"dropout exact channel scale {rr.ST_NAME[storage]} C {C}: elements that differ", bad, bound=0)
