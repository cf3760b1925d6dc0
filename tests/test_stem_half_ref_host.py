"""Host tier of the half-precision stem's referee (tests/stem_half_ref.py): the reference functions against float64 on hand-made
cases, the properties every generated case of tests/test_gpu_stem_half_exact.py must have (headroom, outputs beyond the
exact-integer range, exact ties, half storage that loses nothing), the literal launch-plan tables, the ABI surface, and the model's
predicate for the half stem.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import stem_half_ref as hr
from tests import stem_ref as sr
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = pytest.mark.parametrize("dtype", hr.DTYPES, ids=[hr.NAME[d] for d in hr.DTYPES])
NEW = ("dl_stem_input_nhwc_h", "dl_stem_conv1_h", "dl_stem_pool_fwd_h", "dl_stem_wgrad_h_workspace_bytes", "dl_stem_wgrad_h")


# ---------------------------------------------------------------------------------------------------- the rounding


def test_rounding_on_hand_made_values():
    """Ties go to the even neighbour, both ways; the neighbours of a tie go to the nearer number; overflow starts at max + half an ulp."""
    bf, fp = torch.bfloat16, torch.float16
    for dtype, cases in ((bf, [(1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (257.0, 256.0), (259.0, 260.0), (-257.0, -256.0), (60.1, 60.0),
                               (60.2, 60.25), (3.0, 3.0)]),
                         (fp, [(2049.0, 2048.0), (2051.0, 2052.0), (4098.0, 4096.0), (4102.0, 4104.0), (65519.0, 65504.0), (65520.0, np.inf),
                               (-65520.0, -np.inf), (60.01, 60.0), (60.02, 60.03125), (2.0 ** -25, 0.0), (3 * 2.0 ** -25, 2.0 ** -23)])):
        v = np.array([c[0] for c in cases], dtype=np.float32).astype(np.float64)
        want = np.array([c[1] for c in cases])
        assert np.array_equal(hr.h_f64(v, dtype), want), (hr.NAME[dtype], hr.h_f64(v, dtype), want)
        assert np.array_equal(hr.h(v, dtype), want), (hr.NAME[dtype], hr.h(v, dtype), want)


@DT
def test_torch_conversion_equals_the_float64_definition(dtype):
    r = cr._rng(5)
    v = np.concatenate([(r.standard_normal(20000) * 10.0 ** r.integers(-9, 6, 20000)).astype(np.float32), hr.planted(dtype),
                        np.arange(-5000, 5000).astype(np.float32)]).astype(np.float64)
    assert np.array_equal(hr.h(v, dtype), hr.h_f64(v, dtype))
    assert hr.representable(hr.h(v, dtype)[np.isfinite(hr.h(v, dtype))], dtype)


@DT
def test_a_range_of_60_metres_is_stored_to_a_quarter_metre_in_bf16(dtype):
    """The remark of the documents: the spacing of the type at 60 (a range in metres)."""
    v = np.array([60.0], dtype=np.float64)
    up = hr.h(np.nextafter(np.float32(60.0 + (0.25 if dtype == torch.bfloat16 else 0.03125) * 0.51), np.float32(100)).astype(np.float64).reshape(1), dtype)
    assert up[0] - v[0] == (0.25 if dtype == torch.bfloat16 else 0.03125)


# ---------------------------------------------------------------------------------------------------- generated cases


@DT
def test_input_cases_hold_ties_and_overflow(dtype):
    for case in hr.INPUT_CASES:
        x = hr.input_case(*case, dtype)
        ties, over = hr.input_case_properties(x, dtype)
        assert ties >= 3 and over >= 2, (case, ties, over)
        ref = hr.input_ref(x, dtype)
        assert ref.shape == (case[0], case[1], case[2], 8)
        assert np.array_equal(ref[0, 0, 1], hr.h_f64(x[0, :, 0, 1].astype(np.float64), dtype), equal_nan=True)


def test_conv1_reference_against_plain_loops():
    x8, w = cr.ints((1, 3, 8, 8), 3, 1).numpy(), cr.ints((64, 3, 3, 8), 2, 2).numpy()
    assert np.array_equal(hr.conv1_ref64(x8, w, sr.NONE), cr.conv_loops(x8, w, (1, 2)))
    assert np.array_equal(hr.conv1_ref64(x8, w, sr.RELU), np.maximum(cr.conv_loops(x8, w, (1, 2)), 0))
    x4 = cr.ints((1, 2, 4, 8), 3, 3).numpy()                     # W = 4: the map wraps onto itself
    assert np.array_equal(hr.conv1_ref64(x4, w, sr.NONE), cr.conv_loops(x4, w, (1, 2)))


@DT
@pytest.mark.parametrize("case", [c for c in hr.CONV1_CASES if c[1] * c[2] < 10000], ids=lambda c: "x".join(map(str, c)))
def test_conv1_integer_cases_round_and_tie(case, dtype):
    """conv1_int_case asserts the headroom, outputs beyond the exact-integer range and exact ties; here also: the expected map is the
    float64 definition of the rounding, and it differs from the exact sums (the case exercises the rounding)."""
    for act in (sr.NONE, sr.RELU):
        c = hr.conv1_int_case(*case, dtype, act)
        assert np.array_equal(c["want"], hr.h_f64(c["exact"], dtype))
        assert c["props"]["ties"] > 0 and c["props"]["rounded"] > 0
        t = hr._is_tie(c["exact"], dtype)
        # ties to even: the rounded value of every tie is an even multiple of the spacing
        q = c["want"][t]
        _, e = np.frexp(c["exact"][t])
        spacing = np.exp2((e - hr.BITS[dtype]).astype(np.float64))
        assert np.all(np.isinf(q) | ((q / spacing) % 2 == 0))


@DT
def test_conv1_distinct_case(dtype):
    for act in (sr.NONE, sr.RELU):
        c = hr.conv1_distinct_case(dtype, act)                    # (asserts 4608 different weights, one pixel per window, every tap reached)
        assert hr.representable(c["want"], dtype) and np.count_nonzero(c["want"]) > 1000


def test_conv1_plan_table_and_coverage():
    for case, want in hr.CONV1_PLAN.items():
        assert hr.conv1_plan(*case) == want, (case, hr.conv1_plan(*case))
    assert not hr.conv1_coverage(), hr.conv1_coverage()
    assert hr.conv1_coverage(((1, 3, 128),)), "the coverage list can fail"
    for need in ((1, 1, 4), (1, 2, 4), (2, 3, 8), (1, 5, 12), (1, 3, 128), (1, 3, 132), (2, 5, 72), (3, 2, 260)):
        assert need in hr.CONV1_CASES


def test_pool_cases():
    assert all(c[3] % 8 == 0 for c in hr.POOL_CASES) and (1, 1, 2, 8) in hr.POOL_CASES and (1, 19, 54, 8) in hr.POOL_CASES
    assert {c for c in sr.POOL_CASES if c[3] % 8 == 0} <= set(hr.POOL_CASES)
    assert hr.pool_threads((1, 19, 54, 8)) == 513 and min(hr.pool_threads(c) for c in hr.POOL_CASES) == 1
    for dtype in hr.DTYPES:
        for case in hr.POOL_CASES:
            for act in sr.ACTS:
                for special in (False, True):
                    a, _, _ = sr.pool_case_data(case, act, special)
                    assert hr.representable(a, dtype), (case, act, special)
                    y, _ = sr.pool_fwd_ref(a)
                    assert hr.representable(y, dtype)


@DT
def test_wgrad_cases_lose_nothing_in_half_storage(dtype):
    """All 17 x 3 integer cases: g, a, x8 and gc are numbers of the type (wgrad_case asserts it), the fp32 emulation of the gather
    equals the float64 scatter, and so gc_half is that map itself."""
    for case in hr.WGRAD_CASES:
        if case[0] * case[1] * case[2] > 60000:
            continue                                            # (the largest maps: generated and asserted in the GPU tier)
        for act in sr.ACTS:
            c = hr.wgrad_case(*case, act, dtype)
            gc = sr.pool_bwd_ref(c["g"], c["a"], c["win"], act)
            assert np.array_equal(hr.gc_half(c["g"], c["a"], c["win"], act, dtype), gc)
    assert not hr.coverage()
    for case, (chunks, cps, grid) in hr.WGRAD_PLAN.items():
        p = hr.plan(*case)
        assert (p[0], p[2], p[3]) == (chunks, cps, grid)
        assert hr.workspace_bytes(*case) == p[1] * 64 * 72 * 4
    assert hr.workspace_bytes(1, 2, 6) == 0 and hr.workspace_bytes(0, 2, 8) == 0 and hr.workspace_bytes(1, 1 << 13, 1 << 13) == 0
    assert hr.SKEW_CASE in hr.WGRAD_CASES


@DT
def test_weight_gradient_bound_on_a_float32_emulation(dtype):
    """The bound of the real-valued tier holds for an fp32 emulation that adds the products one by one in pixel order (more rounded
    additions per chain than the kernel's), and fails for a reference that does not round gc: the tier can tell the two apart."""
    N, H, W = 2, 4, 16
    for act in sr.ACTS:
        x8, g, w = hr.real_case(N, H, W, dtype, 5)
        a = hr.h(hr.conv1_ref64(x8, w, act).astype(np.float32).astype(np.float64), dtype)
        win = sr.pool_fwd_ref(a)[1]
        gc = hr.gc_half(g, a, win, act, dtype)
        ref, bound = hr.wgrad_ref_and_bound(gc, x8, N, H, W)
        X = sr._patches(x8, N, H, W).reshape(-1, 72)
        G = gc.reshape(-1, 64).astype(np.float32)
        acc = np.zeros((64, 72), dtype=np.float32)
        for p in range(X.shape[0]):
            acc = (acc.astype(np.float64) + G[p][:, None].astype(np.float64) * X[p][None, :].astype(np.float64)).astype(np.float32)
        emul = acc.reshape(64, 9, 8).transpose(0, 2, 1).reshape(64, 8, 3, 3).astype(np.float64)
        assert hr.wgrad_op_count(N, H, W) >= 16 + 3 + 1 + 3
        # N H W/2 = 64 additions per chain in the emulation, against c = wgrad_op_count: scale the bound to the emulation's count
        assert float((np.abs(emul - ref) / (bound * (N * H * (W // 2)) / hr.wgrad_op_count(N, H, W))).max()) <= 1.0
        unrounded = hr.wgrad_ref_and_bound(sr.pool_bwd_ref(g, a, win, act), x8, N, H, W)[0]
        assert float((np.abs(unrounded - ref) / bound).max()) > 1.0, "a reference with an unrounded gc must be told apart"


# ---------------------------------------------------------------------------------------------------- ABI surface


def test_header_exports_and_signatures_hold_the_new_names():
    from delora_amd import _lib
    header = open(os.path.join(ROOT, "include", "delora_hip.h")).read()
    assert re.search(r"#define\s+DL_ABI_VERSION\s+10\b", header)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    assert int(lib.dl_abi_version()) == 10
    for name in NEW:
        assert hasattr(lib, name), name
    for case in hr.WGRAD_CASES:
        assert int(lib.dl_stem_wgrad_h_workspace_bytes(*case)) == hr.workspace_bytes(*case) > 0
    for bad in ((1, 2, 6), (0, 2, 8), (1, -1, 8), (1, 1 << 13, 1 << 13)):
        assert int(lib.dl_stem_wgrad_h_workspace_bytes(*bad)) == hr.workspace_bytes(*bad) == 0
    # refusals need no device: they come before any launch
    rc = lib.dl_stem_conv1_h(None, None, 1, 1, 4, 0, 2, None, None)
    assert rc == -1 and b"dl_stem_conv1_h" in lib.dl_last_error() and b"x8h" in lib.dl_last_error()


# ---------------------------------------------------------------------------------------------------- the predicate


def _model(**over):
    from delora_amd.models.model import OdometryModel
    cfg = util.repo_config(16, 128, device="cpu", **over)
    torch.manual_seed(1)
    return OdometryModel(cfg)


def test_config_key_reaches_the_network_and_defaults_to_off():
    assert _model().resnet.amp_stem is False
    assert _model(amp_stem=True).resnet.amp_stem is True
    assert _model(amp_stem=False).resnet.amp_stem is False


def test_predicate_says_no_off_the_half_stem_path(monkeypatch):
    """Without a GPU ``hip_half_applicable`` is stubbed to say bf16, so that every OTHER clause of the predicate is what decides."""
    from delora_amd.models import resnet_modified as rm
    x = torch.zeros((2, 8, 16, 128))
    real = rm.ResNetModified.hip_half_applicable
    # a CPU tensor, for real: the trunk's own predicate says no
    m = _model(amp_stem=True)
    assert m.resnet.hip_half_stem_applicable(x) is None
    monkeypatch.setattr(rm.ResNetModified, "hip_half_applicable", lambda self, t: torch.bfloat16)
    assert m.resnet.hip_half_stem_applicable(x) == torch.bfloat16            # the stub alone: every other clause holds
    assert _model().resnet.hip_half_stem_applicable(x) is None               # no key
    md = _model(amp_stem=True, use_dropout=True)
    md.train()
    assert md.resnet.hip_half_stem_applicable(x) is None                     # active dropout
    md.eval()
    assert md.resnet.hip_half_stem_applicable(x) == torch.bfloat16           # ... inactive in eval
    assert m.resnet.hip_half_stem_applicable(x.clone().requires_grad_(True)) is None
    mt = _model(amp_stem=True, pre_feature_extraction=True)
    assert mt.resnet.hip_half_stem_applicable(torch.zeros((2, 80, 16, 128))) is None      # behind the tower: the wide stem
    mn = _model(amp_stem=True, factor_fewer_resnet_channels=2)
    assert mn.resnet.hip_half_stem_applicable(x) is None                     # a narrow network
    assert m.resnet.hip_half_stem_applicable(torch.zeros((2, 8, 16, 130))) is None        # a width that does not halve twice
    monkeypatch.setattr(rm.ResNetModified, "hip_half_applicable", real)
    mm = _model(amp_stem=True, cnn_impl="modules")
    assert mm.resnet.hip_half_applicable(x) is None and mm.resnet.hip_half_stem_applicable(x) is None
