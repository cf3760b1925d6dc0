"""The referee of tests/test_gpu_tail_exact.py checked without a GPU: the float64 references against torch autograd and the model's
own modules, the headroom of every exact case, the case tables, and -- so that the suite is known to be able to fail -- an fp32
CPU evaluation fed to the comparisons as "got": unchanged it must pass both tiers, with each value-only defect it must be rejected
by the exact tier and, on real data, by the float64 bound.
"""
import numpy as np
import pytest
import torch

from tests import tail_ref as tr
from tests import util


# ---------------------------------------------------------------------------------------------------- ICP loss


def _torch_case(case):
    """The generated planes as the arguments of torch_loss_terms: the target image IS the matched planes, nn the identity map."""
    B, _, HW = case["p"].shape
    f = lambda k: torch.from_numpy(case[k])
    nn = torch.where(torch.from_numpy(case["nn"]) >= 0, torch.arange(HW).expand(B, HW), torch.full((B, HW), -1))
    return f("p"), f("n"), f("pt"), f("nt"), nn


@pytest.mark.parametrize("flags", tr.LOSS_FLAG_WORDS)
def test_loss_reference_against_torch_autograd(flags):
    """tail_ref.icp_loss (numpy float64, from the formulas) against float64 autograd of the plainly written loss: every flag word,
    with an empty sample (no valid pixel) and a sample without pairs that lack normals."""
    case = tr.loss_case_real(97, "random", seed=flags)
    case["nn"][0][:] = -1
    v = case["nn"][1] >= 0
    for k in ("n", "nt"):
        case[k][1][0, v & ~tr._has(case[k][1])] = 0.5
    ref = tr.icp_loss(case, flags)
    want = tr.loss_exact64(ref, flags)
    src, src_n, tgt, tgt_n, nn = _torch_case(case)
    T = torch.from_numpy(case["T"]).clone().requires_grad_(True)
    alone, p2p = bool(flags & tr.ALONE), bool(flags & tr.P2P)
    terms, K, K2 = tr.torch_loss_terms(T, src, src_n, tgt, tgt_n, nn, "linear" if flags & tr.LINEAR else "squared", p2p, alone)
    enabled = [p2p, bool(flags & tr.PO2PL) and not alone, bool(flags & tr.PL2PL) and not alone]
    assert ref["pair_counts"][:, 0].tolist() == K and ref["pair_counts"][:, 1].tolist() == K2
    assert K[0] == 0 and K2[0] == 0 and (alone or K2[1] == 0)
    for b in range(3):
        for k in range(3):
            if not (flags & (1 << k)):
                assert ref["loss_terms"][b, k] == 0 and not ref["grad_terms"][b, k].any()
                continue
            if not enabled[k]:
                continue                                          # ALONE with a normal-based term: refused by the entry point
            if not torch.isfinite(terms[b, k]):
                assert np.isnan(ref["loss_terms"][b, k]) and np.isnan(ref["grad_terms"][b, k]).all()
                continue
            g, = torch.autograd.grad(terms[b, k], T, retain_graph=True)
            np.testing.assert_allclose(want["loss_terms"][b, k], float(terms[b, k].detach()), rtol=1e-12)
            np.testing.assert_allclose(want["grad_terms"][b, k], g[b, :3].reshape(-1).numpy(), rtol=1e-9, atol=1e-12 * float(g.abs().max()))
            assert ref["loss_terms"][b, k] == np.float32(want["loss_terms"][b, k])


def test_loss_headroom_of_every_exact_case():
    """Every case the GPU file runs bit for bit is exact: the sums of absolute summands stay below 2^24 for all 38 accumulators.
    This generator reaches about 0.05 of 2^24 at full density and 262 404 pixels."""
    worst = 0.0
    for hw, _ in tr.LOSS_HW:
        case = tr.loss_case_exact(hw)
        words = tr.LOSS_FLAG_WORDS if hw in tr.LOSS_ALL_FLAGS_HW else tr.LOSS_INSTANCES
        worst = max([worst] + [tr.loss_headroom(case, f) for f in words])
    for case in (tr.loss_case_exact(tr.LOSS_B17_HW, B=17, seed=3), tr.loss_case_exact(260, seed=5), tr.loss_case_exact(26000, seed=7)):
        worst = max([worst] + [tr.loss_headroom(case, f) for f in tr.LOSS_FLAG_WORDS])
    full = max(tr.loss_headroom(tr.loss_case_exact(262404, B=1, full=True), f) for f in (7, 15))
    print(f"worst accumulator: {worst:.4f} of 2^24 in the cases, {full:.4f} at full density")
    assert worst < 0.1 and full < 0.1


def test_loss_exact_tier_accepts_fp32_and_rejects_every_mutation():
    for hw in tr.LOSS_ALL_FLAGS_HW:
        case = tr.loss_case_exact(hw)
        for flags in tr.LOSS_FLAG_WORDS:
            tr.loss_headroom(case, flags)
            assert not any(tr.compare_loss_exact(tr.icp_loss_f32(case, flags), tr.icp_loss(case, flags)).values()), (hw, flags)
        for flags in (7, 15):
            ref = tr.icp_loss(case, flags)
            for m in tr.LOSS_MUTATIONS:
                assert any(tr.compare_loss_exact(tr.icp_loss_f32(case, flags, m), ref).values()), f"HW {hw} flags {flags}: {m} not caught"
        ref = tr.icp_loss(case, 7)
        w = np.float32([[0.3, -1.7, 2.1]] * 3)
        good = tr.icp_loss_bwd(ref["grad_terms"], w)
        assert good.shape == (3, 4, 4) and not good[:, 3].any()
        fused = (w[:, 0, None].astype(np.float64) * ref["grad_terms"][:, 0] + w[:, 1, None].astype(np.float64) * ref["grad_terms"][:, 1]
                 + w[:, 2, None].astype(np.float64) * ref["grad_terms"][:, 2]).astype(np.float32)
        assert tr.same_bits(good[:, :3].reshape(3, 12), fused) > 0, "the weights do not tell a fused backward from an unfused one"


@pytest.mark.parametrize("kind,scale", [("random", 1.0), ("converged", 1.0), ("random", 1e-2), ("converged", 1e2)])
def test_loss_float64_tier_accepts_fp32_and_rejects_every_mutation(kind, scale):
    case = tr.loss_case_real(1028, kind, scale=scale, seed=11)
    for flags in (7, 15):
        ref = tr.icp_loss(case, flags, majorant=True)
        ok = tr.compare_loss_real(tr.icp_loss_f32(case, flags), ref, flags, 1028)
        assert max(ok.values()) <= 1.0, (flags, ok)
        off = tr.icp_loss(case, flags & ~tr.P2P, majorant=True)              # a disabled term must be exactly 0 in this tier too
        got = tr.icp_loss_f32(case, flags & ~tr.P2P)
        got["grad_terms"][1, 0, 5] = 1e-30
        assert tr.compare_loss_real(got, off, flags & ~tr.P2P, 1028)["grad_terms"] == float("inf")
        for m in tr.LOSS_MUTATIONS:
            r = tr.compare_loss_real(tr.icp_loss_f32(case, flags, m), ref, flags, 1028)
            assert max(r.values()) > 1.0, f"{kind} scale {scale} flags {flags}: {m} stays inside the bound ({r})"


def test_loss_constants():
    assert tr.LOSS_C_TERM == max(tr.loss_c_term(0).max(), tr.loss_c_term(tr.LINEAR).max()) == 16
    assert [tr.loss_c_sum(hw) for hw in (1, 1024, 131072, 131076, 262404)] == [22, 22, 22, 24, 26]


# ---------------------------------------------------------------------------------------------------- case tables


def test_case_tables_are_what_the_gpu_file_runs_and_cover_what_they_claim():
    from tests import test_gpu_tail_exact as g

    def params(fn):
        return [m.args[1] for m in fn.pytestmark if m.name == "parametrize"][0]
    assert params(g.test_loss_exact) == [1, 3, 4, 252, 255, 256, 257, 260, 1021, 1024, 1028, 25600, 26000, 131072, 131076, 131333, 262404]
    assert params(g.test_heads_exact) == params(g.test_heads_float64) == tr.HEADS_SHAPES
    assert params(g.test_quat_to_T_float64) == [1, 64, 65, 130]
    assert tr.LOSS_FLAG_WORDS == list(range(16)) + [17, 16] and sorted(tr.LOSS_INSTANCES) == [6, 7, 14, 15]
    assert tr.MEAN_P == [1, 63, 64, 65, 127, 128, 129, 4096] and tr.MEAN_C == {"f32": [4, 20, 512], "half": [8, 24, 512]} and tr.MEAN_N == [1, 3]
    # the loss sizes: rows of the reduction against its 25 slices, the workgroup cap, the wave loop
    chunks = lambda hw: -(-hw // 256)
    assert [tr.loss_blocks(hw) for hw in (1024, 1028, 25600, 26000, 131072, 131076)] == [1, 2, 25, 26, 128, 128]
    assert chunks(131072) == 512 and chunks(131076) == 513 and 131076 % 4 == 0 and 131333 % 4 and chunks(262404) > 2 * 512 and 262404 % 256
    assert 260 % 4 == 0 and chunks(260) == 2 and 1028 % 4 == 0 and chunks(1028) == 5
    # the heads: K-chunked staging with a ragged last chunk, R across 40 and 64, idle and surplus waves, both ends of B
    assert tr.heads_kc(16, 768) == 768 and tr.heads_kc(16, 1000) == 768 and 1000 % 768 and tr.heads_kc(5, 2500) == 2432 and 2500 % 2432
    shapes = tr.HEADS_SHAPES
    assert {s[0] for s in shapes} >= {1, 16} and {s[2] for s in shapes} >= {40, 41, 64, 130}
    assert any((2 * s[3]) % 8 for s in shapes) and any(s[2] % 4 for s in shapes) and any((2 * s[3]) % 4 for s in shapes)
    assert all(n % 8 == 0 for n in tr.ELEMENTWISE_N) and min(tr.ELEMENTWISE_N) == 8 and any(n // 8 > 256 for n in tr.ELEMENTWISE_N)


# ---------------------------------------------------------------------------------------------------- pose heads


@pytest.mark.parametrize("act_name,act", [("relu", 2), ("tanh", 1)])
def test_heads_reference_against_the_models_own_modules(act_name, act):
    """tail_ref.heads (with and without the dropout mask) against OdometryModel's resnet.fc + _heads in float64, outputs and all
    eleven gradients; the explicit backward from saved tensors against autograd."""
    from delora_amd.models.model import OdometryModel
    torch.manual_seed(3)
    m = OdometryModel(util.repo_config(16, 128, activation_fct=act_name)).double()
    fr, ft, fc = m.fully_connected_rotation, m.fully_connected_translation, m.resnet.fc
    P = {"fc_w": fc.weight, "fc_b": fc.bias, "r1_w": fr[1].weight, "r1_b": fr[1].bias, "r3_w": fr[3].weight, "r3_b": fr[3].bias,
         "t1_w": ft[1].weight, "t1_b": ft[1].bias, "t3_w": ft[3].weight, "t3_b": ft[3].bias}
    B, F, R, Hd = 8, fc.in_features, fc.out_features, fr[1].out_features
    assert (B, F, R, Hd) == tr.HEADS_MODEL_SHAPE
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, F, generator=g, dtype=torch.float64)
    g_t, g_r = torch.randn(B, 3, generator=g, dtype=torch.float64), torch.randn(B, 4, generator=g, dtype=torch.float64)
    scale = torch.where(torch.rand(B, R, generator=g) < 0.2, 0.0, 1.25).double()
    for sc in (None, scale):
        ref = tr.heads(x, {k: v.detach() for k, v in P.items()}, act, sc, g_t, g_r)
        xr = x.clone().requires_grad_(True)
        m.zero_grad()
        feat = fc(xr)
        translation, rotation = m._heads(feat if sc is None else feat * sc)
        ((translation * g_t).sum() + (rotation * g_r).sum()).backward()
        torch.testing.assert_close(ref["translation"], translation.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(ref["rotation"], rotation.detach(), rtol=1e-12, atol=1e-14)
        torch.testing.assert_close(ref["grad_x"], xr.grad, rtol=1e-10, atol=1e-14)
        explicit = tr.heads_bwd(x, {k: v.detach() for k, v in P.items()}, act, sc, ref, g_t, g_r)
        for k, v in P.items():
            torch.testing.assert_close(ref["d_" + k], v.grad, rtol=1e-10, atol=1e-14)
        for k, v in explicit.items():
            torch.testing.assert_close(v, ref[k], rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("shape", tr.HEADS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_heads_tiers_accept_fp32_and_reject_every_mutation(shape):
    B = shape[0]
    zero = torch.zeros(B, 4, dtype=torch.float64)
    x, P, scale, g_t = tr.heads_case_exact(*shape)
    for act in (0, 2):
        for sc in (None, scale):
            assert tr.heads_headroom(x, P, sc, g_t, act) < 1.0
            ref = tr.heads(x, P, act, sc, g_t, zero)
            exp = tr.heads_exact_expect(ref)
            for mut in (None,) + tr.HEADS_MUTATIONS:
                got = tr.heads_f32(x, P, act, sc, g_t, zero, tr.heads_saved(ref), mut)
                bad = sum(int((~((got[k] == exp[k]) | (torch.isnan(got[k]) & torch.isnan(exp[k])))).sum()) for k in tr.HEADS_FWD_OUT + tr.HEADS_BWD_OUT)
                for k in ("d_r1_w", "d_r1_b", "d_r3_w", "d_r3_b"):
                    assert not got[k].any()
                if mut is None:
                    assert bad == 0, (shape, act, bad)
                elif not (mut == "norm_per_sample" and B == 1):         # one sample: the two norms are the same number
                    assert bad > 0, f"{shape} act {act}: {mut} not caught by the exact tier"
    x, P, scale, g_t, g_r = tr.heads_case_real(*shape)
    for act in (0, 1, 2):
        for sc in (None, scale):
            ref, bnd = tr.heads_bounds(x, P, act, sc, g_t, g_r)
            for mut in (None,) + tr.HEADS_MUTATIONS:
                got = tr.heads_f32(x, P, act, sc, g_t, g_r, tr.heads_saved(ref), mut)
                worst = max(tr.worst_ratio(got[k].numpy(), ref[k].numpy(), bnd[k].numpy()) for k in bnd)
                if mut is None:
                    assert worst <= 1.0, (shape, act, worst)
                elif not (mut == "norm_per_sample" and B == 1):
                    assert worst > 1.0, f"{shape} act {act}: {mut} stays inside the float64 bound"


# ---------------------------------------------------------------------------------------------------- pooling, cast, quaternion


@pytest.mark.parametrize("dtype,lanes", [(torch.float32, 64), (torch.float16, 128), (torch.bfloat16, 128)])
def test_pooling_tiers_accept_fp32_and_reject_every_mutation(dtype, lanes):
    for P in tr.MEAN_P:
        x = tr.mean_case(3, P, 24, dtype, seed=P)
        assert tr.pool_headroom(x) < 1.0
        assert torch.equal(tr.mean_f32(x), tr.mean_exact(x))
        np.testing.assert_allclose(tr.mean_exact(x).double().numpy(), x.mean(dim=1).numpy(), rtol=3e-7, atol=1e-30)
        xr = tr.mean_case(3, P, 24, dtype, seed=P, exact=False)
        ref, bnd = tr.mean_bound(xr, lanes)
        ok = tr.worst_ratio(tr.mean_f32(xr).numpy(), ref.numpy(), bnd.numpy())
        assert ok <= 1.0, (P, ok)
        for mut in ("drop_pixel", "skip_chunk"):
            if P > 1:
                assert not torch.equal(tr.mean_f32(x, mut), tr.mean_exact(x)), (P, mut)
                assert tr.worst_ratio(tr.mean_f32(xr, mut).numpy(), ref.numpy(), bnd.numpy()) > 1.0, (P, mut)


@pytest.mark.parametrize("code", [1, 2])
def test_elementwise_emulations_against_float64(code):
    """The fp32 emulation of dl_mean_hw_bwd_act_h and torch's conversion, the referees of the bit-exact elementwise tests, are
    themselves within half an ulp of the half type (plus the few fp32 roundings of the emulation) of float64."""
    dtype = tr.HALF[code]
    fi = torch.finfo(dtype)
    src = tr.special_values(dtype, 2048, seed=1)
    c = tr.cast_ref(src, dtype)
    fin = torch.isfinite(src) & (src.abs() >= fi.smallest_normal) & (src.abs() <= fi.max)
    assert bool(((c.double() - src.double()).abs()[fin] <= fi.eps / 2 * src.double().abs()[fin]).all())
    assert bool(torch.isnan(c[torch.isnan(src)]).all()) and float(tr.cast_ref(torch.tensor([fi.max * (1 + fi.eps / 2)]), dtype)) == float("inf")
    assert float(tr.cast_ref(torch.tensor([1.0 + fi.eps / 2]), dtype)) == 1.0 and float(tr.cast_ref(torch.tensor([1.0 + 3 * fi.eps / 2]), dtype)) == 1.0 + 2 * fi.eps
    N, P, C = 2, 128, 8
    x = tr.special_values(dtype, N * P * C, seed=2).to(dtype).view(N, P, C)
    gy = torch.randn(N, C, generator=torch.Generator().manual_seed(4))
    for act in (0, 1, 2):
        emu, want = tr.mean_bwd_act(gy, x, P, act, dtype).double(), tr.mean_bwd_act64(gy, x, P, act)
        ok = torch.isfinite(want) & (want.abs() >= fi.smallest_normal) & (want.abs() <= fi.max)
        assert int(ok.sum()) > 100
        assert bool(((emu - want).abs()[ok] <= (fi.eps / 2 + 8 * tr.U) * want.abs()[ok]).all()), act
        assert torch.equal(torch.isnan(emu), torch.isnan(want)) or act == 2          # relu: NaN activations count as "on" in the kernel


def test_quaternion_reference():
    """Unit quaternions give rotations; the reference agrees with the model's torch formulation; at |q| == eps exactly the gradient
    flows through the norm (clamp_min's rule), below it the quaternion is divided by eps."""
    from delora_amd.models.model_parts import GeometryHandler
    eps = np.float32(1e-12)
    q, t, G = tr.quat_case(130, 1e-12, seed=1)
    T, gt, gq = tr.quat_to_T(q, t, eps, G)
    R = T[:, :3, :3]
    big = q.double().norm(dim=1) >= float(eps)
    assert float((R[big] @ R[big].transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-12
    assert torch.equal(gt, G[:, :3, 3].double())
    T32 = GeometryHandler.get_transformation_matrix_quaternion(t, q, torch.device("cpu"))
    assert float((T32.double() - T).abs().max()) < 1e-5
    assert float(q[10].double().norm()) == float(eps) and float((gq[10] * q[10].double()).sum().abs()) < 1e-9 * float(gq[10].abs().max())
    tiny = q.double().norm(dim=1) < float(eps)
    assert int(tiny.sum()) > 10 and int(big.sum()) > 10
