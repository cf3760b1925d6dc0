"""``dl_icp_information`` (csrc/info.hip) against tests/information_ref.py: BIT FOR BIT on small-integer data (the headroom of every
case is asserted in tests/test_information_host.py), against the existing loss kernel on the same operands, within a derived
rounding bound on real data through the real chain (projection -> normals -> search -> information), and the covariance / status
stage on planted scenes.  Every device buffer of the exact tests lives in a tests/conv_ref.Arenas allocation (guard zones, poisoned
outputs and a workspace of exactly the promised size, inputs that must stay unchanged); the C ABI is called directly.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import information_ref as ir
from tests import util

pytestmark = pytest.mark.gpu

# (B, H, W, largest |coordinate|): a ragged single chunk; exactly one chunk of 256 pixels; a ragged second chunk; three samples of
# eight full chunks (two workgroups each); more chunks than the grid cap's 512 waves per sample, so that waves walk twice; and an
# image whose pixel count is no multiple of 4 (scalar loads, planes skewed by 4 bytes)
EXACT_SHAPES = [(1, 3, 20, 8), (1, 4, 64, 8), (1, 5, 36, 8), (3, 16, 128, 8), (1, 66, 2048, 2), (2, 3, 21, 8)]


def exact_case(B, H, W, coord):
    return ir.integer_case(B, H * W, seed=H * W + B, coord=coord)


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


POISON64 = 0x7FF8DEAD7FF8DEAD                          # the word the fp64 outputs hold before a call: a quiet NaN no sum produces


class InfoRun:
    """One case on the device.  The source is channels 0-2 of a [B,4,HW] image (channel 3 holds NaN: it is not an operand), normals
    and match are views into wider buffers (NaN between the samples); where HW % 4 != 0 the sample strides are no multiples of 4 and
    every plane pointer is skewed by 4 bytes, which the entry point allows.  The fp64 outputs are int64 arenas (viewed as float64),
    poisoned with a NaN word before every call."""

    OUT = (("info", 36), ("rhs", 6), ("stats", 2), ("covariance", 36))

    def __init__(self, case, dev):
        self.L, self.lib = _lib()
        B, _, HW = case["p"].shape
        self.B, self.HW, self.vec = B, HW, HW % 4 == 0
        self.A, self.W = cr.Arenas(dev, 0 if self.vec else 4), cr.Arenas(dev, 0)
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
        inp = lambda t, dtype, name: self.A.arena(tuple(t.shape), dtype, t, name, row_elems=0)
        self.src, self.srcn, self.match = inp(src, torch.float32, "src"), inp(srcn, torch.float32, "src normals"), inp(match, torch.float32, "match")
        self.nn = inp(torch.from_numpy(case["nn"]), torch.int32, "nn_pix")
        self.T = inp(torch.from_numpy(case["T"]).reshape(B, 16), torch.float32, "T")
        self.out = {name: self.W.arena((B, n), torch.int64, None, name, row_elems=0) for name, n in self.OUT}
        self.status = self.W.arena((B,), torch.int32, None, "status", row_elems=0)
        nbytes = int(self.lib.dl_icp_information_workspace_bytes(B, 1, HW))
        assert nbytes == B * min(-(-(-(-HW // 256)) // 4), 128) * 32 * 4
        self.wsp = self.W.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)

    def args(self, first=0, B=None):
        s = self
        return (_p(s.src, first * s.ss[0]), s.ss[0], _p(s.srcn, first * s.ss[1]), s.ss[1], _p(s.match, first * s.ss[2]), s.ss[2],
                _p(s.nn, first * s.HW), _p(s.T, first * 16), s.B if B is None else B, 1, s.HW)

    def poison(self):
        for v in self.out.values():
            v.fill_(POISON64)
        self.status.fill_(cr._as_i32(cr.NAN_WORD[torch.int32]))

    def launch(self, first=0, B=None):
        s = self
        s.L.check(s.lib.dl_icp_information(*s.args(first, B), *(_p(s.out[name]) for name, _ in s.OUT), _p(s.status), _p(s.wsp), _stream()),
                  "dl_icp_information")

    def read(self, n=None):
        n = self.B if n is None else n
        got = {name: self.out[name][:n].view(torch.float64).cpu().numpy().copy() for name, _ in self.OUT}
        got["info"], got["covariance"] = got["info"].reshape(n, 6, 6), got["covariance"].reshape(n, 6, 6)
        got["status"] = self.status[:n].cpu().numpy().copy()
        return got

    def run(self, first=0, B=None):
        s = self
        s.poison()
        s.launch(first, B)
        _sync()
        n = s.B if B is None else B
        what = f"information HW={s.HW} B={n}"
        s.A.check(what)                                              # guards and inputs
        s.W.check(what)                                              # guards of outputs and workspace
        for name, _ in s.OUT:
            left = int((s.out[name][:n] == POISON64).sum())
            assert left == 0, f"{what}: {left} elements of {name} were never written"
            if n < s.B:
                assert bool((s.out[name][n:] == POISON64).all()), f"{what}: {name} written behind sample {n}"
        assert int((s.status[:n] == cr._as_i32(cr.NAN_WORD[torch.int32])).sum()) == 0, f"{what}: status was never written"
        return s.read(n)


def _bits_equal(got, ref, keys=("info", "rhs", "stats")):
    for k in keys:
        # (+ 0.0: a numpy sum of -0.0 terms may be -0.0; the kernel's accumulators start at +0.0 and an empty sum must BE +0.0)
        assert got[k].tobytes() == (np.ascontiguousarray(ref[k], dtype=np.float64) + 0.0).tobytes(), (k, got[k], ref[k])


def _check_finish(got, ref):
    """Status and covariance of every sample against the float64 reference evaluated on sums that are the same bits."""
    assert got["status"].tolist() == ref["status"].tolist()
    for b, st in enumerate(ref["status"]):
        cov, A = got["covariance"][b], ref["info"][b]
        if st != ir.OK:
            assert cov.tobytes() == np.zeros((6, 6)).tobytes(), f"sample {b}: status {st} with a covariance that is not +0.0"
            continue
        assert np.array_equal(cov, cov.T)
        cond = np.linalg.cond(ir.scaled(A))
        sigma2 = ref["stats"][b, 0] / (ref["stats"][b, 1] - 6)
        # backward-stable 6x6 Cholesky: ~6 * 2^-53 * cond; the bound scales with the condition number where it exceeds 1e4
        err = np.abs(cov @ A / sigma2 - np.eye(6)).max() if sigma2 > 0 else 0.0
        assert err <= 1e-9 * max(1.0, cond / 1e4), (b, err, cond)


def _ref(case):
    return ir.information(case["p"], case["n"], case["pt"], case["nt"], case["nn"], case["T"])


# ---------------------------------------------------------------------------------------------------- integer data


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=lambda s: "B{}_{}x{}".format(*s[:3]))
def test_information_exact(shape):
    B, H, W, coord = shape
    case = exact_case(B, H, W, coord)
    assert ir.headroom(case) < 0.5
    run = InfoRun(case, _dev())
    got, ref = run.run(), _ref(case)
    _bits_equal(got, ref)
    _check_finish(got, ref)
    assert (ref["stats"][:, 1] > 6).all()
    again = run.run()                                                # deterministic from run to run, every output
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_empty_and_non_finite_samples_stay_in_their_sample():
    """16 x 128, B = 3: sample 0 has no match at all, sample 1 a NaN pose, sample 2 is ordinary.  Samples 0 and 2 are the same bits as
    in a run where sample 1 has a finite pose; the sums of sample 1 are NaN, its status is 2 and its covariance +0.0."""
    B, H, W, coord = EXACT_SHAPES[3]
    clean = exact_case(B, H, W, coord)
    clean["nn"][0][:] = -1
    case = {k: v.copy() for k, v in clean.items()}
    case["T"][1, 0, 1] = np.nan
    dev = _dev()
    want, got = InfoRun(clean, dev).run(), InfoRun(case, dev).run()
    _bits_equal(want, _ref(clean))
    for k in want:
        for b in (0, 2):
            assert got[k][b].tobytes() == want[k][b].tobytes(), (k, b)
    assert got["stats"][0].tolist() == [0.0, 0.0] and got["status"][0] == ir.TOO_FEW_PAIRS and not got["info"][0].any() and not got["covariance"][0].any()
    assert np.isnan(got["info"][1]).any() and got["stats"][1, 1] == want["stats"][1, 1]
    assert got["status"][1] == ir.UNOBSERVABLE and got["covariance"][1].tobytes() == np.zeros((6, 6)).tobytes()
    assert got["status"][2] == ir.OK
    # a sub-batch call writes its own samples and nothing behind them
    run = InfoRun(clean, dev)
    part = run.run(first=1, B=2)
    for k in want:
        assert part[k].tobytes() == want[k][1:].tobytes(), k


def test_non_counting_pixels_contribute_exact_zeros():
    """Finite garbage at every operand of the three classes of non-counting pixel changes no output bit."""
    B, H, W, coord = EXACT_SHAPES[2]
    case = exact_case(B, H, W, coord)
    dirty = {k: v.copy() for k, v in case.items()}
    rng = np.random.default_rng(5)
    for b in range(B):
        off = dirty["nn"][b] < 0
        no_s, no_t = ~(case["n"][b] != 0).any(axis=0), ~(case["nt"][b] != 0).any(axis=0)
        assert off.any() and (no_s & ~off).any() and (no_t & ~off & ~no_s).any()
        for k in ("p", "n", "pt", "nt"):
            dirty[k][b][:, off] = rng.uniform(-1e6, 1e6, (3, int(off.sum()))).astype(np.float32)
        for k in ("p", "pt", "nt"):
            dirty[k][b][:, no_s & ~off] = rng.uniform(-1e6, 1e6, (3, int((no_s & ~off).sum()))).astype(np.float32)
        only_t = no_t & ~off & ~no_s                                 # (a pixel without either normal took garbage as its matched normal above)
        for k in ("p", "pt", "n"):
            dirty[k][b][:, only_t] = rng.uniform(-1e6, 1e6, (3, int(only_t.sum()))).astype(np.float32)
    dirty["p"][:, :, 0], dirty["pt"][:, :, 0] = case["p"][:, :, 0], case["pt"][:, :, 0]       # (pixel 0 is re-read by a ragged chunk: finite)
    dev = _dev()
    want, got = InfoRun(case, dev).run(), InfoRun(dirty, dev).run()
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------- against the loss kernel


def test_cross_check_against_the_loss_kernel():
    """The same operands through dl_icp_loss_fwd (point-to-plane): K, the mean squared residual and, from its gradient moments, rhs.
    The pair count of every sample is trimmed to a power of two, so that the loss kernel's fp32 moments 2 S / K are exact and rhs
    follows from them without a rounding."""
    L, lib = _lib()
    B, H, W, coord = EXACT_SHAPES[3]
    case = exact_case(B, H, W, coord)
    w = ir.weights(case["n"], case["nt"], case["nn"])
    for b in range(B):
        idx = np.nonzero(w[b])[0]
        keep = 1 << (len(idx).bit_length() - 1)
        case["nn"][b, idx[keep:]] = -1
    run = InfoRun(case, _dev())
    got = run.run()
    _bits_equal(got, _ref(case))
    dev = _dev()
    lt = torch.empty((B, 3), dtype=torch.float32, device=dev)
    pc = torch.empty((B, 2), dtype=torch.int32, device=dev)
    gt = torch.empty((B, 36), dtype=torch.float32, device=dev)
    ws = torch.empty((lib.dl_icp_loss_workspace_bytes(B, 1, run.HW) // 4,), dtype=torch.float32, device=dev)
    L.check(lib.dl_icp_loss_fwd(*run.args(), 2, _p(lt), _p(pc), _p(gt), _p(ws), _stream()), "dl_icp_loss_fwd")
    _sync()
    K = pc[:, 0].cpu().numpy().astype(np.float64)
    assert K.tolist() == got["stats"][:, 1].tolist() and all(int(k) & (int(k) - 1) == 0 and k > 64 for k in K)
    assert lt[:, 1].cpu().numpy().tobytes() == (got["stats"][:, 0] / got["stats"][:, 1]).astype(np.float32).tobytes()
    g = gt.cpu().numpy().astype(np.float64).reshape(B, 3, 3, 4)[:, 1]
    T = case["T"].astype(np.float64)
    for b in range(B):
        b_trans = K[b] / 2 * g[b][:, 3]
        M = (K[b] / 2 * g[b][:, :3]) @ T[b, :3, :3].T + np.outer(b_trans, T[b, :3, 3])
        b_rot = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]])
        assert np.concatenate([b_trans, b_rot]).tobytes() == got["rhs"][b].tobytes(), (b, b_trans, b_rot, got["rhs"][b])


# ---------------------------------------------------------------------------------------------------- real data, real chain


def _room_chain(dev):
    """Two synthetic scan pairs at 16 x 128 through projection, normals and the exact search, at the true relative pose."""
    from delora_amd import geometry
    from delora_amd.data import synthetic
    H, W = 16, 128
    sensor = geometry.Sensor(H, W, *util.kitti_fov())
    scans, Ts = [], []
    for b in range(2):
        s1, s2, T21 = synthetic.make_pair(90 + b, rings=16, azimuth_steps=140)
        scans += [torch.from_numpy(np.ascontiguousarray(s1[:3])), torch.from_numpy(np.ascontiguousarray(s2[:3]))]
        Ts.append(torch.from_numpy(np.asarray(T21, dtype=np.float32)))
    offs = torch.tensor(np.cumsum([0] + [s.shape[1] for s in scans]), dtype=torch.int32, device=dev)
    proj = geometry.project(torch.cat(scans, dim=1).contiguous().to(dev), offs, max(s.shape[1] for s in scans), sensor)
    img = proj["image4"]
    nrm, nrm_pk = geometry.normals(img, 1, 2, 0.5, 5, want_packed=True)
    tgt, src = slice(0, None, 2), slice(1, None, 2)
    T = torch.stack(Ts).to(dev)
    src_img, src_n = img[src].contiguous(), nrm[src].contiguous()
    nn_pix, _, match = geometry.nn_correspond(src_img, src_n, proj["packed"][tgt].contiguous(), nrm_pk[tgt].contiguous(), T, sensor, want_visible=False)
    return T, src_img, src_n, match, nn_pix


def test_float_data_through_the_real_chain():
    """Against the float64 reference on the kernel's own match / nn_pix, at the TRUE relative pose of the pairs (the converged regime:
    residuals of centimetres on coordinates of tens of metres).  Bound: about six fp32 roundings per term plus at most about
    twelve sequential fp32 additions before the fp64 stage, relative to the sum of |terms|, which Cauchy-Schwarz bounds by
    sqrt(info_ii info_jj) (by sqrt(info_ii sum r^2) for rhs); 64 * 2^-24 = 3.81e-6 leaves about a 3x margin over that count.

    The residual itself is formed in fp64 and rounded once (include/delora_hip.h), so its error IS relative to its own size; with
    d = q - p_t in fp32 the error of a term J_i r would be relative to |J_i| |q| instead (measured then: rhs 9.6e-6, outside the
    bound, at residuals of 6 cm rms on coordinates of tens of metres).  Every figure is printed before anything is asserted."""
    from delora_amd import geometry
    dev = _dev()
    T, src_img, src_n, match, nn_pix = _room_chain(dev)
    got = geometry.icp_information(T, src_img, src_n, match, nn_pix)
    again = geometry.icp_information(T, src_img, src_n, match, nn_pix)
    _sync()
    B, HW = 2, 16 * 128
    f = lambda t, c: t[:, :c].reshape(B, c, HW).cpu().numpy()
    m = match.reshape(B, 6, HW).cpu().numpy()
    ref = ir.information(f(src_img, 3), f(src_n, 3), m[:, :3], m[:, 3:], nn_pix.reshape(B, HW).cpu().numpy(), T.cpu().numpy())
    info, rhs = got["information"].cpu().numpy(), got["rhs"].cpu().numpy()
    assert (ref["stats"][:, 1] > 200).all(), ref["stats"]
    assert got["pairs"].cpu().numpy().tolist() == ref["stats"][:, 1].tolist()
    eps = 64 * 2.0 ** -24
    d = np.sqrt(np.einsum("bii->bi", ref["info"]))
    worst_info = (np.abs(info - ref["info"]) / (d[:, :, None] * d[:, None, :])).max()
    worst_rhs = (np.abs(rhs - ref["rhs"]) / (d * np.sqrt(ref["stats"][:, :1]))).max()
    worst_r2 = (np.abs(got["sum_r2"].cpu().numpy() - ref["stats"][:, 0]) / ref["stats"][:, 0]).max()
    # the same deviation of rhs against the scale an fp32 rounding of q would give: sqrt(info_ii) * 2^-24 * sqrt(sum w |q|^2)
    J, _ = ir.jacobian(f(src_img, 3), m[:, :3], m[:, 3:], T.cpu().numpy())
    w = ir.weights(f(src_n, 3), m[:, 3:], nn_pix.reshape(B, HW).cpu().numpy())
    Tn = T.cpu().numpy().astype(np.float64)
    q = np.einsum("bij,bjk->bik", Tn[:, :3, :3], f(src_img, 3).astype(np.float64)) + Tn[:, :3, 3:4]
    q_scale = np.sqrt((w * (q * q).sum(axis=1)).sum(axis=1, keepdims=True))
    util.measured("information_real_info_rel", worst_info)
    util.measured("information_real_rhs_rel", worst_rhs)
    util.measured("information_real_sum_r2_rel", worst_r2)
    util.measured("information_real_rhs_vs_q_rounding", (np.abs(rhs - ref["rhs"]) / (d * 2.0 ** -24 * q_scale)).max())
    util.measured("information_real_residual_rms_m", np.sqrt(ref["stats"][:, 0] / ref["stats"][:, 1]).max())
    for b in range(B):
        assert np.array_equal(info[b], info[b].T)
    for k in got:                                                    # deterministic from run to run
        assert torch.equal(got[k], again[k]) or bool(torch.isnan(got[k]).any()), k
    # the finishing stage on the kernel's own sums
    cov, status = got["covariance"].cpu().numpy(), got["status"].cpu().numpy()
    for b in range(B):
        want_cov, want_status = ir.finish(info[b], float(got["sum_r2"][b]), float(got["pairs"][b]))
        assert status[b] == want_status
        if want_status == ir.OK:
            cond = np.linalg.cond(ir.scaled(info[b]))
            sigma2 = float(got["sum_r2"][b]) / (float(got["pairs"][b]) - 6)
            util.measured(f"information_real_cov_identity_{b}", np.abs(cov[b] @ info[b] / sigma2 - np.eye(6)).max(), 1e-9 * max(1.0, cond / 1e4))
    # the two bounds of the sums, last: everything above has been checked and printed by now
    util.measured("information_real_info_rel", worst_info, eps)
    util.measured("information_real_rhs_rel", worst_rhs, eps)


# ---------------------------------------------------------------------------------------------------- covariance and status


def _scene_run(case, dev):
    from delora_amd import geometry
    M = case["p"].shape[2]
    t = lambda k, c: torch.from_numpy(case[k]).reshape(1, c, 1, M).contiguous().to(dev)
    return geometry.icp_information(torch.from_numpy(case["T"]).to(dev), t("p", 3), t("n", 3), torch.cat([t("pt", 3), t("nt", 3)], dim=1).contiguous(),
                                    torch.from_numpy(case["nn"]).reshape(1, 1, M).to(dev))


def test_covariance_on_well_conditioned_scenes():
    """cond(Ah) <= 1e4 (asserted): a backward-stable 6x6 Cholesky gives about 6 * 2^-53 * cond = 7e-12, 1e-9 is a 100x margin."""
    dev = _dev()
    for seed in (0, 1):
        case = ir.box_room(600, seed)
        ref = _ref(case)
        assert ref["status"][0] == ir.OK and np.linalg.cond(ir.scaled(ref["info"][0])) <= 1e4
        got = _scene_run(case, dev)
        _sync()
        info, cov = got["information"][0].cpu().numpy(), got["covariance"][0].cpu().numpy()
        assert int(got["status"][0]) == ir.OK and int(got["pairs"][0]) == 600
        assert np.linalg.cond(ir.scaled(info)) <= 1e4
        sigma2 = float(got["sum_r2"][0]) / (600 - 6)
        util.measured(f"information_cov_identity_seed{seed}", np.abs(cov @ info / sigma2 - np.eye(6)).max(), 1e-9)
        assert np.array_equal(cov, cov.T) and (np.diag(cov) > 0).all()
        # and it is the reference's covariance up to the fp32 rounding of the sums behind it: in the scaled space (unit diagonal) every
        # entry of the information matrix is off by at most eps = 64 * 2^-24 (the bound of the real-data test), so |E|_2 <= 6 eps, and
        # |(A + E)^-1 - A^-1|_2 <= cond |A^-1|_2 |E|_2 (|A|_2 >= 1) with |C|_2 <= 6 max|C|; sigma^2 adds eps
        eps = 64 * 2.0 ** -24
        sd = np.sqrt(np.diag(ref["info"][0]))
        Cs, Cs_ref = cov * sd[:, None] * sd[None, :], ref["covariance"][0] * sd[:, None] * sd[None, :]
        cond = np.linalg.cond(ir.scaled(ref["info"][0]))
        util.measured(f"information_cov_vs_float64_seed{seed}", np.abs(Cs - Cs_ref).max() / np.abs(Cs_ref).max(), (36 * cond + 1) * eps)


def test_planar_and_six_pair_scenes_have_no_covariance():
    dev = _dev()
    plane = _scene_run(ir.planar_scene(), dev)
    six = _scene_run(ir.six_pair_scene(), dev)
    _sync()
    assert int(plane["status"][0]) == ir.UNOBSERVABLE and int(plane["pairs"][0]) == 600
    assert [float(plane["information"][0, i, i]) for i in (0, 1, 5)] == [0.0, 0.0, 0.0]
    assert int(six["status"][0]) == ir.TOO_FEW_PAIRS and int(six["pairs"][0]) == 6
    for got in (plane, six):
        assert got["covariance"].cpu().numpy().tobytes() == np.zeros((1, 6, 6)).tobytes()


# ---------------------------------------------------------------------------------------------------- graph capture


def test_graph_replay_equals_the_eager_call():
    B, H, W, coord = EXACT_SHAPES[3]
    case = exact_case(B, H, W, coord)
    run = InfoRun(case, _dev())
    eager = run.run()
    run.poison()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run.launch()
    torch.cuda.current_stream().wait_stream(side)
    _sync()
    run.poison()                                                     # capture enqueues nothing that survives: replay writes everything
    graph.replay()
    _sync()
    replayed = run.read()
    for k in eager:
        assert eager[k].tobytes() == replayed[k].tobytes(), k
