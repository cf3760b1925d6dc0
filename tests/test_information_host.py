"""Pose covariance of the odometry output, the parts that need no GPU: the float64 reference of tests/information_ref.py against
finite differences and its own status rule on three planted scenes, the headroom of every bit-exact case of
tests/test_gpu_information_exact.py, the refusals of ``dl_icp_information`` / ``dl_odometry_quality`` (all before any launch: the
pointers are host memory and never touched), the ABI bookkeeping, and the host logic of ``ScanToScanOdometry(quality=...)``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import information_ref as ir
from tests import util
from tests.conftest import ROOT

INVALID = -1                                           # DL_ERR_INVALID_ARGUMENT
NEW_SYMBOLS = ("dl_icp_information_workspace_bytes", "dl_icp_information", "dl_odometry_quality_workspace_bytes", "dl_odometry_quality")


def _planes(case):
    return case["p"], case["n"], case["pt"], case["nt"], case["nn"], case["T"]


# ---------------------------------------------------------------------------------------------------- the reference


@pytest.mark.parametrize("make", [ir.box_room, lambda: ir.integer_case(2, 97, seed=3)], ids=["room", "integers"])
def test_rhs_is_half_the_finite_difference_gradient_of_the_cost(make):
    case = make()
    ref = ir.information(*_planes(case))
    h = 1e-6
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        g = (ir.cost(*_planes(case), e) - ir.cost(*_planes(case), -e)) / (2 * h)
        scale = np.sqrt(ref["info"][:, i, i] * ref["stats"][:, 0]) + 1e-30                  # Cauchy-Schwarz: |rhs_i| <= this
        assert np.all(np.abs(0.5 * g - ref["rhs"][:, i]) <= 1e-7 * scale + 1e-9), (i, 0.5 * g, ref["rhs"][:, i])


def test_information_is_symmetric_and_positive_semidefinite():
    for case in (ir.box_room(), ir.planar_scene(), ir.integer_case(3, 501, seed=1)):
        info = ir.information(*_planes(case))["info"]
        for A in info:
            assert np.array_equal(A, A.T)
            assert np.linalg.eigvalsh(A).min() >= -1e-9 * max(np.abs(A).max(), 1.0)


def test_status_rule_on_three_planted_scenes():
    room = ir.information(*_planes(ir.box_room()))
    assert room["status"].tolist() == [ir.OK] and room["stats"][0, 1] == 600
    A = room["info"][0]
    assert np.linalg.cond(ir.scaled(A)) <= 1e4
    sigma2 = room["stats"][0, 0] / (room["stats"][0, 1] - 6)
    assert np.abs(room["covariance"][0] @ A / sigma2 - np.eye(6)).max() <= 1e-9
    assert np.array_equal(room["covariance"][0], room["covariance"][0].T) and np.all(np.diag(room["covariance"][0]) > 0)
    # the residual noise planted along the normals (1 cm) is what sigma estimates
    assert 0.008 < np.sqrt(sigma2) < 0.012
    plane = ir.information(*_planes(ir.planar_scene()))
    assert plane["status"].tolist() == [ir.UNOBSERVABLE] and not plane["covariance"].any() and plane["stats"][0, 1] == 600
    assert [plane["info"][0, i, i] for i in (0, 1, 5)] == [0.0, 0.0, 0.0]                     # x, y and the yaw are not seen at all
    six = ir.information(*_planes(ir.six_pair_scene()))
    assert six["status"].tolist() == [ir.TOO_FEW_PAIRS] and six["stats"][0, 1] == 6 and not six["covariance"].any()
    # a nearly planar scene has positive diagonals and fails on a pivot: a corridor seen through one tilted patch
    case = ir.planar_scene()
    case["nt"][0][:, :3] = np.float32([[1e-6, 0, 0], [0, 1e-6, 0], [1, 1, 1]])
    case["n"][0][:, :3] = case["nt"][0][:, :3]
    near = ir.information(*_planes(case))
    assert near["status"].tolist() == [ir.UNOBSERVABLE] and np.all(np.diag(near["info"][0]) > 0)
    # scale freedom: millimetres instead of metres change neither the status nor the scaled matrix's spectrum
    mm = ir.box_room()
    for k in ("p", "pt"):
        mm[k] = mm[k] * np.float32(1000.0)
    mm["T"][:, :3, 3] *= 1000.0
    got = ir.information(*_planes(mm))
    assert got["status"].tolist() == [ir.OK]
    np.testing.assert_allclose(np.linalg.eigvalsh(ir.scaled(got["info"][0])), np.linalg.eigvalsh(ir.scaled(A)), rtol=1e-4)


def test_headroom_of_every_exact_case():
    """The cases tests/test_gpu_information_exact.py runs bit for bit: every sum of absolute summands stays below 2^24."""
    from tests import test_gpu_information_exact as g
    worst = 0.0
    for (B, H, W, coord) in g.EXACT_SHAPES:
        case = g.exact_case(B, H, W, coord)
        worst = max(worst, ir.headroom(case))
        w = ir.weights(case["n"], case["nt"], case["nn"])
        for b in range(B):                                  # all three classes of non-counting pixel, and counting ones
            has_s, has_t, ok = (case["n"][b] != 0).any(axis=0), (case["nt"][b] != 0).any(axis=0), case["nn"][b] >= 0
            assert (~ok).any() and (ok & ~has_s).any() and (ok & has_s & ~has_t).any()
        assert w.sum() > 0
    print(f"worst accumulator: {worst:.4f} of 2^24")
    assert worst < 0.5
    shapes = [(B, H * W) for (B, H, W, _) in g.EXACT_SHAPES]
    assert shapes[:4] == [(1, 60), (1, 256), (1, 180), (3, 2048)]
    # the last one makes a wave walk more than one chunk under the grid cap of 128 workgroups x 4 waves
    assert shapes[4][1] > 131072 and -(-shapes[4][1] // 256) > 512


# ---------------------------------------------------------------------------------------------------- the C ABI


def test_abi_version_and_declarations():
    from delora_amd import _lib
    lib = _lib.load()
    assert lib.dl_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "delora_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert "dl_scan_geometry" in code and "DL_INFO_MIN_PIVOT 1e-10" in code
    assert (_lib.INFO_OK, _lib.INFO_TOO_FEW_PAIRS, _lib.INFO_UNOBSERVABLE, _lib.INFO_MIN_PIVOT) == (ir.OK, ir.TOO_FEW_PAIRS, ir.UNOBSERVABLE, ir.MIN_PIVOT)
    assert [f[0] for f in _lib.ScanGeometry._fields_] == ["normals", "packed_image", "packed_normals"]


def test_size_functions_are_host_arithmetic_and_refuse_bad_shapes():
    from delora_amd import _lib, geometry
    lib = _lib.load()
    ws = lib.dl_icp_information_workspace_bytes
    # one row of 32 floats per workgroup: a workgroup per four 256-pixel chunks, at most 128 per sample
    assert ws(1, 3, 20) == 128 and ws(1, 4, 64) == 128 and ws(1, 5, 1024) == 5 * 128 and ws(3, 16, 128) == 3 * 2 * 128
    assert ws(1, 64, 2048) == 128 * 128 and ws(2, 66, 2048) == 2 * 128 * 128
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, -1), (1, 1 << 16, 1 << 15), (65536, 4, 4)):
        assert ws(*bad) == 0 and b"dl_icp_information_workspace_bytes" in lib.dl_last_error(), bad
    sensor = geometry.Sensor(16, 128, *util.kitti_fov())
    qs = lib.dl_odometry_quality_workspace_bytes
    n = qs(ctypes.byref(sensor.struct), 16, 128)
    assert n >= 2048 * 28 + lib.dl_nn_workspace_bytes(1, 16, 128) + ws(1, 16, 128) and n % 256 == 0
    assert qs(ctypes.byref(sensor.struct), 16, 64) == 0 and b"dl_odometry_quality_workspace_bytes" in lib.dl_last_error()
    assert qs(None, 16, 128) == 0 and b"null sensor" in lib.dl_last_error()
    bad = geometry.Sensor(1, 128, *util.kitti_fov())
    assert qs(ctypes.byref(bad.struct), 1, 128) == 0 and b"bad sensor" in lib.dl_last_error()


def test_entry_points_refuse_before_any_launch_and_name_themselves():
    from delora_amd import _lib, geometry
    lib = _lib.load()
    raw = (ctypes.c_double * 4096)()
    base = (ctypes.addressof(raw) + 255) // 256 * 256
    p = ctypes.c_void_p(base)                                # host memory, 256-byte aligned: a refused call never touches it
    off = lambda k: ctypes.c_void_p(base + k)
    null = ctypes.c_void_p(0)
    H, W = 4, 16
    HW = H * W

    def refused(rc, who, word):
        err = lib.dl_last_error()
        assert rc == INVALID, (rc, err)
        assert who.encode() in err and word.encode() in err, err

    def info(src=p, srcn=p, match=p, nn=p, T=p, B=1, H=H, W=W, ss=(4 * HW, 3 * HW, 6 * HW), out=(p, p, p, p, p), ws=p):
        return lib.dl_icp_information(src, ss[0], srcn, ss[1], match, ss[2], nn, T, B, H, W, *out, ws, null)

    who = "dl_icp_information"
    for k in ("src", "srcn", "match", "nn", "T", "ws"):
        refused(info(**{k: null}), who, "null")
    for i in range(5):
        refused(info(out=tuple(null if j == i else p for j in range(5))), who, "null")
    for over in (dict(B=0), dict(H=0), dict(W=-3), dict(H=1 << 16, W=1 << 15), dict(B=1 << 16)):
        refused(info(**over), who, "bad sizes")
    refused(info(ss=(3 * HW - 1, 3 * HW, 6 * HW)), who, "stride")
    refused(info(ss=(4 * HW, 3 * HW - 4, 6 * HW)), who, "stride")
    refused(info(ss=(4 * HW, 3 * HW, 6 * HW - 4)), who, "stride")
    refused(info(ss=(4 * HW + 2, 3 * HW, 6 * HW)), who, "16-byte aligned")
    refused(info(src=off(4)), who, "16-byte aligned")
    refused(info(nn=off(8)), who, "16-byte aligned")
    refused(info(ws=off(8)), who, "workspace must be 16-byte aligned")
    refused(info(out=(off(4), p, p, p, p)), who, "aligned to their element size")
    refused(info(out=(p, p, p, p, off(2))), who, "aligned to their element size")

    sensor = geometry.Sensor(16, 128, *util.kitti_fov())
    sp = ctypes.byref(sensor.struct)
    rec = _lib.ScanGeometry(base, base, base)
    rp = ctypes.byref(rec)

    def quality(sensor=sp, prev=p, gprev=rp, cur=p, gcur=rp, T=p, a=3, b=5, ws=p, out=(p, p, p, p, p)):
        return lib.dl_odometry_quality(sensor, prev, gprev, cur, gcur, T, a, b, 0.5, 10, ws, *out, null)

    who = "dl_odometry_quality"
    refused(quality(sensor=None), who, "null sensor")
    refused(quality(cur=null), who, "null")
    refused(quality(gcur=None), who, "null")
    refused(quality(gcur=ctypes.byref(_lib.ScanGeometry(base, 0, base))), who, "null")
    refused(quality(gprev=None), who, "null")
    refused(quality(gprev=ctypes.byref(_lib.ScanGeometry(base, base, 0))), who, "null")
    refused(quality(T=null), who, "null")
    refused(quality(ws=null), who, "null")
    refused(quality(out=(p, p, null, p, p)), who, "null")
    refused(quality(prev=null, cur=off(4)), who, "16-byte aligned")                       # the first scan is checked as well
    refused(quality(gcur=ctypes.byref(_lib.ScanGeometry(base + 8, base, base))), who, "16-byte aligned")
    refused(quality(ws=off(16)), who, "workspace must be 256-byte aligned")
    refused(quality(a=16), who, "bad window")
    refused(quality(b=-1), who, "bad window")
    bad = geometry.Sensor(1, 128, *util.kitti_fov())
    refused(quality(sensor=ctypes.byref(bad.struct)), who, "bad sensor")
    assert not any(raw), "a refused call wrote into its buffers"


# ---------------------------------------------------------------------------------------------------- ScanToScanOdometry


class _FixedModel(torch.nn.Module):
    def forward(self, stacked):
        return torch.tensor([[0.1, 0.0, 0.0]]), torch.tensor([[0.0, 0.0, 0.0, 1.0]])


def _oracle_pair(previous, current, sensor):
    from oracle import delora_oracle as orc
    s = util.oracle_sensor(sensor.H, sensor.W, sensor.vfov, sensor.hfov)
    return torch.cat([orc.project_to_img(c.cpu(), s)[0] for c in (previous, current)], dim=0)


def test_quality_with_normalization_scaling_is_refused():
    from delora_amd.ros_utils.odometry import ScanToScanOdometry
    cfg = util.repo_config(16, 128, normalization_scaling=True)
    with pytest.raises(ValueError, match="normalization_scaling"):
        ScanToScanOdometry(cfg, model=_FixedModel(), project_pair=_oracle_pair, quality=True)
    ScanToScanOdometry(cfg, model=_FixedModel(), project_pair=_oracle_pair)                    # without quality it is served as ever


def test_quality_off_returns_exactly_todays_keys_on_the_cpu():
    from delora_amd.ros_utils.odometry import ScanToScanOdometry
    cfg = util.repo_config(16, 128, normalization_scaling=False)
    rng = np.random.default_rng(0)
    scans = [torch.from_numpy(rng.normal(0, 5, (1, 3, 500)).astype(np.float32)) for _ in range(3)]
    for kwargs in ({}, {"quality": False}):
        odo = ScanToScanOdometry(cfg, model=_FixedModel(), project_pair=_oracle_pair, **kwargs)
        assert odo.quality is False and odo.normal_params is None
        assert odo.push(scans[0]) is None
        for s in scans[1:]:
            assert sorted(odo.push(s)) == ["T_0_t", "global_quaternion", "global_translation", "quaternion", "transformation", "translation"]
    # with quality the normal parameters are read exactly as NormalsComputer reads them
    from delora_amd.preprocessing.normal_computation import NormalsComputer
    odo = ScanToScanOdometry(cfg, model=_FixedModel(), project_pair=_oracle_pair, quality=True)
    assert odo.normal_params == NormalsComputer(cfg, "kitti")._params()
    q = ScanToScanOdometry._quality_result(torch.eye(6, dtype=torch.float64) * 4, torch.tensor(8.0), torch.tensor(32.0), torch.zeros(6, 6, dtype=torch.float64),
                                           torch.tensor(2, dtype=torch.int32))
    assert q["residual_rms"] == 0.5 and q["pairs"] == 32 and q["quality_status"] == 2 and q["covariance"].dtype == np.float64
    np.testing.assert_allclose(q["information_eigenvalues"], np.ones(6))
    q = ScanToScanOdometry._quality_result(torch.zeros(6, 6, dtype=torch.float64), torch.tensor(0.0), torch.tensor(0.0), torch.zeros(6, 6, dtype=torch.float64),
                                           torch.tensor(1, dtype=torch.int32))
    assert np.isnan(q["information_eigenvalues"]).all() and np.isnan(q["residual_rms"]) and q["pairs"] == 0
