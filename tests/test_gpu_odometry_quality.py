"""Pose quality behind the streaming odometry (``dl_odometry_quality``; ``NativeOdometry(quality=True)``;
``ScanToScanOdometry(quality=True)``): both engines return the same bits -- the same kernels on the same operands --, the native
object agrees with the hand-chained geometry calls on its own images, and the poses do not change by a bit.  Full-width network at
16 x 128, random weights, three synthetic scans."""
import os
import subprocess

import numpy as np
import pytest
import torch

from delora_amd import geometry
from delora_amd.data import synthetic
from delora_amd.deploy import native_infer
from delora_amd.preprocessing.normal_computation import NormalsComputer
from delora_amd.ros_utils import odometry
from tests.conftest import ROOT
from tests.test_gpu_native_infer import _dev, _model

pytestmark = pytest.mark.gpu

H, W = 16, 128
QUALITY_KEYS = ("covariance", "information", "pairs", "quality_status")
POSE_KEYS = ("translation", "quaternion", "transformation", "global_translation", "global_quaternion", "T_0_t")


def _messages(n=3):
    """n ``[N,4]`` fp32 messages (x, y, z, intensity) of one synthetic sequence, with a few all-zero records the node's filter drops."""
    scans, _ = synthetic.make_sequence(800, n, rings=16, azimuth_steps=140)
    out = []
    for i, s in enumerate(scans):
        xyz = np.asarray(s[:3], dtype=np.float32)
        msg = np.concatenate([xyz.T, np.full((xyz.shape[1], 1), 0.5, dtype=np.float32)], axis=1)
        msg[np.random.default_rng(i).permutation(msg.shape[0])[:40], :3] = 0.0
        out.append(np.ascontiguousarray(msg))
    return out


def _run(engine, precision, route, quality=True):
    model, cfg, _ = _model(H, W, "tanh")
    node = odometry.ScanToScanOdometry(cfg, model=model, engine=engine, precision=precision, quality=quality)
    out = []
    for m in _messages():
        out.append(node.push_records(m) if route == "records" else node.push(np.ascontiguousarray(m[:, :3].T)[None]))
    torch.cuda.synchronize()
    return out, node


@pytest.mark.parametrize("route", ["push", "records"])
@pytest.mark.parametrize("precision", ["float32", "bfloat16"])
def test_both_engines_return_the_same_quality_bits(precision, route):
    native, node = _run("native", precision, route)
    eager, _ = _run("torch", precision, route)
    plain, _ = _run("native", precision, route, quality=False)
    assert native[0] is None and eager[0] is None and plain[0] is None
    assert node.normal_params == NormalsComputer(node.config, "kitti")._params()
    for k in (1, 2):
        a, b, c = native[k], eager[k], plain[k]
        assert sorted(a) == sorted(b) == sorted(POSE_KEYS + QUALITY_KEYS + ("residual_rms", "information_eigenvalues"))
        assert sorted(c) == sorted(POSE_KEYS)
        for key in QUALITY_KEYS:
            assert np.array_equal(a[key], b[key]), (precision, route, k, key, a[key], b[key])
        assert a["covariance"].shape == (6, 6) and a["covariance"].dtype == np.float64 and a["information"].shape == (6, 6)
        assert a["information_eigenvalues"].shape == (6,) and a["pairs"] > 6
        assert a["residual_rms"] == b["residual_rms"] and a["residual_rms"] > 0
        if a["quality_status"] == 0:
            assert np.all(np.diag(a["covariance"]) > 0) and np.all(np.diff(a["information_eigenvalues"]) >= 0)
        else:
            assert not a["covariance"].any()
        # the poses with and without quality: identical to the bit
        for key in POSE_KEYS:
            assert np.array_equal(a[key], c[key]), (precision, route, k, key)


def test_native_odometry_agrees_with_the_hand_chained_geometry_calls():
    model, cfg, sensor = _model(H, W, "tanh")
    params = NormalsComputer(cfg, "kitti")._params()
    engine = native_infer.NativeOdometry(model, sensor, quality=True, normal_params=params)
    plain = native_infer.NativeOdometry(model, sensor)
    dev = _dev()
    for k, m in enumerate(_messages()):
        pts = torch.from_numpy(np.ascontiguousarray(odometry.filter_scans(np.ascontiguousarray(m[:, :3].T)[None])[0])).to(dev)
        out, ref = engine.push(pts), plain.push(pts)
        nrm, nrm_pk = geometry.normals(engine.image_t[None], *params, want_packed=True)
        # the record of the current image is filled by every push, the first included
        assert torch.equal(engine.normals[engine.cur], nrm[0]) and torch.equal(engine.packed_normals[engine.cur], nrm_pk[0])
        assert torch.equal(engine.packed_images[engine.cur], geometry.pack_image(engine.image_t[None])[0])
        if k == 0:
            assert out is None and ref is None and engine.quality_out is None and bool((nrm != 0).any())
            continue
        for a, b in zip(out, ref):                                   # the poses do not change by a bit
            assert torch.equal(a, b)
        prev_nrm, prev_pk = geometry.normals(engine.image_t_1[None], *params, want_packed=True)
        assert torch.equal(engine.normals[1 - engine.cur], prev_nrm[0])
        nn_pix, _, match = geometry.nn_correspond(engine.image_t[None], nrm, geometry.pack_image(engine.image_t_1[None]), prev_pk, engine.T, sensor,
                                                  need_without_normals=False, want_visible=False)
        want = geometry.icp_information(engine.T, engine.image_t[None], nrm, match, nn_pix)
        q = engine.quality_out
        assert torch.equal(q["information"], want["information"][0]) and torch.equal(q["rhs"], want["rhs"][0])
        assert torch.equal(q["covariance"], want["covariance"][0]) and torch.equal(q["status"], want["status"])
        assert float(q["stats"][0]) == float(want["sum_r2"][0]) and float(q["stats"][1]) == float(want["pairs"][0]) > 6
    torch.cuda.synchronize()


def test_demo_program_prints_the_covariance_diagonal(tmp_path):
    """tools/bin/odometry_demo --records 16 0 4 8 --quality <window>, in a child process of its own: the T words do not change with
    --quality, and status, pair count and covariance diagonal are those of ``NativeOdometry(quality=True)`` on the same messages."""
    model, cfg, sensor = _model(H, W, "tanh")
    params = NormalsComputer(cfg, "kitti")._params()
    binary = os.path.join(ROOT, "tools", "bin", "odometry_demo")
    assert os.path.exists(binary), "tools/bin/odometry_demo is not built (make -C tools)"
    blob = str(tmp_path / "net.dlpose")
    native_infer.export_pose_net(model, blob, sensor)
    msgs, files = _messages(), []
    for i, m in enumerate(msgs):
        files.append(str(tmp_path / f"{i:06d}.bin"))
        m.astype("<f4").tofile(files[-1])
    lines = {}
    for name, args in (("plain", []), ("quality", ["--quality"] + [repr(v) for v in params])):
        out = str(tmp_path / f"{name}.txt")
        run = subprocess.run(["timeout", "-k", "10", "120", binary, "--records", "16", "0", "4", "8"] + args + [blob, out] + files, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.returncode, run.stdout[-2000:], run.stderr[-2000:])
        lines[name] = [line.split() for line in open(out).read().strip().split("\n")]
        if args:
            assert run.stdout.count("covariance diagonal") == 2
    engine = native_infer.NativeOdometry(model, sensor, quality=True, normal_params=params)
    layout = odometry.record_layout(16, (0, 4, 8))
    engine.push_records(msgs[0], layout)
    for k in (1, 2):
        plain, q = lines["plain"][k - 1], lines["quality"][k - 1]
        assert len(plain) == 31 and q[:31] == plain and q[31] == "quality" and q[33] == "pairs" and q[35] == "cov_diag" and len(q) == 42
        engine.push_records(msgs[k], layout)
        want = engine.quality_out
        assert int(q[32]) == int(want["status"][0]) and float(q[34]) == float(want["stats"][1])
        assert [float(v) for v in q[36:]] == [float(f"{float(want['covariance'][i, i]):.9e}") for i in range(6)]
    bad = subprocess.run(["timeout", "-k", "10", "60", binary, "--records", "16", "0", "4", "8", "--quality", "16", "5", "0.5", "10", blob, str(tmp_path / "bad.txt")] + files, capture_output=True,
                         text=True)
    assert bad.returncode == 3 and "dl_odometry_quality" in bad.stderr and "bad window" in bad.stderr
