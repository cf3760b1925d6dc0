"""Streaming odometry from raw point records (dl_odometry_push_records; NativeOdometry.push_records; ScanToScanOdometry.push_records;
tools/odometry_demo --records) against the route that existed before it: the node's filter on the host, a planar [3,N] upload and
dl_odometry_push.  BIT FOR BIT -- the records path skips what the host filter removes inside the vote, which leaves every other key as
it is, so the image, and with it every later number, is the same.  Full-width network at 16 x 128, random weights."""
import os
import subprocess

import numpy as np
import pytest
import torch

from delora_amd.data import synthetic
from delora_amd.deploy import native_infer
from delora_amd.ros_utils import odometry
from tests.conftest import ROOT
from tests.test_gpu_native_infer import _dev, _model

pytestmark = pytest.mark.gpu

H, W = 16, 128
KITTI = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("intensity", "<f4")])


def _messages(n):
    """n different ``[N,4]`` fp32 messages (x, y, z, intensity) of different lengths, as a driver delivers them: with missing returns
    (all-zero records), records with one exactly zero or -0.0 coordinate and returns from within 0.3 m scattered through them."""
    out = []
    for i in range(n):
        xyz = np.asarray(synthetic.make_pair(700 + i, rings=16, azimuth_steps=140 + 9 * i)[i % 2][:3], dtype=np.float32)
        rng = np.random.default_rng(50 + i)
        msg = np.concatenate([xyz.T, rng.uniform(0, 1, (xyz.shape[1], 1)).astype(np.float32)], axis=1)
        pick = rng.permutation(msg.shape[0])
        msg[pick[:60], :3] = 0.0
        msg[pick[60:90], 2] = -0.0
        msg[pick[90:120], 0] = 0.0
        msg[pick[120:180], :3] *= (0.25 / np.linalg.norm(msg[pick[120:180], :3], axis=1, keepdims=True)).astype(np.float32)
        out.append(np.ascontiguousarray(msg))
    assert len({m.shape[0] for m in out}) == n
    return out


def _planar(msg):
    """What the parent route uploads: the node's host filter on ``[1,3,N]``, contiguous ``[3,n]`` on the device."""
    kept = odometry.filter_scans(np.ascontiguousarray(msg[:, :3].T)[None])[0]
    assert 0 < kept.shape[1] < msg.shape[0] - 100
    return torch.from_numpy(np.ascontiguousarray(kept)).to(_dev())


def _snapshot(engine, out):
    return [engine.image_t.clone()] + ([t.clone() for t in out] if out is not None else [])


def _reference(msgs):
    """Per message: image_t and (translation, quaternion, T) of NativeOdometry.push on the host-filtered planar scan."""
    model, _, sensor = _model(H, W, "tanh")
    engine = native_infer.NativeOdometry(model, sensor)
    return [_snapshot(engine, engine.push(_planar(m))) for m in msgs]


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: tensor {k} differs in {int((a != b).sum())} elements"


@pytest.mark.parametrize("source", ["device", "host", "structured"])
def test_push_records_equals_push_on_the_filtered_scan(source):
    model, _, sensor = _model(H, W, "tanh")
    msgs = _messages(3)
    want = _reference(msgs)
    assert len(want[0]) == 1 and len(want[1]) == 4
    engine = native_infer.NativeOdometry(model, sensor)
    layout = odometry.record_layout(16, (0, 4, 8))
    for k, m in enumerate(msgs):
        if source == "device":
            out = engine.push_records(torch.from_numpy(m.reshape(-1)).to(_dev()).view(torch.uint8), layout)
        elif source == "host":
            out = engine.push_records(m, layout)
        else:
            s = m.view(KITTI).reshape(-1)
            out = engine.push_records(s, odometry.record_layout(s.dtype))
        _same(_snapshot(engine, out), want[k], f"{source} message {k}")
    torch.cuda.synchronize()


def test_back_to_back_pushes_from_the_host_reuse_the_staging_buffers_safely():
    """Four different messages pushed without a synchronisation in between; poses are cloned on the device and read only at the end.
    The two staging buffers are each used twice, the second time for a LONGER message (they grow) -- every result equals the
    one-at-a-time result."""
    model, _, sensor = _model(H, W, "tanh")
    msgs = _messages(4)
    want = _reference(msgs)
    engine = native_infer.NativeOdometry(model, sensor)
    layout = odometry.record_layout(16, (0, 4, 8))
    got = [_snapshot(engine, engine.push_records(m, layout)) for m in msgs]
    torch.cuda.synchronize()
    for k in range(4):
        _same(got[k], want[k], f"message {k}")
    # once both staging buffers have seen the longest message, nothing is allocated per push: the same buffers serve another round
    longest = max(msgs, key=lambda m: m.shape[0])
    engine.push_records(longest, layout), engine.push_records(longest, layout)
    grown = ([t.data_ptr() for t in engine._stage], engine._records.data_ptr())
    for m in msgs:
        engine.push_records(m, layout)
    torch.cuda.synchronize()
    assert ([t.data_ptr() for t in engine._stage], engine._records.data_ptr()) == grown


def _dicts_equal(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert sorted(a) == sorted(b), what
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


@pytest.mark.parametrize("engine", ["native", "torch"])
def test_scan_to_scan_push_records_returns_what_push_returns(engine):
    model, cfg, _ = _model(H, W, "tanh")
    msgs = _messages(3)
    ref = odometry.ScanToScanOdometry(cfg, model=model, engine=engine)
    want = [ref.push(np.ascontiguousarray(m.T)[None]) for m in msgs]
    assert want[0] is None and want[1] is not None
    for form in ("array", "structured", "bytes"):
        node = odometry.ScanToScanOdometry(cfg, model=model, engine=engine)
        for k, m in enumerate(msgs):
            if form == "array":
                got = node.push_records(m)
            elif form == "structured":
                got = node.push_records(m.view(KITTI).reshape(-1))
            else:
                got = node.push_records(m.reshape(-1).view(np.uint8), odometry.record_layout(16, (0, 4, 8)))
            _dicts_equal(got, want[k], f"{engine} {form} message {k}")


def test_a_22_byte_layout_takes_the_host_route_and_agrees():
    """Velodyne-style records (x, y, z, intensity, uint16 ring: 22 bytes) are refused by the library -- no misaligned device loads --
    and unpacked on the host instead."""
    model, cfg, _ = _model(H, W, "tanh")
    dt = np.dtype({"names": ["x", "y", "z", "intensity", "ring"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 4, 8, 12, 16],
                   "itemsize": 22})
    msgs = _messages(3)
    ref = odometry.ScanToScanOdometry(cfg, model=model, engine="native")
    node = odometry.ScanToScanOdometry(cfg, model=model, engine="native")
    assert native_infer.why_layout_unsupported(odometry.record_layout(dt)) is not None
    for k, m in enumerate(msgs):
        s = np.zeros(m.shape[0], dtype=dt)
        s["x"], s["y"], s["z"], s["intensity"], s["ring"] = m[:, 0], m[:, 1], m[:, 2], m[:, 3], np.arange(m.shape[0]) % 16
        _dicts_equal(node.push_records(s), ref.push(np.ascontiguousarray(m.T)[None]), f"message {k}")
    with pytest.raises(ValueError, match="point_step=22"):
        node.native.push_records(s, odometry.record_layout(dt))


def test_demo_program_reads_kitti_files(tmp_path):
    """tools/bin/odometry_demo --records 16 0 4 8 on three KITTI-format files, in a child process of its own, prints the T words the
    planar invocation prints for the host-filtered scans."""
    model, _, sensor = _model(H, W, "tanh")
    binary = os.path.join(ROOT, "tools", "bin", "odometry_demo")
    assert os.path.exists(binary), "tools/bin/odometry_demo is not built (make -C tools)"
    blob = str(tmp_path / "net.dlpose")
    native_infer.export_pose_net(model, blob, sensor)
    raw_files, planar_files = [], []
    for i, m in enumerate(_messages(3)):
        raw_files.append(str(tmp_path / f"{i:06d}.bin"))
        m.astype("<f4").tofile(raw_files[-1])
        planar_files.append(str(tmp_path / f"planar{i}.bin"))
        _planar(m).cpu().numpy().astype("<f4").tofile(planar_files[-1])
    outs = []
    for name, args in (("records", ["--records", "16", "0", "4", "8"]), ("planar", [])):
        out = str(tmp_path / f"{name}.txt")
        files = raw_files if args else planar_files
        run = subprocess.run(["timeout", "-k", "10", "120", binary] + args + [blob, out] + files, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.returncode, run.stdout[-2000:], run.stderr[-2000:])
        outs.append([line.split() for line in open(out).read().strip().split("\n")])
    assert len(outs[0]) == 2 and len(outs[1]) == 2
    for a, b in zip(*outs):
        assert a[:18] == b[:18] and a[1] == "T" and len(a) == 31
    # a layout the library refuses ends the program with the library's text
    bad = subprocess.run(["timeout", "-k", "10", "60", binary, "--records", "16", "0", "4", "4", blob, str(tmp_path / "bad.txt")] + raw_files,
                         capture_output=True, text=True)
    assert bad.returncode == 3 and "layout.off_z" in bad.stderr
