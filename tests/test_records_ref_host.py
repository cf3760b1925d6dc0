"""Host side of the records path (include/delora_hip.h: dl_project_records, dl_odometry_push_records): the reference of its filter
against the node's own host filter, proof that the threshold cloud sees a fused range, the workspace arithmetic, and every refusal
with host dummy pointers (a refused call touches none of them).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from delora_amd import _lib, geometry
from delora_amd.deploy import native_infer
from delora_amd.ros_utils import odometry
from tests import project_ref as pr
from tests import records_ref as rr
from tests.test_native_infer_host import BLOCKS, dummy_address, make_net

INVALID, UNSUPPORTED = -1, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _clouds():
    sen = pr.sensor("ragged")
    return {"random": pr.random_mix(20000, 3), "near": pr.random_cloud(20000, 0.3, 5, flat=1.0), "specials": pr.specials(sen),
            "odd values": rr.odd_values(), "threshold": rr.threshold_cloud("ragged"), "removed winner": rr.removed_winner_cloud("ragged")}


@pytest.mark.parametrize("name", ["random", "near", "specials", "odd values", "threshold", "removed winner"])
def test_keep_mask_is_the_nodes_filter(name):
    xyz = _clouds()[name]
    with np.errstate(all="ignore"):
        expected = odometry.filter_scans(xyz[None])
    keep = rr.keep_mask(xyz, rr.DROP_ZERO | rr.MIN_RANGE)
    assert 0 < keep.sum() < keep.size, "the cloud must hold kept and dropped points"
    assert np.array_equal(_bits(expected[0]), _bits(xyz[:, keep]))
    # each flag alone is the matching half of the node's expression
    zero = (xyz[0] != 0.0) & (xyz[1] != 0.0) & (xyz[2] != 0.0)
    with np.errstate(all="ignore"):
        far = np.linalg.norm(xyz, axis=0) > 0.3
    assert np.array_equal(rr.keep_mask(xyz, rr.DROP_ZERO), zero) and np.array_equal(rr.keep_mask(xyz, rr.MIN_RANGE), far)
    assert rr.keep_mask(xyz, 0).all()


def test_zero_rules():
    xyz = np.array([[0.0, 1, 1], [-0.0, 1, 1], [1, -0.0, 1], [1, 1, 0.0], [np.nan, 1, 1], [1e-45, 1, 1], [np.inf, 1, 1], [1, 1, 1]], dtype=np.float32).T
    assert rr.keep_mask(xyz, rr.DROP_ZERO).tolist() == [False, False, False, False, True, True, True, True]
    # a NaN range and a NaN threshold compare false; an infinite range passes
    assert rr.keep_mask(xyz, rr.MIN_RANGE).tolist() == [True, True, True, True, False, True, True, True]
    assert not rr.keep_mask(xyz, rr.MIN_RANGE, float("nan")).any()


def test_threshold_cloud_tells_the_fused_range_from_the_nodes():
    xyz = rr.threshold_cloud("ragged")
    with np.errstate(all="ignore"):
        expected = odometry.filter_scans(xyz[None])[0]
    fused = rr.keep_mask(xyz, 3, fused=True)
    assert int((fused != rr.keep_mask(xyz, 3)).sum()) >= rr.THRESHOLD_MIN_DISAGREE
    assert fused.sum() != expected.shape[1] or not np.array_equal(_bits(xyz[:, fused]), _bits(expected))
    # ... and the images differ too: the defect would be seen through dl_project_records' outputs, not only through n_pass
    sen = pr.sensor("ragged")
    good = rr.project_records_ref([xyz], sen, 3)
    bad = pr.project([np.ascontiguousarray(xyz[:, fused])], sen, 3)
    assert not np.array_equal(_bits(good["image4"]), _bits(bad["image4"]))
    # numpy's norm is the unfused expression, bit for bit
    p = pr._rng(9).normal(size=(3, 200000)).astype(np.float32)
    assert np.array_equal(_bits(rr.range_np(p)), _bits(np.linalg.norm(p, axis=0)))


def test_pack_unpack_and_padding():
    xyz = pr.specials(pr.sensor("ragged"))
    for layout in rr.LAYOUTS + ((22, (0, 4, 8)), (22, (2, 10, 14))):
        a, b = rr.pack(xyz, layout, "ff"), rr.pack(xyz, layout, 4)
        assert a.size == xyz.shape[1] * layout[0] and (layout[0] == 12 or not np.array_equal(a, b))
        for raw in (a, b):
            assert np.array_equal(_bits(rr.unpack(raw, layout)), _bits(xyz))
            lay = odometry.record_layout(layout[0], layout[1])
            assert np.array_equal(_bits(odometry.unpack_records(raw, lay)[0]), _bits(xyz))


def test_record_layout_of_a_structured_dtype():
    dt = np.dtype({"names": ["x", "y", "z", "intensity", "ring"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2"], "offsets": [0, 4, 8, 16, 20],
                   "itemsize": 22})
    lay = odometry.record_layout(dt)
    assert (lay.point_step, lay.off_x, lay.off_y, lay.off_z, lay.filter) == (22, 0, 4, 8, 3) and lay.min_range == np.float32(0.3)
    assert "point_step=22" in native_infer.why_layout_unsupported(lay)
    dt32 = np.dtype({"names": ["z", "x", "y"], "formats": ["<f4", "<f4", "<f4"], "offsets": [16, 0, 8], "itemsize": 32})
    lay = odometry.record_layout(dt32)
    assert (lay.point_step, lay.off_x, lay.off_y, lay.off_z) == (32, 0, 8, 16) and native_infer.why_layout_unsupported(lay) is None
    with pytest.raises(ValueError, match="float32"):
        odometry.record_layout(np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")]))
    with pytest.raises(ValueError, match="x, y, z"):
        odometry.record_layout(np.dtype([("x", "<f4"), ("y", "<f4")]))


@pytest.mark.parametrize("S,H,W", [(1, 64, 720), (3, 5, 9), (1, 5, 9), (9, 16, 130), (2, 2, 2)])
def test_workspace_is_the_key_plane_only(S, H, W):
    lib = _lib.load()
    assert lib.dl_project_records_workspace_bytes(S, H, W) == (S * H * W * 8 + 15) // 16 * 16
    assert lib.dl_project_records_workspace_bytes(S, H, W) == lib.dl_project_workspace_bytes(S, H, W, 0, 3)
    assert lib.dl_project_records_workspace_bytes(0, H, W) == 0 and lib.dl_project_records_workspace_bytes(S, 0, W) == 0


def _layout(step=16, offs=(0, 4, 8), flt=3, min_range=0.3):
    return geometry.record_layout(step, offs, flt, min_range)


BAD_LAYOUTS = [  # (layout arguments, the field the text must name)
    (dict(step=22), "point_step"), (dict(step=8, offs=(0, 4, 4)), "point_step"), (dict(step=260), "point_step"), (dict(step=0), "point_step"),
    (dict(step=-16), "point_step"), (dict(offs=(2, 4, 8)), "off_x"), (dict(offs=(0, 6, 8)), "off_y"), (dict(offs=(0, 4, 13)), "off_z"),
    (dict(offs=(0, 4, 16)), "off_z"), (dict(offs=(16, 4, 8)), "off_x"), (dict(offs=(-4, 4, 8)), "off_x"), (dict(offs=(0, 0, 8)), "off_y"),
    (dict(offs=(0, 4, 0)), "off_z"), (dict(offs=(0, 4, 4)), "off_z"), (dict(min_range=float("nan")), "min_range"),
    (dict(min_range=float("inf")), "min_range"), (dict(min_range=float("-inf"), flt=2), "min_range")]


def _project_records(lib, d, sensor, layout, **over):
    a = dict(records=d, n=10, layout=ctypes.byref(layout) if layout is not None else None, offs=d, S=1, max_n=10,
             sensor=ctypes.byref(sensor.struct) if sensor is not None else None, image4=d, packed=d, pix2pt=d, ws=d, kept=d, n_pass=d)
    a.update(over)
    return lib.dl_project_records(a["records"], a["n"], a["layout"], a["offs"], a["S"], a["max_n"], a["sensor"], a["image4"], a["packed"], a["pix2pt"],
                                  a["ws"], a["kept"], a["n_pass"], None)


def test_project_records_refusals():
    lib, d = _lib.load(), dummy_address()
    sensor = geometry.Sensor(16, 128, (-0.4, 0.03), (-3.1, 3.1))
    for kw, field in BAD_LAYOUTS:
        assert _project_records(lib, d, sensor, _layout(**kw)) == UNSUPPORTED, kw
        text = lib.dl_last_error().decode()
        assert text.startswith("dl_project_records: ") and "layout." + field in text, (kw, text)
    for mis in (1, 2, 3):
        assert _project_records(lib, d, sensor, _layout(), records=d + mis) == UNSUPPORTED and b"records must be 4-byte aligned" in lib.dl_last_error()
    for null in ("records", "offs", "image4", "pix2pt", "ws"):
        assert _project_records(lib, d, sensor, _layout(), **{null: None}) == INVALID and b"dl_project_records: null pointer" in lib.dl_last_error(), null
    assert _project_records(lib, d, None, _layout()) == INVALID and b"null pointer" in lib.dl_last_error()
    assert _project_records(lib, d, sensor, None) == INVALID and b"null pointer" in lib.dl_last_error()
    for flt in (4, 8, 0x80000003):
        assert _project_records(lib, d, sensor, _layout(flt=flt)) == INVALID and b"layout.filter" in lib.dl_last_error()
    for off in (4, 8, 12):
        assert _project_records(lib, d, sensor, _layout(), ws=d + off) == INVALID and b"workspace must be 16-byte aligned" in lib.dl_last_error()
    for over in (dict(S=0), dict(max_n=-1), dict(n=-1)):
        assert _project_records(lib, d, sensor, _layout(), **over) == INVALID and b"bad sizes" in lib.dl_last_error()
    assert _project_records(lib, d, geometry.Sensor(1, 128, (-0.4, 0.03), (-3.1, 3.1)), _layout()) == INVALID and b"bad sizes" in lib.dl_last_error()
    # a misaligned workspace is reported before the layout: invalid arguments first, then the layout's shape
    assert _project_records(lib, d, sensor, _layout(step=22), ws=d + 8) == INVALID


def test_odometry_push_records_refusals():
    lib, d = _lib.load(), dummy_address()
    _, good = make_net()
    sensor = geometry.Sensor(16, 128, (-0.4, 0.03), (-3.1, 3.1))
    sp = ctypes.byref(sensor.struct)

    def push(layout, records=d, n=10, offs=d, image_cur=d, ws=d, translation=d, net=good, sensor_p=sp):
        return lib.dl_odometry_push_records(net, d, sensor_p, records, n, ctypes.byref(layout) if layout is not None else None, offs, d, image_cur, ws,
                                            translation, d, d, None)

    for kw, field in BAD_LAYOUTS:
        assert push(_layout(**kw)) == UNSUPPORTED, kw
        text = lib.dl_last_error().decode()
        assert text.startswith("dl_odometry_push_records: ") and "layout." + field in text, (kw, text)
    assert push(_layout(), records=d + 2) == UNSUPPORTED and b"4-byte aligned" in lib.dl_last_error()
    assert push(_layout(flt=4)) == INVALID and b"layout.filter" in lib.dl_last_error()
    assert push(None) == INVALID and b"dl_odometry_push_records: null pointer" in lib.dl_last_error()
    assert push(_layout(), records=None) == INVALID and b"null pointer" in lib.dl_last_error()
    assert push(_layout(), offs=None) == INVALID and b"null pointer" in lib.dl_last_error()
    assert push(_layout(), n=-1) == INVALID and b"bad sizes n_records=-1" in lib.dl_last_error()
    assert push(_layout(), ws=dummy_address(misalign=128)) == INVALID and b"workspace" in lib.dl_last_error()
    assert push(_layout(), translation=None) == INVALID and b"translation" in lib.dl_last_error()
    # pose_check's refusals apply unchanged
    bad = geometry.Sensor(16, 30, (-0.4, 0.03), (-3.1, 3.1))
    assert push(_layout(), sensor_p=ctypes.byref(bad.struct)) == UNSUPPORTED and b"W=30" in lib.dl_last_error()
    narrow = tuple((cin // 2, cout // 2, s, ds) for (cin, cout, s, ds) in BLOCKS)
    _, net = make_net(blocks=narrow)
    assert push(_layout(), net=net) == UNSUPPORTED and lib.dl_last_error().startswith(b"dl_odometry_push_records: ")
    # the workspace does not grow with the scan: the size for max_points = 0 is the forward's + the pixel map + the key plane
    H, W = 16, 128
    up = lambda n: (n + 255) // 256 * 256
    assert lib.dl_odometry_workspace_bytes(good, sp, 0, H, W) == (lib.dl_pose_net_workspace_bytes(good, 1, H, W) + up(H * W * 4)
                                                                   + up(lib.dl_project_records_workspace_bytes(1, H, W)))


def test_python_side_restates_the_layout_rule():
    for kw, field in BAD_LAYOUTS:
        assert native_infer.why_layout_unsupported(_layout(**kw)) is not None, kw
    for step, offs in rr.LAYOUTS:
        assert native_infer.why_layout_unsupported(_layout(step, offs)) is None
    assert native_infer.why_layout_unsupported(_layout(min_range=float("nan"), flt=1)) is None       # min_range matters under its flag only


def test_abi_number_header_and_signatures():
    lib = _lib.load()
    assert lib.dl_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(ROOT, "include", "delora_hip.h")).read()
    assert re.search(r"#define DL_ABI_VERSION 10\b", header)
    for name in ("dl_project_records_workspace_bytes", "dl_project_records", "dl_odometry_push_records"):
        assert re.search(r"\b(size_t|int) " + name + r"\(", header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define DL_RECORDS_DROP_ZERO 1u", header) and re.search(r"#define DL_RECORDS_MIN_RANGE 2u", header)
    assert (_lib.RECORDS_DROP_ZERO, _lib.RECORDS_MIN_RANGE) == (1, 2) and ctypes.sizeof(_lib.RecordLayout) == 24
    assert [f[0] for f in _lib.RecordLayout._fields_] == ["point_step", "off_x", "off_y", "off_z", "filter", "min_range"]
