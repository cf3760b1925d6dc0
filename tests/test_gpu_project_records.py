"""dl_project_records against the reference of its contract (tests/records_ref.py), BIT FOR BIT: no tolerance anywhere in this file.
The C ABI is called directly; every pointer is a view inside a tests/conv_ref.Arenas allocation, as in test_gpu_project_exact.py: the
record buffer and the offsets are frozen inputs (records that belong to no scan hold NaN coordinates), every output and the workspace
are poisoned, and the workspace is exactly dl_project_records_workspace_bytes long -- the key plane and nothing else -- so that a
write beside a buffer, a key word or an output element never written, a modified record and a promise that is too small all show."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import project_ref as pr
from tests import records_ref as rr
from tests import util
from tests.test_gpu_project_exact import Run as PlanarRun
from tests.test_gpu_project_exact import _bits, _dev, _p, _sync, compare, digest

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -3
POISON = cr._as_i32(cr.NAN_WORD[torch.float32])
OPTIONAL = ("packed", "kept", "n_pass")
FILTERS = ((0, 0.3), (1, 0.3), (2, 0.3), (3, 0.3), (2, 0.0), (3, 0.0))         # (filter bits, min_range)
SENSOR = "ragged"                                                             # 16 x 130: H*W % 256 != 0
OFFS0, TAIL = 5, 3


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    if torch.cuda.is_available():
        util.measured("test_gpu_project_records: wall time of the file [s]", time.time() - t0)


@pytest.fixture(autouse=True)
def _needs_a_gpu():
    _dev()


class Run:
    """One dl_project_records call laid out in arenas.  scans: list of fp32 [3,n]; scan s owns records offs[s]..offs[s+1) with
    offs[0] = offs0 and n_records = offs[S] + tail; ``fill`` is the padding of rr.pack; ``null`` names the optional outputs passed as
    NULL; ``skew`` moves every base that many bytes past a 256-byte boundary (4: the 16-byte records lose their 16-byte alignment)."""

    def __init__(self, sen, scans, layout, fill="ff", offs0=0, tail=0, null=(), skew=0):
        from delora_amd import _lib
        self.L, self.lib, self.sen, self.S, self.layout = _lib, _lib.load(), sen, len(scans), layout
        dev = _dev()
        S, H, W = self.S, sen.H, sen.W
        lens = [s.shape[1] for s in scans]
        offs = offs0 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.offs, self.max_n, self.n_records = offs, max(lens), int(offs[-1]) + tail
        xyz = np.full((3, max(self.n_records, 1)), np.nan, dtype=np.float32)
        for s, scan in enumerate(scans):
            xyz[:, offs[s]:offs[s + 1]] = scan
        raw = rr.pack(xyz, layout, fill)
        self.A, self.Wk = cr.Arenas(dev, skew), cr.Arenas(dev, 0)
        a = lambda shape, dtype, fill_, name: self.A.arena(shape, dtype, fill_, name, row_elems=0)
        self.records = a(raw.shape, torch.int8, torch.from_numpy(raw.view(np.int8)), "records")
        self.d_offs = a((S + 1,), torch.int32, torch.from_numpy(offs.astype(np.int32)), "offs")
        self.struct = _lib.SensorStruct(H, W, sen.hfov[0], sen.hfov[1], sen.vfov[0], sen.vfov[1])
        self.out = {"image4": a((S, 4, H, W), torch.float32, None, "image4"), "pix2pt": a((S, H, W), torch.int32, None, "pix2pt"),
                    "packed": a((S, H, W, 4), torch.float32, None, "packed") if "packed" not in null else None,
                    "kept": a((S,), torch.int32, None, "kept") if "kept" not in null else None,
                    "n_pass": a((S,), torch.int32, None, "n_pass") if "n_pass" not in null else None}
        nbytes = int(self.lib.dl_project_records_workspace_bytes(S, H, W))
        assert nbytes == (S * H * W * 8 + 15) // 16 * 16
        self.ws = self.Wk.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
        assert self.ws.data_ptr() % 16 == 0 and self.records.data_ptr() % 256 == skew

    def poison(self):
        for v in list(self.out.values()) + [self.ws]:
            if v is not None:
                v.view(torch.int32).fill_(POISON)

    def call(self, flt, min_range, max_n=None, ws_offset=0, layout=None):
        o, (step, offs) = self.out, layout or self.layout
        lay = self.L.RecordLayout(step, offs[0], offs[1], offs[2], flt, min_range)
        return self.lib.dl_project_records(_p(self.records), self.n_records, ctypes.byref(lay), _p(self.d_offs), self.S,
                                           self.max_n if max_n is None else max_n, ctypes.byref(self.struct), _p(o["image4"]), _p(o["packed"]),
                                           _p(o["pix2pt"]), _p(self.ws, ws_offset), _p(o["kept"]), _p(o["n_pass"]),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self, what, flt, min_range=rr.THRESHOLD, max_n=None):
        """Poison, call, check guards / inputs / "every key word and every output element written"; returns the outputs as numpy."""
        self.poison()
        self.L.check(self.call(flt, min_range, max_n), "dl_project_records")
        _sync()
        self.A.check(what)
        self.Wk.check(what)
        got = {}
        for k, v in list(self.out.items()) + [("key plane", self.ws[:self.S * self.sen.H * self.sen.W * 2])]:
            if v is None:
                continue
            n = int((v.view(torch.int32) == POISON).sum())
            assert n == 0, f"{what}: {n} elements of {k} were never written"
            if k != "key plane":
                got[k] = v.cpu().numpy()
        return got


_CLOUDS, _REFS = {}, {}


def _cloud(name):
    if name not in _CLOUDS:
        sen = pr.sensor(SENSOR)
        make = {"specials": lambda: pr.specials(sen), "ties": pr.tie_cloud, "boundary": lambda: pr.boundary_points(sen),
                "raster": lambda: pr.raster_cloud(sen, 3000, 41), "threshold": lambda: rr.threshold_cloud(SENSOR),
                "removed winner": lambda: rr.removed_winner_cloud(SENSOR)}
        _CLOUDS[name] = np.ascontiguousarray(make[name]())
    return _CLOUDS[name]


def _ref(key, scans, sen, flt, min_range):
    """The reference of (scans named by ``key``, filter): computed once, shared, never modified."""
    k = (key, sen.name, flt, min_range)
    if k not in _REFS:
        _REFS[k] = rr.project_records_ref(scans, sen, flt, min_range)
    return _REFS[k]


CLOUDS = ("specials", "ties", "boundary", "raster", "threshold", "removed winner")


@pytest.mark.parametrize("layout", rr.LAYOUTS, ids=lambda l: f"{l[0]}-{'-'.join(map(str, l[1]))}")
@pytest.mark.parametrize("cloud", CLOUDS)
def test_clouds_layouts_filters(cloud, layout):
    """Every cloud in every layout under every filter, the padding filled once with 0xFF and once with random bits: each run equals
    the reference and the two fills give the same bits (no byte outside x, y, z influences anything).  The tie cloud holds exact
    duplicates: the lower RECORD index wins.  The threshold cloud holds >= 100 points that a fused range puts on the other side of
    0.3 m; the removed-winner cloud >= 32 pixels whose nearest record the filter drops."""
    sen = pr.sensor("coarse" if cloud == "ties" else SENSOR)
    xyz = _cloud(cloud)
    runs = [Run(sen, [xyz], layout, fill) for fill in ("ff", 17)]
    for flt, min_range in FILTERS:
        what = f"{cloud} step {layout[0]} filter {flt} min_range {min_range}"
        ref = _ref(cloud, [xyz], sen, flt, min_range)
        gots = [r.run(what, flt, min_range) for r in runs]
        compare(gots[0], ref, what + " (0xFF padding)", 3)
        assert digest(gots[0]) == digest(gots[1]), f"{what}: the padding bytes changed the result"


SCAN_LAYOUTS = {  # name -> (sensor, scan lengths, offs[0])
    "S1": ("ragged", [3000], 0),
    "S3-empty-offs5": ("odd", [257, 0, 1000], OFFS0),                         # S*H*W odd: the key plane is padded to 16 bytes
    "S9": ("ragged", [257, 0, 1000, 1, 3000, 255, 256, 1000, 257], OFFS0),    # the XCD mapping, a ghost group
    "S9-short": ("odd", [0, 1, 255, 256, 257, 1, 0, 255, 3000], 0),
    "S1-empty": ("ragged", [0], 0),
    "S3-all-empty": ("odd", [0, 0, 0], OFFS0),
}


def _layout_scans(name):
    _, lens, _ = SCAN_LAYOUTS[name]
    seed = 9000 + sorted(SCAN_LAYOUTS).index(name) * 64
    scans = []
    for j, n in enumerate(lens):
        xyz = np.array(pr.random_cloud(n, (0.2, 0.5, 10.0)[j % 3], seed + j, flat=0.3)) if n else np.zeros((3, 0), dtype=np.float32)
        xyz[j % 3, ::7] = 0.0 if j % 2 else -0.0                              # exact zeros in every scan
        scans.append(pr.settle(xyz, "records layout") if n else xyz)
    return scans


@pytest.mark.parametrize("layout", [rr.LAYOUTS[1], rr.LAYOUTS[3], rr.LAYOUTS[5]], ids=lambda l: f"step{l[0]}")
@pytest.mark.parametrize("name", list(SCAN_LAYOUTS))
def test_scan_layouts(name, layout):
    """S = 1, 3 (an empty scan, offs[0] = 5, records behind the last scan) and 9 (the XCD mapping), lengths from {0, 1, 255, 256, 257,
    1000, 3000}, each optional output given and NULL, filters 0 and 3.  With filter 0 the result also equals dl_project ITSELF on
    the transposed points, pix2pt included (library against library)."""
    sname, _, offs0 = SCAN_LAYOUTS[name]
    sen, scans = pr.sensor(sname), _layout_scans(name)
    nulls = ((), ("packed",), ("kept",), ("n_pass",), OPTIONAL)
    for i, null in enumerate(nulls):
        run = Run(sen, scans, layout, 23 + i, offs0, TAIL, null)
        for flt in (0, 3):
            what = f"{name} step {layout[0]} null={null} filter {flt}"
            got = run.run(what, flt)
            assert set(OPTIONAL) - set(got) == set(null)
            compare(got, _ref(name, scans, sen, flt, rr.THRESHOLD), what, 3)
            if flt == 0 and not null:
                planar = PlanarRun(sen, scans, 3, offs0, TAIL, 7, null=("uvr",)).run(what + " (dl_project)")
                for k in ("image4", "packed", "pix2pt", "kept"):
                    assert np.array_equal(_bits(planar[k]), _bits(got[k])), f"{what}: {k} differs from dl_project's"
                assert got["n_pass"].tolist() == [s.shape[1] for s in scans]
            if max(s.shape[1] for s in scans) == 0:
                assert not got["image4"].any() and (got["pix2pt"] == -1).all() and not np.signbit(got["image4"]).any()


def test_records_off_the_16_byte_grid_take_the_dword_loads():
    """16-byte records whose base is only 4-byte aligned (the 16-byte load would be misaligned): the same bits."""
    sen, xyz = pr.sensor(SENSOR), _cloud("raster")
    for layout in (rr.LAYOUTS[1], rr.LAYOUTS[2]):
        for skew in (4, 8, 16):
            got = Run(sen, [xyz], layout, 5, skew=skew).run(f"skew {skew}", 3)
            compare(got, _ref("raster", [xyz], sen, 3, rr.THRESHOLD), f"step 16 skew {skew}", 3)


def test_vote_grid_cap():
    """project_ref.CAP_POINTS records at step 16: the vote's grid caps at 1024 workgroups and 300 threads walk a second trip, whose
    records are the nearest of their pixels.  Every seventh record of the first trip is dropped by the filter (an exactly zero z)."""
    sen = pr.sensor("kitti")
    xyz = np.array(pr.cap_scans(1)[0])
    xyz[2, :1024 * 256:7] = 0.0
    ref = rr.project_records_ref([xyz], sen, 3)
    assert int((ref["pix2pt"][0] >= 1024 * 256).sum()) >= 250 and int(ref["n_pass"][0]) == xyz.shape[1] - (1024 * 256 + 6) // 7
    got = Run(sen, [xyz], rr.LAYOUTS[1], 3).run("cap", 3)
    compare(got, ref, "cap", 3)


def test_repeatable_max_n_and_offsets_beyond_the_buffer():
    name = "S9"
    sname, _, offs0 = SCAN_LAYOUTS[name]
    sen, scans = pr.sensor(sname), _layout_scans(name)
    run = Run(sen, scans, rr.LAYOUTS[4], 31, offs0, TAIL)
    first, second = run.run("run 1", 3), run.run("run 2", 3)
    assert digest(first) == digest(second)
    assert digest(run.run("max_n + 1000", 3, max_n=run.max_n + 1000)) == digest(first)      # max_n only sizes the grid
    # a record count smaller than the offsets promise: the records beyond it give no load and no vote -- the result is that of the
    # scans cut at n_records (the arena check proves that nothing outside the buffer was touched; reads beyond it would be NaN or poison)
    cut = int(run.offs[-1]) - 700
    run.n_records = cut
    got = run.run("n_records cut", 3)
    cut_scans = [s[:, :max(0, min(s.shape[1], cut - int(run.offs[i])))] for i, s in enumerate(scans)]
    compare(got, rr.project_records_ref(cut_scans, sen, 3), "n_records cut", 3)


def test_refusals_write_nothing():
    sen, xyz = pr.sensor(SENSOR), _cloud("raster")
    run = Run(sen, [xyz], rr.LAYOUTS[1], 9)
    calls = [(lambda: run.call(3, 0.3, ws_offset=8), INVALID, b"16-byte aligned"), (lambda: run.call(4, 0.3), INVALID, b"layout.filter"),
             (lambda: run.call(3, 0.3, layout=(22, (0, 4, 8))), UNSUPPORTED, b"layout.point_step"),
             (lambda: run.call(3, 0.3, layout=(16, (0, 4, 4))), UNSUPPORTED, b"layout.off_z"),
             (lambda: run.call(3, float("nan")), UNSUPPORTED, b"layout.min_range")]
    for call, code, text in calls:
        run.poison()
        assert call() == code and text in run.lib.dl_last_error(), (code, text, run.lib.dl_last_error())
        _sync()
        run.A.check("refused")
        run.Wk.check("refused")
        for k, v in list(run.out.items()) + [("workspace", run.ws)]:
            assert bool((v.view(torch.int32) == POISON).all()), f"{k} was written by a refused call"
    # min_range is not looked at without its flag
    run.L.check(run.call(1, float("nan")), "dl_project_records")
    _sync()


def test_python_wrapper():
    """geometry.project_records: uint8 and float32 record tensors, the dict of geometry.project plus n_pass."""
    from delora_amd import geometry
    sen, xyz = pr.sensor(SENSOR), _cloud("removed winner")
    gsen = geometry.Sensor(sen.H, sen.W, sen.vfov, sen.hfov)
    ref = _ref("removed winner", [xyz], sen, 3, rr.THRESHOLD)
    raw = torch.from_numpy(rr.pack(xyz, rr.LAYOUTS[4], 1)).cuda()
    offs = torch.tensor([0, xyz.shape[1]], dtype=torch.int32, device="cuda")
    lay = geometry.record_layout(32, (0, 4, 8), 3, 0.3)
    for records in (raw, raw.view(torch.float32)):
        out = geometry.project_records(records, offs, xyz.shape[1], gsen, lay)
        _sync()
        assert set(out) == {"image4", "aux", "packed", "packed_aux", "pix2pt", "kept", "uv", "n_pass"}
        compare({k: out[k].cpu().numpy() for k in ("image4", "packed", "pix2pt", "kept", "n_pass")}, ref, "wrapper", 3)
    out = geometry.project_records(raw, offs, xyz.shape[1], gsen, lay, want_kept=False, want_packed=False)
    assert out["kept"] is None and out["packed"] is None and np.array_equal(_bits(out["image4"].cpu().numpy()), _bits(ref["image4"]))
    with pytest.raises(ValueError, match="whole records"):
        geometry.project_records(raw[:-4], offs, xyz.shape[1], gsen, lay)
