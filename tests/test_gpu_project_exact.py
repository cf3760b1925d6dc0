"""dl_project against the reference of its contract (tests/project_ref.py), BIT FOR BIT: there is no tolerance anywhere in this file.
The C ABI is called directly; every pointer is a view inside a tests/conv_ref.Arenas allocation: points, offsets are frozen inputs
(columns of the point buffer that belong to no scan hold NaN), every output and the workspace are poisoned, and the workspace is
exactly dl_project_workspace_bytes long, so that a write beside a buffer, an element never written and a promise that is too small
all show.  `uvr` legitimately holds NaN (NaN inputs) and pix2pt / kept are integers, so "written" means: no element still holds
the arena's poison word -- except the uvr columns outside the scans, which must still hold it.

Sensors, generators and cases are those of tests/project_ref.py; tests/test_project_ref_host.py proves on the host that each of a
list of plausible defects is told from the reference by at least one of them."""
import ctypes
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import project_ref as pr
from tests import util

pytestmark = pytest.mark.gpu

INVALID = -1                                           # DL_ERR_INVALID_ARGUMENT
POISON = cr._as_i32(cr.NAN_WORD[torch.float32])
OPTIONAL = ("packed", "packed_aux", "kept", "uvr")
CHILD_CASE = "ragged-S9-C7-all"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _p(t, offset_bytes=0):
    return ctypes.c_void_p(t.data_ptr() + offset_bytes) if t is not None else ctypes.c_void_p(0)


def _bits(a):
    """uint32 view; every NaN becomes one pattern (which NaN an operation produces is the platform's choice)."""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    t0 = time.time()
    yield
    if torch.cuda.is_available():
        util.measured("test_gpu_project_exact: wall time of the file [s]", time.time() - t0)


@pytest.fixture(autouse=True)
def _needs_a_gpu():
    _dev()


class Run:
    """One dl_project call laid out in arenas.  scans: list of fp32 [C,n]; scan s owns columns offs[s]..offs[s+1) with
    offs[0] = offs0, n_cols = offs[S] + tail, pts_cs = n_cols + pad; ``null`` names the optional outputs passed as NULL."""

    def __init__(self, sen, scans, C, offs0=0, tail=0, pad=0, null=(), skew=0, dev=None):
        from delora_amd import _lib
        self.L, self.lib, self.sen, self.C, self.S = _lib, _lib.load(), sen, C, len(scans)
        dev = dev or _dev()
        S, H, W = self.S, sen.H, sen.W
        lens = [s.shape[1] for s in scans]
        offs = offs0 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.offs, self.max_n = offs, max(lens)
        self.n_cols, self.cs = int(offs[-1]) + tail, int(offs[-1]) + tail + pad
        pts = np.full((C, max(self.cs, 1)), np.nan, dtype=np.float32)
        for s, scan in enumerate(scans):
            pts[:, offs[s]:offs[s + 1]] = scan
        self.A, self.Wk = cr.Arenas(dev, skew), cr.Arenas(dev, skew)
        a = lambda shape, dtype, fill, name: self.A.arena(shape, dtype, fill, name, row_elems=0)
        self.pts = a(pts.shape, torch.float32, torch.from_numpy(pts), "pts")
        self.d_offs = a((S + 1,), torch.int32, torch.from_numpy(offs.astype(np.int32)), "offs")
        self.struct = _lib.SensorStruct(H, W, sen.hfov[0], sen.hfov[1], sen.vfov[0], sen.vfov[1])
        self.out = {"image4": a((S, 4, H, W), torch.float32, None, "image4"), "pix2pt": a((S, H, W), torch.int32, None, "pix2pt"),
                    "aux": a((S, C - 3, H, W), torch.float32, None, "aux") if C > 3 else None,
                    "packed": a((S, H, W, 4), torch.float32, None, "packed") if "packed" not in null else None,
                    "packed_aux": a((S, H, W, 4), torch.float32, None, "packed_aux") if C >= 6 and "packed_aux" not in null else None,
                    "kept": a((S,), torch.int32, None, "kept") if "kept" not in null else None,
                    "uvr": a((3, max(self.cs, 1)), torch.float32, None, "uvr") if "uvr" not in null else None}
        nbytes = int(self.lib.dl_project_workspace_bytes(S, H, W, self.n_cols, C))
        assert nbytes == (S * H * W * 8 + 15) // 16 * 16 + self.n_cols * 16 * (2 if C > 3 else 1)
        self.ws = self.Wk.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
        assert self.ws.data_ptr() % 16 == 0

    def poison(self):
        for v in list(self.out.values()) + [self.ws]:
            if v is not None:
                v.view(torch.int32).fill_(POISON)

    def call(self, max_n=None, ws_offset=0):
        o = self.out
        return self.lib.dl_project(_p(self.pts), self.cs, self.n_cols, _p(self.d_offs), self.S, self.C, self.max_n if max_n is None else max_n,
                                   ctypes.byref(self.struct), _p(o["image4"]), _p(o["aux"]), _p(o["packed"]), _p(o["packed_aux"]), _p(o["pix2pt"]),
                                   _p(self.ws, ws_offset), _p(o["kept"]), _p(o["uvr"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def run(self, what, max_n=None):
        """Poison, call, check guards / inputs / "every element written"; returns the outputs as numpy arrays."""
        self.poison()
        self.L.check(self.call(max_n), "dl_project")
        _sync()
        self.A.check(what)
        self.Wk.check(what)
        got = {}
        for k, v in self.out.items():
            if v is None:
                continue
            left = v.view(torch.int32) == POISON
            if k == "uvr":
                lo, hi = int(self.offs[0]), int(self.offs[-1])
                outside = torch.ones(v.shape[1], dtype=torch.bool, device=v.device)
                outside[lo:hi] = False
                assert bool(left[:, outside].all()), f"{what}: uvr columns outside the scans were written"
                left = left[:, lo:hi]
            n = int(left.sum())
            assert n == 0, f"{what}: {n} elements of {k} were never written"
            got[k] = v.cpu().numpy()
        if "uvr" in got:
            got["uvr"] = got["uvr"][:, int(self.offs[0]):int(self.offs[-1])]
        return got


def compare(got, ref, what, C):
    """Bit equality of every output that was asked for."""
    for k, g in got.items():
        if k == "packed_aux" and C < 6:
            continue
        r = ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        gb, rb = _bits(g), _bits(r)
        if not np.array_equal(gb, rb):
            bad = np.argwhere(gb != rb)
            lines = [f"{what}: {k}: {len(bad)} of {g.size} elements differ"]
            for idx in bad[:8]:
                t = tuple(idx)
                lines.append(f"    at {t}: got {g[t]!r} (0x{int(gb[t]) & 0xFFFFFFFF:08x}), expected {r[t]!r} (0x{int(rb[t]) & 0xFFFFFFFF:08x})")
            pytest.fail("\n".join(lines))


def digest(got):
    h = hashlib.sha256()
    for k in sorted(got):
        h.update(k.encode())
        h.update(np.ascontiguousarray(_bits(got[k])).tobytes())
    return h.hexdigest()


_REF = {}


def _coord_ref(name):
    """(points, reference outputs) of the coordinate tests at one sensor: computed once, shared, never modified."""
    if name not in _REF:
        p = np.array(pr.coordinate_points(name))
        _REF[name] = (p, pr.project([p], pr.sensor(name), 3))
    return _REF[name]


# ------------------------------------------------------------------------------------------------ coordinates and the fast path


@pytest.mark.parametrize("name", list(pr.SENSOR_TABLE))
def test_uvr_bitwise(name):
    """With uvr given every point takes the fp64 evaluation: u, v and the range of ~20 000 random points over seven decades, the
    specials, the planted boundary points and the exact halves equal the reference bit for bit -- and so does the image."""
    p, ref = _coord_ref(name)
    got = Run(pr.sensor(name), [p], 3).run(f"uvr[{name}]")
    for i, plane in enumerate("uvr"):
        compare({"uvr": got["uvr"][i]}, {"uvr": ref["uvr"][i]}, f"uvr[{name}] plane {plane}", 3)
    compare(got, ref, f"uvr[{name}]", 3)


@pytest.mark.parametrize("name", list(pr.SENSOR_TABLE))
def test_fast_path_pixels(name):
    """uvr = NULL: atan2f plus the distance test decide, with the fp64 evaluation as the fallback.  The image must be the one of the
    reference, whose coordinates are the fp64 contract: the independent check of tol_u / tol_v at this sensor."""
    p, ref = _coord_ref(name)
    got = Run(pr.sensor(name), [p], 3, null=("uvr",)).run(f"fast[{name}]")
    assert set(got) == {"image4", "packed", "pix2pt", "kept"}
    compare(got, ref, f"fast[{name}]", 3)


# ------------------------------------------------------------------------------------------------ ties and order


@pytest.mark.parametrize("name", ["coarse", "ragged"])
def test_ties_and_order(name):
    """Lattice points of bit-equal range sharing a pixel (at least 4 per group on the coarse sensor), exact duplicates, and points
    whose squares overflow (range +inf: they vote, lose to every finite point and win only a pixel they have to themselves; the
    host tier asserts that both happen).  The same cloud in two index orders: each equals the reference, so the winner follows
    the index and nothing else."""
    sen, tc = pr.sensor(name), pr.tie_cloud()
    winners = []
    for perm, cloud in enumerate((tc, np.ascontiguousarray(tc[:, ::-1]))):
        for null in ((), ("uvr",)):
            ref = pr.project([cloud], sen, 3)
            got = Run(sen, [cloud], 3, null=null).run(f"ties[{name}] order {perm}")
            compare(got, ref, f"ties[{name}] order {perm} null={null}", 3)
        winners.append(got["pix2pt"])
    occupied = winners[0] >= 0
    assert np.array_equal(occupied, winners[1] >= 0)
    n = tc.shape[1]
    moved = winners[0][occupied] != n - 1 - winners[1][occupied]            # the same POINT won in both orders
    assert moved.any(), "no tie was decided by the index"
    assert np.array_equal(got["image4"][:, 3][occupied], pr.project([tc], sen, 3)["image4"][:, 3][occupied]), "the winning range depends on the order"


# ------------------------------------------------------------------------------------------------ layout


@pytest.mark.parametrize("case", pr.layout_cases(), ids=lambda c: c["name"])
def test_layout(case):
    """S from 1 to 24 (S >= 8 with S % 8 != 0: ghost workgroups; G up to 12), scans of 0 ... 3000 points, C = 3 ... 8, each optional
    output given and NULL, offs[0] = 5, n_cols = offs[S] + 3, pts_cs = n_cols + 7; sensors with H*W % 256 != 0 and with an odd
    S*H*W (key plane padded to 16 bytes); one case with every base 16 bytes past a 256-byte boundary."""
    sen, scans, C = pr.sensor(case["sensor"]), pr.case_scans(case), case["C"]
    ref = pr.project(scans, sen, C)
    run = Run(sen, scans, C, pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS, case["null"], case["skew"])
    got = run.run(case["name"])
    assert set(OPTIONAL) - set(got) == set(case["null"]) | ({"packed_aux"} if C < 6 else set())
    compare(got, ref, case["name"], C)
    if max(case["lens"]) == 0:
        assert run.max_n == 0 and not got["image4"].any() and (got["pix2pt"] == -1).all() and not got["kept"].any()
        assert not np.signbit(got["image4"]).any() and not np.signbit(got["packed"]).any()


def test_misaligned_workspace_is_refused_and_nothing_is_written():
    case = [c for c in pr.layout_cases() if c["name"] == CHILD_CASE][0]
    run = Run(pr.sensor(case["sensor"]), pr.case_scans(case), case["C"], pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS)
    for off in (4, 8):
        run.poison()
        assert run.call(ws_offset=off) == INVALID and b"16-byte aligned" in run.lib.dl_last_error()
        _sync()
        run.A.check("misaligned workspace")
        run.Wk.check("misaligned workspace")
        for k, v in list(run.out.items()) + [("workspace", run.ws)]:
            assert bool((v.view(torch.int32) == POISON).all()), f"{k} was written by a refused call"


# ------------------------------------------------------------------------------------------------ the G cap


@pytest.mark.parametrize("S", [1, 8])
def test_vote_grid_cap(S):
    """A scan of 1024 * 256 + 300 points: the vote's G caps at 1024 and 300 threads walk a second stride -- whose points are the
    nearest of their pixels, so that they must win them.  Alone (plain grid) and with seven short scans (XCD mapping)."""
    sen, scans = pr.sensor("kitti"), list(pr.cap_scans(S))
    assert max(s.shape[1] for s in scans) == pr.CAP_POINTS
    ref = pr.project(scans, sen, 3)
    big = [s.shape[1] for s in scans].index(pr.CAP_POINTS)
    assert int((ref["pix2pt"][big] >= 1024 * 256).sum()) >= 250
    got = Run(sen, scans, 3, null=("uvr",)).run(f"cap S={S}")
    compare(got, ref, f"cap S={S}", 3)


# ------------------------------------------------------------------------------------------------ repeatability, max_n, plain grid


def _child_case():
    case = [c for c in pr.layout_cases() if c["name"] == CHILD_CASE][0]
    return case, pr.sensor(case["sensor"]), pr.case_scans(case)


def test_repeatable_and_independent_of_the_batch():
    case, sen, scans = _child_case()
    C = case["C"]
    run = Run(sen, scans, C, pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS)
    first, second = run.run("run 1"), run.run("run 2")
    assert digest(first) == digest(second)
    # max_n only sizes the grid: a larger one changes nothing
    assert digest(run.run("max_n + 1000", max_n=run.max_n + 1000)) == digest(first)
    # a scan alone equals the same scan inside the batch of 9
    s = int(np.argmax(case["lens"]))
    alone = Run(sen, [scans[s]], C).run("alone")
    lo, hi = int(run.offs[s] - run.offs[0]), int(run.offs[s + 1] - run.offs[0])
    for k in ("image4", "aux", "packed", "packed_aux", "pix2pt", "kept"):
        assert np.array_equal(_bits(alone[k][0]), _bits(first[k][s])), k
    assert np.array_equal(_bits(alone["uvr"]), _bits(first["uvr"][:, lo:hi]))


def test_plain_grid_gives_the_same_bits():
    """DL_PROJECT_PLAIN_GRID=1 (read once per process) selects the plain workgroup -> scan mapping for S >= 8 too: a fresh child
    process runs the S = 9 case with it and prints the digest of its outputs."""
    assert os.environ.get("DL_PROJECT_PLAIN_GRID", "") != "1", "this process must run the XCD mapping"
    case, sen, scans = _child_case()
    mine = digest(Run(sen, scans, case["C"], pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS).run("parent"))
    from tests.conftest import ROOT
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_project_exact"], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env={**os.environ, "DL_PROJECT_PLAIN_GRID": "1"})
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith("sha256 ")]
    assert len(lines) == 1 and lines[0].split()[1] == mine, (lines, mine)


if __name__ == "__main__":
    assert os.environ.get("DL_PROJECT_PLAIN_GRID") == "1"
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    case_, sen_, scans_ = _child_case()
    got_ = Run(sen_, scans_, case_["C"], pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS, dev=torch.device("cuda:0")).run("child")
    compare(got_, pr.project(scans_, sen_, case_["C"]), "child", case_["C"])
    print("sha256", digest(got_))
