"""dl_project_rotated and dl_rotations_from_draws against their contracts (tests/rotate_ref.py), the projection BIT FOR BIT: no
tolerance anywhere but the one the header states for the fp32 sine and cosine of dl_rotations_from_draws.

dl_project_rotated(scans, rot) must equal dl_project on the scans pre-rotated on the host in numpy float32 -- the same library, the
same launches after the vote -- on EVERY output: image4, aux, packed, packed_aux, pix2pt, kept and uvr.  The C ABI is called directly;
every pointer is a view inside a tests/conv_ref.Arenas allocation: points, offsets and rotations are frozen inputs (the point buffer
must come back unchanged: cached scans are reused across steps), every output and the workspace are poisoned, and the workspace is
exactly dl_project_workspace_bytes long.

Defects the cases of rotate_ref.cases() tell from the contract (tests/test_rotate_ref_host.py proves the first four on the host):
  * a transposed matrix                      (2 and 90 degrees; a half turn is its own transpose)
  * rot[s - 1] used for scan s               (rotated and unrotated scans alternate, neighbouring rotated scans turn opposite ways)
  * normals not rotated                      (C = 6 and 7: aux / packed_aux of the rotated scans)
  * staging record or uvr taken from the unrotated point   (image4 / packed hold the staged x, y, z and range; uvr is compared)
  * a contracted multiply-add                (random 10 m clouds: a fused sum differs in a share of the coordinates of every scan)
and, beside them: rotating channels 3..5 of a scan that has only 4 or 5, touching channels 6 and above, multiplying an identity
scan (-0.0, inf and NaN would not survive), writing the caller's points."""
import ctypes
import time

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import project_ref as pr
from tests import rotate_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

INVALID = -1                                           # DL_ERR_INVALID_ARGUMENT
POISON = cr._as_i32(cr.NAN_WORD[torch.float32])
OUTPUTS = ("image4", "aux", "packed", "packed_aux", "pix2pt", "kept", "uvr")


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
        util.measured("test_gpu_project_rotated: wall time of the file [s]", time.time() - t0)


@pytest.fixture(autouse=True)
def _needs_a_gpu():
    _dev()


class Run:
    """One projection call laid out in arenas.  scans: list of fp32 [C,n]; scan s owns columns offs[s]..offs[s+1) with offs[0] = offs0,
    n_cols = offs[S] + tail, pts_cs = n_cols + pad.  ``rot``: None -> dl_project; "null" -> dl_project_rotated with rot = NULL; an
    fp32 [S,9] array -> dl_project_rotated with it (a frozen input)."""

    def __init__(self, sen, scans, C, rot=None, offs0=0, tail=0, pad=0):
        from delora_amd import _lib
        self.L, self.lib, self.sen, self.C, self.S = _lib, _lib.load(), sen, C, len(scans)
        dev = _dev()
        S, H, W = self.S, sen.H, sen.W
        lens = [s.shape[1] for s in scans]
        offs = offs0 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        self.offs, self.max_n = offs, max(lens)
        self.n_cols, self.cs = int(offs[-1]) + tail, int(offs[-1]) + tail + pad
        pts = np.full((C, max(self.cs, 1)), np.nan, dtype=np.float32)
        for s, scan in enumerate(scans):
            pts[:, offs[s]:offs[s + 1]] = scan
        self.A, self.Wk = cr.Arenas(dev), cr.Arenas(dev)
        a = lambda shape, dtype, fill, name: self.A.arena(shape, dtype, fill, name, row_elems=0)
        self.pts = a(pts.shape, torch.float32, torch.from_numpy(pts), "pts")
        self.d_offs = a((S + 1,), torch.int32, torch.from_numpy(offs.astype(np.int32)), "offs")
        self.rot_mode = "project" if rot is None else ("null" if isinstance(rot, str) else "rot")
        self.rot = a((S, 9), torch.float32, torch.from_numpy(np.ascontiguousarray(rot, dtype=np.float32)), "rot") if self.rot_mode == "rot" else None
        self.struct = _lib.SensorStruct(H, W, sen.hfov[0], sen.hfov[1], sen.vfov[0], sen.vfov[1])
        self.out = {"image4": a((S, 4, H, W), torch.float32, None, "image4"), "pix2pt": a((S, H, W), torch.int32, None, "pix2pt"),
                    "aux": a((S, C - 3, H, W), torch.float32, None, "aux") if C > 3 else None,
                    "packed": a((S, H, W, 4), torch.float32, None, "packed"),
                    "packed_aux": a((S, H, W, 4), torch.float32, None, "packed_aux") if C >= 6 else None,
                    "kept": a((S,), torch.int32, None, "kept"),
                    "uvr": a((3, max(self.cs, 1)), torch.float32, None, "uvr")}
        nbytes = int(self.lib.dl_project_workspace_bytes(S, H, W, self.n_cols, C))
        assert nbytes == (S * H * W * 8 + 15) // 16 * 16 + self.n_cols * 16 * (2 if C > 3 else 1)
        self.ws = self.Wk.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
        assert self.ws.data_ptr() % 16 == 0

    def poison(self):
        for v in list(self.out.values()) + [self.ws]:
            if v is not None:
                v.view(torch.int32).fill_(POISON)

    def call(self, ws_offset=0, **over):
        o = self.out
        args = [_p(self.pts), self.cs, self.n_cols, _p(self.d_offs), over.get("S", self.S), over.get("C", self.C), self.max_n, ctypes.byref(self.struct),
                _p(o["image4"]), _p(o["aux"]) if "aux" not in over else ctypes.c_void_p(0), _p(o["packed"]), _p(o["packed_aux"]), _p(o["pix2pt"]),
                _p(self.ws, ws_offset), _p(o["kept"]), _p(o["uvr"])]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.rot_mode == "project":
            return self.lib.dl_project(*args, stream)
        return self.lib.dl_project_rotated(*args, _p(self.rot, over.get("rot_offset", 0)), stream)

    def untouched(self, what):
        _sync()
        self.A.check(what)
        self.Wk.check(what)
        for k, v in list(self.out.items()) + [("workspace", self.ws)]:
            if v is not None:
                assert bool((v.view(torch.int32) == POISON).all()), f"{what}: {k} was written by a refused call"

    def run(self, what):
        """Poison, call, check guards / inputs / "every element written"; returns the outputs as numpy arrays."""
        self.poison()
        self.L.check(self.call(), "dl_project" if self.rot_mode == "project" else "dl_project_rotated")
        _sync()
        self.A.check(what)                          # guards intact, and pts / offs / rot hold the bits they were given
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
        got["uvr"] = got["uvr"][:, int(self.offs[0]):int(self.offs[-1])]
        return got


def compare(got, ref, what):
    """Bit equality of every output."""
    assert set(got) == set(ref), (what, sorted(got), sorted(ref))
    for k, g in got.items():
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


LAYOUT = dict(offs0=rr.OFFS0, tail=rr.TAIL_COLS, pad=rr.PAD_COLS)
_PLAIN = {}


def _special_scans(C):
    """A ragged batch of nine scans, two of them the specials of the sensor (-0.0, NaN, inf, exact zeros, subnormals, overflowing
    squares) with aux channels -- and its dl_project result, computed once."""
    if C not in _PLAIN:
        sen = pr.sensor(rr.SENSOR)
        sp = pr.specials(sen)
        scans = [pr.with_aux(x, C, 70 + i) for i, x in enumerate(
            [sp, pr.random_cloud(257, 10.0, 71), np.zeros((3, 0), dtype=np.float32), sp[:, ::-1], pr.random_cloud(1, 1.0, 72),
             pr.random_cloud(3000, 10.0, 73), pr.random_cloud(255, 0.1, 74), pr.random_cloud(256, 100.0, 75), pr.random_cloud(1000, 10.0, 76)])]
        _PLAIN[C] = (scans, Run(sen, scans, C, None, **LAYOUT).run(f"dl_project C={C}"))
    return _PLAIN[C]


# ------------------------------------------------------------------------------------------------ (a), (b): nothing to rotate


@pytest.mark.parametrize("C", [3, 6, 7])
def test_null_rotations_are_dl_project(C):
    scans, ref = _special_scans(C)
    got = Run(pr.sensor(rr.SENSOR), scans, C, "null", **LAYOUT).run(f"rot = NULL, C={C}")
    compare(got, ref, f"rot = NULL, C={C}")


@pytest.mark.parametrize("C", [3, 6, 7])
def test_identity_rotations_are_dl_project(C):
    """Every row the identity: no scan is multiplied, so -0.0, NaN, inf and exact zeros come out as dl_project leaves them."""
    scans, ref = _special_scans(C)
    assert any(np.signbit(s[:3]).any() and np.isnan(s[:3]).any() for s in scans)
    got = Run(pr.sensor(rr.SENSOR), scans, C, np.tile(rr.IDENTITY9, (len(scans), 1)), **LAYOUT).run(f"identity, C={C}")
    compare(got, ref, f"identity, C={C}")


# ------------------------------------------------------------------------------------------------ (c): odd scans rotated


@pytest.mark.parametrize("case", rr.cases(), ids=lambda c: c["name"])
def test_rotated_scans_equal_dl_project_on_prerotated_input(case):
    sen, C, rot = pr.sensor(rr.SENSOR), case["C"], rr.case_rotations(case)
    for layout in case["layouts"]:
        scans = rr.case_scans(case, layout)
        what = f"{case['name']} lengths {[s.shape[1] for s in scans]}"
        ref = Run(sen, rr.rotate_scans(scans, rot), C, None, **LAYOUT).run(what + " (dl_project, pre-rotated)")
        got = Run(sen, scans, C, rot, **LAYOUT).run(what)
        compare(got, ref, what)


@pytest.mark.parametrize("C", [3, 4, 5, 6, 8])
def test_rotated_specials_and_partial_aux_channels(C):
    """The specials rotated (IEEE products and sums of -0.0, inf, NaN and subnormals: numpy's), every C from 3 to 8 around the "whole
    vector" rule: C = 4 and 5 leave channels 3 and 4 alone."""
    sen = pr.sensor(rr.SENSOR)
    scans, _ = _special_scans(8)
    scans = [np.ascontiguousarray(s[:C]) for s in scans]
    assert all(s.shape[0] == C for s in scans)
    rot = np.tile(rr.IDENTITY9, (len(scans), 1))
    for s in (0, 3, 5, 8):
        rot[s] = rr.rodrigues((0.3, 0.5, 0.8), 0.4 * (s + 1)).reshape(9).astype(np.float32)
    ref = Run(sen, rr.rotate_scans(scans, rot), C, None, **LAYOUT).run(f"specials C={C} (dl_project, pre-rotated)")
    got = Run(sen, scans, C, rot, **LAYOUT).run(f"specials C={C}")
    compare(got, ref, f"specials C={C}")


# ------------------------------------------------------------------------------------------------ (d): refusals


def test_refusals_come_before_any_launch():
    scans, _ = _special_scans(6)
    run = Run(pr.sensor(rr.SENSOR), scans, 6, np.tile(rr.IDENTITY9, (len(scans), 1)), **LAYOUT)
    for kw, text in ((dict(ws_offset=4), b"16-byte aligned"), (dict(ws_offset=8), b"16-byte aligned"), (dict(S=0), b"bad sizes"),
                     (dict(C=2), b"bad sizes"), (dict(aux=None), b"needs an aux image"), (dict(C=5), b"packed_aux needs C >= 6"),
                     (dict(rot_offset=2), b"rot must be 4-byte aligned")):
        run.poison()
        assert run.call(**kw) == INVALID
        err = run.lib.dl_last_error()
        assert err.startswith(b"dl_project_rotated:") and text in err, (kw, err)
        run.untouched(f"refused {kw}")


# ------------------------------------------------------------------------------------------------ dl_rotations_from_draws


@pytest.mark.parametrize("only_yaw", [False, True])
@pytest.mark.parametrize("magnitude_deg", [4.0, 90.0, 360.0])
def test_rotations_from_draws(only_yaw, magnitude_deg):
    """Identity rows exact; the others within 1e-6 absolute of the float64 reference: a dozen fp32 operations on values <= 1 and
    sinf / cosf at a few ulp, 2^-24 ~ 6e-8 each.  B = 300: more than one workgroup, the last one ragged."""
    from delora_amd import _lib
    lib, dev, B, mag = _lib.load(), _dev(), 300, float(np.deg2rad(magnitude_deg))
    d = np.random.default_rng(int(magnitude_deg) + only_yaw).random((B, 4), dtype=np.float32)
    d[5, 3] = 0.5                                                   # angle 0
    d[6, :3] = 0.0                                                  # no axis
    d[7, :3] = (0.0, 0.0, 0.25)
    A = cr.Arenas(dev)
    draws = A.arena((B, 4), torch.float32, torch.from_numpy(d), "draws", row_elems=0)
    rot = A.arena((2 * B, 9), torch.float32, None, "rot", row_elems=0)
    _lib.check(lib.dl_rotations_from_draws(_p(draws), B, int(only_yaw), mag, _p(rot), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "dl_rotations_from_draws")
    _sync()
    A.check("dl_rotations_from_draws")
    assert int((rot.view(torch.int32) == POISON).sum()) == 0
    got = rot.cpu().numpy().reshape(B, 2, 9)
    eye = rr.IDENTITY9.view(np.uint32)
    assert all(np.array_equal(got[b, 0].view(np.uint32), eye) for b in range(B)), "scan 1 rows must be the exact identity"
    assert np.array_equal(got[5, 1].view(np.uint32), eye), "angle 0 must give the exact identity"
    if only_yaw:
        G = got[:, 1].reshape(B, 3, 3)
        for sl in (G[:, 2, :], G[:, :, 2]):
            assert np.array_equal(sl.view(np.uint32), np.broadcast_to(np.array([0.0, 0.0, 1.0], dtype=np.float32).view(np.uint32), (B, 3)))
    else:
        assert np.array_equal(got[6, 1].view(np.uint32), eye)
    ref = rr.rotations_from_draws(d, only_yaw, mag).reshape(B, 2, 9)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"[measured] dl_rotations_from_draws only_yaw={only_yaw} magnitude={magnitude_deg}: largest |entry - float64 reference| = {err:.3g}")
    assert err <= 1e-6, err
    # and through the package's wrapper: the same bits
    from delora_amd import geometry
    again = geometry.rotations_from_draws(draws, only_yaw, mag)
    assert again.shape == (2 * B, 9) and torch.equal(again.view(torch.int32), rot.view(torch.int32))


def test_wrapper_passes_rotations_through():
    """geometry.project(rotations=...) binds dl_project_rotated: equal to geometry.project on the pre-rotated points, [S,9] and
    [S,3,3] alike; a wrong row count is refused in Python."""
    from delora_amd import geometry
    dev, sen_r = _dev(), pr.sensor(rr.SENSOR)
    case = [c for c in rr.cases() if c["name"] == "C6-S9-general-2"][0]
    scans, rot = rr.case_scans(case, case["layouts"][0]), rr.case_rotations(case)
    sensor = geometry.Sensor(sen_r.H, sen_r.W, sen_r.vfov, sen_r.hfov)
    offs = torch.tensor(np.concatenate([[0], np.cumsum([s.shape[1] for s in scans])]), dtype=torch.int32, device=dev)
    mx = max(s.shape[1] for s in scans)
    pts = torch.from_numpy(np.concatenate(scans, axis=1)).to(dev)
    pre = torch.from_numpy(np.concatenate(rr.rotate_scans(scans, rot), axis=1)).to(dev)
    keep = pts.clone()
    want = geometry.project(pre, offs, mx, sensor, want_uv=True)
    for r in (torch.from_numpy(rot).to(dev), torch.from_numpy(rot).to(dev).view(-1, 3, 3)):
        got = geometry.project(pts, offs, mx, sensor, want_uv=True, rotations=r)
        for k, v in want.items():
            assert v is not None and np.array_equal(_bits(got[k].cpu().numpy()), _bits(v.cpu().numpy())), k
    assert torch.equal(pts.view(torch.int32), keep.view(torch.int32))
    with pytest.raises(ValueError, match="rotations"):
        geometry.project(pts, offs, mx, sensor, rotations=torch.from_numpy(rot[:-1].copy()).to(dev))
