"""dl_reproject against the reference of its contract (tests/reproject_ref.py), BIT FOR BIT: there is no tolerance anywhere in this file.
The C ABI is called directly; every pointer is a view inside a tests/conv_ref.Arenas allocation: the source image, normals, matches,
nn_pix and poses are frozen inputs laid out with scan strides larger than dense (the gaps hold NaN), every output and the workspace
are poisoned, and the workspace is exactly dl_reproject_workspace_bytes long -- a write beside a buffer, an element never written and
a promise that is too small all show.  "Written" means: no element still holds the arena's poison word.

Sensors, poses and planted collisions are those of tests/reproject_ref.py; tests/test_reproject_ref_host.py proves on the host that
each of a list of plausible defects is told from the reference by at least one of the cases."""
import ctypes

import numpy as np
import pytest
import torch

from tests import conv_ref as cr
from tests import reproject_ref as rr

pytestmark = pytest.mark.gpu

INVALID = -1                                           # DL_ERR_INVALID_ARGUMENT
POISON = cr._as_i32(cr.NAN_WORD[torch.float32])
GAPS = (5, 3, 7)                                       # elements between two samples of src / srcn / match


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
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


@pytest.fixture(autouse=True)
def _needs_a_gpu():
    _dev()


def _strided(a, gap):
    """[B, ...] -> ([B, dense + gap] with NaN in the gaps, stride)."""
    B = a.shape[0]
    flat = a.reshape(B, -1)
    out = np.full((B, flat.shape[1] + gap), np.nan, dtype=np.float32)
    out[:, :flat.shape[1]] = flat
    return out, flat.shape[1] + gap


class Run:
    """One dl_reproject call laid out in arenas.  ``null`` names what is passed as NULL: "paired9", "src_pix", "pairs" (src_normals,
    match and nn_pix together)."""

    def __init__(self, c, null=(), T=None, skew=0):
        from delora_amd import _lib
        self.L, self.lib, self.c, self.null = _lib, _lib.load(), c, tuple(null)
        dev, sen, B = _dev(), c["sen"], c["B"]
        H, W = sen.H, sen.W
        self.B, self.H, self.W = B, H, W
        self.A, self.Wk = cr.Arenas(dev, skew), cr.Arenas(dev, skew)
        a = lambda shape, dtype, fill, name: self.A.arena(shape, dtype, fill, name, row_elems=0)
        src, self.src_ss = _strided(c["src"], GAPS[0])
        srcn, self.srcn_ss = _strided(c["srcn"], GAPS[1])
        match, self.match_ss = _strided(c["match"], GAPS[2])
        self.src = a(src.shape, torch.float32, torch.from_numpy(src), "src_image4")
        pairs = "pairs" not in null
        self.srcn = a(srcn.shape, torch.float32, torch.from_numpy(srcn), "src_normals") if pairs else None
        self.match = a(match.shape, torch.float32, torch.from_numpy(match), "match") if pairs else None
        self.nn = a((B, H, W), torch.int32, torch.from_numpy(np.array(c["nn"])), "nn_pix") if pairs else None
        self.T = a((B, 4, 4), torch.float32, torch.from_numpy(np.array(c["T"] if T is None else T)), "T")
        self.struct = _lib.SensorStruct(H, W, sen.hfov[0], sen.hfov[1], sen.vfov[0], sen.vfov[1])
        self.out = {"moved4": a((B, 4, H, W), torch.float32, None, "moved4"),
                    "paired9": a((B, 9, H, W), torch.float32, None, "paired9") if "paired9" not in null else None,
                    "src_pix": a((B, 2, H, W), torch.int32, None, "src_pix") if "src_pix" not in null else None}
        nbytes = int(self.lib.dl_reproject_workspace_bytes(B, H, W))
        assert nbytes == (B * 2 * H * W * 8 + 15) // 16 * 16
        self.ws = self.Wk.arena((nbytes // 4,), torch.float32, None, "workspace", row_elems=0)
        assert self.ws.data_ptr() % 16 == 0

    def poison(self):
        for v in list(self.out.values()) + [self.ws]:
            if v is not None:
                v.view(torch.int32).fill_(POISON)

    def call(self, ws_offset=0, **over):
        o = self.out
        args = dict(src=_p(self.src), src_ss=self.src_ss, srcn=_p(self.srcn), srcn_ss=self.srcn_ss, match=_p(self.match), match_ss=self.match_ss,
                    nn=_p(self.nn), T=_p(self.T), B=self.B, sensor=self.struct, moved4=_p(o["moved4"]), paired9=_p(o["paired9"]),
                    src_pix=_p(o["src_pix"]), ws=_p(self.ws, ws_offset))
        args.update(over)
        return self.lib.dl_reproject(args["src"], args["src_ss"], args["srcn"], args["srcn_ss"], args["match"], args["match_ss"], args["nn"],
                                     args["T"], args["B"], ctypes.byref(args["sensor"]), args["moved4"], args["paired9"], args["src_pix"],
                                     args["ws"], ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    def still_poisoned(self, what):
        _sync()
        self.A.check(what)
        self.Wk.check(what)
        for k, v in list(self.out.items()) + [("workspace", self.ws)]:
            if v is not None:
                assert bool((v.view(torch.int32) == POISON).all()), f"{what}: {k} was written by a refused call"

    def run(self, what):
        """Poison, call, check guards / inputs / "every element written"; returns the outputs as numpy arrays."""
        self.poison()
        self.L.check(self.call(), "dl_reproject")
        _sync()
        self.A.check(what)
        self.Wk.check(what)
        got = {}
        for k, v in self.out.items():
            if v is None:
                continue
            n = int((v.view(torch.int32) == POISON).sum())
            assert n == 0, f"{what}: {n} elements of {k} were never written"
            got[k] = v.cpu().numpy()
        return got


def compare(got, ref, what):
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


# ------------------------------------------------------------------------------------------------ every case, every output


@pytest.mark.parametrize("name", list(rr.CASES))
def test_every_output_bitwise(name):
    """Sensors min (2x2), odd (5x9: odd key planes), ragged (16x130: H*W % 256 != 0), flipped, kitti (64x720); B = 1, 3 and 9 (the
    scan-to-XCD mapping with a ghost group); identity, trained-regime, large, emptying and NaN poses; twins, shadowed pairs, -0.0."""
    c = rr.case(name)
    assert rr.REDRAWS[name] <= rr.MAX_REDRAWS
    got = Run(c).run(name)
    assert set(got) == {"moved4", "paired9", "src_pix"}
    compare(got, c["ref"], name)


def test_identity_gives_back_the_source_image():
    c = rr.case("ragged-identity")
    got = Run(c).run("identity")
    sp = got["src_pix"][0, 0].reshape(-1)
    own = sp == np.arange(sp.size)
    assert own.sum() >= 0.9 * (sp >= 0).sum()
    a, b = np.array(c["src"][0]).reshape(4, -1)[:, own], got["moved4"][0].reshape(4, -1)[:, own]
    differ = _bits(a) != _bits(b)
    assert np.array_equal(a, b) and (not differ.any() or (np.signbit(a[differ]).all() and (a[differ] == 0).all() and not np.signbit(b[differ]).any()))


def test_a_nan_pose_stays_in_its_sample():
    c = rr.case(rr.NAN_CASE)
    with_nan = Run(c).run("nan pose")
    T = np.array(c["T"])
    T[rr.NAN_SAMPLE] = np.eye(4, dtype=np.float32)
    without = Run(c, T=T).run("finite pose instead")
    for b in range(c["B"]):
        if b == rr.NAN_SAMPLE:
            assert not with_nan["moved4"][b].any() and not with_nan["paired9"][b].any() and (with_nan["src_pix"][b] == -1).all()
            assert without["moved4"][b].any()
            continue
        for k in with_nan:
            assert np.array_equal(_bits(with_nan[k][b]), _bits(without[k][b])), (k, b)


def test_a_sample_alone_equals_the_sample_in_its_batch():
    c = rr.case("ragged-mixed-B9")
    batch = Run(c).run("batch of 9")
    for b in (0, 2, 8):
        one = dict(c, B=1, src=c["src"][b:b + 1], srcn=c["srcn"][b:b + 1], match=c["match"][b:b + 1], nn=c["nn"][b:b + 1], T=c["T"][b:b + 1])
        alone = Run(one).run(f"sample {b} alone")
        for k in alone:
            assert np.array_equal(_bits(alone[k][0]), _bits(batch[k][b])), (k, b)


# ------------------------------------------------------------------------------------------------ NULL combinations


@pytest.mark.parametrize("name", ["odd-small-B3", "ragged-rotation"])
@pytest.mark.parametrize("null", [("paired9",), ("src_pix",), ("paired9", "src_pix"), ("pairs", "paired9"), ("pairs", "paired9", "src_pix")],
                         ids=lambda n: "+".join(n))
def test_null_combinations(name, null):
    c = rr.case(name)
    ref = dict(c["ref"])
    if "paired9" in null:
        ref["src_pix"] = np.array(ref["src_pix"])
        ref["src_pix"][:, 1] = -1                                       # plane 1 is still written: all -1
    got = Run(c, null=null).run(f"{name} null={null}")
    assert set(got) == {"moved4", "paired9", "src_pix"} - set(null)
    compare(got, ref, f"{name} null={null}")


# ------------------------------------------------------------------------------------------------ refusals


def test_documented_refusals_write_nothing():
    c = rr.case("ragged-small")
    run = Run(c)
    HW, N = run.H * run.W, ctypes.c_void_p(0)
    from delora_amd import _lib
    refusals = [({"ws_offset": 4}, b"16-byte aligned"), ({"ws_offset": 8}, b"16-byte aligned"),
                ({"src": N}, b"null pointer"), ({"T": N}, b"null pointer"), ({"moved4": N}, b"null pointer"), ({"ws": N}, b"null pointer"),
                ({"B": 0}, b"B=0"), ({"sensor": _lib.SensorStruct(1, run.W, -3.1, 3.1, -0.4, 0.03)}, b"H=1"),
                ({"srcn": N}, b"only together"), ({"match": N}, b"only together"), ({"nn": N}, b"only together"),
                ({"srcn": N, "match": N, "nn": N}, b"paired9 needs"),
                ({"src_ss": 3 * HW - 1}, b"src_ss="), ({"srcn_ss": 3 * HW - 1}, b"srcn_ss="), ({"match_ss": 6 * HW - 1}, b"match_ss=")]
    for kw, text in refusals:
        run.poison()
        assert run.call(**kw) == INVALID, kw
        assert text in run.lib.dl_last_error(), (kw, run.lib.dl_last_error())
        run.still_poisoned(f"refused call {kw}")
