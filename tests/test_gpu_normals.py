"""The normals kernel (csrc/normals.hip through geometry.normals) against a per-pixel float64 reference (tests/normals_ref.py):
every pixel of every case, both instantiations (<3,5> and the generic one), the three eigen solves, every window the entry point
accepts, the exact gate / validity / clamping rules, degenerate neighbourhoods, non-finite input, scale and layout.

Assertions of every case (check_case):
  * has-normal mask equal to the reference on every non-ambiguous pixel (zero vector exactly where the reference has none); the
    ambiguous share (normals_ref.reference) is itself bounded by 0.2 %, and is zero on planted cases;
  * angle to the float64 normal <= 2e-4 + 50 eps32 / gap at EVERY pixel with a normal on both sides (the project's conditioning bound
    of check_normals, gap from the float64 eigenvalues).  The sign is ignored where the reference normal grazes the line of sight,
    |n.p| / |p| < 1e-3 as in check_normals, AND -- wider than that rule, which was written for a statistical comparison -- where it is
    closer to grazing than the angle bound of that pixel (gaps below ~4e-3; every pixel once the gap is below ~2e-6): a normal
    within the bound may then lie across the grazing plane and has to point the other way, because n.p <= 0 is asserted on its own;
  * Rayleigh excess (n^T A64 n - l0) / lmax <= normals_ref.rayleigh_bound(...): 10 x the larger of the worst excess of the
    fp32-moment model on that case (moment_model32 against reference, no kernel involved) and eps32^2 / NRM_FP32_GAP = 3.6e-12, i.e.
    3.6e-11 on every case but those with gaps near 1e-6 and below -- the check that still bites where the gap is below 1e-3 and the
    angle bound says little;
  * | |n| - 1 | <= 1e-5 and n.p <= 0 (up to the fp32 rounding of the stored components) wherever a normal is given.
The pixels whose window duplicates clamped edges (first / last a rows, b columns) are asserted as a group of their own.

Coverage of the eigen solves: the fp32 solve (gap >= NRM_FP32_GAP) on every scan; the fp64 solve started at the LARGEST eigenvalue on
thin poles, collinear runs and the few hundred thin structures of every scan; the fp64 solve started at the SMALLEST eigenvalue
(all three eigenvalues within 1e-3) on the near-isotropic clouds.  In the fp64 solve the choice of the adjugate column that starts
the Rayleigh iteration is NOT pinned by any test, and cannot be: every column is a multiple of the same eigenvector up to
rounding, two cubic steps repair a poor one, and whichever eigenvector the iteration reaches, the 2x2 problem in the plane
perpendicular to it plus the comparison of Rayleigh quotients gives the smallest one -- a build that takes the second-largest
column passes every case here with figures equal to within rounding.
"""
import numpy as np
import pytest
import torch

from tests import normals_ref as R
from tests import util

pytestmark = pytest.mark.gpu

_REF = {}
_GOT = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def run(img, a, b, eps, min_n, **kw):
    """geometry.normals on a numpy image [3,H,W] or batch [S,3,H,W] -> numpy of the same rank."""
    from delora_amd import geometry
    t = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).to(_dev())
    single = t.dim() == 3
    out = geometry.normals(t[None] if single else t, a, b, float(eps), int(min_n), **kw)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return out[0] if single else out


def _first(mask):
    v, u = np.argwhere(mask)[0]
    return f"{int(mask.sum())} pixels, first at (v={int(v)}, u={int(u)})"


def check_case(name, img, got, a, b, eps, min_n, planted=False, exact_ranges=False, ref=None):
    """Every assertion of the module's docstring for one image; returns the reference."""
    ref = ref if ref is not None else R.reference(img, a, b, eps, min_n, exact_ranges=exact_ranges)
    H, W = ref["has"].shape
    amb, valid = ref["ambiguous"], ref["valid"]
    share = amb.sum() / max(1, int(valid.sum()))
    util.measured(f"normals {name}: ambiguous share", share, bound=0.0 if planted else R.AMBIGUOUS_SHARE_CAP)
    assert np.all(np.isfinite(got)), f"{name}: non-finite output"
    got_has = np.any(got != 0, axis=0)
    border = R.border_mask(H, W, a, b)
    both = got_has & ref["has"] & ~amb
    gap = ref["gap"]
    ratio = np.where(both, R.angle_to_reference(got, ref) / R.angle_bound(gap), 0.0)
    solved = both & (ref["evals"][2] > 0)
    excess = np.where(solved, R.rayleigh_excess(got, ref), 0.0)
    mod = R.moment_model32(img, a, b, eps, min_n)
    assert np.array_equal(mod["has"], ref["has"])
    model_excess = float(np.where(ref["has"], R.rayleigh_excess(mod["normal"], ref), 0.0).max())
    rbound = R.rayleigh_bound(model_excess)
    p = ref["image"].astype(np.float64)
    g64 = got.astype(np.float64)
    norm_err = np.where(got_has, np.abs(np.linalg.norm(g64, axis=0) - 1.0), 0.0)
    # n.p <= 0 is decided on the fp64 normal, which is then rounded to fp32: half an ulp per component may remain
    facing = np.where(got_has, np.sum(g64 * p, axis=0) - 1.001 * 2.0 ** -24 * np.sum(np.abs(g64 * p), axis=0), 0.0)
    for group, m in (("pixels with clamped (duplicated) neighbours", border), ("interior pixels", ~border)):
        bad = (got_has != ref["has"]) & ~amb & m
        assert not bad.any(), f"{name}, {group}: has-normal mask differs from the reference: {_first(bad)}; N there {ref['N'][bad][:4]}"
        bad = (ratio > 1.0) & m
        assert not bad.any(), (f"{name}, {group}: angle beyond 2e-4 + 50 eps32 / gap: {_first(bad)}; worst ratio {ratio[m].max():.3g} "
                               f"at gap {gap[m].reshape(-1)[np.argmax(ratio[m])]:.3g}")
        bad = (excess > rbound) & m
        assert not bad.any(), (f"{name}, {group}: Rayleigh excess beyond {rbound:.3g}: {_first(bad)}; worst {excess[m].max():.3g} "
                               f"at gap {gap[m].reshape(-1)[np.argmax(excess[m])]:.3g}")
        bad = (norm_err > 1e-5) & m
        assert not bad.any(), f"{name}, {group}: normal not of unit length: {_first(bad)}"
        bad = (facing > 0.0) & m
        assert not bad.any(), f"{name}, {group}: normal faces away from the sensor: {_first(bad)}"
    util.measured(f"normals {name}: worst angle / (2e-4 + 50 eps32 / gap)", ratio.max(), bound=1.0)
    util.measured(f"normals {name}: worst Rayleigh excess", excess.max(), bound=rbound)
    return ref


_CASES = {c[0]: c for c in R.natural_cases()}


def _natural(name):
    """Run (once per session) and check a case of normals_ref.natural_cases(); returns (image, output, reference)."""
    if name not in _GOT:
        _, build, a, b, eps, min_n = _CASES[name]
        img = build()
        got = run(img, a, b, eps, min_n)
        _REF[name] = check_case(name, img, got, a, b, eps, min_n)
        _GOT[name] = (img, got)
    return _GOT[name][0], _GOT[name][1], _REF[name]


# --------------------------------------------------------------------------------------------------- scenes and shapes
@pytest.mark.parametrize("name", ["64x720 7x11", "64x2048 7x11"])
def test_scan_7x11(name):
    _natural(name)


def test_min_neighbors_boundary_is_exercised_on_the_64x720_scan():
    """N == min_n gives a normal, N == min_n - 1 none: both sets are populated (N from the reference, non-ambiguous pixels)."""
    img, got, ref = _natural("64x720 7x11")
    sel = ref["valid"] & ~ref["ambiguous"]
    at, below = sel & (ref["N"] == 10), sel & (ref["N"] == 9)
    assert at.sum() > 20 and below.sum() > 20
    has = np.any(got != 0, axis=0)
    assert has[at].all() and not has[below].any()
    gap = ref["gap"][ref["has"]]
    assert (gap < R.NRM_FP32_GAP).sum() > 100 and (gap >= R.NRM_FP32_GAP).sum() > 10000     # both eigen solves at work


def test_batch_of_three_128x256_scans():
    names = [n for n in R.SCENES if n.startswith("128x256")]
    imgs = np.stack([R.scene(n) for n in names])
    got = run(imgs, 3, 5, 0.5, 10)
    for s, n in enumerate(names):
        check_case(f"{n} 7x11 (in a batch of 3)", imgs[s], got[s], 3, 5, 0.5, 10)


@pytest.mark.parametrize("shape", R.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_images_partial_tiles_and_images_smaller_than_the_window(shape):
    H, W = shape
    img, got, ref = _natural(f"small {H}x{W} 7x11")
    assert ref["valid"].sum() > 0
    if H * W >= 64:
        assert ref["has"].sum() > 0


# --------------------------------------------------------------------------------------------------------- windows
@pytest.mark.parametrize("window", R.GENERIC_WINDOWS, ids=lambda w: f"a{w[0]}b{w[1]}")
def test_windows_through_the_generic_instantiation(window):
    """Every window class: no row pairs (a = 0), no column pairs (b = 0), the single tap, odd ones, the largest that fits 64 KiB of
    LDS (15,28) and the two above it -- (15,29) and (15,31) ask for 66 368 and 68 544 B, which dl_normals has to be granted."""
    a, b = window
    for scene in ("64x720", "small 16x130"):
        img, got, ref = _natural(f"{scene} window ({a},{b})")
        if (a, b) == (0, 0):
            assert not np.any(got != 0)                  # one neighbour (the centre itself) is below any min_neighbors >= 2
        else:
            assert ref["has"].sum() > 0.5 * ref["valid"].sum()


def test_entry_point_refuses_windows_outside_its_documented_range():
    from delora_amd import _lib, geometry
    t = torch.zeros((1, 3, 8, 70), device=_dev())
    for a, b in ((16, 5), (3, 32), (-1, 5), (3, -1)):
        with pytest.raises(_lib.DeloraHipError):
            geometry.normals(t, a, b, 0.5, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- exact rules
def test_exact_gate_equality_keeps_the_neighbour():
    """Integer triples times k on a 1/8 grid: every range is exact, neighbours sit exactly at eps and one step (1/8) beyond; the mask
    must equal the reference on EVERY pixel, and must depend on the neighbours at eps (min_n is placed inside the counts)."""
    img, eps = R.gate_image()
    assert R.ranges_are_exact(img)
    min_n = 30
    got = run(img, 3, 5, eps, min_n)
    ref = check_case("exact gate", img, got, 3, 5, eps, min_n, planted=True, exact_ranges=True)
    strict = R.reference(img, 3, 5, float(eps) - 2.0 ** -20, min_n, exact_ranges=True)       # what dropping the neighbours at eps would give
    only_by_equality = ref["has"] & ~strict["has"]
    assert only_by_equality.sum() > 10 and ref["has"].sum() > 100 and (~ref["has"] & ref["valid"]).sum() > 100
    assert np.any(got != 0, axis=0)[only_by_equality].all()
    # one step beyond is dropped: a gate 1/8 wider gives other counts, and the kernel follows the reference there as well
    wide = float(eps) + 0.125
    got_w = run(img, 3, 5, wide, min_n)
    ref_w = check_case("exact gate, eps one step wider", img, got_w, 3, 5, wide, min_n, planted=True, exact_ranges=True)
    assert (ref_w["has"] & ~ref["has"]).sum() > 10


def test_centre_validity_is_and_neighbour_presence_is_or():
    """A column of points with exactly one zero coordinate: no normal there, yet they count as neighbours of the columns around."""
    img = R.small_image(16, 130)
    u0 = int(np.argmin(np.abs(img[1]).max(axis=0)))      # where y is smallest: zeroing it leaves the range (and the gate) as it was
    planted = img.copy()
    occupied = np.any(img[:, :, u0] != 0, axis=0)
    planted[1, :, u0] = 0.0
    assert occupied.sum() >= 12 and np.abs(img[1, :, u0]).max() < 0.05
    got = run(planted, 3, 5, 0.5, 10)
    ref = check_case("zero-coordinate column", planted, got, 3, 5, 0.5, 10)
    assert not ref["valid"][:, u0].any() and not np.any(got[:, :, u0] != 0)
    emptied = img.copy()
    emptied[:, :, u0] = 0.0
    other = R.reference(emptied, 3, 5, 0.5, 10)
    near = slice(u0 - 5, u0 + 6)
    assert (ref["N"][:, near] > other["N"][:, near]).sum() > 100          # the reference counts those points
    differs = R.angle(ref["normal"], other["normal"])[:, near] > 10 * R.angle_bound(ref["gap"][:, near])
    assert differs.sum() > 20                              # ... and a kernel that skipped them would be outside the bound


# -------------------------------------------------------------------------------------------- degenerate neighbourhoods
def test_collinear_windows_rank_one():
    img, dirs = R.collinear_image()
    got = run(img, 3, 5, 100.0, 5)
    ref = check_case("collinear runs (rank 1)", img, got, 3, 5, 100.0, 5, planted=True)
    rows = np.nonzero(np.any(dirs != 0, axis=1))[0]
    assert ref["has"][rows].all() and (ref["evals"][1][rows] <= 1e-12 * ref["evals"][2][rows]).all()
    worst = 0.0
    for r in rows:
        d = dirs[r] / np.linalg.norm(dirs[r])
        n = got[:, r].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(n, axis=0) - 1.0) <= 1e-5)
        assert np.all(np.sum(n * img[:, r].astype(np.float64), axis=0) <= 0)
        worst = max(worst, float(np.abs(d @ n).max()))
    util.measured("normals collinear runs: worst |n . line direction|", worst, bound=1e-6)


def test_identical_neighbours_rank_zero():
    img = R.constant_image()
    got = run(img, 3, 5, 0.5, 10)
    ref = check_case("identical neighbours (rank 0)", img, got, 3, 5, 0.5, 10, planted=True)
    assert ref["has"].all() and np.all(ref["evals"] == 0)
    n = got.astype(np.float64)
    assert np.all(np.isfinite(n)) and np.all(np.abs(np.linalg.norm(n, axis=0) - 1.0) <= 1e-5)
    assert np.all(np.sum(n * img, axis=0) <= 0)


def test_thin_poles_fp64_branch_and_both_sides_of_the_fp32_threshold():
    img = R.thin_pole_image()
    got = run(img, 3, 5, 100.0, 5)
    ref = check_case("thin poles", img, got, 3, 5, 100.0, 5, planted=True)
    gap = ref["gap"][ref["has"]]
    T = R.NRM_FP32_GAP
    assert ((gap >= 1e-6) & (gap < T)).sum() > 300                               # the fp64 Rayleigh iteration
    assert ((gap >= 0.8 * T) & (gap < T)).sum() >= 5 and ((gap >= T) & (gap < 1.25 * T)).sum() >= 5
    assert (gap < 1e-6).sum() > 50 and (gap > 2 * T).sum() > 50


def test_near_isotropic_clouds_fp64_branch_started_at_the_smallest_eigenvalue():
    """All three eigenvalues within 1e-3 (relative), the smallest the better separated: the one class of pixels whose fp64 solve starts
    at the smallest eigenvalue.  The angle bound says little at these gaps; the Rayleigh excess decides (a wrong eigenvector misses by
    the gap: 8e-6 .. 2e-3 here, against a bound of 10 x what fp32 moments cost on this case)."""
    img = R.isotropic_image()
    got = run(img, 0, 3, 100.0, 5)
    ref = check_case("near-isotropic clouds", img, got, 0, 3, 100.0, 5, planted=True)
    ev = ref["evals"]
    tr = np.where(ref["has"], ev.sum(axis=0), 1.0)       # the kernel's threshold is on gaps in units of the trace
    low, top = (ev[1] - ev[0]) / tr, (ev[2] - ev[1]) / tr
    cls = ref["has"] & (low < R.NRM_FP32_GAP) & (top <= low)
    assert ref["has"].all() and all(cls[row].sum() >= 40 for row in range(img.shape[1]))      # every delta is represented


# ---------------------------------------------------------------------------------------------------- non-finite input
def test_infinite_coordinate_is_an_empty_pixel():
    img = R.small_image(16, 130)
    v0, u0 = 8, 70
    assert np.all(img[:, v0, u0] != 0)
    emptied = img.copy()
    emptied[:, v0, u0] = 0.0
    base = run(emptied, 3, 5, 0.5, 10)
    for c, val in ((0, np.inf), (2, -np.inf)):
        bad = img.copy()
        bad[c, v0, u0] = val
        got = run(bad, 3, 5, 0.5, 10)
        assert np.array_equal(got.view(np.uint32), base.view(np.uint32))
        check_case(f"infinite coordinate (plane {c})", bad, got, 3, 5, 0.5, 10)


def test_nan_pixel_stays_inside_its_window():
    """NaN passes the gate (as in the reference implementation) and poisons the covariance of the pixels whose window holds it; they
    hold a finite unit vector along x today (the solve's answer to a covariance without a positive trace), or no normal -- never a
    NaN -- and every other pixel is bit-identical to the run without the NaN."""
    img = R.small_image(16, 130)
    v0, u0, a, b = 8, 50, 3, 5                          # away from the range steps: whether the gate sees the pixel changes no count
    base = run(img, a, b, 0.5, 10)
    bad = img.copy()
    bad[1, v0, u0] = np.nan
    got = run(bad, a, b, 0.5, 10)
    vv, uu = np.meshgrid(np.arange(16), np.arange(130), indexing="ij")
    inside = (np.abs(vv - v0) <= a) & (np.abs(uu - u0) <= b)
    assert np.array_equal(got[:, ~inside].view(np.uint32), base[:, ~inside].view(np.uint32))
    assert np.all(np.isfinite(got))
    g = got[:, inside]
    given = np.any(g != 0, axis=0)
    assert np.all(np.abs(g[0, given]) == 1.0) and np.all(g[1:, given] == 0.0)
    assert np.array_equal(given, np.any(base[:, inside] != 0, axis=0))          # the counts do not see the NaN


# -------------------------------------------------------------------------------------------------------------- scale
@pytest.mark.parametrize("label", [s[1] for s in R.SCALES])
def test_scaled_scan(label):
    """The 64x720 scan and eps times a power of two, against the reference at that scale; the count of pixels whose bits differ from
    the unscaled run is recorded (every operation of the kernel but the closed-form shift's thresholds scales exactly)."""
    _, got, _ = _natural(f"64x720 scaled by {label}")
    _, base, _ = _natural("64x720 7x11")
    differ = np.any(got.view(np.uint32) != base.view(np.uint32), axis=0)
    util.measured(f"normals 64x720 scaled by {label}: pixels that differ bitwise from the unscaled run", int(differ.sum()))


def test_wall_at_150_m_with_millimetre_relief():
    _, _, ref = _natural("wall at 150 m, mm relief")
    assert ref["has"].all()


# ------------------------------------------------------------------------------------------------------------- layout
def test_layout_strided_batch_packed_twin_and_determinism():
    from delora_amd import geometry
    dev = _dev()
    names = [n for n in R.SCENES if n.startswith("128x256")]
    imgs = np.stack([R.scene(n) for n in names])
    t = torch.from_numpy(imgs).to(dev)
    planar, packed = geometry.normals(t, want_packed=True)
    again = geometry.normals(t)
    assert torch.equal(planar, again)                                           # two runs are bit-identical
    assert torch.equal(packed[..., :3], planar.permute(0, 2, 3, 1)) and torch.all(packed[..., 3] == 0)
    for s in range(3):                                                          # a sample alone == the same sample in the batch
        assert torch.equal(geometry.normals(t[s:s + 1])[0], planar[s])
    big = torch.full((3, 7, 128, 256), float("nan"), device=dev)                # a view into a larger buffer: scan stride 7 planes
    big[:, 2:5] = t
    view = big[:, 2:5]
    assert not view.is_contiguous()
    assert torch.equal(geometry.normals(view), planar)
    other = geometry.normals(t, 2, 3, 0.5, 5, want_packed=True)                 # the generic instantiation's packed twin
    assert torch.equal(other[1][..., :3], other[0].permute(0, 2, 3, 1)) and torch.all(other[1][..., 3] == 0)
    torch.cuda.synchronize()
