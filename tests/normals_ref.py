"""Float64 per-pixel reference of the normals kernel (delora_amd/csrc/normals.hip), numpy only -- no GPU, no torch maths.

`reference` restates the contract of include/delora_hip.h (dl_normals) pixel by pixel:
  * a pixel is a valid centre iff x != 0 && y != 0 && z != 0; a neighbour is present iff any component != 0;
  * the window is (2a+1) x (2b+1) with CLAMPED coordinates (edge pixels are duplicated, no wrap);
  * a present neighbour is dropped iff |range - centre range| > eps, on fp32 ranges with an fp32 eps (equality keeps it);
  * a point with an infinite range is an empty pixel;
  * N >= min_neighbors present neighbours are needed;
  * the normal is the eigenvector of the smallest eigenvalue of the covariance about the mean, flipped so that n.p <= 0.
Moments are taken about the centre pixel in float64 from the fp32 data, the eigen solve is numpy.linalg.eigh in float64.

`moment_model32` is the same computation with the differences, products and running sums in fp32 (solved in float64): the error
that fp32 moments alone cause, against which the tolerances of tests/test_gpu_normals.py are sized.
"""
import numpy as np

EPS32 = 6e-8                 # the fp32 unit roundoff as the project's conditioning bound writes it (check_normals)
NRM_FP32_GAP = 1e-3          # normals.hip: relative gap above which the kernel takes its fp32 eigenvector
AMBIGUOUS_ULPS = 8           # gate decisions within this many ulp of the centre range are not decisive (see reference())
AMBIGUOUS_SHARE_CAP = 2e-3   # a case whose ambiguous share exceeds this says too little

# Floor of the bound on the kernel's Rayleigh excess (n^T A n - lambda_0) / lambda_max: eps32^2 / NRM_FP32_GAP -- the angle error
# eps32 / gap that normals.hip documents for its fp32 eigen solve, squared and multiplied by the gap, at the smallest gap that solve
# is used for.
RAYLEIGH_FLOOR = EPS32 ** 2 / NRM_FP32_GAP
RAYLEIGH_MARGIN = 10.0       # for another summation order than the model's and the fp32 rounding of the output


def rayleigh_bound(model_worst_excess):
    """Bound of the kernel's Rayleigh excess on a case: RAYLEIGH_MARGIN x the larger of (a) the worst excess fp32 moments alone cause
    on that case (moment_model32 against reference: no kernel involved) and (b) RAYLEIGH_FLOOR.  3.6e-11 wherever the model stays
    below the floor; it grows only on cases that hold pixels with a relative gap of ~1e-6 and less, where an fp32 rounding of the
    moments (~eps32 of lambda_max) turns the eigenvector by eps32 / gap and costs eps32^2 / gap.  A wrong eigenvector misses by about
    the gap itself."""
    return RAYLEIGH_MARGIN * max(float(model_worst_excess), RAYLEIGH_FLOOR)


def angle_bound(gap):
    """The project's conditioning bound on the angle to a float64 normal (tests/test_gpu_geometry.py: check_normals), per pixel."""
    with np.errstate(divide="ignore"):
        return 2e-4 + 50.0 * EPS32 / np.maximum(gap, 0.0)


def _prepare(image):
    img = np.ascontiguousarray(np.asarray(image)[:3], dtype=np.float32).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        r64 = np.sqrt(np.sum(img.astype(np.float64) ** 2, axis=0))
        r32 = r64.astype(np.float32)                       # the correctly rounded fp32 range
        # the contract's range is an fp32 computation: squares that overflow fp32 make it infinite although the point is finite
        r32 = np.where(np.isinf(img[0] * img[0] + img[1] * img[1] + img[2] * img[2]), np.float32(np.inf), r32)
    img[:, np.isinf(r32)] = 0.0                            # an infinite range: staged as an empty pixel
    r32 = np.where(np.isinf(r32), np.float32(0.0), r32)
    present = (img[0] != 0) | (img[1] != 0) | (img[2] != 0)
    valid = (img[0] != 0) & (img[1] != 0) & (img[2] != 0)
    return img, r32, present, valid


def _solve(img, valid, N, M, C, min_n):
    """Covariance about the mean from moments about the centre, eigh, flip.  M [3,H,W], C [3,3,H,W], N [H,W] (float64)."""
    H, W = N.shape
    has = valid & (N >= min_n)
    normal = np.zeros((3, H, W))
    evals = np.zeros((3, H, W))
    cov = np.zeros((H, W, 3, 3))
    if has.any():
        n = N[has]
        m = M[:, has]                                                      # [3,K]
        c = np.moveaxis(C[:, :, has], 2, 0)                                # [K,3,3]
        A = (c - m.T[:, :, None] * m.T[:, None, :] / n[:, None, None]) / np.maximum(n - 1.0, 1.0)[:, None, None]
        A = 0.5 * (A + np.swapaxes(A, 1, 2))
        w, V = np.linalg.eigh(A)
        nv = V[:, :, 0]
        p = img[:, has].astype(np.float64).T
        nv = np.where((np.sum(nv * p, axis=1) > 0)[:, None], -nv, nv)
        normal[:, has] = nv.T
        evals[:, has] = w.T
        cov[has] = A
    return has, normal, evals, cov


def _taps(H, W, a, b):
    vv, uu = np.arange(H), np.arange(W)
    for dv in range(-a, a + 1):
        vn = np.clip(vv + dv, 0, H - 1)
        for du in range(-b, b + 1):
            yield vn[:, None], np.clip(uu + du, 0, W - 1)[None, :]


def reference(image, a, b, eps, min_n, exact_ranges=False):
    """image [>=3,H,W] fp32 -> dict of per-pixel float64 results (full-image arrays; meaningful where `has`):
    normal [3,H,W] (zeros where none), evals [3,H,W] ascending, cov [H,W,3,3], N [H,W], has, valid, ambiguous [H,W] bool,
    gap [H,W] = (l1 - l0) / lmax (0 where lmax == 0).
    `ambiguous`: a valid centre whose window holds a present neighbour with | |dr| - eps | within AMBIGUOUS_ULPS ulp of the
    centre range -- the kernel's fmaf-chain range may round differently from the correctly rounded one there.  `exact_ranges`: the
    caller vouches (ranges_are_exact) that every range is exact however it is rounded; nothing is ambiguous then."""
    img, r32, present, valid = _prepare(image)
    _, H, W = img.shape
    eps32 = np.float32(eps)
    x64 = img.astype(np.float64)
    N = np.zeros((H, W))
    M = np.zeros((3, H, W))
    C = np.zeros((3, 3, H, W))
    amb = np.zeros((H, W), dtype=bool)
    tol = AMBIGUOUS_ULPS * np.spacing(np.abs(r32)).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for vn, un in _taps(H, W, a, b):
            rn = r32[vn, un]
            dr = np.abs(rn - r32)                                          # fp32 subtraction, as the kernel's and torch's
            keep = present[vn, un] & ~(dr > eps32)
            if not exact_ranges:
                amb |= present[vn, un] & (np.abs(np.abs(rn.astype(np.float64) - r32.astype(np.float64)) - float(eps32)) <= tol)
            d = np.where(keep[None], x64[:, vn, un] - x64, 0.0)
            N += keep
            M += d
            for i in range(3):
                for j in range(i, 3):
                    C[i, j] += d[i] * d[j]
    for i in range(3):
        for j in range(i):
            C[i, j] = C[j, i]
    has, normal, evals, cov = _solve(img, valid, N, M, C, min_n)
    lmax = evals[2]
    gap = np.where(lmax > 0, (evals[1] - evals[0]) / np.where(lmax > 0, lmax, 1.0), 0.0)
    return {"normal": normal, "evals": evals, "cov": cov, "N": N, "has": has, "valid": valid, "ambiguous": amb & valid, "gap": gap,
            "image": img}


def moment_model32(image, a, b, eps, min_n):
    """`reference` with fp32 differences, fp32 products and fp32 running sums along each window row; the rows are combined, the
    covariance about the mean is formed and the eigen problem is solved in float64 -- the precision normals.hip documents for its
    moments (fp32 partial sums of a row or two, combined in fp64).  Same gate decisions, same result layout (no `ambiguous`)."""
    img, r32, present, valid = _prepare(image)
    _, H, W = img.shape
    eps32 = np.float32(eps)
    N = np.zeros((H, W))
    M = np.zeros((3, H, W))
    C = np.zeros((3, 3, H, W))
    vv, uu = np.arange(H), np.arange(W)
    with np.errstate(invalid="ignore", over="ignore"):
        for dv in range(-a, a + 1):
            vn = np.clip(vv + dv, 0, H - 1)[:, None]
            m = np.zeros((3, H, W), dtype=np.float32)
            c = np.zeros((3, 3, H, W), dtype=np.float32)
            for du in range(-b, b + 1):
                un = np.clip(uu + du, 0, W - 1)[None, :]
                keep = present[vn, un] & ~(np.abs(r32[vn, un] - r32) > eps32)
                d = np.where(keep[None], img[:, vn, un] - img, np.float32(0.0))
                N += keep
                m += d
                for i in range(3):
                    for j in range(i, 3):
                        c[i, j] += d[i] * d[j]
            M += m
            C += c
    for i in range(3):
        for j in range(i):
            C[i, j] = C[j, i]
    has, normal, evals, cov = _solve(img, valid, N, M, C, min_n)
    return {"normal": normal, "evals": evals, "cov": cov, "N": N, "has": has, "valid": valid}


# --------------------------------------------------------------------------------------------------- per-pixel figures
def angle(a, b):
    """Angle between the vectors a, b [3,...] by atan2(|a x b|, a.b) (arccos has a noise floor of sqrt(eps) on unit vectors)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b, axis=0), axis=0), np.sum(a * b, axis=0))


def angle_to_reference(n, ref):
    """Per-pixel angle [H,W] of normals n [3,H,W] to ref["normal"].  The sign is ignored where the reference normal grazes the line
    of sight: |n.p| / |p| < 1e-3 as in check_normals -- and, because this comparison is per pixel, also where it is closer to grazing
    than the angle the conditioning bound allows at that pixel: a normal within that angle of the reference may lie on the other
    side of the line of sight, and must then (n.p <= 0 is asserted on its own) point the other way.  This matters only where the
    bound exceeds 1e-3, i.e. at gaps below 4e-3.  Meaningful where both sides have a normal."""
    ang = angle(n, ref["normal"])
    p = ref["image"].astype(np.float64)
    pn = np.linalg.norm(p, axis=0)
    margin = np.abs(np.sum(ref["normal"] * p, axis=0)) / np.where(pn > 0, pn, 1.0)
    graze = margin < np.maximum(1e-3, np.sin(np.minimum(angle_bound(ref["gap"]), 0.5 * np.pi)))
    return np.where(graze, np.minimum(ang, np.pi - ang), ang)


def rayleigh_excess(n, ref):
    """(n^T A n / n^T n - lambda_0) / lambda_max per pixel [H,W] against the float64 covariance of `ref` (0 where lambda_max == 0)."""
    n = np.asarray(n, dtype=np.float64)
    An = np.einsum("hwij,jhw->ihw", ref["cov"], n)
    nn = np.sum(n * n, axis=0)
    q = np.sum(n * An, axis=0) / np.where(nn > 0, nn, 1.0)
    lmax = ref["evals"][2]
    return np.where(lmax > 0, (q - ref["evals"][0]) / np.where(lmax > 0, lmax, 1.0), 0.0)


def border_mask(H, W, a, b):
    """Pixels whose window duplicates clamped edge pixels: the first and last a rows and b columns."""
    m = np.zeros((H, W), dtype=bool)
    if a:
        m[:a] = True
        m[-a:] = True
    if b:
        m[:, :b] = True
        m[:, -b:] = True
    return m


# ------------------------------------------------------------------------------------------------------------- scenes
def scan_image(seed, H, W, azimuth_steps, vfov_deg=(-24.5, 2.0)):
    """[3,H,W] fp32 range image of a synthetic scan (delora_amd.data.synthetic), projected by the CPU oracle."""
    import torch
    from delora_amd.data import synthetic
    from oracle import delora_oracle as orc
    scan = synthetic.make_pair(seed, rings=H, azimuth_steps=azimuth_steps, vfov_deg=vfov_deg)[0]
    sensor = orc.Sensor(int(H), int(W), [v * np.pi / 180.0 for v in vfov_deg], [-179.9 * np.pi / 180.0, 179.9 * np.pi / 180.0])
    img = orc.project_to_img(torch.from_numpy(scan).view(1, 3, -1), sensor)[0]
    return np.ascontiguousarray(img[0, :3].numpy())


SCENES = {                              # name -> (seed, H, W, azimuth steps, vertical field of view [deg])
    "64x720": (720, 64, 720, 800, (-24.5, 2.0)),
    "64x2048": (2048, 64, 2048, 2250, (-24.5, 2.0)),
    "128x256/0": (500, 128, 256, 290, (-22.5, 22.5)),
    "128x256/1": (501, 128, 256, 290, (-22.5, 22.5)),
    "128x256/2": (502, 128, 256, 290, (-22.5, 22.5)),
}
_SCENE_CACHE = {}


def scene(name):
    if name not in _SCENE_CACHE:
        _SCENE_CACHE[name] = scan_image(*SCENES[name])
    return _SCENE_CACHE[name].copy()


SMALL_SHAPES = [(16, 130), (5, 67), (1, 64), (3, 1), (2, 2)]


def small_image(H, W, seed=0):
    """A gently rolling surface (range within +-0.25 m) with 1.2 m steps and a few empty pixels, every coordinate non-zero: with
    eps = 0.5 a neighbour is either clearly inside the gate or clearly outside, whatever the window."""
    rng = np.random.default_rng(1000 * H + W + seed)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    az = -0.5013 + 0.004 * uu
    el = -0.3 + 0.006 * vv
    r = 9.0 + 0.15 * np.sin(0.11 * uu) + 0.04 * np.cos(0.7 * vv) + np.where(uu % 37 > 30, 1.2, 0.0) + rng.normal(0, 0.01, size=(H, W))
    img = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)]).astype(np.float32)
    img[:, rng.uniform(size=(H, W)) < 0.04] = 0.0
    return img


def wall_150m(H=32, W=200, seed=5):
    """A wall at x = 150 m with millimetre relief: the moments about the centre are ~1e-6 of the coordinates' squares."""
    rng = np.random.default_rng(seed)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    y = -3.0 + 0.03 * uu + rng.normal(0, 1e-3, size=(H, W))
    z = -0.5 + 0.03 * vv + rng.normal(0, 1e-3, size=(H, W))
    x = 150.0 + 1e-3 * np.sin(0.9 * uu) * np.cos(0.8 * vv) + rng.normal(0, 1e-3, size=(H, W))
    return np.stack([x, y, z]).astype(np.float32)


def plane_image(H=16, W=64, normal=(1.0, 0.25, -0.5), offset=10.0):
    """Points exactly (to fp32 rounding of the coordinates) on the plane n.p = offset, seen through a pinhole fan of rays."""
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    az, el = -0.5 + uu / (W - 1.0), -0.35 + 0.4 * vv / max(H - 1.0, 1.0)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    t = offset / np.einsum("i,ihw->hw", n, d)
    return (d * t).astype(np.float32), n


def two_planes_image(H=16, W=96):
    """Two walls meeting at an edge (x = 10 for y < 0, the plane x + y = 10 for y >= 0): left and right of the edge the answer is
    the wall's own normal, provided the window stays on one wall."""
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    az, el = -0.6 + 1.2 * (uu + 0.5) / W, -0.3 + 0.35 * vv / (H - 1.0)
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)])
    left = az < 0
    t = np.where(left, 10.0 / d[0], 10.0 / (d[0] + d[1]))
    n = np.where(left[None], np.array([1.0, 0.0, 0.0])[:, None, None], (np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0))[:, None, None])
    return (d * t).astype(np.float32), n, left


LINE_DIRS = [(0.25, 0.5, 0.125), (0.5, -0.25, 0.0), (0.0, 0.0, 0.25), (0.125, 0.125, 0.125)]


def collinear_image(W=40):
    """H = 4 * len(LINE_DIRS) rows; every fourth row holds the points p0 + j d (dyadic numbers: the fp32 differences, products and
    sums of the kernel's moments are exact), the others are empty -- with a <= 3 every window sees one line only (rank 1).
    Returns (image, direction per row [H,3], zero on empty rows)."""
    H = 4 * len(LINE_DIRS)
    img = np.zeros((3, H, W), dtype=np.float32)
    dirs = np.zeros((H, 3))
    j = np.arange(W, dtype=np.float64)
    for k, d in enumerate(LINE_DIRS):
        p0 = np.array([8.0 + k, 3.0625, -1.53125])                       # offsets that no multiple of a step cancels
        pts = p0[:, None] + np.asarray(d)[:, None] * (j - 7.0)[None]
        assert not np.any(pts == 0)                                      # every centre valid
        img[:, 4 * k] = pts
        dirs[4 * k] = d
    return img, dirs


def constant_image(H=6, W=20, point=(5.0, -2.0, 1.25)):
    return np.broadcast_to(np.asarray(point, dtype=np.float32)[:, None, None], (3, H, W)).copy()


def thin_pole_image(W=512, seed=9):
    """Rows 0 and 4 of 8 hold a line of points plus two perpendicular perturbations whose amplitude grows along the row, so that the
    relative gap (l1 - l0) / lmax of the windows sweeps from ~1e-7 to ~1e-2: the fp64 Rayleigh branch, and pixels just either
    side of NRM_FP32_GAP."""
    rng = np.random.default_rng(seed)
    img = np.zeros((3, 8, W), dtype=np.float32)
    j = np.arange(W, dtype=np.float64)
    for row, (d, e1, e2) in ((0, ((0.0, 0.0, 0.05), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))),
                             (4, ((0.03, 0.04, 0.0), (0.0, 0.0, 1.0), (0.8, -0.6, 0.0)))):
        s = 6e-5 * np.exp(np.log(2e-2 / 6e-5) * j / (W - 1.0))
        p = (np.array([7.0, 2.5, -12.0])[:, None] + np.asarray(d)[:, None] * j[None]
             + np.asarray(e1)[:, None] * (s * rng.normal(0, 1.0, W))[None] + np.asarray(e2)[:, None] * (s * rng.normal(0, 0.5, W))[None])
        img[:, row] = p
    return img


ISOTROPIC_DELTAS = [5e-4, 2e-4, 5e-5, 1e-5, 2e-6]


def isotropic_image(W=70):
    """One row per delta of ISOTROPIC_DELTAS, for the window (0,3): the row repeats, with period 7, a centre point and the six
    vertices of an octahedron whose axes are scaled so that the covariance of ANY seven consecutive points has the eigenvalues
    (1 - 4 delta, 1, 1 + delta) x const along three rotated axes -- all three within 1e-3 of each other, the SMALLEST the better
    separated one: the fp64 branch of the kernel that starts its iteration at the smallest eigenvalue."""
    c, s = np.cos(0.7), np.sin(0.7)
    c2, s2 = np.cos(-0.4), np.sin(-0.4)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[1.0, 0.0, 0.0], [0.0, c2, -s2], [0.0, s2, c2]])
    verts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    img = np.zeros((3, len(ISOTROPIC_DELTAS), W), dtype=np.float32)
    for row, delta in enumerate(ISOTROPIC_DELTAS):
        scale = 0.25 * np.sqrt(np.array([1.0 - 4.0 * delta, 1.0, 1.0 + delta]))
        pts = np.array([8.0, 3.0, -2.0])[None] + (verts * scale[None]) @ rot.T
        img[:, row] = pts[np.arange(W) % 7].T
    return img


GATE_TRIPLES = [((2, 1, 2), 3), ((2, 3, 6), 7), ((1, 4, 8), 9)]


def gate_image(H=12, W=48, seed=3):
    """Points t * k with t one of the integer triples (2,1,2), (2,3,6), (1,4,8) (|t| = 3, 7, 9) and k on a 1/8 grid: coordinates, their
    squares, the sum of squares and its root are all exact in fp32, so the range is exactly 3k, 7k or 9k whichever way it is rounded.
    Ranges fall in [9, 13.5] on a 1/8 grid; with eps = 1 many neighbours sit exactly AT eps (kept) and one step (1/8) beyond
    (dropped).  Returns (image, eps)."""
    rng = np.random.default_rng(seed)
    which = rng.integers(0, 3, size=(H, W))
    img = np.zeros((3, H, W), dtype=np.float32)
    for i, (t, nrm) in enumerate(GATE_TRIPLES):
        lo, hi = int(np.ceil(9.0 / nrm * 8)), int(np.floor(13.5 / nrm * 8))
        k = rng.integers(lo, hi + 1, size=(H, W)) / 8.0
        sign = np.where(rng.uniform(size=(H, W)) < 0.5, -1.0, 1.0)
        for c in range(3):
            img[c] = np.where(which == i, t[c] * k * (sign if c == 1 else 1.0), img[c])
    return img, np.float32(1.0)


def ranges_are_exact(image):
    """True iff the sum of squares of every pixel is a perfect square of an fp32 number and small enough for every partial sum to be
    exact in fp32: any correctly or fmaf-chain rounded range is then the same number, and no gate decision is ambiguous."""
    x = np.asarray(image[:3], dtype=np.float64)
    s = np.sum(x * x, axis=0)
    r = np.sqrt(s)
    return bool(np.all(r.astype(np.float32).astype(np.float64) ** 2 == s) and np.all(s * 2.0 ** 10 == np.round(s * 2.0 ** 10))
                and np.all(s < 2.0 ** 13))


# -------------------------------------------------------------------------------------------------------------- cases
GENERIC_WINDOWS = [(0, 0), (0, 5), (3, 0), (1, 1), (2, 3), (7, 9), (15, 28), (15, 29), (15, 31)]
SCALES = [(-10, "2^-10"), (10, "2^10"), (20, "2^20")]


def window_min_n(a, b):
    """min_neighbors of the window cases: a third of the window, between 2 (below it the covariance divides by zero) and 10."""
    return int(max(2, min(10, ((2 * a + 1) * (2 * b + 1)) // 3)))


def natural_cases():
    """(name, image builder, a, b, eps, min_n) of every non-planted case of tests/test_gpu_normals.py; the host test records the
    fp32-moment model on the same list."""
    cases = [(f"{n} 7x11", (lambda n=n: scene(n)), 3, 5, 0.5, 10) for n in SCENES]
    cases += [(f"small {H}x{W} 7x11", (lambda H=H, W=W: small_image(H, W)), 3, 5, 0.5, 10) for H, W in SMALL_SHAPES]
    for a, b in GENERIC_WINDOWS:
        # the share of centres with SOME neighbour within a few ulp of the gate grows with the number of taps: at 31 rows x 57..63
        # columns the scan has 0.8 % of them with eps = 0.5 and 0.01 % with eps = 8 (which still gates 4 % of the taps)
        cases.append((f"64x720 window ({a},{b})", (lambda: scene("64x720")), a, b, 8.0 if a == 15 else 0.5, window_min_n(a, b)))
        cases.append((f"small 16x130 window ({a},{b})", (lambda: small_image(16, 130)), a, b, 0.5, window_min_n(a, b)))
    for e, label in SCALES:
        cases.append((f"64x720 scaled by {label}", (lambda e=e: scene("64x720") * np.float32(2.0 ** e)), 3, 5, 0.5 * 2.0 ** e, 10))
    cases.append(("wall at 150 m, mm relief", wall_150m, 3, 5, 5.0, 10))
    return cases


def planted_cases():
    """(name, image builder, a, b, eps, min_n) of the planted degenerate scenes, for the host test's record of the model."""
    return [("thin poles", thin_pole_image, 3, 5, 100.0, 5), ("collinear runs (rank 1)", lambda: collinear_image()[0], 3, 5, 100.0, 5),
            ("exact gate", lambda: gate_image()[0], 3, 5, 1.0, 30), ("near-isotropic clouds", isotropic_image, 0, 3, 100.0, 5)]
