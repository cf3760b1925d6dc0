"""The contract of dl_project (include/delora_hip.h, the coordinate comments of csrc/common.h) as a plain reference: numpy float64 /
float32 and exact rational arithmetic, no GPU, nothing taken from the kernel's structure.

  range  = sqrt(fma(z, z, fma(y, y, x * x)))  and  norm2 = sqrt(fma(y, y, x * x)), every step correctly rounded to fp32
  a      = fp32(atan2(y, x)),  e = fp32(atan2(z, norm2)): evaluated in fp64, rounded once
  u      = ((a - fp32(hfov0)) / fp32(hfov1 - hfov0)) * fp32(W - 1) in fp32 (the difference of the field of view formed in fp64); v likewise
  pixel  = rint(u), rint(v), half to even; inside iff 0 <= rint(u) <= W-1 and 0 <= rint(v) <= H-1 (-0.0 is 0, NaN is outside)
  winner = the smallest (uint32 bits of the range, index within the scan); empty pixels are +0.0 / -1

Every fp32 step is formed in float64 and rounded once where that is provably the correctly rounded fp32 result (a product of two fp32
numbers is exact in fp64; a square root taken in fp64 and rounded to fp32 is correctly rounded because 53 >= 2 * 24 + 2), and by
exact rational arithmetic where it is not (the fused multiply-add: see ``fma32``).

fp64 atan2 is not correctly rounded by any libm (glibc documents <= 1 ulp, OCML <= 2 ulp), so two correct implementations may give
doubles a few ulp64 apart -- which round to the same fp32 number unless a float32 rounding midpoint lies between them.  ``settled``
marks the points whose fp64 atan2 values (azimuth and elevation) lie at least 8 ulp64 from every such midpoint; the generators
replace the others (REPLACED counts them: at most 1e-5 of a set), so that the reference is THE answer for every generated point.

The generators are seeded (PCG64: the same stream on every platform).
"""
import functools
from fractions import Fraction

import numpy as np

f32, f64 = np.float32, np.float64
DEG = np.pi / 180.0

# name -> (H, W, vfov [deg], hfov [deg])
SENSOR_TABLE = {
    "kitti": (64, 720, (-24.5, 2.0), (-179.9, 179.9)),            # shipped training size
    "kitti-pre": (64, 2250, (-24.5, 2.0), (-179.9, 179.9)),       # preprocessing width, largest tol_u
    "darpa": (64, 512, (-22.5, 22.5), (-179.9, 179.9)),           # shipped
    "ouster": (128, 2048, (-22.5, 22.5), (-179.9, 179.9)),        # shipped
    "min": (2, 2, (-90.0, 90.0), (-180.0, 180.0)),                # smallest legal image, seam exactly at +-pi
    "coarse": (3, 4, (-90.0, 90.0), (-180.0, 180.0)),             # ties
    "odd": (5, 9, (-24.5, 2.0), (-179.9, 179.9)),                 # S*H*W odd for odd S: padded key plane
    "ragged": (16, 130, (-24.5, 2.0), (-179.9, 179.9)),           # H*W % 256 != 0: last resolve chunk
    "narrow": (16, 2048, (-5.0, 5.0), (-45.0, 45.0)),             # many pixels per radian, most points outside
    "flipped": (16, 130, (2.0, -24.5), (179.9, -179.9)),          # negative spans
    "span": (16, 130, (-24.8, 2.0), (-179.9, 179.9)),             # fp32(f1) - fp32(f0) != fp32(f1 - f0) (equal at all the others)
}
DATASET_SENSORS = ("kitti", "kitti-pre", "darpa", "ouster")
SETTLED_ULPS = 8.0
REPLACED = {}            # generator name -> (points replaced as unsettled, points generated)


class Sensor:
    """H, W, the fp64 field of view (radians) and the six fp32 constants of the coordinate expression."""

    def __init__(self, H, W, vfov, hfov, name=""):
        self.H, self.W, self.name = int(H), int(W), name
        self.vfov, self.hfov = (float(vfov[0]), float(vfov[1])), (float(hfov[0]), float(hfov[1]))
        self.hf0f, self.hspanf, self.wm1f = f32(self.hfov[0]), f32(self.hfov[1] - self.hfov[0]), f32(self.W - 1)
        self.vf0f, self.vspanf, self.hm1f = f32(self.vfov[0]), f32(self.vfov[1] - self.vfov[0]), f32(self.H - 1)


def sensor_constants(H, W, vfov, hfov, name=""):
    """vfov, hfov in radians (python floats).  fp32(f0), fp32(f1 - f0) with the difference formed in fp64, fp32(cells - 1)."""
    return Sensor(H, W, vfov, hfov, name)


@functools.lru_cache(maxsize=None)
def sensor(name):
    H, W, vf, hf = SENSOR_TABLE[name]
    return sensor_constants(H, W, (vf[0] * DEG, vf[1] * DEG), (hf[0] * DEG, hf[1] * DEG), name)


# ------------------------------------------------------------------------------------------------ correctly rounded fp32 steps


def round_fraction_to_f32(q):
    """A rational number rounded to the nearest fp32, ties to even, subnormals and overflow included (zero comes out as +0.0)."""
    q = Fraction(q)
    if q == 0:
        return f32(0.0)
    sign, a = (-1.0 if q < 0 else 1.0), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                                    # 2^e <= a < 2^(e+1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(a, ulp)
    n = int(n)
    if 2 * rem > ulp or (2 * rem == ulp and n % 2 == 1):
        n += 1
    v = n * ulp
    if v >= Fraction(2) ** 128:
        return f32(sign * np.inf)
    return f32(sign * float(v))                                   # (exact: at most 24 significant bits)


def _at_f32_midpoint(s):
    """True where the float64 ``s`` lies exactly half way between two neighbouring fp32 numbers (the overflow threshold counts)."""
    with np.errstate(over="ignore", invalid="ignore"):
        r = s.astype(f32)
        r64 = r.astype(f64)
        other = np.where(r64 < s, np.nextafter(r, f32(np.inf)), np.nextafter(r, f32(-np.inf))).astype(f64)
        big = 2.0 ** 128
        r64 = np.where(np.isinf(r64), np.sign(r64) * big, r64)
        other = np.where(np.isinf(other), np.sign(other) * big, other)
        return np.isfinite(s) & (r64 != s) & (0.5 * r64 + 0.5 * other == s)


def mul32(a, b):
    with np.errstate(over="ignore", invalid="ignore"):
        return (a.astype(f64) * b.astype(f64)).astype(f32)        # the fp64 product of two fp32 numbers is exact: one rounding


def fma32(a, b, c):
    """fp32 fma(a, b, c) = a * b + c rounded once.  The product is exact in fp64; the fp64 sum rounds once more, and rounding that to
    fp32 can differ from the single rounding only where the sum was inexact (TwoSum error term non-zero) AND landed exactly on a
    float32 midpoint: those elements are settled in rational arithmetic."""
    a, b, c = (np.atleast_1d(np.asarray(t, dtype=f32)) for t in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    with np.errstate(over="ignore", invalid="ignore"):
        p, c64 = a.astype(f64) * b.astype(f64), c.astype(f64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        r = s.astype(f32)
    need = (err != 0) & _at_f32_midpoint(s)
    for i in zip(*np.nonzero(need)):
        r[i] = round_fraction_to_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return r


def sqrt32(a):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(a, dtype=f32).astype(f64)).astype(f32)   # innocuous double rounding: 53 >= 2 * 24 + 2


def norm2(x, y):
    return sqrt32(fma32(y, y, mul32(x, x)))


def norm3(x, y, z):
    return sqrt32(fma32(z, z, fma32(y, y, mul32(x, x))))


def _angles64(xyz):
    x, y, z = (np.asarray(xyz[i], dtype=f32) for i in range(3))
    with np.errstate(invalid="ignore"):
        return np.arctan2(y.astype(f64), x.astype(f64)), np.arctan2(z.astype(f64), norm2(x, y).astype(f64))


def coordinates(xyz, sen):
    """u, v, range of fp32 points ``[3,N]`` as float32 arrays (compare their uint32 views)."""
    x, y, z = (np.asarray(xyz[i], dtype=f32) for i in range(3))
    a64, e64 = _angles64(xyz)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, e = a64.astype(f32), e64.astype(f32)
        u = ((a - sen.hf0f) / sen.hspanf) * sen.wm1f               # np.float32 arithmetic: every operation correctly rounded
        v = ((e - sen.vf0f) / sen.vspanf) * sen.hm1f
    assert u.dtype == f32 and v.dtype == f32
    return u, v, norm3(x, y, z)


def midpoint_distance_ulps(a64):
    """Distance of fp64 values from the nearest float32 rounding midpoint, in ulp64 of the value (NaN for NaN)."""
    with np.errstate(invalid="ignore", over="ignore"):
        r = a64.astype(f32)
        r64 = r.astype(f64)
        up, dn = np.nextafter(r, f32(np.inf)).astype(f64), np.nextafter(r, f32(-np.inf)).astype(f64)
        d = np.minimum(np.abs(a64 - (0.5 * r64 + 0.5 * up)), np.abs(a64 - (0.5 * r64 + 0.5 * dn)))
        return d / np.spacing(np.abs(a64))


def settled(xyz):
    """Mask of the points whose fp64 azimuth AND elevation lie at least 8 ulp64 from a float32 rounding midpoint: every libm within
    2 ulp of the true value rounds them to the same fp32 number as this one (which is within 1).  NaN angles count as settled."""
    a64, e64 = _angles64(xyz)
    return ~(midpoint_distance_ulps(a64) < SETTLED_ULPS) & ~(midpoint_distance_ulps(e64) < SETTLED_ULPS)


def step_ulps(v, n):
    """fp32 array moved by n float ulps in magnitude (n may be an array; 0 and subnormals step through the subnormals)."""
    bits = np.asarray(v, dtype=f32).view(np.int32).astype(np.int64)
    mag = np.maximum((bits & 0x7FFFFFFF) + np.asarray(n, dtype=np.int64), 0)
    return ((bits & 0x80000000) | mag).astype(np.uint32).view(f32)


def settle(xyz, name):
    """Replace the unsettled points of a generated set (y and z moved by 32 ulps until settled); REPLACED[name] counts them."""
    xyz = np.array(xyz, dtype=f32)
    bad = ~settled(xyz)
    n_bad = int(bad.sum())
    for _ in range(16):
        if not bad.any():
            break
        xyz[1, bad], xyz[2, bad] = step_ulps(xyz[1, bad], 32), step_ulps(xyz[2, bad], 32)
        bad = ~settled(xyz)
    assert not bad.any()
    done, total = REPLACED.get(name, (0, 0))
    REPLACED[name] = (done + n_bad, total + xyz.shape[1])
    return xyz


# ------------------------------------------------------------------------------------------------ the image builder


def winners(u, v, r, sen):
    """(point index, pixel) of the winner of every occupied pixel of one scan, pixels ascending."""
    ru, rv = np.rint(u), np.rint(v)                                # half to even, stays float32
    with np.errstate(invalid="ignore"):
        inside = (ru >= 0) & (ru <= sen.wm1f) & (rv >= 0) & (rv <= sen.hm1f)
    idx = np.nonzero(inside)[0]
    pix = rv[idx].astype(np.int64) * sen.W + ru[idx].astype(np.int64)
    order = np.lexsort((idx, r[idx].view(np.uint32), pix))
    ps = pix[order]
    first = np.ones(len(ps), dtype=bool)
    first[1:] = ps[1:] != ps[:-1]
    return idx[order][first], ps[first]


def project(scans, sen, C, coords=None):
    """scans: list of fp32 ``[C,n]`` arrays (``coords``: their precomputed ``coordinates``, to save time).  Returns dict(image4 [S,4,H,W], aux [S,C-3,H,W], packed [S,H,W,4], packed_aux [S,H,W,4]
    (channels 3..5 where the scan has them, +0.0 otherwise), pix2pt [S,H,W] int32, kept [S] int32, uvr [3, sum n])."""
    S, H, W = len(scans), sen.H, sen.W
    image4, aux = np.zeros((S, 4, H * W), dtype=f32), np.zeros((S, max(C - 3, 0), H * W), dtype=f32)
    packed, packed_aux = np.zeros((S, H * W, 4), dtype=f32), np.zeros((S, H * W, 4), dtype=f32)
    pix2pt, kept, uvr = np.full((S, H * W), -1, dtype=np.int32), np.zeros((S,), dtype=np.int32), []
    for s, scan in enumerate(scans):
        scan = np.asarray(scan, dtype=f32)
        assert scan.shape[0] == C
        u, v, r = coords[s] if coords is not None else coordinates(scan[:3], sen)
        uvr.append(np.stack([u, v, r]))
        win, pix = winners(u, v, r, sen)
        image4[s, :3, pix], image4[s, 3, pix] = scan[:3, win].T, r[win]
        packed[s, pix, :3], packed[s, pix, 3] = scan[:3, win].T, r[win]
        for c in range(3, C):
            aux[s, c - 3, pix] = scan[c, win]
            if c < 6:
                packed_aux[s, pix, c - 3] = scan[c, win]
        pix2pt[s, pix], kept[s] = win, len(win)
    return {"image4": image4.reshape(S, 4, H, W), "aux": aux.reshape(S, max(C - 3, 0), H, W), "packed": packed.reshape(S, H, W, 4),
            "packed_aux": packed_aux.reshape(S, H, W, 4), "pix2pt": pix2pt.reshape(S, H, W), "kept": kept,
            "uvr": np.concatenate(uvr, axis=1) if uvr else np.zeros((3, 0), dtype=f32)}


# ------------------------------------------------------------------------------------------------ generators

SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)
STEPS = (0, 1, -1, 2, -2, 4, -4, 8, -8, 16, -16)


def _rng(seed):
    return np.random.default_rng(int(seed))


def _polar(az, el, r):
    return np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)]).astype(f32)


def _inside_angles(sen, n, rng, which):
    """n azimuths (which = "az") or elevations ("el") inside the field of view, away from its ends."""
    f0, f1 = sen.hfov if which == "az" else sen.vfov
    return f0 + rng.uniform(0.1, 0.9, n) * (f1 - f0)


def random_cloud(n, scale, seed, flat=0.15):
    """Normal cloud of the given scale; z is flattened so that lidar-like fields of view keep a fair share of it."""
    p = _rng(seed).normal(size=(3, int(n))).astype(f32) * f32(scale)
    p[2] *= f32(flat)
    return settle(p, "random_cloud")


def random_mix(n, seed):
    """n points spread over the scales 1e-3 ... 1e3."""
    per = -(-int(n) // len(SCALES))
    return np.concatenate([random_cloud(per, sc, seed * 16 + i) for i, sc in enumerate(SCALES)], axis=1)[:, :int(n)]


def _boundary_candidates(sen, which, steps, ranges, seed):
    """Points on the k + 1/2 boundaries of u (which = "u": every k in [-1, W-1], a handful of elevations) or of v (every row
    boundary, a handful of azimuths), y (resp. z) stepped by ``steps`` float ulps, at ``ranges``.  Returns (xyz, k)."""
    rng = _rng(seed)
    cells, (f0, f1) = (sen.W, sen.hfov) if which == "u" else (sen.H, sen.vfov)
    k = np.arange(-1, cells, dtype=np.float64)
    ang = f0 + (k + 0.5) * (f1 - f0) / (cells - 1)
    lim = np.pi if which == "u" else np.pi / 2
    k, ang = k[np.abs(ang) <= lim], ang[np.abs(ang) <= lim]
    other = _inside_angles(sen, 5, rng, "el" if which == "u" else "az")
    kk, aa, oo, rr, ss = [], [], [], [], []
    for j, r in enumerate(ranges):
        if which == "u":                                           # one of the handful per boundary, another one per range
            o = other[(np.arange(len(k)) + j) % len(other)]
            kk.append(k), aa.append(ang), oo.append(o), rr.append(np.full(len(k), r))
        else:                                                      # few rows: every azimuth of the handful
            for o in other:
                kk.append(k), aa.append(ang), oo.append(np.full(len(k), o)), rr.append(np.full(len(k), r))
    k, ang, oth, r = (np.concatenate(t) for t in (kk, aa, oo, rr))
    base = _polar(ang, oth, r) if which == "u" else _polar(oth, ang, r)
    out, ks = [], []
    for st in steps:
        p = base.copy()
        row = 1 if which == "u" else 2
        p[row] = step_ulps(p[row], st)
        out.append(p), ks.append(k)
    return np.concatenate(out, axis=1), np.concatenate(ks)


def boundary_points(sen, seed=11):
    pu, _ = _boundary_candidates(sen, "u", STEPS, (0.7, 61.0), seed)
    pv, _ = _boundary_candidates(sen, "v", STEPS, (0.7, 9.3, 61.0), seed + 1)
    return settle(np.concatenate([pu, pv], axis=1), "boundary_points")


def exact_halves(sen, seed=23, per_k=2):
    """Points whose contract u (resp. v) is EXACTLY k + 1/2: found by stepping y (z) by up to +-6 float ulps around the analytic
    boundary and keeping the hits.  Returns (xyz, ku, kv): ku / kv hold the k of a point's exact half in u / v, -9 where none."""
    found, kus, kvs = [], [], []
    for which, ranges in (("u", (0.7, 9.3, 61.0)), ("v", (0.7, 9.3, 61.0))):
        p, k = _boundary_candidates(sen, which, tuple(range(-6, 7)), ranges, seed)
        ok = settled(p)
        u, v, _ = coordinates(p, sen)
        c = u if which == "u" else v
        hit = ok & (c == (k + 0.5).astype(f32)) & (k >= 0) & (k <= (sen.W if which == "u" else sen.H) - 2)
        idx = np.nonzero(hit)[0]
        idx = idx[np.argsort(k[idx], kind="stable")]
        _, first, inv = np.unique(k[idx], return_index=True, return_inverse=True)
        keep = idx[np.arange(len(idx)) - first[inv] < per_k]       # per_k points per boundary at the most
        found.append(p[:, keep])
        kus.append(k[keep].astype(np.int64) if which == "u" else np.full(len(keep), -9))
        kvs.append(k[keep].astype(np.int64) if which == "v" else np.full(len(keep), -9))
    return np.concatenate(found, axis=1), np.concatenate(kus), np.concatenate(kvs)


def specials(sen):
    """The origin, signed zeros on the axes, subnormals, overflowing squares, NaN and inf in every coordinate, and points just
    outside the image whose coordinate still rounds to the first / last cell (u in [-0.5, 0) and (W-1, W-1+0.5], v likewise)."""
    nan, inf, z = float("nan"), float("inf"), 0.0
    p = [(z, z, z), (-z, z, z), (z, -z, z), (-z, -z, z), (z, z, -z), (-z, -z, -z)]
    for a in (5.0, -5.0):
        for sz in (z, -z):
            p += [(a, sz, z), (a, sz, -z), (sz, a, z), (sz, a, -z), (sz, z, a), (sz, -z, a), (-z, sz, a)]
    p += [(-5.0, z, 0.1), (-5.0, -z, 0.1), (-5.0, 1e-38, 0.1), (-5.0, -1e-38, 0.1), (-5.0, 1e-45, -0.1), (-5.0, -1e-45, -0.1)]
    p += [(1e-40, z, z), (1e-40, 1e-40, 1e-40), (-1e-40, 1e-40, z), (1e-40, -1e-40, -1e-41), (3.0, 1e-40, -1e-40), (1e-40, 2.0, 1e-40),
          (1e-20, 1e-20, 1e-21), (1e-23, -1e-23, 1e-24)]
    for big in (1e19, 1e20, 3e38):
        p += [(big, z, z), (big, big, z), (-big, big * 0.5, big * 0.01), (big, -big, -big * 0.1), (1.0, big, z), (big, 1.0, -1.0)]
    for bad in (nan, inf, -inf):
        p += [(bad, 1.0, 0.1), (1.0, bad, 0.1), (4.0, 1.0, bad), (bad, bad, 0.1), (bad, bad, bad)]
    p = np.array(p, dtype=np.float64).T
    edge = []
    for which in ("u", "v"):
        cells, (f0, f1) = (sen.W, sen.hfov) if which == "u" else (sen.H, sen.vfov)
        lim = np.pi if which == "u" else np.pi / 2
        c = np.array([-0.51, -0.5, -0.49, -0.3, -1e-3, -1e-6, 1e-6, 1e-3, 0.3, 0.49, 0.5, 0.51])
        c = np.concatenate([c[c < 0], (cells - 1) + c[c > 0], c[c > 0], (cells - 1) + c[c < 0]])
        ang = f0 + c * (f1 - f0) / (cells - 1)
        ang = ang[np.abs(ang) <= lim]
        mid = 0.5 * (sen.vfov[0] + sen.vfov[1]) if which == "u" else 0.37 * sen.hfov[0] + 0.63 * sen.hfov[1]
        for r in (0.9, 17.0):
            edge.append(_polar(ang, np.full(len(ang), mid), r) if which == "u" else _polar(np.full(len(ang), mid), ang, r))
    return settle(np.concatenate([p.astype(f32)] + edge, axis=1), "specials")


def with_aux(xyz, C, seed):
    """``[C,n]``: xyz plus C - 3 finite channels, every value different from its neighbours'."""
    n = xyz.shape[1]
    aux = (_rng(seed).permutation(max(n, 1) * max(C - 3, 1))[:n * (C - 3)].reshape(C - 3, n) + 1).astype(f32) * f32(0.25)
    return np.concatenate([np.asarray(xyz, dtype=f32), aux], axis=0)


TIE_MIN_GROUP = 4


def tie_cloud(seed=5, box=7, duplicates=12, far=40):
    """Integer lattice points of [-box, box]^3 that share a pixel of the coarse sensor with at least three others of the same integer
    x^2 + y^2 + z^2 (bit-equal range), exact duplicates of some of them, and ``far`` points scaled by 1e20 (their squares overflow:
    range +inf) -- in shuffled order.  Returns xyz ``[3,n]``."""
    sen = sensor("coarse")
    g = np.arange(-box, box + 1)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1).astype(f32)
    p = p[:, settled(p)]
    u, v, r = coordinates(p, sen)
    ru, rv = np.rint(u), np.rint(v)
    inside = (ru >= 0) & (ru <= sen.wm1f) & (rv >= 0) & (rv <= sen.hm1f)
    p, pix, rb = p[:, inside], (rv[inside].astype(np.int64) * sen.W + ru[inside].astype(np.int64)), r[inside].view(np.uint32).astype(np.int64)
    key = pix * (1 << 32) + rb
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    p = p[:, cnt[inv] >= TIE_MIN_GROUP]
    rng = _rng(seed)
    dup = p[:, rng.choice(p.shape[1], duplicates, replace=False)]
    d = rng.normal(size=(3, far))
    d[2] *= 0.2
    lone = (d / np.linalg.norm(d, axis=0) * 1e20).astype(f32)
    lone = lone[:, settled(lone)]
    allp = np.concatenate([p, dup, dup, lone, p[:, :far] * f32(1e20)], axis=1)
    allp = allp[:, settled(allp)]
    return np.ascontiguousarray(allp[:, rng.permutation(allp.shape[1])])


def tie_groups(xyz, sen):
    """Sizes of the (pixel, range bits) groups of the inside points of a cloud."""
    u, v, r = coordinates(xyz, sen)
    ru, rv = np.rint(u), np.rint(v)
    with np.errstate(invalid="ignore"):
        inside = (ru >= 0) & (ru <= sen.wm1f) & (rv >= 0) & (rv <= sen.hm1f)
    key = (rv[inside].astype(np.int64) * sen.W + ru[inside].astype(np.int64)) * (1 << 32) + r[inside].view(np.uint32).astype(np.int64)
    return np.unique(key, return_counts=True)[1]


def raster_cloud(sen, n, seed, near_tail=300):
    """n points in raster order of the sensor's image (row by row, jittered inside their cells), the last ``near_tail`` of them
    nearer than all the others, so that each of those wins the pixel it falls into."""
    rng = _rng(seed)
    t = (np.arange(n) + 0.5) / n * sen.H * sen.W
    row, col = np.floor(t / sen.W), np.mod(t, sen.W)
    v = np.clip(row + rng.uniform(-0.35, 0.35, n), 0.0, sen.H - 1.0)
    u = np.clip(col + rng.uniform(-0.35, 0.35, n) - 0.5, 0.0, sen.W - 1.0)
    az = sen.hfov[0] + u / (sen.W - 1) * (sen.hfov[1] - sen.hfov[0])
    el = sen.vfov[0] + v / (sen.H - 1) * (sen.vfov[1] - sen.vfov[0])
    r = rng.uniform(5.0, 80.0, n)
    if near_tail:
        sel = rng.permutation(n)[:near_tail]
        az[n - near_tail:], el[n - near_tail:], r[n - near_tail:] = az[sel], el[sel], rng.uniform(0.5, 2.0, near_tail)
    return settle(_polar(az, el, r), "raster_cloud")


# ------------------------------------------------------------------------------------------------ the cases both tiers run

COORD_RANDOM = 20000


@functools.lru_cache(maxsize=None)
def coordinate_points(name):
    """The point set of test_uvr_bitwise / test_fast_path_pixels at one sensor: random + specials + boundaries + exact halves."""
    sen = sensor(name)
    seed = 100 + sorted(SENSOR_TABLE).index(name)
    p = np.concatenate([random_mix(COORD_RANDOM, seed), specials(sen), boundary_points(sen), exact_halves(sen)[0]], axis=1)
    p.setflags(write=False)
    return p


LAYOUT_S = (1, 2, 7, 8, 9, 15, 16, 17, 24)
LAYOUT_LENGTHS = (0, 1, 255, 256, 257, 1000, 3000)
LAYOUT_C = (3, 4, 5, 6, 7, 8)
OFFS0, TAIL_COLS, PAD_COLS = 5, 3, 7


def layout_cases():
    """One case per (sensor, S): scan lengths drawn from LAYOUT_LENGTHS (S = 9 and 17 get a 3000-point scan: G = 12), C and the
    set of optional outputs left NULL cycle through their values; offs[0] = 5, n_cols = offs[S] + 3, pts_cs = n_cols + 7."""
    cases, i = [], 0
    nulls = ((), ("packed",), ("packed_aux",), ("kept",), ("uvr",), ("packed", "packed_aux", "kept", "uvr"))
    for sname in ("ragged", "odd"):
        for S in LAYOUT_S:
            rng = _rng(4000 + i)
            lens = [int(x) for x in rng.choice(LAYOUT_LENGTHS, S)]
            if S in (9, 17):
                lens[int(rng.integers(S))] = 3000
            if S == 24:
                lens[-1] = 1000                                    # the last scan of the last (ghost) group carries points
            C = LAYOUT_C[(i + (0 if sname == "ragged" else 3)) % len(LAYOUT_C)]
            cases.append({"name": f"{sname}-S{S}-C{C}", "sensor": sname, "lens": lens, "C": C, "seed": 5000 + i,
                          "null": nulls[(i * 5 + 1) % len(nulls)] if S not in (9, 17) else (), "skew": 0})
            i += 1
    # every C on a ghost-group batch with every output, the all-empty batch, and the skewed bases
    for C in LAYOUT_C:
        cases.append({"name": f"ragged-S9-C{C}-all", "sensor": "ragged", "lens": [257, 0, 1000, 1, 3000, 255, 256, 1000, 257], "C": C,
                      "seed": 6000 + C, "null": (), "skew": 0})
    cases.append({"name": "odd-S9-empty", "sensor": "odd", "lens": [0] * 9, "C": 6, "seed": 1, "null": (), "skew": 0})
    cases.append({"name": "ragged-S1-empty", "sensor": "ragged", "lens": [0], "C": 3, "seed": 1, "null": (), "skew": 0})
    cases.append({"name": "odd-S17-C7-skew16", "sensor": "odd", "lens": [1000, 257, 0, 3000, 1, 255, 256, 1000, 257, 3000, 0, 1, 255, 1000, 256, 257, 1000],
                  "C": 7, "seed": 7001, "null": (), "skew": 16})
    return cases


def case_scans(case):
    """The scans ``[C,n]`` of a layout case: random clouds of mixed scale, aux channels from a seeded permutation."""
    scans = []
    for j, n in enumerate(case["lens"]):
        xyz = random_cloud(n, SCALES[(j + case["seed"]) % len(SCALES)], case["seed"] * 64 + j) if n else np.zeros((3, 0), dtype=f32)
        scans.append(with_aux(xyz, case["C"], case["seed"] * 64 + j))
    return scans


CAP_POINTS = 1024 * 256 + 300            # the vote's G caps at 1024 workgroups of 256 threads: the last 300 points are a second trip


@functools.lru_cache(maxsize=None)
def cap_scans(S):
    """S = 1: one scan of CAP_POINTS points in raster order of the kitti sensor; S = 8: that scan and seven short ones."""
    big = raster_cloud(sensor("kitti"), CAP_POINTS, 31)
    scans = [big] + [random_cloud(n, 10.0, 900 + n) for n in (0, 1, 255, 256, 257, 1000, 3000)][:S - 1]
    if S > 1:
        scans = scans[1:4] + [scans[0]] + scans[4:]
    return tuple(scans)
