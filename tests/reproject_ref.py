"""The contract of dl_reproject (include/delora_hip.h) as a plain reference: numpy, no GPU, nothing taken from the kernel's structure.
It is built from the pieces of tests/project_ref.py (the contract of dl_project, on which this one rests):

  occupied   !(x == 0 && y == 0 && z == 0) of the source pixel
  q          fma(m2, z, fma(m1, y, m0 * x)) + m3 per row of T: ``mul32`` / ``fma32`` and one np.float32 addition
  R n        the same chain without the addition;  d = q - m: one np.float32 subtraction
  pixel      ``coordinates`` of q (range, u, v), half to even, the inside test, and ``winners``: the smallest (uint32 bits of the
             range, source pixel index) -- over all occupied source pixels for moved4 / src_pix plane 0, over the PAIRED ones
             (occupied, nn_pix >= 0, source normal != 0, matched normal != 0) for paired9 / src_pix plane 1
  empty      +0.0, -1 in src_pix

and the seeded case generator both tiers run (tests/test_reproject_ref_host.py on the host, tests/test_gpu_reproject_exact.py on the
GPU).  No fp64 atan2 is correctly rounded, so a transformed point counts only when ``project_ref.settled`` holds for it: the
generator draws a case from a seed and re-draws (seed + 1) while any occupied transformed point is unsettled; REDRAWS counts that.
"""
import functools

import numpy as np

from tests import project_ref as pr

f32 = np.float32
MAX_REDRAWS = 3
REDRAWS = {}             # case name -> re-draws it needed


def _rows(T):
    T = np.asarray(T, dtype=f32)
    return [[np.full((1,), T[r, c], dtype=f32) for c in range(4)] for r in range(3)]


def transform(T, x, y, z):
    """q = R p + t in the loss kernel's operation order; fp32 arrays in and out."""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for m in _rows(T):
            out.append((pr.fma32(m[2], z, pr.fma32(m[1], y, pr.mul32(m[0], x))) + m[3]).astype(f32))
    return out


def rotate(T, x, y, z):
    with np.errstate(invalid="ignore", over="ignore"):
        return [pr.fma32(m[2], z, pr.fma32(m[1], y, pr.mul32(m[0], x))) for m in _rows(T)]


def occupied(x, y, z):
    return ~((x == 0) & (y == 0) & (z == 0))


def nonzero3(a, b, c):
    return (a != 0) | (b != 0) | (c != 0)


def paired_mask(src, srcn, match, nn):
    """The pair set of icp_losses.py:48-52,110-121 on flat planes."""
    return occupied(src[0], src[1], src[2]) & (nn >= 0) & nonzero3(srcn[0], srcn[1], srcn[2]) & nonzero3(match[3], match[4], match[5])


def reproject_one(src, srcn, match, nn, T, sen, want_paired=True):
    """One sample on flat planes: src [>=3,HW], srcn [3,HW] | None, match [6,HW] | None, nn [HW] | None, T [4,4].
    Returns (moved4 [4,HW], paired9 [9,HW] | None, src_pix [2,HW], q [3,n_occupied])."""
    HW = sen.H * sen.W
    src = np.asarray(src, dtype=f32)
    moved4, src_pix = np.zeros((4, HW), dtype=f32), np.full((2, HW), -1, dtype=np.int32)
    occ = np.nonzero(occupied(src[0], src[1], src[2]))[0]
    q = np.stack(transform(T, src[0, occ], src[1, occ], src[2, occ])) if len(occ) else np.zeros((3, 0), dtype=f32)
    u, v, r = pr.coordinates(q, sen)
    win, pix = pr.winners(u, v, r, sen)
    moved4[:3, pix], moved4[3, pix], src_pix[0, pix] = q[:, win], r[win], occ[win]
    paired9 = None
    if want_paired and srcn is not None:
        srcn, match, nn = np.asarray(srcn, dtype=f32), np.asarray(match, dtype=f32), np.asarray(nn)
        paired9 = np.zeros((9, HW), dtype=f32)
        sel = np.nonzero(paired_mask(src, srcn, match, nn)[occ])[0]           # positions inside `occ`: ascending source pixel
        win, pix = pr.winners(u[sel], v[sel], r[sel], sen)
        s = occ[sel[win]]
        paired9[0:3, pix] = q[:, sel[win]]
        paired9[3:6, pix] = np.stack(rotate(T, srcn[0, s], srcn[1, s], srcn[2, s])) if len(s) else np.zeros((3, 0), dtype=f32)
        with np.errstate(invalid="ignore", over="ignore"):
            paired9[6:9, pix] = (q[:, sel[win]] - match[0:3, s]).astype(f32)
        src_pix[1, pix] = s
    return moved4, paired9, src_pix, q


def reproject(src, srcn, match, nn, T, sen, want_paired=True):
    """src [B,>=3,H,W], srcn [B,3,H,W] | None, match [B,6,H,W] | None, nn [B,H,W] | None, T [B,4,4].
    Returns dict(moved4 [B,4,H,W], paired9 [B,9,H,W] | None, src_pix [B,2,H,W] int32, q: list of [3,n_b])."""
    B, H, W = len(src), sen.H, sen.W
    rows = [reproject_one(np.asarray(src[b]).reshape(-1, H * W), None if srcn is None else np.asarray(srcn[b]).reshape(3, H * W),
                          None if match is None else np.asarray(match[b]).reshape(6, H * W),
                          None if nn is None else np.asarray(nn[b]).reshape(H * W), T[b], sen, want_paired) for b in range(B)]
    paired = want_paired and srcn is not None
    return {"moved4": np.stack([r[0] for r in rows]).reshape(B, 4, H, W),
            "paired9": np.stack([r[1] for r in rows]).reshape(B, 9, H, W) if paired else None,
            "src_pix": np.stack([r[2] for r in rows]).reshape(B, 2, H, W), "q": [r[3] for r in rows]}


# ------------------------------------------------------------------------------------------------ poses


def rotation(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(kind, rng):
    """identity | small (<= 0.5 m, <= 2 deg: the trained regime) | rotation (a large one, no translation: collisions, points leaving
    the field of view) | large (rotation + metres of translation) | away (every point leaves the field of view) | nan."""
    T = np.eye(4)
    if kind == "small":
        T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(-2.0, 2.0) * pr.DEG)
        t = rng.normal(size=3)
        T[:3, 3] = t / np.linalg.norm(t) * rng.uniform(0.05, 0.5)
    elif kind in ("rotation", "large"):
        T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(0.5, 3.0))
        if kind == "large":
            T[:3, 3] = rng.normal(size=3) * 3.0
    elif kind == "away":
        T[:3, :3] = rotation(rng.normal(size=3), rng.uniform(-2.0, 2.0) * pr.DEG)
        T[:3, 3] = (0.0, 0.0, 1e5)                                 # elevation ~ +90 deg: above every sensor but the full sphere
    elif kind == "nan":
        T[:3, :3] = rotation(rng.normal(size=3), 0.3)
        T[1, 2] = np.nan
    else:
        assert kind == "identity"
    return T.astype(f32)


# ------------------------------------------------------------------------------------------------ cases

# name -> (sensor, poses of the B samples, source cloud ("random" | "raster" | "halves": project_ref.exact_halves in front of a random
# cloud), points per scan)
CASES = {
    "min-identity": ("min", ("identity",), "random", 40),
    "min-large-B3": ("min", ("large", "small", "rotation"), "random", 40),
    "odd-identity": ("odd", ("identity",), "raster", 200),
    "odd-small-B3": ("odd", ("small", "rotation", "large"), "random", 400),
    "odd-away": ("odd", ("away",), "raster", 200),
    "ragged-identity": ("ragged", ("identity",), "raster", 6000),
    "ragged-identity-halves": ("ragged", ("identity",), "halves", 600),       # coordinates EXACTLY k + 1/2: half to even
    "ragged-small": ("ragged", ("small",), "raster", 6000),
    "ragged-rotation": ("ragged", ("rotation",), "raster", 6000),
    "ragged-large-B3": ("ragged", ("large", "rotation", "small"), "random", 9000),
    "ragged-away": ("ragged", ("away",), "random", 5000),
    "ragged-nan-B3": ("ragged", ("small", "nan", "rotation"), "raster", 6000),
    "flipped-small-B3": ("flipped", ("small", "identity", "large"), "raster", 6000),
    "flipped-rotation": ("flipped", ("rotation",), "random", 9000),
    # B >= 8: the entry point maps workgroups to samples in groups of eight (B = 9: a ghost group of seven)
    "odd-mixed-B9": ("odd", ("small", "rotation", "large", "identity", "small", "away", "large", "rotation", "small"), "random", 400),
    "ragged-mixed-B9": ("ragged", ("small", "rotation", "large", "identity", "small", "away", "large", "nan", "small"), "raster", 3000),
    "kitti-small": ("kitti", ("small",), "raster", 60000),
}
NAN_CASE, NAN_SAMPLE = "ragged-nan-B3", 1


def _unit(rng, n):
    v = rng.normal(size=(3, n))
    return (v / np.linalg.norm(v, axis=0)).astype(f32)


def _draw(name, seed):
    sname, kinds, cloud, n = CASES[name]
    sen, rng = pr.sensor(sname), np.random.default_rng(seed)
    H, W, B = sen.H, sen.W, len(kinds)
    HW = H * W
    src, srcn, match, nn, T = (np.zeros((B, 4, HW), dtype=f32), np.zeros((B, 3, HW), dtype=f32), np.zeros((B, 6, HW), dtype=f32),
                               np.zeros((B, HW), dtype=np.int32), np.zeros((B, 4, 4), dtype=f32))
    planted = {"duplicates": 0, "shadowed": 0, "negative_zeros": 0}
    for b, kind in enumerate(kinds):
        if cloud == "raster":
            pts = pr.raster_cloud(sen, n, seed * 8 + b, near_tail=min(300, n // 4))
        elif cloud == "halves":
            pts = np.concatenate([pr.exact_halves(sen)[0], pr.random_cloud(n, 100.0, seed * 8 + b)], axis=1)
        else:
            pts = pr.random_cloud(n, 10.0, seed * 8 + b)
        src[b] = pr.project([pts], sen, 3)["image4"][0].reshape(4, HW)
        T[b] = pose(kind, rng)
        occ = np.nonzero(occupied(*src[b, :3]))[0]
        # synthetic normals and matches; random subsets zeroed, nn_pix = -1 with a zero match there
        srcn[b] = _unit(rng, HW) * (rng.random(HW) < 0.7)
        match[b, :3] = rng.normal(size=(3, HW)).astype(f32) * f32(10.0)
        match[b, 3:] = _unit(rng, HW) * (rng.random(HW) < 0.7)
        nn[b] = rng.integers(0, HW, HW)
        gone = rng.random(HW) < 0.2
        nn[b, gone], match[b][:, gone] = -1, 0.0
        nn[b, rng.random(HW) < 0.05] = -1                          # ... and a few with a stale match left behind: nn_pix decides
        # (empty source pixels keep normals / matches / nn_pix >= 0 here and there: only an OCCUPIED pixel is a pair)
        if len(occ) >= 8:
            pick = rng.permutation(occ)
            # identical points in several source pixels: the lower pixel must win
            a, twins = pick[0], pick[1:3]
            src[b][:, twins] = src[b][:, [a]]
            planted["duplicates"] += 1
            # a near UNPAIRED point in front of a far PAIRED one (same direction, so the same pixel under a pure rotation)
            if kind in ("identity", "rotation"):
                far, near = pick[3], pick[4]
                src[b][:3, near] = src[b][:3, far] * f32(0.5)
                src[b][3, near] = src[b][3, far] * f32(0.5)
                nn[b, near], match[b][:, near] = -1, 0.0
                nn[b, far] = 0
                srcn[b][:, far], match[b][3:, far] = (0.6, 0.0, 0.8), (0.0, 1.0, 0.0)
                planted["shadowed"] += 1
            # components equal to -0.0
            for k, j in enumerate(pick[5:8]):
                if src[b][(k + 1) % 3, j] != 0:                      # the pixel stays occupied
                    src[b][k, j] = -0.0
                    planted["negative_zeros"] += 1
            srcn[b][0, pick[5]], match[b][1, pick[6]], match[b][4, pick[7]] = -0.0, -0.0, -0.0
        src[b][3] = pr.norm3(src[b][0], src[b][1], src[b][2])          # the range plane of the planted points (dl_reproject does not read it)
    shape = lambda a, c: a.reshape(B, c, H, W)
    return {"name": name, "sensor": sname, "sen": sen, "B": B, "kinds": kinds, "src": shape(src, 4), "srcn": shape(srcn, 3),
            "match": shape(match, 6), "nn": nn.reshape(B, H, W), "T": T, "planted": planted}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a case and the reference's outputs (``ref``), drawn from seeds until every occupied transformed point is settled."""
    base = 1000 + 17 * sorted(CASES).index(name)
    for redraw in range(MAX_REDRAWS + 1):
        c = _draw(name, base + redraw)
        ref = reproject(c["src"], c["srcn"], c["match"], c["nn"], c["T"], c["sen"])
        if all(bool(pr.settled(q).all()) for q in ref["q"]):
            REDRAWS[name] = redraw
            c["ref"], c["seed"] = ref, base + redraw
            for v in (c["src"], c["srcn"], c["match"], c["nn"], c["T"], ref["moved4"], ref["paired9"], ref["src_pix"]):
                v.setflags(write=False)
            return c
    raise AssertionError(f"{name}: more than {MAX_REDRAWS} re-draws")
