"""The contract of dl_project_records (include/delora_hip.h) as a plain reference on top of tests/project_ref.py: numpy only, no GPU,
nothing taken from the kernel's structure.

  x, y, z  = the fp32 words at the three byte offsets of record i; no other byte of a record matters
  keep     = (!(filter & 1) or (x != 0 and y != 0 and z != 0))          -0.0 counts as zero, NaN does not
         and (!(filter & 2) or range_np > fp32(min_range))                 a NaN comparison is false
  range_np = sqrt((x*x + y*y) + z*z), every operation rounded to fp32, nothing fused: numpy.linalg.norm(xyz, axis=0), NOT the
             fused range of dl_project (project_ref.norm3)
  result   = project_ref.project of the kept points in their order, pix2pt mapped back to record indices, n_pass = their number

A layout here is ``(point_step, (off_x, off_y, off_z))`` in bytes.  The generators are seeded.
"""
import functools

import numpy as np

from tests import project_ref as pr

f32 = np.float32
DROP_ZERO, MIN_RANGE = 1, 2
THRESHOLD = 0.3                              # the node's minimum range [m] (odometry_publisher.py:96-97)
# (point_step; off_x, off_y, off_z) of the GPU tests: packed xyz, KITTI, xyz behind a leading word, permuted, PointCloud2-like strides
LAYOUTS = ((12, (0, 4, 8)), (16, (0, 4, 8)), (16, (4, 8, 12)), (20, (8, 0, 16)), (32, (0, 4, 8)), (48, (16, 20, 4)))


def range_np(xyz):
    """sqrt((x*x + y*y) + z*z) in np.float32 arithmetic (every numpy float32 operation is correctly rounded, nothing is fused)."""
    x, y, z = (np.asarray(xyz[i], dtype=f32) for i in range(3))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        r = np.sqrt((x * x + y * y) + z * z)
    assert r.dtype == f32
    return r


def keep_mask(xyz, flt, min_range=THRESHOLD, fused=False):
    """Which records take part.  ``fused``: the DEFECTIVE variant that compares dl_project's fused range (for the host tier)."""
    x, y, z = (np.asarray(xyz[i], dtype=f32) for i in range(3))
    keep = np.ones(x.shape, dtype=bool)
    if flt & DROP_ZERO:
        keep &= (x != 0) & (y != 0) & (z != 0)
    if flt & MIN_RANGE:
        with np.errstate(invalid="ignore"):
            keep &= (pr.norm3(x, y, z) if fused else range_np(xyz)) > f32(min_range)
    return keep


def pack(xyz, layout, fill):
    """fp32 ``[3,n]`` -> the ``n * point_step`` bytes of its records.  ``fill``: "ff" (every padding byte 0xFF) or an integer seed
    (random padding bits)."""
    step, offs = layout
    n = xyz.shape[1]
    if fill == "ff":
        raw = np.full((n, step), 0xFF, dtype=np.uint8)
    else:
        raw = pr._rng(fill).integers(0, 256, (n, step), dtype=np.uint8)
    for c, o in enumerate(offs):
        raw[:, o:o + 4] = np.ascontiguousarray(xyz[c], dtype="<f4").view(np.uint8).reshape(n, 4)
    return raw.reshape(-1)


def unpack(raw, layout):
    step, offs = layout
    raw = np.asarray(raw, dtype=np.uint8).reshape(-1, step)
    return np.stack([np.ascontiguousarray(raw[:, o:o + 4]).view("<f4")[:, 0] for o in offs]).astype(f32)


def project_records_ref(scans, sen, flt, min_range=THRESHOLD):
    """scans: list of fp32 ``[3,n]`` (the unpacked records).  The outputs of dl_project_records: image4, packed, pix2pt (record indices),
    kept, n_pass."""
    keeps = [keep_mask(s, flt, min_range) for s in scans]
    ref = pr.project([np.ascontiguousarray(s[:, k]) for s, k in zip(scans, keeps)], sen, 3)
    pix2pt = ref["pix2pt"].copy()
    for s, k in enumerate(keeps):
        idx = np.nonzero(k)[0].astype(np.int32)
        occ = pix2pt[s] >= 0
        pix2pt[s][occ] = idx[pix2pt[s][occ]]
    return {"image4": ref["image4"], "packed": ref["packed"], "pix2pt": pix2pt, "kept": ref["kept"],
            "n_pass": np.array([int(k.sum()) for k in keeps], dtype=np.int32)}


# ------------------------------------------------------------------------------------------------ generators

THRESHOLD_CANDIDATES = 100000
THRESHOLD_MIN_DISAGREE = 100


@functools.lru_cache(maxsize=None)
def threshold_cloud(name, seed=77):
    """Directions inside the sensor's field of view times ranges within +-4 ulp of fp32(0.3): the fused and the unfused range fall
    on different sides of the threshold for 0.6 % of such points (642 of the 100 000 generated here).  Asserts that at least 100 of them do."""
    sen, rng = pr.sensor(name), pr._rng(seed)
    n = THRESHOLD_CANDIDATES
    az, el = pr._inside_angles(sen, n, rng, "az"), pr._inside_angles(sen, n, rng, "el")
    r = pr.step_ulps(np.full(n, THRESHOLD, dtype=f32), rng.integers(-4, 5, n)).astype(np.float64)
    p = pr._polar(az, el, r)
    p = np.ascontiguousarray(p[:, pr.settled(p)])
    differ = keep_mask(p, MIN_RANGE) != keep_mask(p, MIN_RANGE, fused=True)
    assert int(differ.sum()) >= THRESHOLD_MIN_DISAGREE, int(differ.sum())
    p.setflags(write=False)
    return p


REMOVED_MIN_PIXELS = 32


@functools.lru_cache(maxsize=None)
def removed_winner_cloud(name):
    """A valid point at the centre of every pixel (range 10 ... 20) and, in front of many of them, a record the filter removes:
      * two pixels out of three: the same direction at range 0.2 (<= 0.3: removed by MIN_RANGE only),
      * the row that holds elevation 0: z = +0.0 / -0.0 alternating at range 5 (removed by DROP_ZERO only),
      * the column that holds azimuth +90 degrees: x = +0.0 / -0.0 at range 4 (DROP_ZERO only).
    Blockers stand before their pixel's valid point in the even columns and behind it in the odd ones.  Asserts on the host reference
    that at least 32 pixels change winner between filter 0 and filter 3, and at least 8 under each single flag."""
    sen = pr.sensor(name)
    rows, cols = np.meshgrid(np.arange(sen.H), np.arange(sen.W), indexing="ij")
    rows, cols = rows.reshape(-1), cols.reshape(-1)
    az = sen.hfov[0] + cols / (sen.W - 1) * (sen.hfov[1] - sen.hfov[0])
    el = sen.vfov[0] + rows / (sen.H - 1) * (sen.vfov[1] - sen.vfov[0])
    valid = pr._polar(az, el, 10.0 + 10.0 * ((rows * 7 + cols * 3) % 11) / 11.0)
    near = pr._polar(az, el, np.full(len(az), 0.2))
    flat = pr._polar(az[:sen.W], np.zeros(sen.W), np.full(sen.W, 5.0))
    flat[2] = np.where(np.arange(sen.W) % 2 == 0, f32(0.0), f32(-0.0))
    side = pr._polar(np.full(sen.H, np.pi / 2), el[::sen.W], np.full(sen.H, 4.0))
    side[0] = np.where(np.arange(sen.H) % 2 == 0, f32(0.0), f32(-0.0))
    has_near, before = (rows + cols) % 3 != 0, cols % 2 == 0          # (a pixel without a near blocker shows its zero-coordinate one)
    cloud = np.concatenate([near[:, has_near & before], flat[:, ::2], side[:, ::2], valid, near[:, has_near & ~before], flat[:, 1::2],
                            side[:, 1::2]], axis=1)
    cloud = np.ascontiguousarray(cloud[:, pr.settled(cloud)])
    win = {flt: project_records_ref([cloud], sen, flt)["pix2pt"][0] for flt in (0, 1, 2, 3)}
    assert int((win[0] != win[3]).sum()) >= REMOVED_MIN_PIXELS, int((win[0] != win[3]).sum())
    assert int((win[0] != win[1]).sum()) >= 8 and int((win[0] != win[2]).sum()) >= 8 and int((win[1] != win[3]).sum()) >= 8
    cloud.setflags(write=False)
    return cloud


def odd_values():
    """Zeros, -0.0, NaN, +-inf and denormals in every coordinate, next to ordinary values on either side of the threshold."""
    v = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 0.1, -0.2, 0.3, 5.0], dtype=f32)
    return np.stack(np.meshgrid(v, v, v, indexing="ij")).reshape(3, -1)
