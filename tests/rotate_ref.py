"""The contracts of dl_project_rotated and dl_rotations_from_draws (include/delora_hip.h) as plain references, no GPU, nothing taken
from the kernels' structure.

  rotated point   p' = R p with one coordinate = (r0 * x + r1 * y) + r2 * z, every operation rounded to fp32, nothing fused: numpy
                  float32 arithmetic is exactly that (``rotate_points``).  A matrix whose nine words are the bit pattern of the
                  identity is not applied at all, so -0.0, inf and NaN pass through (``is_identity_bits``).
  rotated scan    rows 0..2 are rotated; rows 3..5 too when the scan has at least six channels (stored normals); everything else passes
                  through (``rotate_scan``).  dl_project_rotated(scans, rot) is dl_project(rotate_scans(scans, rot)) on every output.
  draws -> matrix float64 (``rotations_from_draws``): row 2b the identity, row 2b+1 Rodrigues' matrix cos(a) I + sin(a) [d]x +
                  (1 - cos(a)) d d^T, d = (0, 0, 1) with only_yaw, else draws 0..2 normalised, a = (draw 3 - 0.5) * magnitude_rad.

``rotate_scans`` can also evaluate four plausible DEFECTS of an implementation; tests/test_rotate_ref_host.py proves that the cases
below tell each of them from the contract (the fifth defect of the list in tests/test_gpu_project_rotated.py -- staging record or uvr
taken from the unrotated point -- is a property of the kernel's data flow: every output compared there would show it).
"""
import functools

import numpy as np

from tests import project_ref as pr

f32, f64 = np.float32, np.float64
IDENTITY9 = np.eye(3, dtype=f32).reshape(9)
DEFECTS = ("transposed", "previous-row", "normals-unrotated", "contracted")


def is_identity_bits(R9):
    """True iff the nine fp32 words are 1.0 on the diagonal and +0.0 elsewhere (a -0.0 entry is NOT the identity)."""
    return bool(np.array_equal(np.asarray(R9, dtype=f32).reshape(9).view(np.uint32), IDENTITY9.view(np.uint32)))


def rotate_points(R9, xyz, contracted=False):
    """fp32 ``[3,n]`` -> R xyz, row k = (R[k,0] * x + R[k,1] * y) + R[k,2] * z in float32 arithmetic.  ``contracted``: the DEFECTIVE
    variant a compiler would produce by fusing: fma(r2, z, fma(r1, y, r0 * x))."""
    R = np.asarray(R9, dtype=f32).reshape(3, 3)
    x, y, z = (np.asarray(xyz[i], dtype=f32) for i in range(3))
    out = np.empty((3, x.shape[0]), dtype=f32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for k in range(3):
            if contracted:
                out[k] = pr.fma32(np.full_like(z, R[k, 2]), z, pr.fma32(np.full_like(y, R[k, 1]), y, pr.mul32(np.full_like(x, R[k, 0]), x)))
            else:
                a, b, c = R[k, 0] * x, R[k, 1] * y, R[k, 2] * z
                out[k] = (a + b) + c
    assert out.dtype == f32
    return out


def rotate_scan(R9, scan, defect=None):
    """fp32 ``[C,n]`` scan -> the scan dl_project_rotated projects.  An identity matrix (by its bits) returns the scan's own bits."""
    scan = np.asarray(scan, dtype=f32)
    if is_identity_bits(R9):
        return scan.copy()
    R9 = np.asarray(R9, dtype=f32).reshape(9)
    if defect == "transposed":
        R9 = np.ascontiguousarray(R9.reshape(3, 3).T).reshape(9)
    out = scan.copy()
    out[:3] = rotate_points(R9, scan[:3], contracted=defect == "contracted")
    if scan.shape[0] >= 6 and defect != "normals-unrotated":
        out[3:6] = rotate_points(R9, scan[3:6], contracted=defect == "contracted")
    return out


def rotate_scans(scans, rot, defect=None):
    """scans: list of fp32 ``[C,n]``; rot ``[S,9]`` fp32.  ``defect`` "previous-row": scan s takes row s - 1 (scan 0 the identity)."""
    rot = np.asarray(rot, dtype=f32).reshape(len(scans), 9)
    if defect == "previous-row":
        rot = np.concatenate([IDENTITY9[None], rot[:-1]], axis=0)
    return [rotate_scan(rot[s], scan, defect) for s, scan in enumerate(scans)]


def rodrigues(axis, angle):
    """float64 3x3 of a rotation by ``angle`` [rad] about ``axis`` (normalised here).  angle == 0 gives the identity exactly."""
    d = np.asarray(axis, dtype=f64)
    d = d / np.sqrt((d * d).sum())
    K = np.array([[0.0, -d[2], d[1]], [d[2], 0.0, -d[0]], [-d[1], d[0], 0.0]])
    return np.cos(angle) * np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * np.outer(d, d)


def angles_from_draws(draws, magnitude_rad):
    """float64 angles of fp32 draws ``[B,4]``; the magnitude is the fp32 number the C entry point receives."""
    return (np.asarray(draws, dtype=f32)[:, 3].astype(f64) - 0.5) * f64(f32(magnitude_rad))


def rotations_from_draws(draws, only_yaw, magnitude_rad):
    """float64 ``[2B,9]``: what dl_rotations_from_draws computes in fp32."""
    draws = np.asarray(draws, dtype=f32)
    B = draws.shape[0]
    out = np.zeros((2 * B, 9), dtype=f64)
    ang = angles_from_draws(draws, magnitude_rad)
    for b in range(B):
        out[2 * b] = np.eye(3).reshape(9)
        axis = (0.0, 0.0, 1.0) if only_yaw else draws[b, :3].astype(f64)
        if ang[b] == 0.0 or not np.any(np.asarray(axis) != 0.0):
            out[2 * b + 1] = np.eye(3).reshape(9)
        elif only_yaw:                                   # row and column 2 exact (cos + (1 - cos) need not round to 1)
            c, s = np.cos(ang[b]), np.sin(ang[b])
            out[2 * b + 1] = (c, -s, 0.0, s, c, 0.0, 0.0, 0.0, 1.0)
        else:
            out[2 * b + 1] = rodrigues(axis, ang[b]).reshape(9)
    return out


# ------------------------------------------------------------------------------------------------ the cases both tiers run

SENSOR = "ragged"                                    # 16 x 130: H*W % 256 != 0, a few milliseconds per call
CASE_C = (3, 6, 7)
CASE_S = (1, 2, 9, 16)
CASE_LENGTHS = (0, 1, 255, 256, 257, 3000)           # around the workgroup size; 3000: twelve workgroups per scan
CASE_AXES = {"yaw": (0.0, 0.0, 1.0), "general": (0.3, 0.5, 0.8)}
CASE_ANGLES_DEG = (2.0, 90.0, 180.0)
OFFS0, TAIL_COLS, PAD_COLS = pr.OFFS0, pr.TAIL_COLS, pr.PAD_COLS


def cases():
    """Every combination of C, S, axis and angle.  Which scans are rotated: the odd ones (the layout of a training batch: b.scan_2),
    and scan 0 when it is the only one.  Scan lengths cycle through CASE_LENGTHS from a start that moves with the case, so that every
    length is met by rotated and by unrotated scans; S = 1 and S = 2 run all six starts (``layouts``)."""
    out, i = [], 0
    for C in CASE_C:
        for S in CASE_S:
            for axis in CASE_AXES:
                for deg in CASE_ANGLES_DEG:
                    out.append({"name": f"C{C}-S{S}-{axis}-{deg:g}", "C": C, "S": S, "axis": axis, "deg": deg, "seed": 9000 + i,
                                "layouts": tuple(range(len(CASE_LENGTHS))) if S <= 2 else ((i // len(CASE_ANGLES_DEG)) % len(CASE_LENGTHS),)})
                    i += 1
    return out


def case_lengths(case, layout):
    L = len(CASE_LENGTHS)
    # odd and even scans walk the list in opposite directions: S = 9 meets four lengths on its rotated scans, S = 16 all six
    return [CASE_LENGTHS[(layout + s // 2) % L] if s % 2 else CASE_LENGTHS[(layout + 3 - s // 2) % L] for s in range(case["S"])]


@functools.lru_cache(maxsize=None)
def _cloud(n, scale, seed):
    p = pr.random_cloud(n, scale, seed) if n else np.zeros((3, 0), dtype=f32)
    p.setflags(write=False)
    return p


def case_scans(case, layout):
    """fp32 ``[C,n]`` scans of one layout of a case: random clouds of 10 m scale, aux channels from a seeded permutation (channels 3..5
    stand for stored normals: any vector shows whether it was rotated)."""
    scans = []
    for s, n in enumerate(case_lengths(case, layout)):
        seed = 7 * n + s + 100 * layout                 # (shared between cases: the clouds are generated once)
        scans.append(pr.with_aux(_cloud(n, 10.0, seed), case["C"], seed))
    return scans


def case_rotations(case):
    """fp32 ``[S,9]``: identity rows for the unrotated scans; rotated scan s turns by +angle, the next rotated one by -angle, ..."""
    S, a = case["S"], case["deg"] * np.pi / 180.0
    rot = np.tile(IDENTITY9, (S, 1))
    for s in range(S):
        if s % 2 or S == 1:
            rot[s] = rodrigues(CASE_AXES[case["axis"]], a if (s // 2) % 2 == 0 else -a).reshape(9).astype(f32)
    return rot
