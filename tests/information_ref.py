"""Plain float64 restatement of ``dl_icp_information`` (include/delora_hip.h, csrc/info.hip): the point-to-plane normal equations of
matched pairs at a pose, their covariance and the status rule with the Cholesky written out.  numpy only; the planes are those the
kernel streams:

    p  [B,3,HW]  source points          n  [B,3,HW]  source normals (only "is it the zero vector" matters)
    pt [B,3,HW]  matched target points  nt [B,3,HW]  matched target normals       nn [B,HW] int  (only the sign matters)
    T  [B,4,4]

Everything is evaluated in float64 from the inputs as given (fp32 inputs are promoted exactly), so on small-integer data the sums are
the exact integers the kernel's fp32 arithmetic produces as well, and on real data the result is the referee of a rounding bound.
Also here: the generators of the planted scenes both test files use.
"""
import numpy as np

OK, TOO_FEW_PAIRS, UNOBSERVABLE = 0, 1, 2
MIN_PIVOT = 1e-10


def weights(n, nt, nn):
    """w [B,HW] in {0,1}: matched, with a source normal and a matched normal."""
    return ((np.asarray(nn) >= 0) & (np.asarray(n) != 0).any(axis=1) & (np.asarray(nt) != 0).any(axis=1)).astype(np.float64)


def jacobian(p, pt, nt, T):
    """(J [B,HW,6], r [B,HW]) of every pixel, unmasked: q = R p + t, r = nt . (q - pt), J = (nt, q x nt)."""
    p, pt, nt, T = (np.asarray(a, dtype=np.float64) for a in (p, pt, nt, T))
    q = np.einsum("bij,bjk->bik", T[:, :3, :3], p) + T[:, :3, 3:4]
    r = ((q - pt) * nt).sum(axis=1)
    arm = np.cross(q, nt, axis=1)
    return np.concatenate([nt, arm], axis=1).transpose(0, 2, 1), r


def cholesky_status(A, K):
    """(status, L or None, s or None) of one 6x6 information matrix by the rule of the header."""
    if K <= 6.0:
        return TOO_FEW_PAIRS, None, None
    d = np.diag(A)
    if not all(x > 0.0 for x in d):
        return UNOBSERVABLE, None, None
    s = 1.0 / np.sqrt(d)
    L = np.zeros((6, 6))
    for j in range(6):
        piv = (A[j, j] * s[j]) * s[j]
        for c in range(j):
            piv -= L[j, c] * L[j, c]
        if not piv > MIN_PIVOT:
            return UNOBSERVABLE, None, None
        L[j, j] = np.sqrt(piv)
        for i in range(j + 1, 6):
            v = (A[i, j] * s[i]) * s[j]
            for c in range(j):
                v -= L[i, c] * L[j, c]
            L[i, j] = v / L[j, j]
    return OK, L, s


def finish(A, sum_r2, K):
    """(covariance [6,6], status) of one sample."""
    with np.errstate(all="ignore"):
        status, L, s = cholesky_status(A, K)
    if status != OK:
        return np.zeros((6, 6)), status
    Li = np.zeros((6, 6))
    for c in range(6):
        for i in range(c, 6):
            v = 1.0 if i == c else 0.0
            for j in range(c, i):
                v -= L[i, j] * Li[j, c]
            Li[i, c] = v / L[i, i]
    sigma2 = sum_r2 / (K - 6.0)
    cov = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            v = 0.0
            for c in range(j, 6):
                v += Li[c, i] * Li[c, j]
            cov[i, j] = cov[j, i] = sigma2 * ((v * s[i]) * s[j])
    return cov, status


def information(p, n, pt, nt, nn, T):
    """dict(info [B,6,6], rhs [B,6], stats [B,2], covariance [B,6,6], status [B] int32), float64."""
    w = weights(n, nt, nn)
    J, r = jacobian(p, pt, nt, T)
    Jw = J * w[:, :, None]
    with np.errstate(all="ignore"):
        info = np.einsum("bpi,bpj->bij", Jw, J)
        rhs = np.einsum("bpi,bp->bi", Jw, r)
        stats = np.stack([(w * r * r).sum(axis=1), w.sum(axis=1)], axis=1)
    B = info.shape[0]
    cov, status = np.zeros((B, 6, 6)), np.zeros((B,), dtype=np.int32)
    for b in range(B):
        cov[b], status[b] = finish(info[b], stats[b, 0], stats[b, 1])
    return {"info": info, "rhs": rhs, "stats": stats, "covariance": cov, "status": status}


def cost(p, n, pt, nt, nn, T, xi):
    """sum w r^2 [B] after the left perturbation q <- exp(omega^) q + v of every transformed point, xi = (v, omega) [6]."""
    v, om = np.asarray(xi[:3], dtype=np.float64), np.asarray(xi[3:], dtype=np.float64)
    th = np.linalg.norm(om)
    Kx = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * (Kx @ Kx)
    T = np.asarray(T, dtype=np.float64)
    T2 = T.copy()
    T2[:, :3, :3] = R @ T[:, :3, :3]
    T2[:, :3, 3] = (R @ T[:, :3, 3:4])[:, :, 0] + v
    _, r = jacobian(p, pt, nt, T2)
    return (weights(n, nt, nn) * r * r).sum(axis=1)


def scaled(info):
    """Ah = D^-1/2 info D^-1/2 of one sample."""
    s = 1.0 / np.sqrt(np.diag(info))
    return (info * s[:, None]) * s[None, :]


# ---------------------------------------------------------------------------------------------------- planted scenes


def integer_case(B, HW, seed=0, coord=8, density=0.8):
    """Small-integer planes: coordinates in [-coord, coord], normal entries in {-1, 0, 1}, T a quarter turn about z plus an integer
    translation.  All three classes of non-counting pixel occur (and hold finite garbage-free integers)."""
    rng = np.random.default_rng(seed)
    p = rng.integers(-coord, coord + 1, (B, 3, HW)).astype(np.float32)
    pt = rng.integers(-coord, coord + 1, (B, 3, HW)).astype(np.float32)
    n = rng.integers(-1, 2, (B, 3, HW)).astype(np.float32)
    nt = rng.integers(-1, 2, (B, 3, HW)).astype(np.float32)
    nn = np.where(rng.random((B, HW)) < density, rng.integers(0, HW, (B, HW)), -1).astype(np.int32)
    for b in range(B):                                               # plant each class where the draw did not
        k = np.arange(HW)
        nn[b, k % 7 == 3] = -1
        n[b][:, k % 11 == 5] = 0
        nt[b][:, k % 13 == 6] = 0
    T = np.zeros((B, 4, 4), dtype=np.float32)
    for b in range(B):
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][(seed + b) % 4]
        T[b] = np.eye(4)
        T[b, :2, :2] = [[c, -s], [s, c]]
        T[b, :3, 3] = rng.integers(-2, 3, 3)
    return {"p": p, "n": n, "pt": pt, "nt": nt, "nn": nn, "T": T}


def headroom(case):
    """Largest sum of absolute summands over the 29 accumulators and samples, as a fraction of 2^24 (< 1: every fp32 partial sum of
    the kernel is an exactly representable integer whatever the order)."""
    w = weights(case["n"], case["nt"], case["nn"])
    J, r = jacobian(case["p"], case["pt"], case["nt"], case["T"])
    with np.errstate(all="ignore"):
        Ja = np.abs(np.nan_to_num(J)) * w[:, :, None]
        ra = np.abs(np.nan_to_num(r))
        worst = max(np.einsum("bpi,bpj->bij", Ja, np.abs(np.nan_to_num(J))).max(), np.einsum("bpi,bp->bi", Ja, ra).max(), (w * ra * ra).sum(axis=1).max(),
                    w.sum(axis=1).max())
    return float(worst) / 2.0 ** 24


def _scene(points, normals, T_true, jitter, rng):
    """A matched case from target points with unit normals: the source is the target moved by T_true^-1 plus noise along the normal,
    the pose under test is T_true.  Returns planes [1,3,M] (float32) and T [1,4,4]."""
    pt = np.asarray(points, dtype=np.float64)
    nt = np.asarray(normals, dtype=np.float64)
    M = pt.shape[1]
    q = pt + nt * rng.normal(0.0, jitter, (1, M))
    Rt, tt = T_true[:3, :3], T_true[:3, 3:4]
    p = Rt.T @ (q - tt)
    n = Rt.T @ nt
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)[None]
    return {"p": f(p), "n": f(n), "pt": f(pt), "nt": f(nt), "nn": np.arange(M, dtype=np.int32)[None], "T": np.asarray(T_true, dtype=np.float32)[None]}


def small_pose(seed=0):
    rng = np.random.default_rng(seed)
    om = rng.normal(0, 0.02, 3)
    Kx = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + Kx + 0.5 * Kx @ Kx
    u, _, vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = u @ vt
    T[:3, 3] = rng.normal(0, 0.2, 3)
    return T


def box_room(M=600, seed=0, jitter=0.01):
    """Points on the six faces of a 10 x 8 x 3 box seen from inside: every direction is constrained (status 0)."""
    rng = np.random.default_rng(seed)
    half = np.array([5.0, 4.0, 1.5])
    face = rng.integers(0, 6, M)
    axis, sign = face // 2, np.where(face % 2 == 0, -1.0, 1.0)
    pts = rng.uniform(-1.0, 1.0, (3, M)) * half[:, None]
    nrm = np.zeros((3, M))
    pts[axis, np.arange(M)] = sign * half[axis]
    nrm[axis, np.arange(M)] = -sign
    return _scene(pts, nrm, small_pose(seed), jitter, rng)


def planar_scene(M=600, seed=0, jitter=0.01):
    """An open field: every normal is (0, 0, 1).  x, y and the rotation about z are unobservable (status 2)."""
    rng = np.random.default_rng(seed)
    pts = np.stack([rng.uniform(-20, 20, M), rng.uniform(-20, 20, M), np.full(M, -1.7)])
    nrm = np.zeros((3, M))
    nrm[2] = 1.0
    T = np.eye(4)
    T[:3, 3] = (0.3, -0.1, 0.05)
    return _scene(pts, nrm, T, jitter, rng)


def six_pair_scene(seed=0):
    """The box room with all but six pairs unmatched: K = 6 (status 1)."""
    case = box_room(64, seed)
    case["nn"][0, 6:] = -1
    return case
