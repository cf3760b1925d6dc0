"""Referee of the kernels between the trunk's last convolution and the scalar that is minimised: global average pooling (fp32, half,
fused backward), the fp32 -> half cast, the fused pose heads (csrc/heads.hip), quaternion -> T (csrc/pose.hip) and the ICP loss
with its gradient moments (csrc/loss.hip).

Two tiers, as for the convolutions (tests/conv_ref.py):

  * EXACT.  On small-integer data every product and every partial sum is an fp32 number whatever order a kernel adds them in
    (``loss_headroom`` / ``heads_headroom`` / ``pool_headroom`` prove it per case: the sum of the ABSOLUTE values of the summands of
    every accumulator stays below 2^24 grid steps), so the kernel's result must equal a float64 evaluation BIT FOR BIT after the
    kernel's own last step (one float64 division rounded to fp32, one fp32 square root, one fp32 quotient).
  * FLOAT64.  On real-valued data the deviation from float64 is bounded, per output element, by a first-order rounding bound
    that is derived from the operation counts of the formulas (written out below), never from what a GPU returned.

The references are written from the formulas in include/delora_hip.h and the header of csrc/loss.hip.  ``*_f32`` are plain
fp32 CPU evaluations of the same formulas (numpy / torch, no fused multiply-add, pairwise sums): what tests/test_tail_ref_host.py
feeds the comparisons as "got", unchanged (must pass) and with value-only mutations (must be rejected).

No GPU is needed to import this module.
"""
import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32 (round to nearest)
LIMIT = 2.0 ** 24                    # integers below this magnitude are fp32 numbers
P2P, PO2PL, PL2PL, LINEAR, ALONE = 1, 2, 4, 8, 16

# ---------------------------------------------------------------------------------------------------- case tables
# H*W of the loss cases and why (B = 3 unless said otherwise; the share of valid pixels differs per sample)
LOSS_HW = [
    (1, "one pixel"), (3, "below a chunk, scalar"), (4, "below a chunk, vector flag set"),
    (252, "under one 256-pixel chunk, multiple of 4"), (255, "under one chunk, scalar only"), (256, "exactly one vector chunk"),
    (257, "one chunk + 1, scalar only"), (260, "vector chunk plus ragged chunk in the next wave"),
    (1021, "several chunks, unaligned"), (1024, "exactly one workgroup"), (1028, "a second workgroup with one partial chunk"),
    (25600, "25 partial rows: the reduction's 25 slices exactly full"), (26000, "26 partial rows: the slices wrap"),
    (131072, "the workgroup cap reached exactly, one chunk per wave"), (131076, "513 chunks: wave 0 runs a vector chunk, then the ragged one"),
    (131333, "odd size: all scalar, with the wave loop"), (262404, "more than two rounds of the wave loop plus a tail"),
]
LOSS_ALL_FLAGS_HW = (260, 1028)                       # these run all 16 flag words, ALONE | P2P and ALONE
LOSS_B17_HW = 260                                     # dl_icp_loss_bwd crosses its 256-thread block at B = 17 (272 threads)
LOSS_INSTANCES = [PO2PL | PL2PL, PO2PL | PL2PL | LINEAR, P2P | PO2PL | PL2PL, P2P | PO2PL | PL2PL | LINEAR]   # (P2P x LINEAR) of k_icp_loss
LOSS_FLAG_WORDS = list(range(16)) + [ALONE | P2P, ALONE]
VALID_SHARE = (0.9, 0.55, 0.2)                        # per sample b % 3
ZERO_SRC_NORMAL, ZERO_TGT_NORMAL = 0.3, 0.25          # planted zero normals on either side

# (B, F, R, Hd) of the heads
HEADS_SHAPES = [(1, 4, 1, 1), (3, 70, 41, 5), (16, 768, 40, 8), (5, 2500, 64, 64), (16, 1000, 130, 33), (8, 512, 1000, 100)]
HEADS_MODEL_SHAPE = HEADS_SHAPES[-1]

MEAN_P = [1, 63, 64, 65, 127, 128, 129, 4096]
MEAN_C = {"f32": [4, 20, 512], "half": [8, 24, 512]}
MEAN_N = [1, 3]
QUAT_B = [1, 64, 65, 130]
ELEMENTWISE_N = [8, 2040, 2048, 2056]                  # n = 8, and either side of one 256-thread block of 8-element groups


def loss_blocks(HW):
    """Workgroups (= partial rows) per sample, from the description in csrc/loss.hip: 256-pixel chunks, 4 waves, at most 128."""
    chunks = -(-HW // 256)
    return min(-(-chunks // 4), 128)


def heads_kc(B, K):
    """Reduction elements per sample that k_heads_rows stages in LDS at a time (48 KiB, a multiple of 64)."""
    kc = (48 * 1024 // 4 // B) & ~63
    return K if kc >= K else kc


# ---------------------------------------------------------------------------------------------------- ICP loss: reference

ACC_NAMES = (["rr"] + [f"rn{i}" for i in range(3)] + [f"rnp{i}{j}" for i in range(3) for j in range(3)] + ["ss"]
             + [f"G{i}{j}" for i in range(3) for j in range(3)] + ["K", "dd"] + [f"d{i}" for i in range(3)]
             + [f"dp{i}{j}" for i in range(3) for j in range(3)] + ["K2"])
assert len(ACC_NAMES) == 38


def _has(n):
    return (n != 0).any(axis=0)


def loss_summands(p, n, pt, nt, nn, T, flags, xp=np.float64, has=_has, absolute=False):
    """The 38 per-pixel summands [38, P] of one sample in dtype ``xp``:
         0 r^2 | 1-3 r nt | 4-12 r nt p^T | 13 |Rn - nt|^2 or (1 - Rn.nt)^2 | 14-22 (Rn - nt) n^T or -(1 - Rn.nt) nt n^T | 23 pair
         24 |d|^2 | 25-27 d | 28-36 d p^T | 37 pair without normals              r = nt.d, d = R p + t - pt
       masked by the pair selection (valid, both normals non-zero / neither, ALONE: every valid pixel is point-to-point).
       ``absolute`` gives the majorant: the same expression with every operand replaced by its absolute value."""
    a = (lambda v: np.abs(v)) if absolute else (lambda v: v)
    p, n, pt, nt = (a(np.asarray(v, dtype=xp)) for v in (p, n, pt, nt))
    R, t = a(np.asarray(T, dtype=xp)[:3, :3]), a(np.asarray(T, dtype=xp)[:3, 3:4])
    one = xp(1.0)
    valid = np.asarray(nn) >= 0
    hs, ht = has(n), has(nt)
    alone = bool(flags & ALONE)
    w = (valid & hs & ht & (not alone)).astype(xp)
    w2 = (valid & (np.ones_like(hs) if alone else (~hs & ~ht))).astype(xp)
    sub = (lambda x, y: x + y) if absolute else (lambda x, y: x - y)
    d = sub((R @ p) + t, pt)
    rn = R @ n
    r = w * (d * nt).sum(axis=0)
    g = r[None] * nt
    out = [r * r, g[0], g[1], g[2]] + [g[i] * p[j] for i in range(3) for j in range(3)]
    if flags & LINEAR:
        c = w * sub(one, (rn * nt).sum(axis=0))
        e = (c[None] * nt) if absolute else (-c[None] * nt)
        out.append(c * c)
    else:
        e = w[None] * sub(rn, nt)
        out.append((e * e).sum(axis=0))
    out += [e[i] * n[j] for i in range(3) for j in range(3)] + [w]
    u = w2[None] * d
    out += [(u * u).sum(axis=0), u[0], u[1], u[2]] + [u[i] * p[j] for i in range(3) for j in range(3)] + [w2]
    return np.stack(out)


def loss_finish(tot, flags):
    """The last step of dl_icp_loss_reduce on the 38 float64 totals of one sample: (loss_terms [3] fp32, pair_counts [2] int32,
    grad_terms [3][12] fp32).  Means as torch's MSELoss: an enabled term over an empty set is 0/0 = NaN; a disabled term is 0;
    the pair counts do not depend on which terms are enabled, except that K' is counted only when point-to-point is."""
    tot = np.asarray(tot, dtype=np.float64).copy()
    p2p = bool(flags & P2P)
    if not p2p:
        tot[24:] = 0.0
    K, K2 = tot[23], tot[37]
    lt, g = np.zeros(3, np.float32), np.zeros((3, 12), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        if p2p:
            lt[0] = np.float32(tot[24] / (3.0 * K2))
        if flags & PO2PL:
            lt[1] = np.float32(tot[0] / K)
        if flags & PL2PL:
            lt[2] = np.float32(tot[13] / K)
        for i in range(3):
            for j in range(4):
                e = i * 4 + j                                             # row-major [R | t]: column 3 is d/dt
                if p2p:
                    g[0, e] = np.float32(2.0 * (tot[28 + i * 3 + j] if j < 3 else tot[25 + i]) / (3.0 * K2))
                if flags & PO2PL:
                    g[1, e] = np.float32(2.0 * (tot[4 + i * 3 + j] if j < 3 else tot[1 + i]) / K)
                if flags & PL2PL:
                    g[2, e] = np.float32(2.0 * (tot[14 + i * 3 + j] if j < 3 else 0.0) / K)
    return lt, np.array([int(K), int(K2)], np.int32), g


def loss_totals(case, flags, what="tot"):
    """[B,38] float64 per sample: "tot" the sums of the summands, "abssum" the sums of their absolute values (the headroom's
    quantity), "abs" the sums of the majorants.  They depend on LINEAR and ALONE only, so one evaluation serves every flag word
    that shares those two bits (kept with the case)."""
    key = (bool(flags & LINEAR), bool(flags & ALONE))
    cache = case.setdefault("_totals", {})
    B = case["T"].shape[0]
    args = lambda b: (case["p"][b], case["n"][b], case["pt"][b], case["nt"][b], case["nn"][b], case["T"][b], flags)
    if ("tot",) + key not in cache:
        s = [loss_summands(*args(b)) for b in range(B)]
        cache[("tot",) + key] = np.stack([v.sum(axis=1) for v in s])
        cache[("abssum",) + key] = np.stack([np.abs(v).sum(axis=1) for v in s])
    if what == "abs" and ("abs",) + key not in cache:
        cache[("abs",) + key] = np.stack([loss_summands(*args(b), absolute=True).sum(axis=1) for b in range(B)])
    return cache[(what,) + key]


def icp_loss(case, flags, majorant=False):
    """float64 reference of dl_icp_loss_fwd on a generated case: dict of loss_terms [B,3], pair_counts [B,2], grad_terms [B,3,12]
    (fp32 / int32, after the kernel's last step), tot [B,38] (float64 totals) and, with ``majorant``, abs [B,38] (float64 sums of
    the majorants)."""
    tot = loss_totals(case, flags)
    fin = [loss_finish(t, flags) for t in tot]
    out = {"loss_terms": np.stack([f[0] for f in fin]), "pair_counts": np.stack([f[1] for f in fin]),
           "grad_terms": np.stack([f[2] for f in fin]), "tot": tot}
    if majorant:
        out["abs"] = loss_totals(case, flags, "abs")
    return out


def icp_loss_bwd(grad_terms, w):
    """grad_T [B,4,4] fp32 of dl_icp_loss_bwd: ((w0 g0) + (w1 g1)) + (w2 g2), every operation rounded to fp32, row 3 zero."""
    g, w = np.asarray(grad_terms, np.float32), np.asarray(w, np.float32)
    with np.errstate(invalid="ignore"):
        v = ((w[:, 0, None] * g[:, 0]) + (w[:, 1, None] * g[:, 1])) + (w[:, 2, None] * g[:, 2])
    out = np.zeros((g.shape[0], 4, 4), np.float32)
    out[:, :3, :] = v.reshape(-1, 3, 4)
    return out


def torch_loss_terms(T, src, src_n, tgt, tgt_n, nn, mode, p2p, alone=False):
    """The three loss modules as plain torch ops (icp_losses.py:102-121,168-240 with the gathers the reference performs) in the
    dtype and on the device of the arguments, differentiable with respect to T.  src / tgt [B,>=3,...], normals [B,3,...], nn
    [B,...] target pixel per source pixel (-1: none).  Returns (terms [B,3] = po2po, po2pl, pl2pl; K per sample; K' per sample)."""
    rows = []
    for b in range(src.shape[0]):
        idx = nn[b].reshape(-1).long()
        valid = idx >= 0
        idx = idx.clamp(min=0)
        p, n = src[b, :3].reshape(3, -1), src_n[b].reshape(3, -1)
        pt, nt = tgt[b, :3].reshape(3, -1)[:, idx], tgt_n[b].reshape(3, -1)[:, idx]
        R, t = T[b, :3, :3], T[b, :3, 3:4]
        q, rn = R @ p + t, R @ n
        has_s, has_t = (n != 0).any(dim=0), (nt != 0).any(dim=0)
        m = valid & has_s & has_t & (not alone)
        K = m.sum()
        r = ((q - pt) * nt).sum(dim=0)
        po2pl = (r[m] ** 2).sum() / K
        if mode == "linear":
            pl2pl = ((1.0 - (rn * nt).sum(dim=0))[m] ** 2).sum() / K
        else:
            pl2pl = ((rn - nt)[:, m] ** 2).sum() / K
        po2po = torch.zeros((), device=src.device, dtype=T.dtype)
        K2 = torch.zeros((), device=src.device)
        if p2p:
            m2 = valid & (torch.ones_like(has_s) if alone else (~has_s & ~has_t))
            K2 = m2.sum()
            po2po = ((q - pt)[:, m2] ** 2).sum() / (3 * K2)
        rows.append((torch.stack((po2po, po2pl, pl2pl)), int(K), int(K2)))
    return torch.stack([r[0] for r in rows]), [r[1] for r in rows], [r[2] for r in rows]


# ---------------------------------------------------------------------------------------------------- ICP loss: generators


def _rng(*seed):
    return np.random.default_rng([int(s) for s in seed])      # PCG64: the same stream on every platform


def _with_zero_vectors(r, v, rate):
    v = v.copy()
    v[:, r.random(v.shape[1]) < rate] = 0
    return v


def loss_case_exact(HW, B=3, seed=0, full=False):
    """Small-integer planes of B samples: dict of float64 arrays p, n, pt, nt [B,3,HW], nn [B,HW] int32, T [B,4,4].
    Source points in [-4,4], normals and matched normals in {-1,0,1}^3 with zero vectors planted (ZERO_*_NORMAL), a different
    full non-symmetric R per sample with entries in {-1,0,1}, integer t in [-3,3], matched point R p + t + delta with delta in
    [-2,2]^3, nn >= 0 on VALID_SHARE[b % 3] of the pixels and negative (-1, or INT32_MIN) elsewhere, where the matched planes
    hold zeros as dl_nn_correspond leaves them.  ``full``: every pixel valid (the headroom's worst case)."""
    c = {k: [] for k in ("p", "n", "pt", "nt", "nn", "T")}
    for b in range(B):
        r = _rng(seed, HW, b)
        p = r.integers(-4, 5, (3, HW)).astype(np.float64)
        n = _with_zero_vectors(r, r.integers(-1, 2, (3, HW)).astype(np.float64), ZERO_SRC_NORMAL)
        nt = _with_zero_vectors(r, r.integers(-1, 2, (3, HW)).astype(np.float64), ZERO_TGT_NORMAL)
        R = r.integers(-1, 2, (3, 3)).astype(np.float64)
        while np.array_equal(R, R.T) or np.count_nonzero(R) < 6:
            R = r.integers(-1, 2, (3, 3)).astype(np.float64)
        t = r.integers(-3, 4, (3, 1)).astype(np.float64)
        pt = R @ p + t + r.integers(-2, 3, (3, HW))
        valid = np.ones(HW, bool) if full else r.random(HW) < VALID_SHARE[b % 3]
        nn = np.where(valid, r.integers(0, 2 ** 31 - 1, HW), np.where(r.random(HW) < 0.5, -1, -2 ** 31)).astype(np.int32)
        pt[:, ~valid] = 0
        nt[:, ~valid] = 0
        T = np.eye(4)
        T[:3, :3], T[:3, 3:] = R, t
        for k, v in zip(("p", "n", "pt", "nt", "nn", "T"), (p, n, pt, nt, nn, T)):
            c[k].append(v)
    return {k: np.stack(v) for k, v in c.items()}


def _rot(r, angle):
    a = r.normal(size=3)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def loss_case_real(HW, kind, B=3, seed=0, scale=1.0):
    """Real-valued fp32 planes (returned as float64 arrays holding fp32 values).  kind "random": unrelated clouds and poses;
    "converged": the matched point is the transformed source point plus noise of 1e-3 of the scene, matched normal = rotated
    normal plus small noise -- the gradient is then a cancelling sum; ``scale``: size of the scene in metres."""
    c = {k: [] for k in ("p", "n", "pt", "nt", "nn", "T")}
    for b in range(B):
        r = _rng(seed, HW, b, 77)
        p = r.normal(size=(3, HW)) * 10.0 * scale
        n = r.normal(size=(3, HW))
        n /= np.linalg.norm(n, axis=0)
        n = _with_zero_vectors(r, n, ZERO_SRC_NORMAL)
        n[0, r.random(HW) < 0.1] = 0                                      # normals in the y-z plane: has-normal must look at all components
        R = _rot(r, r.uniform(0.0, 0.3) if kind == "converged" else r.uniform(0.0, np.pi))
        t = r.normal(size=(3, 1)) * scale
        if kind == "converged":
            pt = R @ p + t + r.normal(size=(3, HW)) * 1e-3 * scale
            nt = R @ n + r.normal(size=(3, HW)) * 1e-3
        else:
            pt = r.normal(size=(3, HW)) * 10.0 * scale
            nt = r.normal(size=(3, HW))
        nt /= np.maximum(np.linalg.norm(nt, axis=0), 1e-30)
        nt = _with_zero_vectors(r, nt, ZERO_TGT_NORMAL)
        nt[:, ~_has(n)] *= (r.random(int((~_has(n)).sum())) < 0.5)       # pairs without a normal on either side exist as well
        valid = r.random(HW) < VALID_SHARE[b % 3]
        nn = np.where(valid, r.integers(0, 2 ** 31 - 1, HW), -1).astype(np.int32)
        pt[:, ~valid] = 0
        nt[:, ~valid] = 0
        T = np.eye(4)
        T[:3, :3], T[:3, 3:] = R, t
        f = lambda v: v.astype(np.float32).astype(np.float64)
        for k, v in zip(("p", "n", "pt", "nt", "nn", "T"), (f(p), f(n), f(pt), f(nt), nn, f(T))):
            c[k].append(v)
    return {k: np.stack(v) for k, v in c.items()}


def loss_garbage(case, seed=1):
    """The same case with non-zero INTEGER garbage in all thirteen planes at pixels with nn < 0 (nn itself another negative
    number), and non-zero integer normals swapped in at valid pixels whose PARTNER has no normal -- nothing may change: the
    kernel masks by multiplication, so finite operands at pixels that do not count contribute exact zeros."""
    g = {k: v.copy() for k, v in case.items() if not k.startswith("_")}
    r = _rng(seed, 99)
    for b in range(g["nn"].shape[0]):
        bad = g["nn"][b] < 0
        for k in ("p", "n", "pt", "nt"):
            junk = r.integers(1, 6, g[k][b].shape) * r.choice([-1, 1], g[k][b].shape)
            g[k][b][:, bad] = junk[:, bad]
        g["nn"][b][bad] = -r.integers(1, 2 ** 31, int(bad.sum()))
        hs, ht = _has(case["n"][b]), _has(case["nt"][b])
        g["n"][b][:, ~bad & hs & ~ht] *= 5                               # a normal whose partner has none: the pair counts nowhere
        g["nt"][b][:, ~bad & ~hs & ht] *= -3
    return g


def loss_headroom(case, flags):
    """Proof obligation of the exact tier: per sample and accumulator (all 38) the float64 sum of the ABSOLUTE values of the
    summands is below 2^24, and the data are integers.  Then every partial sum in any order is an integer below 2^24, i.e. exact
    in fp32, and the fp64 stage is exact.  Returns the worst sum as a fraction of 2^24."""
    for k in ("p", "n", "pt", "nt", "T"):
        assert np.array_equal(case[k], np.rint(case[k])), f"loss_headroom: {k} is not integer-valued"
    worst = float(loss_totals(case, flags, "abssum").max())
    assert worst < LIMIT, f"loss_headroom: an accumulator reaches {worst:.0f} >= 2^24 -- the case would no longer be exact"
    return worst / LIMIT


# ---------------------------------------------------------------------------------------------------- ICP loss: float64 bound
# Rounded fp32 operations on the way to ONE summand, counted from csrc/loss.hip's accumulate_pair2 (every fma, mul, add, sub
# rounds once; a product inside an fma does not; multiplying by the 0/1 mask is exact).  First order: a value with c roundings
# carries a relative error of at most c u of its majorant, a product of two such values the sum of their counts.
#   q   = fma(m2, z, fma(m1, y, mul(m0, x))) + m3                                4
#   d   = q - pt                                                                  5
#   r   = w * fma(dz, ntz, fma(dy, nty, dx * ntx))                            5 + 3 = 8
#   rr  : fma(r, r, acc) -> the product r r                                    8 + 8 = 16      (the fma's rounding is the lane's addition)
#   g   = r * nt                                                                  9     -> acc 1-3 (added), acc 4-12 (fma(g, p, acc))
#   Rn  = fma(m2, nz, fma(m1, ny, mul(m0, nx)))                                   3
#   squared: e = w * (Rn - nt)  4;  ss = fma(ez, ez, fma(ey, ey, ex * ex))   2 * 4 + 3 = 11;  G = fma(e, n, acc)  4
#   linear:  c = w * (1 - fma(Rnz, ntz, fma(Rny, nty, Rnx * ntx)))       3 + 3 + 1 = 7;  ss = fma(c, c, acc)  14;  e = -c * nt  8 = G
#   point-to-point: u = w2 * d  5;  dd = fma(uz, uz, fma(uy, uy, ux * ux))   2 * 5 + 3 = 13;  d, d p^T  5
#   the two pair counts are sums of 0 / 1 far below 2^24: exact
LOSS_C_TERM = 16                     # the longest of these paths (r^2); per accumulator:


def loss_c_term(flags):
    lin = bool(flags & LINEAR)
    return np.array([16] + [9] * 12 + [14 if lin else 11] + [8 if lin else 4] * 9 + [0] + [13] + [5] * 12 + [0], dtype=np.float64)


def loss_c_sum(HW):
    """fp32 additions a summand passes through before the fp64 stage (csrc/loss.hip): a lane adds two pixel pairs per 256-pixel
    chunk into each of its even/odd partial sums and walks ceil(chunks / waves) chunks (waves = 4 per workgroup), then the
    even/odd add (1), two quad steps (2), two row rotations (2) and 16 LDS rows added to zero (15 that round)."""
    chunks = -(-HW // 256)
    per_wave = -(-chunks // (4 * loss_blocks(HW)))
    return 2 * per_wave + 1 + 2 + 2 + 15


def _ulp32(v):
    v = np.abs(np.asarray(v, dtype=np.float64))
    return np.where(np.isfinite(v), np.spacing(np.maximum(v, 2.0 ** -126).astype(np.float32)).astype(np.float64), 0.0)


def loss_bounds(ref, flags, HW):
    """Per output element the bound (c_term + c_sum) 2^-24 S_abs on its accumulator, carried through the final division, plus
    one ulp of the output (0 for a disabled term): dict of loss_terms [B,3], grad_terms [B,3,12]."""
    ba = (loss_c_term(flags) + loss_c_sum(HW))[None] * U * ref["abs"]                  # [B,38]
    B = ba.shape[0]
    K, K2 = ref["tot"][:, 23], ref["tot"][:, 37] * (1 if flags & P2P else 0)
    lt, g = np.zeros((B, 3)), np.zeros((B, 3, 12))
    with np.errstate(invalid="ignore", divide="ignore"):
        lt[:, 0], lt[:, 1], lt[:, 2] = ba[:, 24] / (3 * K2), ba[:, 0] / K, ba[:, 13] / K
        for i in range(3):
            for j in range(4):
                e = i * 4 + j
                g[:, 0, e] = 2 * (ba[:, 28 + i * 3 + j] if j < 3 else ba[:, 25 + i]) / (3 * K2)
                g[:, 1, e] = 2 * (ba[:, 4 + i * 3 + j] if j < 3 else ba[:, 1 + i]) / K
                g[:, 2, e] = 2 * (ba[:, 14 + i * 3 + j] if j < 3 else 0.0) / K
    lt, g = lt + _ulp32(ref["loss_terms"]), g + _ulp32(ref["grad_terms"])
    for k, bit in enumerate((P2P, PO2PL, PL2PL)):              # a disabled term is exactly 0: anything else is an error of any size
        if not flags & bit:
            lt[:, k], g[:, k] = 0.0, 0.0
    return {"loss_terms": lt, "grad_terms": g}


def loss_exact64(ref, flags):
    """The unrounded float64 outputs (the same last step without the rounding to fp32): what the float64 tier measures against."""
    B = ref["tot"].shape[0]
    lt, g = np.zeros((B, 3)), np.zeros((B, 3, 12))
    tot = ref["tot"]
    K, K2 = tot[:, 23], tot[:, 37] * (1 if flags & P2P else 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if flags & P2P:
            lt[:, 0] = tot[:, 24] / (3 * K2)
        if flags & PO2PL:
            lt[:, 1] = tot[:, 0] / K
        if flags & PL2PL:
            lt[:, 2] = tot[:, 13] / K
        for i in range(3):
            for j in range(4):
                e = i * 4 + j
                if flags & P2P:
                    g[:, 0, e] = 2 * (tot[:, 28 + i * 3 + j] if j < 3 else tot[:, 25 + i]) / (3 * K2)
                if flags & PO2PL:
                    g[:, 1, e] = 2 * (tot[:, 4 + i * 3 + j] if j < 3 else tot[:, 1 + i]) / K
                if flags & PL2PL:
                    g[:, 2, e] = 2 * (tot[:, 14 + i * 3 + j] if j < 3 else 0.0 * K) / K
    return {"loss_terms": lt, "grad_terms": g}


def same_bits(got, ref):
    """Number of elements that differ in value, as tests/conv_ref.mismatches counts them: NaN equals NaN (the sign and payload of
    an invalid operation's NaN are the machine's) and the two zeros equal each other; anything else is compared exactly."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    if got.dtype.kind == "f":
        return int((~((got == ref) | (np.isnan(got) & np.isnan(ref)))).sum())
    return int((got != ref).sum())


def compare_loss_exact(got, ref):
    """Mismatching elements of loss_terms, pair_counts and grad_terms (bitwise tier)."""
    return {k: same_bits(np.asarray(got[k]), ref[k]) for k in ("loss_terms", "pair_counts", "grad_terms")}


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements, NaN positions having to agree (returned as inf if they do not)."""
    got, want, bound = (np.asarray(v, dtype=np.float64) for v in (got, want, bound))
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    err = np.abs(got - want)[~nan]
    b = bound[~nan]
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    return float(ratio.max())


def compare_loss_real(got, ref, flags, HW):
    """Worst error / bound of loss_terms and grad_terms against float64; the pair counts must be equal (-> inf otherwise)."""
    want, bnd = loss_exact64(ref, flags), loss_bounds(ref, flags, HW)
    out = {k: worst_ratio(got[k], want[k], bnd[k]) for k in ("loss_terms", "grad_terms")}
    if not np.array_equal(np.asarray(got["pair_counts"]), ref["pair_counts"]):
        out["loss_terms"] = float("inf")
    return out


# ---------------------------------------------------------------------------------------------------- ICP loss: fp32 CPU evaluation


def _sum32(v):
    return np.sum(v, axis=1, dtype=np.float32)          # numpy's pairwise summation in fp32


def icp_loss_f32(case, flags, mutation=None):
    """fp32 CPU evaluation of the same formulas (every operation rounded to fp32, no fma, pairwise sums, the last step in
    float64 as the kernel's) -- a stand-in for a kernel in the host tests -- optionally with ONE value-only defect:
      "drop_pixel"   the counted pixel with the largest residual of every sample is left out
      "swap_columns" two moment columns (d/dR[:,0] and d/dR[:,1]) of every gradient are exchanged
      "skip_chunk"   the last 256-pixel chunk is not summed
      "has_one"      has-normal is tested on the x component only"""
    B = case["T"].shape[0]
    has = (lambda n: n[0] != 0) if mutation == "has_one" else _has
    out = {"loss_terms": [], "pair_counts": [], "grad_terms": []}
    for b in range(B):
        s = loss_summands(case["p"][b], case["n"][b], case["pt"][b], case["nt"][b], case["nn"][b], case["T"][b], flags, xp=np.float32, has=has)
        HW = s.shape[1]
        if mutation == "drop_pixel":
            s[:, int(np.argmax(np.abs(s[0]) + np.abs(s[24]) + s[23] + s[37]))] = 0
        if mutation == "skip_chunk":
            s = s[:, :max((-(-HW // 256) - 1) * 256, 0)]
        lt, cnt, g = loss_finish(_sum32(s).astype(np.float64) if s.shape[1] else np.zeros(38), flags)
        if mutation == "swap_columns":
            g = g.reshape(3, 3, 4)[:, :, [1, 0, 2, 3]].reshape(3, 12).copy()
        out["loss_terms"].append(lt), out["pair_counts"].append(cnt), out["grad_terms"].append(g)
    return {k: np.stack(v) for k, v in out.items()}


LOSS_MUTATIONS = ("drop_pixel", "swap_columns", "skip_chunk", "has_one")


# ---------------------------------------------------------------------------------------------------- pose heads

HEAD_PARAMS = ("fc_w", "fc_b", "r1_w", "r1_b", "r3_w", "r3_b", "t1_w", "t1_b", "t3_w", "t3_b")


def head_param_shapes(F, R, Hd):
    return {"fc_w": (R, F), "fc_b": (R,), "r1_w": (Hd, R), "r1_b": (Hd,), "r3_w": (4, Hd), "r3_b": (4,), "t1_w": (Hd, R), "t1_b": (Hd,),
            "t3_w": (3, Hd), "t3_b": (3,)}


def _act(v, act):
    return torch.tanh(v) if act == 1 else (torch.relu(v) if act == 2 else v)


def heads(x, P, act, fc_scale=None, g_t=None, g_r=None, per_sample_norm=False):
    """The pose heads in torch float64 under autograd: a1 = act((fc(x)) * fc_scale), the two heads `[act, Linear, act, Linear]`
    on it, rotation = rot_raw / ||rot_raw||_F with ONE norm over the whole batch.  With g_t / g_r also the gradients of
    sum(translation g_t) + sum(rotation g_r) with respect to the ten parameters ("d_<name>") and x ("grad_x")."""
    x = x.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    pre = x @ P["fc_w"].t() + P["fc_b"]
    if fc_scale is not None:
        pre = pre * fc_scale
    a1 = _act(pre, act)
    hr, ht = _act(a1 @ P["r1_w"].t() + P["r1_b"], act), _act(a1 @ P["t1_w"].t() + P["t1_b"], act)
    rot_raw, tr = hr @ P["r3_w"].t() + P["r3_b"], ht @ P["t3_w"].t() + P["t3_b"]
    norm = rot_raw.norm(dim=1, keepdim=True) if per_sample_norm else rot_raw.norm()
    rotation = rot_raw / norm
    out = {"a1": a1, "a2": torch.stack((hr, ht), dim=1), "rot_raw": rot_raw, "translation": tr, "rotation": rotation,
           "norm": norm.reshape(-1)[:1] if not per_sample_norm else norm.reshape(-1)}
    if g_t is not None:
        ((tr * g_t).sum() + (rotation * g_r).sum()).backward()
        out["grad_x"] = x.grad
        for k in HEAD_PARAMS:
            out["d_" + k] = P[k].grad
    return {k: v.detach() for k, v in out.items()}


def heads_case_exact(B, F, R, Hd, seed=0):
    """Integer inputs and sparse integer weights: x in [-2,2], about 64 / 4 / 2 non-zero weights in {-2..2} \\ {0} per row of the
    fc / first / last layers (2 / 1 in the rotation head, so that the sum of squares under the norm stays exact), biases in [-1,1], a dropout mask of 0 / 1.25,
    integer grad_translation in [-2,2]."""
    for attempt in range(64):                          # a batch whose raw quaternions are all zero has no norm to divide by
        # (at seed 0 the six HEADS_SHAPES need 1, 1, 1, 2, 1, 1 attempts: under 0.4 s for all of them; the liveness test is cheap,
        # the four float64 forwards per attempt are what costs at F = 2500)
        x, P, scale, g_t = _heads_case_exact(B, F, R, Hd, seed + 1000 * attempt)
        if all(float(heads(x, P, act, sc)["norm"]) > 0 for act in (0, 2) for sc in (None, scale)) and _last_feature_is_live(x, P, scale):
            return x, P, scale, g_t
    raise AssertionError("no exact heads case with a non-zero norm and a live last feature")


def _last_feature_is_live(x, P, scale):
    """The last input feature reaches a1 under relu and under the mask: some unmasked fc output is positive with or without its
    contribution (so that a kernel that loses the end of the reduction cannot hide behind relu or dropout)."""
    contrib = x[:, -1:] * P["fc_w"][:, -1][None]                        # [B,R]
    pre = x @ P["fc_w"].t() + P["fc_b"]
    return bool(((contrib != 0) & (scale != 0) & (torch.maximum(pre, pre - contrib) > 0)).any())


def _heads_case_exact(B, F, R, Hd, seed):
    r = _rng(seed, B, F, R, Hd)
    shapes = head_param_shapes(F, R, Hd)

    def w(shape, nnz):
        v = r.integers(1, 3, shape) * r.choice([-1, 1], shape)
        return torch.from_numpy((v * (r.random(shape) < min(1.0, nnz / shape[-1]))).astype(np.float64))
    P = {"fc_w": w(shapes["fc_w"], 64), "r1_w": w(shapes["r1_w"], 2), "t1_w": w(shapes["t1_w"], 4), "r3_w": w(shapes["r3_w"], 1), "t3_w": w(shapes["t3_w"], 2)}
    for k in ("fc_b", "r1_b", "t1_b", "r3_b", "t3_b"):
        P[k] = torch.from_numpy(r.integers(-1, 2, shapes[k]).astype(np.float64))
    x = torch.from_numpy(r.integers(-2, 3, (B, F)).astype(np.float64))
    scale = torch.from_numpy(np.where(r.random((B, R)) < 0.2, 0.0, 1.25))
    g_t = torch.from_numpy(r.integers(-2, 3, (B, 3)).astype(np.float64))
    return x, P, scale, g_t


def heads_case_real(B, F, R, Hd, seed=0):
    """Real-valued fp32 case (x, P, mask, grad_translation, grad_rotation) as float64 tensors."""
    r = _rng(seed, B, F, R, Hd, 5)
    shapes = head_param_shapes(F, R, Hd)
    f = lambda v: torch.from_numpy(v.astype(np.float32).astype(np.float64))
    P = {k: f(r.normal(size=s) / np.sqrt(s[-1]) if k.endswith("_w") else r.normal(size=s) * 0.1) for k, s in shapes.items()}
    x = f(r.normal(size=(B, F)))
    scale = f(np.where(r.random((B, R)) < 0.2, 0.0, 1.25))
    scale[0, 0] = 1.25                                              # never a mask that drops everything
    return x, P, scale, f(r.normal(size=(B, 3))), f(r.normal(size=(B, 4)))


def _maj(a, w, b=None):
    m = a.abs() @ w.abs().t()
    return m + b.abs() if b is not None else m


def heads_headroom(x, P, scale, g_t, act):
    """Every sum of the forward and of the backward with grad_rotation = 0 stays exact: the majorants (absolute values through the
    layers, activations bounded by the identity) times 4 (all values live on the grid 1/4: the mask's 1.25) are below 2^24, and
    the sum of squares under the norm, on the grid 1/16, is as well.  Returns the worst case as a fraction of 2^24."""
    ref = heads(x, P, act, scale, g_t, torch.zeros(x.shape[0], 4, dtype=torch.float64))
    sc = scale.abs() if scale is not None else 1.0
    m1 = _maj(x, P["fc_w"], P["fc_b"]) * sc
    mr, mt = _maj(m1, P["r1_w"], P["r1_b"]), _maj(m1, P["t1_w"], P["t1_b"])
    m3r, m3t = _maj(mr, P["r3_w"], P["r3_b"]), _maj(mt, P["t3_w"], P["t3_b"])
    gh = g_t.abs() @ P["t3_w"].abs()                          # [B,Hd]
    gout = (gh @ P["t1_w"].abs()) * sc                        # [B,R]
    sums = [m1, mr, mt, m3r, m3t, g_t.abs().t() @ mt, gh, gh.t() @ m1, gout, gout.t() @ x.abs(), gout @ P["fc_w"].abs(), gh.sum(0), gout.sum(0)]
    worst = max(float(s.max()) for s in sums) * 4.0
    worst = max(worst, float((ref["rot_raw"] ** 2).sum()) * 16.0)
    for k in ("a1", "a2", "rot_raw", "translation"):
        assert torch.equal(ref[k] * 4.0, torch.round(ref[k] * 4.0)), f"heads_headroom: {k} left the grid 1/4"
    assert worst < LIMIT, f"heads_headroom: {worst:.0f} grid steps >= 2^24 -- the case would no longer be exact"
    return worst / LIMIT


def _inv32(P):
    """fp32(1 / P) as a tensor: formed in float64 and rounded once, which is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2
    bits), independent of how the host's vector units divide."""
    return torch.tensor(1.0 / float(P), dtype=torch.float64).to(torch.float32)


def norm_and_rotation32(rot_raw32):
    """(norm [1], rotation) in correctly rounded fp32 from an fp32 rot_raw whose sum of squares is exact: sqrt and quotient are
    formed in float64 and rounded once (double rounding cannot occur for these two operations at 53 against 24 bits)."""
    ss = (rot_raw32.double() ** 2).sum().to(torch.float32)
    norm = torch.sqrt(ss.double()).to(torch.float32)
    return norm.reshape(1), (rot_raw32.double() / norm.double()).to(torch.float32)


def heads_exact_expect(ref):
    """fp32 expectations of the exact tier from the float64 reference: norm = fp32 sqrt of the exact sum of squares, rotation =
    the fp32 quotient rot_raw / norm; everything else the float64 value itself (exactly representable)."""
    out = {k: v.to(torch.float32) for k, v in ref.items()}
    out["norm"], out["rotation"] = norm_and_rotation32(out["rot_raw"])     # the sum of squares is exact (heads_headroom)
    return out


# First-order rounding bound of the heads, propagated layer by layer in float64 next to the reference.  For y = act(x W^T + b):
#     E(pre) = (n + 2) u (|x| |W|^T + |b|)  +  E(x) |W|^T          n products and n additions of a dot product of length n in any
#                                                                   order (each summand passes through at most n roundings; the
#                                                                   kernels use fma: n + lane reduction), the bias add, one spare
#     dropout: E = E(pre) s + u |pre s|;   tanh: E(y) = E(pre) + 2.5 ulp(y)  (|tanh'| <= 1; dl_tanh is within 2.5 ulp, pinned by
#     test_epilogue_tanh_is_within_two_ulp_of_float64);   relu, none: E(y) = E(pre)
# norm = sqrt(sum r^2): E(norm) = sum |r| E(r) / norm + (4B + 2) u norm;  rotation = r / norm: E = E(r)/norm + |r| E(norm)/norm^2 + u |r/norm|.
# Backward: dl_heads_bwd takes the saved activations (a1, a2, rot_raw, norm) as ARGUMENTS, so the tests hand it the float64
# reference's values rounded to fp32: their error is one rounding, E(a) = u |a| (rotation = r / norm, formed in the kernel from two
# rounded inputs and one division: 3 u |y|), and relu's derivative is decided by the sign of an input, which rounding keeps.  Then
# the same rule runs on the transposed products, the activation derivative from the saved output (tanh: 1 - a^2 -> 2 |a| E(a) + 2 u).


def _ulp32_t(v):
    return torch.from_numpy(_ulp32(v.numpy()))


def heads_bounds(x, P, act, fc_scale, g_t, g_r):
    """(float64 autograd reference, dict name -> per-element bound as float64 tensors) for every output of dl_heads_fwd / dl_heads_bwd."""
    u = U
    ref = heads(x, P, act, fc_scale, g_t, g_r)
    B, F = x.shape
    R, Hd = P["fc_w"].shape[0], P["r1_w"].shape[0]
    zero = torch.zeros_like

    def lin(a, Ea, W, b, n):
        return (n + 2) * u * _maj(a, W, b) + Ea @ W.abs().t()

    def actb(E, y):
        return E + 2.5 * _ulp32_t(y) if act == 1 else E

    def dact(a, Ea):
        """(value, bound) of act' from the saved output."""
        if act == 1:
            return 1 - a * a, 2 * a.abs() * Ea + 2 * u
        return ((a > 0).double() if act == 2 else torch.ones_like(a)), zero(a)

    s = fc_scale if fc_scale is not None else torch.ones(B, R, dtype=torch.float64)
    pre1 = (x @ P["fc_w"].t() + P["fc_b"]) * s
    E1 = actb(lin(x, zero(x), P["fc_w"], P["fc_b"], F) * s.abs() + u * pre1.abs(), ref["a1"])
    a1, hr, ht = ref["a1"], ref["a2"][:, 0], ref["a2"][:, 1]
    Ehr, Eht = actb(lin(a1, E1, P["r1_w"], P["r1_b"], R), hr), actb(lin(a1, E1, P["t1_w"], P["t1_b"], R), ht)
    Er, Et = lin(hr, Ehr, P["r3_w"], P["r3_b"], Hd), lin(ht, Eht, P["t3_w"], P["t3_b"], Hd)
    r, n = ref["rot_raw"], ref["norm"][0]
    En = (r.abs() * Er).sum() / n + (4 * B + 2) * u * n
    y = r / n
    Ey = Er / n + r.abs() * En / n ** 2 + u * y.abs()
    out = {"a1": E1, "a2": torch.stack((Ehr, Eht), 1), "rot_raw": Er, "translation": Et, "norm": En.reshape(1), "rotation": Ey}
    # backward from the rounded saved tensors.  g_raw (rotation) = (g - y (y . g)) / n
    E1, Ehr, Eht, En, Ey = u * a1.abs(), u * hr.abs(), u * ht.abs(), u * n, 3 * u * y.abs()
    dot = (g_r * y).sum()
    Edot = (g_r.abs() * Ey).sum() + (4 * B + 2) * u * (g_r.abs() * y.abs()).sum()
    gq = (g_r - y * dot) / n
    Egq = (Ey * dot.abs() + y.abs() * Edot + 3 * u * (g_r.abs() + (y * dot).abs())) / n + gq.abs() * En / n + u * gq.abs()
    gt, Egt = g_t, zero(g_t)

    def outer(g, Eg, a, Ea):                  # d_w[i][m] = sum_b g[b][i] a[b][m]
        return (B + 2) * u * (g.abs().t() @ a.abs()) + Eg.t() @ a.abs() + g.abs().t() @ Ea

    def colsum(g, Eg):
        return (B + 1) * u * g.abs().sum(0) + Eg.sum(0)
    out["d_r3w"], out["d_t3w"] = outer(gq, Egq, hr, Ehr), outer(gt, Egt, ht, Eht)
    out["d_r3b"], out["d_t3b"] = colsum(gq, Egq), colsum(gt, Egt)

    def back(g, Eg, W, a, Ea, n_terms, extra=None):
        """(value, bound) of (g W) * act'(a) [* extra]"""
        v = g @ W
        Ev = (n_terms + 2) * u * (g.abs() @ W.abs()) + Eg @ W.abs()
        d, Ed = dact(a, Ea)
        val = v * d
        E = Ev * d.abs() + v.abs() * Ed + u * val.abs()
        if extra is not None:
            val, E = val * extra, E * extra.abs() + u * (val * extra).abs()
        return val, E
    ghr, Eghr = back(gq, Egq, P["r3_w"], hr, Ehr, 4)
    ght, Eght = back(gt, Egt, P["t3_w"], ht, Eht, 3)
    out["d_r1w"], out["d_t1w"] = outer(ghr, Eghr, a1, E1), outer(ght, Eght, a1, E1)
    out["d_r1b"], out["d_t1b"] = colsum(ghr, Eghr), colsum(ght, Eght)
    gh, Egh = torch.cat((ghr, ght), 1), torch.cat((Eghr, Eght), 1)
    W1 = torch.cat((P["r1_w"], P["t1_w"]), 0)
    gout, Egout = back(gh, Egh, W1, a1, E1, 2 * Hd + 8, extra=fc_scale)
    out["d_fcw"], out["d_fcb"] = outer(gout, Egout, x, zero(x)), colsum(gout, Egout)
    out["grad_x"] = (R + 2 + (R + 39) // 40) * u * (gout.abs() @ P["fc_w"].abs()) + Egout @ P["fc_w"].abs()
    names = {"d_r3w": "d_r3_w", "d_t3w": "d_t3_w", "d_r3b": "d_r3_b", "d_t3b": "d_t3_b", "d_r1w": "d_r1_w", "d_t1w": "d_t1_w", "d_r1b": "d_r1_b",
             "d_t1b": "d_t1_b", "d_fcw": "d_fc_w", "d_fcb": "d_fc_b"}
    out = {names.get(k, k): v for k, v in out.items()}
    return ref, {k: v + _ulp32_t(ref[k]) for k, v in out.items()}


def heads_saved(ref):
    """The saved tensors dl_heads_bwd is handed: the reference's a1, a2, rot_raw, norm rounded to fp32."""
    return {k: ref[k].to(torch.float32) for k in ("a1", "a2", "rot_raw", "norm")}



def heads_bwd(x, P, act, fc_scale, saved, g_t, g_r, per_sample_norm=False):
    """dl_heads_bwd written out in the dtype of ``x``: the eleven gradients from the SAVED tensors (a1, a2, rot_raw, norm), the way the
    entry point receives them.  In float64 on the reference's own activations it equals autograd (the host test checks that)."""
    dt = x.dtype
    a1, a2, r, n = (saved[k].to(dt) for k in ("a1", "a2", "rot_raw", "norm"))
    hr, ht = a2[:, 0], a2[:, 1]
    d = (lambda a: 1 - a * a) if act == 1 else ((lambda a: (a > 0).to(dt)) if act == 2 else torch.ones_like)
    if per_sample_norm:
        n = r.norm(dim=1, keepdim=True)
        y = r / n
        gq = (g_r - y * (g_r * y).sum(dim=1, keepdim=True)) / n
    else:
        y = r / n
        gq = (g_r - y * (g_r * y).sum()) / n
    out = {"d_r3_w": gq.t() @ hr, "d_r3_b": gq.sum(0), "d_t3_w": g_t.t() @ ht, "d_t3_b": g_t.sum(0)}
    ghr, ght = (gq @ P["r3_w"]) * d(hr), (g_t @ P["t3_w"]) * d(ht)
    out.update({"d_r1_w": ghr.t() @ a1, "d_r1_b": ghr.sum(0), "d_t1_w": ght.t() @ a1, "d_t1_b": ght.sum(0)})
    gout = (ghr @ P["r1_w"] + ght @ P["t1_w"]) * d(a1)
    if fc_scale is not None:
        gout = gout * fc_scale
    out.update({"d_fc_w": gout.t() @ x, "d_fc_b": gout.sum(0), "grad_x": gout @ P["fc_w"]})
    return out


def heads_f32(x, P, act, fc_scale, g_t, g_r, saved, mutation=None):
    """fp32 torch-CPU evaluation of both entry points (forward from x, backward from ``saved``), optionally with one value-only
    defect: "drop_fc_column" (the last input feature does not reach fc, forward or backward) or "norm_per_sample"."""
    f = lambda v: None if v is None else v.to(torch.float32)
    x32 = f(x).clone()
    if mutation == "drop_fc_column":
        x32[:, -1] = 0
    P32 = {k: f(v) for k, v in P.items()}
    out = heads(x32, P32, act, f(fc_scale), per_sample_norm=mutation == "norm_per_sample")
    if mutation == "norm_per_sample":
        out["norm"] = out["norm"][:1]
    elif float((out["rot_raw"].double() ** 2).sum()) * 16.0 < LIMIT:       # exact sum of squares: one rounding each for sqrt and quotient
        out["norm"], out["rotation"] = norm_and_rotation32(out["rot_raw"])
    out.update(heads_bwd(x32, P32, act, f(fc_scale), saved, f(g_t), f(g_r), per_sample_norm=mutation == "norm_per_sample"))
    return out


HEADS_MUTATIONS = ("drop_fc_column", "norm_per_sample")
HEADS_FWD_OUT = ("a1", "a2", "rot_raw", "translation", "rotation", "norm")
HEADS_BWD_OUT = tuple("d_" + k for k in HEAD_PARAMS) + ("grad_x",)


# ---------------------------------------------------------------------------------------------------- pooling, cast, quaternion

HALF = {1: torch.float16, 2: torch.bfloat16}


def mean_case(N, P, C, dtype, seed=0, exact=True):
    """x [N,P,C] float64: integers in [-8,8] (exact in every storage type) or real values rounded to the storage type."""
    r = _rng(seed, N, P, C)
    v = r.integers(-8, 9, (N, P, C)).astype(np.float64) if exact else r.normal(size=(N, P, C)) * 3.0
    return torch.from_numpy(v).to(dtype).to(torch.float64)


def pool_headroom(x):
    worst = float(x.abs().sum(dim=1).max())
    assert torch.equal(x, torch.round(x)) and worst < LIMIT, f"pool_headroom: {worst:.0f} >= 2^24"
    return worst / LIMIT


def mean_exact(x):
    """fp32 sum (exact on integer data) times the fp32 reciprocal of P, one rounding each: [N,C] fp32."""
    P = x.shape[1]
    inv = _inv32(P)
    return x.sum(dim=1).to(torch.float32) * inv


def mean_bound(x, lanes):
    """(float64 mean, bound) [N,C]: (adds + 1) 2^-24 sum|x| carried through the division by P.  adds = ceil(P / lanes) additions in
    a pixel lane + log2(lanes) in the LDS tree; a lane's first addition (to zero) is exact, which leaves room for the two roundings
    of the product with the rounded 1 / P inside the + 1."""
    P = x.shape[1]
    adds = -(-P // lanes) + int(np.log2(lanes))
    return x.mean(dim=1), (adds + 1) * U * x.abs().sum(dim=1) / P


def mean_f32(x, mutation=None):
    """fp32 torch-CPU pooling; mutations "drop_pixel" (the last pixel) and "skip_chunk" (the last 64 pixels)."""
    P = x.shape[1]
    v = x.to(torch.float32)
    if mutation == "drop_pixel":
        v = v[:, :P - 1]
    if mutation == "skip_chunk":
        v = v[:, :max(P - 64, 0)]
    inv = _inv32(P)
    return v.sum(dim=1) * inv


def special_values(dtype, n, seed=0):
    """n fp32 values that exercise the rounding to ``dtype``: +-0, subnormals of the half type, ties to even, values that round
    up to infinity, +-inf, NaN, the largest finite values, and random fill."""
    fi = torch.finfo(dtype)
    tiny, eps, mx = float(fi.smallest_normal), float(fi.eps), float(fi.max)
    sub = tiny * eps                                             # smallest subnormal of the half type
    base = [0.0, -0.0, sub, -sub, sub * 0.5, sub * 0.5000001, sub * 1.5, sub * 2.5, tiny, tiny * (1 - eps / 2), tiny - sub, 3 * sub,
            1.0 + eps / 2, 1.0 + 3 * eps / 2, 1.0 + eps / 2 * 1.0000002, -(1.0 + eps / 2), 1.0 + eps, mx, -mx, mx * (1 + eps / 4), mx * (1 + eps / 2),
            mx * (1 + eps / 4 * 0.99), float("inf"), -float("inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1e-45, -1e-45,
            1.1754943508222875e-38, 0.1, -2.5, 65519.99, 65520.0]
    r = _rng(seed, n)
    fill = r.normal(size=n) * np.exp(r.uniform(-12, 12, n))
    v = torch.from_numpy(fill).to(torch.float32)
    k = min(n, len(base))
    pos = torch.from_numpy(r.permutation(n)[:k].copy())
    v[pos] = torch.tensor(base[:k], dtype=torch.float32)
    return v


def cast_ref(src, dtype):
    return src.to(dtype)                                          # torch's round-to-nearest-even conversion


def mean_bwd_act(gy, x, P, act, dtype):
    """Op-by-op fp32 emulation of dl_mean_hw_bwd_act_h followed by torch's rounding: ((gy * (1/P)) * act'(x)) with act' from the stored
    half value (tanh: 1 - x*x, two roundings; relu: 0 where x <= 0, else 1 -- NaN included), x [N,P,C] half, gy [N,C] fp32."""
    inv = _inv32(P)
    xf = x.to(torch.float32)
    if act == 1:
        d = 1.0 - xf * xf
    elif act == 2:
        d = torch.where(xf <= 0, torch.zeros_like(xf), torch.ones_like(xf))
    else:
        d = torch.ones_like(xf)
    return ((gy.to(torch.float32) * inv)[:, None, :] * d).to(dtype)


def mean_bwd_act64(gy, x, P, act):
    xf = x.to(torch.float64)
    d = 1.0 - xf * xf if act == 1 else ((xf > 0).double() if act == 2 else torch.ones_like(xf))
    return gy.to(torch.float64)[:, None, :] / P * d


def quat_case(B, eps, seed=0):
    """Unnormalised quaternions (fp32): random, tiny on both sides of eps, exactly eps, large up to 1e18; translations; grad_T."""
    r = _rng(seed, B)
    q = r.normal(size=(B, 4))
    scales = [1.0, 1e-3, 1e4, eps * 0.25, eps * 4.0, 1e18 / 4, 1e-20, 1e9, eps * 0.9, eps * 1.5]
    for b in range(B):
        q[b] *= scales[b % len(scales)]
    q = torch.from_numpy(q).to(torch.float32)
    if B > 3:
        q[3] = torch.tensor([0.0, 0.0, 0.0, 1.0])
    if B > 10:
        q[10] = torch.tensor([eps, 0.0, 0.0, 0.0], dtype=torch.float32)         # |q| == eps exactly, in fp32 and in float64
        q[11 % B] = torch.tensor([0.0, 0.0, 1e18, 0.0])
    t = torch.from_numpy(r.normal(size=(B, 3)) * 10).to(torch.float32)
    G = torch.from_numpy(r.normal(size=(B, 4, 4))).to(torch.float32)
    return q, t, G


def quat_to_T(q, t, eps, G=None):
    """float64: q / max(|q|, eps), then the element-wise rotation formula (x, y, z, w), T = [[R, t], [0, 1]]; with G also
    (grad_t, grad_q) of sum(T G) by torch autograd (clamp: the gradient flows through |q| where |q| >= eps)."""
    q = q.to(torch.float64).clone().requires_grad_(True)
    t = t.to(torch.float64).clone().requires_grad_(True)
    n = q.norm(dim=1, keepdim=True).clamp_min(float(eps))
    x, y, z, w = (q / n).unbind(dim=1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    T = torch.zeros(q.shape[0], 4, 4, dtype=torch.float64)
    T[:, 3, 3] = 1.0
    T = T.clone()
    T[:, :3, :3] = R
    T[:, :3, 3] = t
    if G is None:
        return T.detach()
    (T * G.to(torch.float64)).sum().backward()
    return T.detach(), t.grad, q.grad
