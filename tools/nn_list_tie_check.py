"""CPU check that goes with tests/test_gpu_nn_list.py: on every seeded input of tests/test_gpu_nn_list.py the exact nearest neighbour is unambiguous.

For each (source, target) pair: cKDTree k=2 on the float64 copy of the fp32 points, both squared distances recomputed in fp64 from
the coordinates, relative gap between them; prints the smallest gap per pair and the number of queries with a gap <= 1e-12
(candidates for a rounding-dependent winner), plus the number of duplicate target points.  Run from the repository root:
    python tools/nn_list_tie_check.py
Measured when the tests were written: no duplicates, no near-ties, smallest gap 6.4e-10 (portable pair 9101, n = 262144, random pose).
"""
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, ".")
from delora_amd.data import synthetic as syn  # noqa: E402


def minrel(src, tgt):
    t64 = tgt.T.astype(np.float64)
    q64 = src.T.astype(np.float64)
    if len(t64) < 2:
        return 1.0, 0
    _, i = cKDTree(t64).query(q64, k=2)
    a = ((q64 - t64[i[:, 0]]) ** 2).sum(1)
    b = ((q64 - t64[i[:, 1]]) ** 2).sum(1)
    rel = np.abs(b - a) / np.maximum(b, 1e-300)
    return float(rel.min()), int((rel <= 1e-12).sum())


def poses(seed, s1, s2):
    rng = np.random.default_rng(seed)
    Rr = syn._rot_zyx(*rng.uniform(-3.1, 3.1, 3)).astype(np.float32)
    tr = rng.normal(size=(3, 1)).astype(np.float32)
    R = syn._rot_zyx(0.3, -0.1, 0.05).astype(np.float32)
    return {"identity": s2, "tilted": (R @ s2 + np.array([[30.0], [2.0], [0.5]], np.float32)).astype(np.float32),
            "random": (Rr @ s2 + tr).astype(np.float32), "self": s1}


worst = 1.0
for n in (1, 63, 64, 65, 1000, 32768, 131072, 262144):
    for seed in (9101, 9102):
        if n == 262144 and seed == 9102:
            continue
        p = syn.portable_pair(seed, n)
        s1, s2 = p["scan_1"], p["scan_2"]
        dup = n - len(np.unique(s1.T, axis=0))
        for k, src in poses(seed, s1, s2).items():
            m, c = minrel(src, s1)
            worst = min(worst, m)
            print(f"n={n} seed={seed} {k}: duplicate targets {dup}, smallest relative gap {m:.3e}, near-ties {c}", flush=True)

p, q = syn.portable_pair(9101, 70001), syn.portable_pair(9102, 1000)
for name, (src, tgt) in {"1000 vs 70001": (q["scan_2"], p["scan_1"]), "70001 vs 1000": (p["scan_2"], q["scan_1"])}.items():
    m, c = minrel(src, tgt)
    worst = min(worst, m)
    print(f"ragged {name}: smallest relative gap {m:.3e}, near-ties {c}", flush=True)

n = 131072
rng = np.random.default_rng(5)
u_t = rng.uniform(-50, 50, (3, n)).astype(np.float32)
u_s = rng.uniform(-60, 60, (3, n)).astype(np.float32)
m, c = minrel(u_s, u_t)
worst = min(worst, m)
print(f"uniform cloud: smallest relative gap {m:.3e}, near-ties {c}", flush=True)
core = rng.normal(0, 0.01, (3, n // 2)).astype(np.float32)
far = (rng.normal(0, 1, (3, n // 2)) * 5000).astype(np.float32)
mix = np.concatenate([core, far], 1)
m, c = minrel((mix[:, rng.permutation(n)] * np.float32(1.001)).astype(np.float32), mix)
worst = min(worst, m)
print(f"scale mixture: smallest relative gap {m:.3e}, near-ties {c}", flush=True)
print("smallest gap over all inputs:", worst)
