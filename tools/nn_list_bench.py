#!/usr/bin/env python3
"""Exact nearest neighbour between free-form lists: the tree search (dl_nn_list_build / dl_nn_list_query) against the exhaustive
kernel (dl_nn_bruteforce), in ONE process on one GPU, after warm-up, the contenders alternating, timed with device events over enough
repeats to fill --seconds each.  Ms = Mt = n on synthetic.portable_pair clouds in four pose regimes (identity, tilted, random, the
target list itself).  For orientation only: cKDTree on the host (the reference's method, build + query, 16 workers) and
dl_nn_correspond on the projected form of the same pair (a 64-row range image keeps one point per pixel: a smaller problem).
The whole table is measured twice in the one run; `spread` is the larger relative difference between the two passes.

    python tools/nn_list_bench.py [--sizes 2048,8192,...] [--seconds 0.5] [--out profiles/nn_list_bench.json] [--no-host]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from delora_amd import geometry as G  # noqa: E402
from delora_amd.data import synthetic as syn  # noqa: E402

ROUNDS = 4                    # the contenders take turns this many times per cell
REGIMES = ("identity", "tilted", "random", "self")


def poses(seed):
    rng = np.random.default_rng(seed)
    Rr, tr = syn._rot_zyx(*rng.uniform(-3.1, 3.1, 3)), rng.normal(size=(3, 1))
    return {"identity": (np.eye(3), np.zeros((3, 1))), "tilted": (syn._rot_zyx(0.3, -0.1, 0.05), np.array([[30.0], [2.0], [0.5]])),
            "random": (Rr, tr), "self": (np.eye(3), np.zeros((3, 1)))}


def device_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(contenders, seconds):
    """{name: ms per call}: one calibration call each after two warm-up calls, then ROUNDS turns of equal length."""
    reps = {}
    for name, fn in contenders.items():
        fn(), fn()
        torch.cuda.synchronize()
        once = max(device_ms(fn, 1), 1e-3)
        reps[name] = max(1, math.ceil(seconds * 1e3 / once / ROUNDS))
    total = {name: 0.0 for name in contenders}
    for _ in range(ROUNDS):
        for name, fn in contenders.items():
            total[name] += device_ms(fn, reps[name])
    return {name: total[name] / (ROUNDS * reps[name]) for name in contenders}, {name: ROUNDS * reps[name] for name in contenders}


def projected_contender(s1, s2, R, t, dev):
    """dl_nn_correspond on 64 x (n / 64) range images of the two lists (source untransformed, the pose as T)."""
    n = s1.shape[1]
    sensor = G.Sensor(64, max(32, n // 64), (math.radians(-24.9), math.radians(2.0)), (-math.pi, math.pi))
    pts = torch.from_numpy(np.concatenate([s1, s2], 1)).to(dev)
    offs = torch.tensor([0, n, 2 * n], dtype=torch.int32, device=dev)
    pr = G.project(pts, offs, n, sensor)
    img, nrm = pr["image4"], G.normals(pr["image4"])
    tgt_pk, tgt_npk = pr["packed"][0:1].contiguous(), G.pack_image(nrm[0:1])
    T = torch.eye(4, device=dev).view(1, 4, 4).clone()
    T[0, :3, :3], T[0, :3, 3] = torch.from_numpy(R.astype(np.float32)).to(dev), torch.from_numpy(t[:, 0].astype(np.float32)).to(dev)
    ws = torch.empty((G.nn_workspace_bytes(1, sensor.H, sensor.W) // 8 + 1,), dtype=torch.int64, device=dev)
    src_img, src_nrm = img[1:2].contiguous(), nrm[1:2].contiguous()
    occupied = int((pr["pix2pt"] >= 0).sum(dim=(1, 2)).min())
    return (lambda: G.nn_correspond(src_img, src_nrm, tgt_pk, tgt_npk, T, sensor, workspace=ws)), occupied


def one_table(sizes, seconds, host, dev):
    rows = []
    for n in sizes:
        pair = syn.portable_pair(9101, n)
        s1, s2 = pair["scan_1"], pair["scan_2"]
        tgt = torch.from_numpy(s1).to(dev)
        for regime, (R, t) in poses(9101).items():
            base = s1 if regime == "self" else s2
            src_h = (R.astype(np.float32) @ base + t.astype(np.float32)).astype(np.float32)
            src = torch.from_numpy(src_h).to(dev)
            tree = G.PointTree(tgt)
            out = torch.empty((n,), dtype=torch.int32, device=dev)
            assert torch.equal(tree.query(src), G.nn_bruteforce(src, tgt)), (n, regime)        # the contenders compute the same thing

            def both():
                tree.rebuild()
                tree.query(src, out=out)
            contenders = {"bruteforce": lambda: G.nn_bruteforce(src, tgt), "build": tree.rebuild, "query": lambda: tree.query(src, out=out),
                          "build_query": both}
            row = {"n": n, "regime": regime}
            try:
                contenders["correspond_projected"], row["projected_occupied_pixels"] = projected_contender(s1, base, R, t, dev)
            except Exception as e:      # noqa: BLE001 -- orientation only: a size the image search does not take is reported, not fatal
                row["correspond_projected_error"] = f"{type(e).__name__}: {e}"[:200]
            ms, calls = measure(contenders, seconds)
            row.update({k + "_ms": round(v, 5) for k, v in ms.items()})
            row["calls"] = calls
            if host:
                from scipy.spatial import cKDTree
                t64, q64 = s1.T.astype(np.float64), src_h.T.astype(np.float64)
                t0 = time.perf_counter()
                tr = cKDTree(t64)
                t1 = time.perf_counter()
                _, idx = tr.query(q64, k=1, workers=16)
                t2 = time.perf_counter()
                row["ckdtree_host_build_ms"], row["ckdtree_host_query_ms"] = round((t1 - t0) * 1e3, 3), round((t2 - t1) * 1e3, 3)
                row["ckdtree_agrees"] = bool(np.array_equal(idx.astype(np.int64), out.cpu().numpy().astype(np.int64)))
            row["speedup_build_query_vs_bruteforce"] = round(ms["bruteforce"] / ms["build_query"], 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="2048,8192,32768,131072,262144")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn_list_bench.json"))
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sizes = [int(s) for s in args.sizes.split(",")]
    x = torch.randn((4096, 4096), device=dev)
    for _ in range(20):                 # clocks up before the first cell
        x = (x @ x).tanh()
    torch.cuda.synchronize()
    passes = [one_table(sizes, args.seconds, not args.no_host, dev) for _ in range(2)]
    table = []
    for a, b in zip(*passes):
        row = {"n": a["n"], "regime": a["regime"]}
        spread = 0.0
        for k in a:
            if k.endswith("_ms") and not k.startswith("ckdtree"):
                row[k] = [a[k], b[k]]
                spread = max(spread, abs(a[k] - b[k]) / min(a[k], b[k]))
            elif k.startswith("ckdtree") or k.startswith("projected") or k.endswith("_error"):
                row[k] = [a[k], b.get(k)]
        row["spread"] = round(spread, 4)
        lo, hi = min(a["bruteforce_ms"], b["bruteforce_ms"]), max(a["build_query_ms"], b["build_query_ms"])
        row["speedup_build_query_vs_bruteforce_worst_pass"] = round(lo / hi, 3)
        row["tree_wins_beyond_spread"] = bool(lo > hi * (1.0 + spread))
        table.append(row)
    result = {"tool": "tools/nn_list_bench.py", "device": torch.cuda.get_device_name(0), "seconds_per_contender": args.seconds,
              "rounds": ROUNDS, "unit": "ms per call, [first pass, second pass]", "table": table}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
