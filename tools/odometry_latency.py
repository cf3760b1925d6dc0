#!/usr/bin/env python3
"""Latency of one ``ScanToScanOdometry.push`` at the reference's shipped operating point (unmodified YAML: 64x720, batch 1), engine
"torch" (the module path) against engine "native" (``dl_odometry_push``): same process, same weights, same scans, the engines
ALTERNATING in blocks so that drift of the host hits both.   python tools/odometry_latency.py [--pushes N] [--rounds R] [--out FILE]

Per push two numbers: the host wall time of the call (it ends in the ``.cpu()`` of the pose, i.e. in a device synchronise) and the
stream time between two events recorded around it.  Scans are resident fp32 tensors (the numpy filter of raw messages is the same
host work for both engines and is left out).  Reported per engine and measure: median, 10th / 90th percentile, minimum; plus the
per-round medians (the spread between repetitions of the same code).

``--half`` measures the half-precision legs instead and writes profiles/odometry_latency_half.json: at 64x720 and at 64x2048, batch 1,
one push on (1) the native half path (``engine="native", precision="bfloat16" | "float16"``: ``dl_odometry_push_h``, every trunk weight
converted once), (2) the native fp32 path and (3) the Python autocast eval path (``engine="torch"`` with the same precisions: the model
call inside ``torch.autocast``, the weights converted per forward pass).  Same process, weights and scans; the five legs alternate in
blocks; before anything is timed the native half poses are checked against the Python autocast poses, bit for bit, at the size timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(values):
    v = np.asarray(values, dtype=np.float64)
    return {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)), "p90_ms": float(np.percentile(v, 90)), "min_ms": float(v.min()),
            "n": int(v.size)}


HALF_SHAPES = ((64, 720), (64, 2048))
HALF_LEGS = (("native_bf16", "native", "bfloat16"), ("native_fp16", "native", "float16"), ("native_fp32", "native", "float32"),
             ("torch_autocast_bf16", "torch", "bfloat16"), ("torch_autocast_fp16", "torch", "float16"))


def time_legs(push, names, args):
    """Warm every leg up, then ``args.rounds`` rounds of ``args.pushes`` timed pushes per leg, the legs alternating in blocks: per leg the
    host wall times, the stream times and the per-round medians."""
    for name in names:
        for _ in range(args.warmup):
            push(name)
    torch.cuda.synchronize()
    wall, stream, rounds = ({name: [] for name in names} for _ in range(3))
    for _ in range(args.rounds):
        for name in names:
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pushes)]
            w = []
            for e0, e1 in events:
                t0 = time.perf_counter()
                e0.record()
                push(name)
                e1.record()
                w.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            s = [e0.elapsed_time(e1) for e0, e1 in events]
            wall[name] += w
            stream[name] += s
            rounds[name].append({"wall_median_ms": float(np.median(w)), "stream_median_ms": float(np.median(s))})
    return {name: {"wall": stats(wall[name]), "stream": stats(stream[name]), "per_round": rounds[name]} for name in names}


def main_half(args):
    from delora_amd import config as cfgmod
    from delora_amd.data import synthetic
    from delora_amd.models import model as model_module
    from delora_amd.ros_utils import odometry
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    result = {"what": "ScanToScanOdometry.push latency, batch 1, random weights, resident scans; native half (dl_odometry_push_h) against native "
                      "fp32 (dl_odometry_push) and the Python autocast eval path (engine torch inside torch.autocast); legs alternate in blocks",
              "pushes_per_round": args.pushes, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for (H, W) in HALF_SHAPES:
        cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
        cfg["datasets"] = ["kitti"]
        cfgmod.degrees_to_radians(cfg)
        cfg.update(device=dev, checkpoint=None, integrate_odometry=True)
        cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = H, W
        torch.manual_seed(0)
        model = model_module.OdometryModel(config=cfg).to(dev).eval()
        model.resnet.trunk_weights_channels_last()
        scans = []
        for i in range(args.scans):                                # full-size scans: 64 rings x 2250 azimuth steps
            s = odometry.filter_scans(synthetic.make_pair(900 + i)[i % 2][None].astype(np.float32))
            scans.append(torch.from_numpy(np.ascontiguousarray(s)).to(dev))
        engines = {name: odometry.ScanToScanOdometry(cfg, model=model, engine=engine, precision=precision) for name, engine, precision in HALF_LEGS}
        counter = {name: 0 for name in engines}

        def push(name):
            counter[name] += 1
            return engines[name].push(scans[counter[name] % len(scans)])

        for k in range(4):
            got = {name: push(name) for name in engines}
            for half in ("bf16", "fp16"):
                a, b = got["native_" + half], got["torch_autocast_" + half]
                assert (a is None) == (b is None) and (a is None or np.array_equal(a["transformation"], b["transformation"])), \
                    f"{H}x{W} {half}: the native half path and the Python autocast path disagree"
        legs = time_legs(push, list(engines), args)
        result["shapes"][f"{H}x{W}"] = {"image": [H, W], "points_per_scan": [int(s.shape[2]) for s in scans], "legs": legs}
        for name in engines:
            e = legs[name]
            print(f"odometry_latency {H}x{W} {name:20s}: wall median {e['wall']['median_ms']:.3f} ms (p10 {e['wall']['p10_ms']:.3f}, p90 "
                  f"{e['wall']['p90_ms']:.3f}), stream median {e['stream']['median_ms']:.3f} ms (p10 {e['stream']['p10_ms']:.3f}, p90 "
                  f"{e['stream']['p90_ms']:.3f})", flush=True)
        del engines, model
        torch.cuda.empty_cache()
    out = args.out or os.path.join(ROOT, "profiles", "odometry_latency_half.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("->", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=200, help="timed pushes per engine and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--out", default=None, help="default: profiles/odometry_latency.json, with --half profiles/odometry_latency_half.json")
    ap.add_argument("--half", action="store_true", help="the half-precision legs at 64x720 and 64x2048 (see the module text)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("odometry_latency: no GPU -- nothing is measured without one")
    if args.half:
        return main_half(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "odometry_latency.json")
    from delora_amd import config as cfgmod
    from delora_amd.data import synthetic
    from delora_amd.models import model as model_module
    from delora_amd.ros_utils import odometry
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = ["kitti"]
    cfgmod.degrees_to_radians(cfg)
    cfg.update(device=dev, checkpoint=None, integrate_odometry=True)
    H, W = cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"]
    torch.manual_seed(0)
    model = model_module.OdometryModel(config=cfg).to(dev).eval()
    model.resnet.trunk_weights_channels_last()
    scans = []
    for i in range(args.scans):                                    # full-size scans: 64 rings x 2250 azimuth steps
        s = odometry.filter_scans(synthetic.make_pair(900 + i)[i % 2][None].astype(np.float32))
        scans.append(torch.from_numpy(np.ascontiguousarray(s)).to(dev))
    engines = {name: odometry.ScanToScanOdometry(cfg, model=model, engine=name) for name in ("torch", "native")}
    counter = {name: 0 for name in engines}

    def push(name):
        counter[name] += 1
        return engines[name].push(scans[counter[name] % len(scans)])

    # the two engines give the same poses on these scans (checked here at the size that is timed)
    for k in range(4):
        a, b = push("torch"), push("native")
        assert (a is None) == (b is None) and (a is None or np.array_equal(a["transformation"], b["transformation"])), "the engines disagree"
    for name in engines:
        for _ in range(args.warmup):
            push(name)
    torch.cuda.synchronize()
    wall = {name: [] for name in engines}
    stream = {name: [] for name in engines}
    rounds = {name: [] for name in engines}
    for _ in range(args.rounds):
        for name in engines:
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.pushes)]
            w = []
            for e0, e1 in events:
                t0 = time.perf_counter()
                e0.record()
                push(name)
                e1.record()
                w.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            s = [e0.elapsed_time(e1) for e0, e1 in events]
            wall[name] += w
            stream[name] += s
            rounds[name].append({"wall_median_ms": float(np.median(w)), "stream_median_ms": float(np.median(s))})
    result = {"what": "ScanToScanOdometry.push latency, 64x720, batch 1, fp32, random weights, resident scans; engines alternate in blocks",
              "image": [H, W], "points_per_scan": [int(s.shape[2]) for s in scans], "pushes_per_round": args.pushes, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0),
              "engines": {name: {"wall": stats(wall[name]), "stream": stats(stream[name]), "per_round": rounds[name]} for name in engines}}
    t, n = result["engines"]["torch"], result["engines"]["native"]
    result["native_not_slower"] = {"wall": n["wall"]["median_ms"] <= t["wall"]["median_ms"], "stream": n["stream"]["median_ms"] <= t["stream"]["median_ms"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for name in engines:
        e = result["engines"][name]
        print(f"odometry_latency {name:6s}: wall median {e['wall']['median_ms']:.3f} ms (p10 {e['wall']['p10_ms']:.3f}, p90 {e['wall']['p90_ms']:.3f}), "
              f"stream median {e['stream']['median_ms']:.3f} ms (p10 {e['stream']['p10_ms']:.3f}, p90 {e['stream']['p90_ms']:.3f})")
    print("native_not_slower:", result["native_not_slower"], "->", args.out)


if __name__ == "__main__":
    main()
