#!/usr/bin/env python3
"""What the pose quality costs per push: ``ScanToScanOdometry.push`` with and without ``quality=True`` on both engines, at 64x720 and
at 64x2048, batch 1, fp32.   python tools/odometry_quality_latency.py [--pushes N] [--rounds R] [--out FILE]

Four legs per shape -- engine "torch" and engine "native", each without quality (the push as it was before the quality path existed:
nothing new is launched) and with it (normals of the new image, the exact search, the normal equations and their read-back) --, same
process, same weights, same scans, the legs ALTERNATING in blocks so that drift of the host hits all of them.  Before anything is timed
the two engines' quality outputs are checked against each other, bit for bit, at the size timed.  Per leg (tools/odometry_latency.py's
measures): host wall time of the call (it ends in the ``.cpu()`` of the pose and, with quality, of the 6x6 matrices) and the stream
time between two events; median, 10th / 90th percentile, minimum, and the per-round medians with their range (the run-to-run spread of
the same code).  ``extra_ms`` is the difference of the medians with and without quality.  Writes profiles/odometry_quality.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from odometry_latency import time_legs  # noqa: E402

SHAPES = ((64, 720), (64, 2048))
LEGS = (("torch", "torch", False), ("torch_quality", "torch", True), ("native", "native", False), ("native_quality", "native", True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=100, help="timed pushes per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--scans", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_quality.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("odometry_quality_latency: no GPU -- nothing is measured without one")
    from delora_amd import config as cfgmod
    from delora_amd.data import synthetic
    from delora_amd.models import model as model_module
    from delora_amd.ros_utils import odometry
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    result = {"what": "ScanToScanOdometry.push latency with and without quality=True, batch 1, fp32, random weights, resident scans of one "
                      "synthetic sequence; the four legs alternate in blocks",
              "pushes_per_round": args.pushes, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for (H, W) in SHAPES:
        cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
        cfg["datasets"] = ["kitti"]
        cfgmod.degrees_to_radians(cfg)
        cfg.update(device=dev, checkpoint=None, integrate_odometry=True)
        cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = H, W
        torch.manual_seed(0)
        model = model_module.OdometryModel(config=cfg).to(dev).eval()
        model.resnet.trunk_weights_channels_last()
        # consecutive full-size scans of one scene (64 rings x 2250 azimuth steps): the pairs the search sees overlap as real ones do
        scans = [torch.from_numpy(np.ascontiguousarray(odometry.filter_scans(s[None].astype(np.float32)))).to(dev)
                 for s in synthetic.make_sequence(900, args.scans)[0]]
        engines = {name: odometry.ScanToScanOdometry(cfg, model=model, engine=engine, quality=quality) for name, engine, quality in LEGS}
        counter = {name: 0 for name in engines}

        def push(name):
            counter[name] += 1
            return engines[name].push(scans[counter[name] % len(scans)])

        status = []
        for k in range(4):
            got = {name: push(name) for name in engines}
            a, b = got["torch_quality"], got["native_quality"]
            assert (a is None) == (b is None), "the engines disagree"
            if a is not None:
                for key in ("transformation", "covariance", "information", "pairs", "quality_status"):
                    assert np.array_equal(a[key], b[key]), f"{H}x{W}: the engines disagree on {key}"
                assert np.array_equal(a["transformation"], got["native"]["transformation"]), f"{H}x{W}: quality changed the pose"
                status.append({"quality_status": a["quality_status"], "pairs": a["pairs"], "residual_rms": a["residual_rms"]})
        legs = time_legs(push, list(engines), args)
        entry = {"image": [H, W], "points_per_scan": [int(s.shape[2]) for s in scans], "checked_pushes": status, "legs": legs, "extra_ms": {}}
        for engine in ("torch", "native"):
            base, with_q = legs[engine], legs[engine + "_quality"]
            entry["extra_ms"][engine] = {m: with_q[m]["median_ms"] - base[m]["median_ms"] for m in ("wall", "stream")}
            for name in (engine, engine + "_quality"):
                for m in ("wall", "stream"):
                    r = [x[m + "_median_ms"] for x in legs[name]["per_round"]]
                    legs[name][m]["round_medians_range_ms"] = [min(r), max(r)]
        result["shapes"][f"{H}x{W}"] = entry
        for name in engines:
            e = legs[name]
            print(f"odometry_quality_latency {H}x{W} {name:15s}: wall median {e['wall']['median_ms']:.3f} ms (rounds {e['wall']['round_medians_range_ms'][0]:.3f}.."
                  f"{e['wall']['round_medians_range_ms'][1]:.3f}), stream median {e['stream']['median_ms']:.3f} ms (rounds "
                  f"{e['stream']['round_medians_range_ms'][0]:.3f}..{e['stream']['round_medians_range_ms'][1]:.3f})", flush=True)
        print(f"odometry_quality_latency {H}x{W} extra per push: {entry['extra_ms']}", flush=True)
        del engines, model
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
