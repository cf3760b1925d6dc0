#!/usr/bin/env python3
"""From a raw message to a pose: what the ingest of a scan costs at the reference's shipped operating point (unmodified YAML: 64x720,
batch 1), by the method of tools/odometry_latency.py -- one process, the same weights and the same messages for every leg, the legs
ALTERNATING in rounds so that drift of the host hits all of them, medians and 10th / 90th percentiles, a push ending in the ``.cpu()``
of the pose.   python tools/odometry_ingest.py [--pushes N] [--rounds R] [--out FILE]

Messages are PAGEABLE numpy ``[N,4]`` fp32 arrays (a KITTI .bin file: x, y, z, intensity; ~141 k points, 16 bytes per point) holding
missing returns (all-zero records) and returns from within 0.3 m, as a driver delivers them.  The legs:

  torch           engine "torch",  ``push(numpy [1,4,N])``: the node's filter on the host, upload, projection of the pair, the modules
  native          engine "native", ``push(numpy [1,4,N])``: the node's filter on the host, upload, ``dl_odometry_push``
  native_records  engine "native", ``push_records(numpy [N,4])``: staged upload of the raw records, ``dl_odometry_push_records``

Then, by HIP events on resident data (S = 1, the same points): ``dl_project`` on the host-filtered planar scan against
``dl_project_records`` (filter 3, 0.3 m) on raw records of 16, 32 and 48 bytes; and ``dl_project_records`` with filter 0 on the
FILTERED points packed as records, which is the planar vote's work on the same points.  Each timed window holds ``--kernel-calls``
calls between two events, queued behind a matrix product of a few milliseconds (the host enqueues a projection's three short launches
no faster than the GPU runs them; without it the events time the host); medians and percentiles over ``--kernel-windows`` windows,
the variants alternating."""
import argparse
import ctypes
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


def make_messages(n):
    """n ``[N,4]`` fp32 messages: a full-size synthetic scan, 2 % of its records zeroed (missing returns) and 0.5 % pulled inside 0.3 m."""
    from delora_amd.data import synthetic
    out = []
    for i in range(n):
        xyz = np.asarray(synthetic.make_pair(900 + i)[i % 2][:3], dtype=np.float32)
        rng = np.random.default_rng(1900 + i)
        msg = np.concatenate([xyz.T, rng.uniform(0, 1, (xyz.shape[1], 1)).astype(np.float32)], axis=1)
        pick = rng.permutation(msg.shape[0])
        a, b = msg.shape[0] // 50, msg.shape[0] // 50 + msg.shape[0] // 200
        msg[pick[:a]] = 0.0
        msg[pick[a:b], :3] *= (0.2 / np.maximum(np.linalg.norm(msg[pick[a:b], :3], axis=1, keepdims=True), 1e-6)).astype(np.float32)
        out.append(np.ascontiguousarray(msg))
    return out


def widen(msg, step):
    """The same points as ``step``-byte records (x, y, z first, the rest of the record zero)."""
    out = np.zeros((msg.shape[0], step // 4), dtype=np.float32)
    out[:, :3] = msg[:, :3]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=60, help="timed pushes per leg and round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--messages", type=int, default=6)
    ap.add_argument("--kernel-calls", type=int, default=20, help="projection calls per timed window")
    ap.add_argument("--kernel-windows", type=int, default=25, help="timed windows per variant and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "odometry_ingest.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("odometry_ingest: no GPU -- nothing is measured without one")
    from delora_amd import _lib, geometry
    from delora_amd import config as cfgmod
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
    msgs = make_messages(args.messages)
    planar = [np.ascontiguousarray(m.T)[None] for m in msgs]          # [1,4,N]: what ``push`` takes (prepared outside the timed region)
    legs = {"torch": ("torch", "push"), "native": ("native", "push"), "native_records": ("native", "push_records")}
    nodes = {leg: odometry.ScanToScanOdometry(cfg, model=model, engine=engine) for leg, (engine, _) in legs.items()}
    counter = {leg: 0 for leg in legs}

    def push(leg):
        counter[leg] += 1
        k = counter[leg] % len(msgs)
        return nodes[leg].push_records(msgs[k]) if legs[leg][1] == "push_records" else nodes[leg].push(planar[k])

    # the three legs give the same poses on these messages (checked here at the size that is timed)
    for k in range(4):
        got = [push(leg) for leg in legs]
        assert all((g is None) == (got[0] is None) for g in got), "the legs disagree"
        assert got[0] is None or all(np.array_equal(g["transformation"], got[0]["transformation"]) for g in got), "the legs disagree"
    for leg in legs:
        for _ in range(args.warmup):
            push(leg)
    torch.cuda.synchronize()
    wall = {leg: [] for leg in legs}
    rounds = {leg: [] for leg in legs}
    for _ in range(args.rounds):
        for leg in legs:
            w = []
            for _ in range(args.pushes):
                t0 = time.perf_counter()
                push(leg)
                w.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            wall[leg] += w
            rounds[leg].append(float(np.median(w)))
    # the host filter alone, on the GPU machine's host (numpy, one message; it is inside the two ``push`` legs)
    host_filter = []
    for k in range(3 * len(msgs)):
        t0 = time.perf_counter()
        odometry.filter_scans(planar[k % len(msgs)])
        host_filter.append(1e3 * (time.perf_counter() - t0))

    # ---- the projection kernels alone, HIP events, resident data
    sensor = nodes["native"].sensor
    m = msgs[0]
    kept = np.ascontiguousarray(odometry.filter_scans(planar[0])[0, :3])
    n_raw, n_kept = m.shape[0], kept.shape[1]
    d_planar = torch.from_numpy(kept).to(dev)
    offs_kept = torch.tensor([0, n_kept], dtype=torch.int32, device=dev)
    offs_raw = torch.tensor([0, n_raw], dtype=torch.int32, device=dev)
    flt = _lib.RECORDS_DROP_ZERO | _lib.RECORDS_MIN_RANGE
    # the C ABI called directly on preallocated buffers (no allocation, one ctypes call per projection); the host's enqueue time per call
    # is recorded next to the stream time
    lib, p, sp = _lib.load(), geometry._ptr, ctypes.byref(sensor.struct)
    image4 = torch.empty((1, 4, H, W), dtype=torch.float32, device=dev)
    pix2pt = torch.empty((1, H, W), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.dl_project_workspace_bytes(1, H, W, n_raw, 3) // 8,), dtype=torch.int64, device=dev)

    def planar_call():
        _lib.check(lib.dl_project(p(d_planar), d_planar.stride(0), n_kept, p(offs_kept), 1, 3, n_kept, sp, p(image4), None, None, None, p(pix2pt),
                                  p(ws), None, None, geometry._stream()), "dl_project")
        return image4

    def records_call(rec, n, offs, lay):
        _lib.check(lib.dl_project_records(p(rec), n, ctypes.byref(lay), p(offs), 1, n, sp, p(image4), None, p(pix2pt), p(ws), None, None,
                                          geometry._stream()), "dl_project_records")
        return image4

    variants = {"dl_project planar (filtered points)": planar_call}
    for step in (16, 32, 48):
        raw = torch.from_numpy(widen(m, step).reshape(-1)).to(dev)
        packed_kept = torch.from_numpy(widen(np.ascontiguousarray(kept.T), step).reshape(-1)).to(dev)
        lay_f, lay_0 = geometry.record_layout(step, (0, 4, 8), flt, 0.3), geometry.record_layout(step, (0, 4, 8), 0, 0.0)
        variants[f"dl_project_records step {step} (raw records, filter in the vote)"] = (
            lambda raw=raw, lay=lay_f: records_call(raw, n_raw, offs_raw, lay))
        variants[f"dl_project_records step {step} (filtered points, no filter)"] = (
            lambda rec=packed_kept, lay=lay_0: records_call(rec, n_kept, offs_kept, lay))
    ref_img = planar_call().clone()
    for name, fn in variants.items():                                # every variant yields the planar path's image, to the bit
        assert torch.equal(fn(), ref_img), name
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    ktimes = {name: [] for name in variants}
    khost = {name: [] for name in variants}
    kblock = {name: [] for name in variants}
    blocker_a = torch.randn((6144, 6144), dtype=torch.float32, device=dev)
    blocker_c = torch.empty_like(blocker_a)
    torch.mm(blocker_a, blocker_a, out=blocker_c)
    torch.cuda.synchronize()
    krounds = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.kernel_windows)]
            blockers = []
            for e0, e1 in events:
                # one projection is ~3 short launches: the host enqueues them no faster than the GPU runs them.  A matrix product of a few
                # milliseconds goes first, the calls queue up behind it, and the two events then bracket kernels that run back to back
                torch.cuda.synchronize()
                eb = torch.cuda.Event(enable_timing=True)
                eb.record()
                torch.mm(blocker_a, blocker_a, out=blocker_c)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.kernel_calls):
                    fn()
                e1.record()
                khost[name].append(1e3 * (time.perf_counter() - t0) / args.kernel_calls)
                blockers.append(eb)
            torch.cuda.synchronize()
            t = [e0.elapsed_time(e1) / args.kernel_calls for e0, e1 in events]
            kblock[name] += [eb.elapsed_time(e0) for eb, (e0, _) in zip(blockers, events)]
            ktimes[name] += t
            krounds[name].append(float(np.median(t)))

    spread = {leg: max(r) - min(r) for leg, r in rounds.items()}
    b, c = float(np.median(wall["native"])), float(np.median(wall["native_records"]))
    result = {"what": "message -> pose, 64x720, batch 1, fp32, random weights; pageable numpy [N,4] fp32 messages; legs alternate in rounds; a push "
                      "ends in the .cpu() of the pose",
              "image": [H, W], "records_per_message": [int(x.shape[0]) for x in msgs], "pushes_per_round": args.pushes, "rounds": args.rounds,
              "device": torch.cuda.get_device_name(0),
              "legs": {leg: {"engine": legs[leg][0], "entry": legs[leg][1], "wall": stats(wall[leg]), "per_round_median_ms": rounds[leg],
                             "spread_between_rounds_ms": spread[leg]} for leg in legs},
              "host_filter_alone": stats(host_filter),
              "records_below_native": {"native_median_ms": b, "native_records_median_ms": c, "difference_ms": b - c,
                                       "largest_spread_between_rounds_ms": max(spread["native"], spread["native_records"]),
                                       "holds": bool(b - c > max(spread["native"], spread["native_records"]))},
              "projection_kernels": {"what": "one projection call (key-plane fill + vote + resolve, image4 + pix2pt only), S = 1, HIP events around "
                                             f"{args.kernel_calls} direct C ABI calls on preallocated buffers, per call; host_enqueue_per_call is the host's time to "
                                             "enqueue one call; every window starts behind a matrix product of blocker_ms so that the calls are queued "
                                             "before the first one runs (enqueued_behind_the_blocker: true for every window) and the events time kernels "
                                             "running back to back, not the host",
                                     "raw_records": n_raw, "filtered_points": n_kept,
                                     "variants": {name: {"per_call": stats(ktimes[name]), "per_round_median_ms": krounds[name],
                                                         "host_enqueue_per_call": stats(khost[name]), "blocker_ms": stats(kblock[name]),
                                                         "enqueued_behind_the_blocker": bool(args.kernel_calls * np.max(khost[name]) < np.min(kblock[name]))}
                                                  for name in variants}},
              "lds_staging": "not built: see DESIGN.md section 6.6 for what the step 32 / 48 timings above say about it"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for leg in legs:
        e = result["legs"][leg]
        print(f"odometry_ingest {leg:15s}: wall median {e['wall']['median_ms']:.3f} ms (p10 {e['wall']['p10_ms']:.3f}, p90 {e['wall']['p90_ms']:.3f}), "
              f"round medians spread {e['spread_between_rounds_ms']:.3f} ms")
    print(f"odometry_ingest host filter alone: median {result['host_filter_alone']['median_ms']:.3f} ms")
    for name in variants:
        e, h = result["projection_kernels"]["variants"][name]["per_call"], result["projection_kernels"]["variants"][name]["host_enqueue_per_call"]
        print(f"odometry_ingest {name}: median {1e3 * e['median_ms']:.1f} us (p10 {1e3 * e['p10_ms']:.1f}, p90 {1e3 * e['p90_ms']:.1f}); host enqueue "
              f"{1e3 * h['median_ms']:.1f} us, behind the blocker: {result['projection_kernels']['variants'][name]['enqueued_behind_the_blocker']}")
    print("records_below_native:", result["records_below_native"], "->", args.out)


if __name__ == "__main__":
    main()
