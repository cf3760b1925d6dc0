#!/usr/bin/env python3
"""Training-step time of the NARROW pose networks (``factor_fewer_resnet_channels`` 2 and 4), HIP routing against the module path:

    python tools/narrow_step_time.py [--out profiles/narrow_step.json] [--steps 20] [--rounds 7] [--warmup 10] [--kernels]

Per point -- factor 2 and 4, 64x720 with B = 1 (the reference's shipped image and batch) and 64x2048 with B = 8 (the README's headline
size), fp32 -- two trainers are built from the same seed in ONE process: ``cnn_impl: auto`` (the narrow layers on csrc/narrow.hip, the
rest on the Winograd / direct kernels) and ``cnn_impl: modules`` (library convolutions: what such a network ran before).  Both are
warmed up, then ``--rounds`` rounds ALTERNATE between them: ``--steps`` eager ``Trainer.step`` calls on one resident batch between two
device synchronisations each.  Reported per path: the median over the rounds and their range (the run-to-run spread the comparison has
to beat); per point: the ratio of the medians.  As in tools/tower_step_time.py the network is put into the state identity pre-training
leaves it in, so that the correspondence search runs in the regime training sees.  ``--kernels`` adds, per point, the ten kernels with
the most device time over five profiled steps of the HIP trainer (torch.profiler, after the timed rounds: tracing slows the host)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from tower_step_time import identity_pretrained_state, make_batch  # noqa: E402

POINTS = ((2, 64, 720, 1), (4, 64, 720, 1), (2, 64, 2048, 8), (4, 64, 2048, 8))       # (factor, H, W, B)


def build_config(factor, height, width, batch_size, impl, device):
    from delora_amd import config as cfgmod
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = ["kitti"]
    cfgmod.degrees_to_radians(cfg)
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"]
    cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = height, width
    cfg.update(device=device, batch_size=batch_size, unsupervised_at_start=True, inference_only=False, checkpoint=None,
               training_run_name="narrow_step_time", run_name="narrow_step_time", mode="training", factor_fewer_resnet_channels=factor,
               cnn_impl=impl)
    return cfg


def make_stepper(factor, height, width, batch_size, impl, host_batch, device):
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    torch.manual_seed(0)
    trainer = Trainer(build_config(factor, height, width, batch_size, impl, device), dataset=ListDataset(host_batch))
    identity_pretrained_state(trainer.raw_model)
    batch = trainer.to_device([dict(d) for d in host_batch])

    def step():
        trainer.optimizer.zero_grad(set_to_none=True)
        return trainer.step(preprocessed_dicts=[dict(d) for d in batch], epoch_losses=trainer.new_epoch_losses())

    return trainer, step


def timed(step, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        ep, _ = step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps, float(ep["loss_epoch"])


def top_kernels(step, n=10, steps=5):
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    rows = [(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0), e.count, e.key) for e in prof.key_averages()
            if getattr(e, "device_type", None) is not None and str(e.device_type).endswith("CUDA")]
    rows.sort(reverse=True)
    total = sum(r[0] for r in rows) or 1.0
    return [{"kernel": k[:120], "launches_per_step": c / steps, "ms_per_step": round(t / steps * 1e-3, 4), "share": round(t / total, 3)}
            for t, c, k in rows[:n]]


def measure_point(a, factor, height, width, batch_size, device, batches):
    key = (height, batch_size)
    if key not in batches:
        batches[key] = make_batch(height, batch_size)
    paths = {}
    for impl in ("auto", "modules"):
        paths[impl] = make_stepper(factor, height, width, batch_size, impl, batches[key], device)
        for _ in range(a.warmup):
            paths[impl][1]()
    rounds = {"auto": [], "modules": []}
    loss = {}
    for _ in range(a.rounds):
        for impl in ("auto", "modules"):
            ms, loss[impl] = timed(paths[impl][1], a.steps)
            rounds[impl].append(ms)
    rec = {"factor": factor, "image": f"{height}x{width}", "batch": batch_size, "steps_per_round": a.steps, "rounds": a.rounds}
    for impl, name in (("auto", "hip"), ("modules", "modules")):
        r = sorted(rounds[impl])
        noted = getattr(paths[impl][0].raw_model.resnet, "_module_path_noted", None)
        rec[name] = {"cnn_path": "modules" if (noted or impl == "modules") else "hip", "ms_per_step": round(r[len(r) // 2], 4),
                     "range_ms": round(r[-1] - r[0], 4), "rounds_ms_per_step": [round(v, 4) for v in rounds[impl]], "loss": loss[impl]}
    rec["modules_over_hip"] = round(rec["modules"]["ms_per_step"] / rec["hip"]["ms_per_step"], 3)
    if a.kernels:
        rec["hip_kernels"] = top_kernels(paths["auto"][1])
    print(json.dumps(rec), flush=True)
    del paths
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("narrow_step_time.py measures on the GPU: none found")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    batches = {}
    summary = {"what": "eager Trainer.step, fp32, narrow pose networks: cnn_impl auto (HIP) against modules, alternating rounds in one process",
               "device": torch.cuda.get_device_name(0), "points": [measure_point(a, f, h, w, b, device, batches) for (f, h, w, b) in POINTS]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
