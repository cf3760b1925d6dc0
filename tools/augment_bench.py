#!/usr/bin/env python3
"""Training-step time with ``random_point_cloud_rotations`` off and on:

    python tools/augment_bench.py [--out profiles/augment_step.json] [--steps 200] [--repeats 3] [--warmup 20] [--bench-lines FILE]

Per point -- 64x720 with B = 1 (the reference's shipped image and batch) and 64x2048 with B = 8 (the README's headline size), fp32,
the full-width network -- two trainers are built from the same seed in ONE process, one with the option off and one with it on
(``magnitude_random_rot`` 4 degrees, any axis: the shipped values).  Both are warmed up, then ``--repeats`` repeats ALTERNATE between
them: ``--steps`` eager ``Trainer.step`` calls on one resident batch between two device synchronisations each.  Reported per setting:
the median over the repeats and their range (the spread the difference has to beat); per point: on minus off.  What the option adds to
a step: one ``torch.rand`` of 4B numbers, one launch of B threads for the matrices, and nine multiplies and six adds per point of scan
2 inside the projection's vote -- no pass of its own over the points.  As in tools/tower_step_time.py the network is put into the state
identity pre-training leaves it in, so that the correspondence search runs in the regime training sees.

``--bench-lines FILE``: a text file with the JSON result lines of ``bench.py --gpus 1 --steps 100 --warmup 5`` run on the parent commit
and on this one, alternating, each line prefixed by its label (``parent`` / ``this``) and a space; they are stored under
``unaugmented_bench`` next to the parent's own spread, which the difference has to stay inside.  Nothing about training quality is
measured here."""
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

POINTS = ((64, 720, 1), (64, 2048, 8))       # (H, W, B)


def build_config(height, width, batch_size, augment, device):
    from delora_amd import config as cfgmod
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = ["kitti"]
    cfgmod.degrees_to_radians(cfg)
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"]
    cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = height, width
    cfg.update(device=device, batch_size=batch_size, unsupervised_at_start=True, inference_only=False, checkpoint=None,
               training_run_name="augment_bench", run_name="augment_bench", mode="training", random_point_cloud_rotations=bool(augment))
    return cfg


def make_stepper(height, width, batch_size, augment, host_batch, device):
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    torch.manual_seed(0)
    trainer = Trainer(build_config(height, width, batch_size, augment, device), dataset=ListDataset(host_batch))
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


def measure_point(a, height, width, batch_size, device):
    host_batch = make_batch(height, batch_size)
    paths = {}
    for name, augment in (("off", False), ("on", True)):
        paths[name] = make_stepper(height, width, batch_size, augment, host_batch, device)
        for _ in range(a.warmup):
            paths[name][1]()
    assert paths["off"][0].last_step["rotations"] is None and paths["on"][0].last_step["rotations"] is not None
    repeats, loss = {"off": [], "on": []}, {}
    for _ in range(a.repeats):
        for name in ("off", "on"):
            ms, loss[name] = timed(paths[name][1], a.steps)
            repeats[name].append(ms)
    rec = {"image": f"{height}x{width}", "batch": batch_size, "steps_per_repeat": a.steps, "repeats": a.repeats}
    for name in ("off", "on"):
        r = sorted(repeats[name])
        rec[name] = {"ms_per_step": round(r[len(r) // 2], 4), "range_ms": round(r[-1] - r[0], 4),
                     "repeats_ms_per_step": [round(v, 4) for v in repeats[name]], "loss": loss[name]}
    rec["on_minus_off_ms"] = round(rec["on"]["ms_per_step"] - rec["off"]["ms_per_step"], 4)
    print(json.dumps(rec), flush=True)
    del paths
    torch.cuda.empty_cache()
    return rec


def bench_lines(path):
    """{"parent": [result, ...], "this": [...]} from lines "<label> <json>", in the order they were run."""
    runs, order = {"parent": [], "this": []}, []
    with open(path) as f:
        for line in f:
            label, _, text = line.strip().partition(" ")
            if label in runs and text.startswith("{"):
                runs[label].append(json.loads(text))
                order.append(label)
    return {"command": "python bench.py --gpus 1 --steps 100 --warmup 5", "order": order, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bench-lines", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench.py measures on the GPU: none found")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    summary = {"what": "eager Trainer.step, fp32, full-width network: random_point_cloud_rotations off against on, alternating repeats in one process",
               "device": torch.cuda.get_device_name(0), "points": [measure_point(a, h, w, b, device) for (h, w, b) in POINTS]}
    if a.bench_lines:
        summary["unaugmented_bench"] = bench_lines(a.bench_lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
