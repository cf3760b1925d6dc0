#!/usr/bin/env python3
"""Time of the product's training step with ``use_dropout`` on or off:   python tools/dropout_step_time.py [--amp bfloat16] [--dropout 1]

``Trainer.step`` on one resident batch at 64x2048, B = 8 (the size of the README's headline), eager, every shape warmed up, then
``--steps`` steps between two synchronisations; one JSON line.  Uses nothing but the trainer's public configuration, so the same file
times any commit of the project (A/B against a commit without dropout on the HIP path: ``cnn_path`` says which path the CNN took)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--amp", default="")
    ap.add_argument("--dropout", type=int, default=0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    a.channels_last, a.cnn = False, ""
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = bench.build_config(a, device)
    cfg["use_dropout"] = bool(a.dropout)
    torch.manual_seed(0)
    host_batch = bench.make_batch(a, 0)
    trainer = Trainer(cfg, dataset=ListDataset(host_batch))
    batch = bench.to_device(host_batch, device)

    def step():
        trainer.optimizer.zero_grad(set_to_none=True)
        return trainer.step(preprocessed_dicts=[dict(d) for d in batch], epoch_losses=trainer.new_epoch_losses())

    for _ in range(a.warmup):
        ep, _ = step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ep, _ = step()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    noted = getattr(trainer.raw_model.resnet, "_module_path_noted", None)
    print(json.dumps({"label": a.label, "image": f"{a.height}x{a.width}", "batch": a.batch, "amp": a.amp or "float32", "use_dropout": bool(a.dropout),
                      "cnn_path": "modules" if noted else "hip", "steps": a.steps, "ms_per_step": round(1e3 * el / a.steps, 4),
                      "host_enqueue_ms_per_step": round(1e3 * host / a.steps, 4), "pairs_per_s": round(a.batch * a.steps / el, 1),
                      "loss": float(ep["loss_epoch"])}), flush=True)


if __name__ == "__main__":
    main()
