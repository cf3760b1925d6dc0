#!/usr/bin/env python3
"""Training-step time under ``amp_dtype`` with the stem in half precision (``amp_stem: true``) against the fp32 stem (``amp_stem: false``,
the path of every commit before the key existed):

    python tools/half_stem_step_time.py [--out profiles/half_stem_step.json] [--steps 20] [--rounds 9] [--warmup 10]

Per point -- bf16 and fp16, 64x2048 with B = 8 (the README's headline size) and 64x720 with B = 1 (the reference's shipped image and
batch) -- two trainers are built from the same seed in ONE process, both warmed up, then ``--rounds`` rounds ALTERNATE between them:
``--steps`` eager ``Trainer.step`` calls on one resident batch between two device synchronisations each.  Reported per setting: the
median over the rounds and their range (the run-to-run spread the comparison has to beat: a difference counts beyond three times the
larger range); per point: the difference of the medians in units of that range.  As in tools/tower_step_time.py
the network is put into the state identity pre-training leaves it in.

After the timed rounds every new kernel's own stream time is taken from the library's launch profile (``dl_profile_begin`` /
``dl_profile_end``: begin / end timestamps of each launch on its stream) over ``--profile-steps`` steps of the ``amp_stem: true`` trainer, and
set against the bytes the kernel has to move (derived, not counted: the table in DESIGN.md section 4.4) as achieved GB/s; the fp32
stem's fused weight gradient is listed from the other trainer for comparison."""
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

POINTS = (("bfloat16", 64, 2048, 8), ("float16", 64, 2048, 8), ("bfloat16", 64, 720, 1), ("float16", 64, 720, 1))      # (amp, H, W, B)


def derived_bytes(N, H, W):
    """Compulsory bytes per launch of the half stem: x is N 8 H W fp32, x8h the same elements in half, a has N H W/2 64 elements, y and
    win N H W/4 64; the weight gradient reads g, a, win and x8h once."""
    px = N * H * W
    a, y = px // 2 * 64, px // 4 * 64
    return {"k_stemh_input": px * 8 * 4 + px * 8 * 2, "k_stemh_conv1": px * 8 * 2 + a * 2, "k_stemh_pool": a * 2 + y * 2 + y,
            "k_stemh_wgrad": y * 2 + a * 2 + y + px * 8 * 2,
            "k_stem_wgrad": y * 4 + a * 4 + y + px * 8 * 4}


def build_config(amp, height, width, batch_size, amp_stem, device):
    from delora_amd import config as cfgmod
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = ["kitti"]
    cfgmod.degrees_to_radians(cfg)
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"]
    cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = height, width
    cfg.update(device=device, batch_size=batch_size, unsupervised_at_start=True, inference_only=False, checkpoint=None,
               training_run_name="half_stem_step_time", run_name="half_stem_step_time", mode="training", amp_dtype=amp, amp_stem=amp_stem)
    return cfg


def make_stepper(amp, height, width, batch_size, amp_stem, host_batch, device):
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    torch.manual_seed(0)
    trainer = Trainer(build_config(amp, height, width, batch_size, amp_stem, device), dataset=ListDataset(host_batch))
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


def stem_kernels(step, steps, N, H, W):
    """Stream time per launch of the stem's tagged kernels over ``steps`` steps (the library's own launch profile)."""
    from delora_amd import _lib
    want = derived_bytes(N, H, W)
    torch.cuda.synchronize()
    _lib.profile_begin(4096)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    rows, untimed = _lib.profile_end(1024)
    out = {}
    for r in rows:
        kernel = r["name"].split()[0] if r["name"] else ""
        for k, nbytes in want.items():
            if kernel == k and r["launches"]:
                us = 1e3 * r["ms"] / r["launches"]
                out[k] = {"row": r["name"], "launches_per_step": r["launches"] / steps, "us_per_launch": round(us, 2), "derived_bytes": nbytes,
                          "achieved_GBps": round(nbytes / (us * 1e-6) / 1e9, 1) if us > 0 else None}
    return out, untimed


def measure_point(a, amp, height, width, batch_size, device, batches):
    key = (height, batch_size)
    if key not in batches:
        batches[key] = make_batch(height, batch_size)
    paths = {}
    for amp_stem in (True, False):
        paths[amp_stem] = make_stepper(amp, height, width, batch_size, amp_stem, batches[key], device)
        for _ in range(a.warmup):
            paths[amp_stem][1]()
    rounds, loss = {True: [], False: []}, {}
    for _ in range(a.rounds):
        for amp_stem in (True, False):
            ms, loss[amp_stem] = timed(paths[amp_stem][1], a.steps)
            rounds[amp_stem].append(ms)
    rec = {"amp": amp, "image": f"{height}x{width}", "batch": batch_size, "steps_per_round": a.steps, "rounds": a.rounds}
    for amp_stem, name in ((True, "amp_stem_true"), (False, "amp_stem_false")):
        r = sorted(rounds[amp_stem])
        noted = getattr(paths[amp_stem][0].raw_model.resnet, "_module_path_noted", None)
        rec[name] = {"cnn_path": "modules" if noted else "hip", "ms_per_step": round(r[len(r) // 2], 4), "range_ms": round(r[-1] - r[0], 4),
                     "rounds_ms_per_step": [round(v, 4) for v in rounds[amp_stem]], "loss": loss[amp_stem]}
    spread = max(rec["amp_stem_true"]["range_ms"], rec["amp_stem_false"]["range_ms"])
    diff = rec["amp_stem_false"]["ms_per_step"] - rec["amp_stem_true"]["ms_per_step"]
    rec["false_minus_true_ms"] = round(diff, 4)
    rec["difference_over_range"] = round(diff / spread, 2) if spread > 0 else None
    rec["verdict"] = "faster" if spread > 0 and diff > 3 * spread else "slower" if spread > 0 and -diff > 3 * spread else "within the run-to-run range"
    if a.profile_steps > 0:
        rec["kernels_amp_stem_true"], untimed = stem_kernels(paths[True][1], a.profile_steps, batch_size, height, width)
        rec["kernels_amp_stem_false"], _ = stem_kernels(paths[False][1], a.profile_steps, batch_size, height, width)
        rec["untimed_launches"] = untimed
    print(json.dumps(rec), flush=True)
    del paths
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("half_stem_step_time.py measures on the GPU: none found")
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    batches = {}
    summary = {"what": "eager Trainer.step under amp_dtype: amp_stem true (half-precision stem) against false (fp32 stem), alternating rounds in "
                       "one process; kernel rows from the library's launch profile, bytes derived",
               "device": torch.cuda.get_device_name(0), "points": [measure_point(a, amp, h, w, b, device, batches) for (amp, h, w, b) in POINTS]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
