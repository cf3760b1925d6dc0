#!/usr/bin/env python3
"""Time of the product's training step with ``pre_feature_extraction: True``:   python tools/tower_step_time.py [--label branch]
                                            [--dropout] [--single-mlp] [--no-tower] [--case 64x2048x8] [--amp float32] [--kernel-times]

``Trainer.step`` on one resident batch, eager, in fp32 and under bf16 autocast, at 64x2048 with B = 8 (the README's headline size) and
at the reference's shipped 64x720 with B = 1.  Per case: ``--warmup`` steps, then ``--reps`` repetitions of ``--steps`` steps between two
synchronisations; the median and the range of the repetitions are reported, one JSON line per case and one summary line at the end.
The network is put into the state the reference's identity pre-training leaves it in (it predicts T = I: the last linear layer of both
heads zeroed, the quaternion biased to (0,0,0,1)), as every step benchmark of bench.py does: an untrained network predicts a random
rotation and every step's correspondence search would fall into its exhaustive fallback, a regime training never sees.
Uses nothing but the package's public configuration, data and ``Trainer`` interfaces, so the same file times any commit of the project
(A/B against a commit whose tower runs as library convolutions: ``cnn_path`` says which path the CNN took).
``--dropout`` / ``--single-mlp`` switch ``use_dropout`` / ``use_single_mlp_at_output`` on, ``--no-tower`` the tower off; ``--case`` and
``--amp`` restrict the run to one case, so that a caller can give every case a time limit of its own.  ``--kernel-times`` adds the
two element-wise kernels of dropout behind the tower (``dl_tower_wide_drop_f32`` / ``_bwd_f32``) at the case's size, timed alone
between events, with the bytes they must move."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((64, 2048, 8), (64, 720, 1))
_BATCHES = {}


def build_config(height, width, batch_size, amp, device, a=None):
    """The flat run config from config/*.yaml the way bin/run_training.py builds it, with the tower switched on."""
    from delora_amd import config as cfgmod
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = ["kitti"]
    cfgmod.degrees_to_radians(cfg)
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"]
    cfg["kitti"]["vertical_cells"], cfg["kitti"]["horizontal_cells"] = height, width
    cfg.update(device=device, batch_size=batch_size, unsupervised_at_start=True, inference_only=False, checkpoint=None,
               training_run_name="tower_step_time", run_name="tower_step_time", mode="training", pre_feature_extraction=True)
    if a is not None:
        cfg.update(pre_feature_extraction=not a.no_tower, use_dropout=bool(a.dropout), use_single_mlp_at_output=bool(a.single_mlp))
    if amp:
        cfg["amp_dtype"] = amp
    return cfg


def make_batch(height, batch_size):
    """B synthetic scan pairs (ray-cast scenes of delora_amd.data.synthetic, points in raster order), on the host."""
    from delora_amd.data import synthetic
    samples = []
    for j in range(batch_size):
        s1, s2, _ = synthetic.make_pair(2000 + j, rings=height, azimuth_steps=2250)
        samples.append({"dataset": "kitti", "scan_1": torch.from_numpy(s1).unsqueeze(0), "scan_2": torch.from_numpy(s2).unsqueeze(0),
                        "normal_list_1": None, "normal_list_2": None})
    return samples


def identity_pretrained_state(model):
    with torch.no_grad():
        if hasattr(model, "fully_connected_rot_trans"):                      # the single MLP: rows 0..3 quaternion, 4..6 translation
            last = model.fully_connected_rot_trans[-1]
            last.weight.zero_()
            last.bias.copy_(torch.tensor([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]))
            return
        rot, tra = model.fully_connected_rotation[-1], model.fully_connected_translation[-1]
        rot.weight.zero_()
        rot.bias.copy_(torch.tensor([0.0, 0.0, 0.0, 1.0]))
        tra.weight.zero_()
        tra.bias.zero_()


def time_case(a, height, width, batch_size, amp, device):
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = build_config(height, width, batch_size, amp, device, a)
    torch.manual_seed(0)
    key = (height, batch_size)
    if key not in _BATCHES:                              # (ray casting costs ~0.4 s per pair: once per size)
        _BATCHES[key] = make_batch(height, batch_size)
    host_batch = _BATCHES[key]
    trainer = Trainer(cfg, dataset=ListDataset(host_batch))
    identity_pretrained_state(trainer.raw_model)
    batch = trainer.to_device([dict(d) for d in host_batch])

    def step():
        trainer.optimizer.zero_grad(set_to_none=True)
        return trainer.step(preprocessed_dicts=[dict(d) for d in batch], epoch_losses=trainer.new_epoch_losses())

    for _ in range(a.warmup):
        ep, _ = step()
    reps = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ep, _ = step()
        torch.cuda.synchronize()
        reps.append(1e3 * (time.perf_counter() - t0) / a.steps)
    noted = getattr(trainer.raw_model.resnet, "_module_path_noted", None)
    rec = {"label": a.label, "image": f"{height}x{width}", "batch": batch_size, "amp": amp or "float32", "tower": not a.no_tower,
           "dropout": bool(a.dropout), "single_mlp": bool(a.single_mlp),
           "cnn_path": "modules" if noted else "hip", "steps": a.steps, "reps_ms_per_step": [round(r, 4) for r in reps],
           "ms_per_step": round(sorted(reps)[len(reps) // 2], 4), "range_ms": round(max(reps) - min(reps), 4), "loss": float(ep["loss_epoch"])}
    print(json.dumps(rec), flush=True)
    del trainer, batch
    torch.cuda.empty_cache()
    return rec


def kernel_times(height, width, batch_size, device, reps=20):
    """``dl_tower_wide_drop_f32`` / ``dl_tower_wide_drop_bwd_f32`` alone at the case's size: median of ``reps`` event-timed launches
    after two warm-up launches, next to the bytes each must move (forward: the compact map in, the whole pitch-128 buffer out;
    backward: the 80 live channels of the gradient and the compact map in, the compact gradient out)."""
    import ctypes
    from delora_amd import _lib
    from delora_amd.models import ring_conv as rc
    lib = _lib.load()
    B, H, W, CH, P = batch_size, height, width, rc.TOWER_CHANNELS // 2, rc.TOWER_PITCH
    y5 = torch.tanh(torch.randn((2 * B, H, W, CH), device=device))
    gx = torch.randn((B, H, W, P), device=device)
    xw, g5 = torch.empty_like(gx), torch.empty_like(y5)
    seed = rc.draw_seed(device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)          # noqa: E731
    calls = {"dl_tower_wide_drop_f32": (lambda: lib.dl_tower_wide_drop_f32(vp(y5), vp(seed), 0.2, B, H, W, CH, P, vp(xw), st()),
                                        4 * B * H * W * (2 * CH + P)),
             "dl_tower_wide_drop_bwd_f32": (lambda: lib.dl_tower_wide_drop_bwd_f32(vp(gx), vp(y5), vp(seed), 0.2, 1, B, H, W, CH, P, vp(g5), st()),
                                            4 * B * H * W * 6 * CH)}
    out = {}
    for name, (fn, nbytes) in calls.items():
        ms = []
        for i in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(fn(), name)
            e1.record()
            torch.cuda.synchronize()
            if i >= 2:
                ms.append(e0.elapsed_time(e1))
        med = sorted(ms)[len(ms) // 2]
        out[name] = {"ms": round(med, 4), "range_ms": round(max(ms) - min(ms), 4), "bytes": nbytes, "TB_per_s": round(nbytes / med * 1e-9, 3)}
    rec = {"image": f"{height}x{width}", "batch": batch_size, "kernels": out}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--dropout", action="store_true", help="use_dropout: True")
    ap.add_argument("--single-mlp", action="store_true", help="use_single_mlp_at_output: True")
    ap.add_argument("--no-tower", action="store_true", help="pre_feature_extraction: False")
    ap.add_argument("--case", default="", help="HxWxB: only this case (default: 64x2048x8 and 64x720x1)")
    ap.add_argument("--amp", default="", choices=("", "float32", "bfloat16"), help="only this precision (default: both)")
    ap.add_argument("--kernel-times", action="store_true", help="also time the two tower dropout kernels alone")
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cases = (tuple(int(v) for v in a.case.split("x")),) if a.case else CASES
    amps = {"": ("", "bfloat16"), "float32": ("",), "bfloat16": ("bfloat16",)}[a.amp]
    records = [time_case(a, h, w, b, amp, device) for (h, w, b) in cases for amp in amps]
    summary = {"label": a.label, "cases": records}
    if a.kernel_times:
        summary["kernel_times"] = [kernel_times(h, w, b, device) for (h, w, b) in cases]
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
