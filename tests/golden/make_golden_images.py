#!/usr/bin/env python3
"""Generate tests/golden/step_images_b2.npz by RUNNING THE REFERENCE: the six logged images of ``Trainer.step(log_images_bool=True)``
on the 16x128, B = 2 small configuration of the ``step_b2`` fixture (same scans, same initial weights), with one boolean
``ambiguous`` pixel mask per image.  Like make_golden.py it runs only where the reference tree is present and uses its stubs.

The mask of an image is computed in float64 from the reference's OWN candidate points of that image (the arguments it hands to its
projection layer).  A pixel is ambiguous if
  * a candidate lies within 2e-3 px of a rounding boundary of that pixel (make_golden.ambiguity_mask's tolerance; both pixels that
    share the boundary are marked), or
  * its two smallest candidate ranges differ by less than 1e-4 m (another correct evaluation may rank them the other way round).
The mask may cover at most 5 % of an image's occupied pixels: asserted here and again by the test.  If a seed breaks that cap the
seed changes, not the cap.

Usage:  python tests/golden/make_golden_images.py
"""
import copy
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                       # noqa: E402

SEEDS, PICKS = (41, 42), [0, 2]                                # those of make_golden.fx_model_and_step / step_b2
IMAGES = ("log_img_1", "log_img_2", "log_img_2_transformed", "log_pointwise_loss", "log_normals_target", "log_normals_transformed_source")
TOL_PX, TOL_RANGE, CAP = 2e-3, 1e-4, 0.05


def ambiguous_pixels(points, sensor):
    """Boolean [H,W] from float64 candidate points [3,n]."""
    p = np.asarray(points, dtype=np.float64)
    H, W = sensor.H, sensor.W
    u = (np.arctan2(p[1], p[0]) - sensor.hfov[0]) / (sensor.hfov[1] - sensor.hfov[0]) * (W - 1)
    v = (np.arctan2(p[2], np.hypot(p[0], p[1])) - sensor.vfov[0]) / (sensor.vfov[1] - sensor.vfov[0]) * (H - 1)
    mask = np.zeros((H, W), dtype=bool)
    near = (np.abs(u - np.floor(u) - 0.5) < TOL_PX) | (np.abs(v - np.floor(v) - 0.5) < TOL_PX)
    for du in (-2 * TOL_PX, 2 * TOL_PX):
        for dv in (-2 * TOL_PX, 2 * TOL_PX):
            uu, vv = np.rint(u[near] + du).astype(np.int64), np.rint(v[near] + dv).astype(np.int64)
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            mask[vv[ok], uu[ok]] = True
    uu, vv = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
    pix, rng = vv[ok] * W + uu[ok], np.sqrt((p[:, ok] ** 2).sum(axis=0))
    order = np.lexsort((rng, pix))
    ps, rs = pix[order], rng[order]
    close = (ps[1:] == ps[:-1]) & (rs[1:] - rs[:-1] < TOL_RANGE)
    first = np.ones(len(ps), dtype=bool)
    first[1:] = ps[1:] != ps[:-1]
    second = np.zeros(len(ps), dtype=bool)
    second[1:] = first[:-1] & close                                # the runner-up of a pixel, close to its winner
    mask.reshape(-1)[ps[second]] = True
    return mask


def main():
    mg.install_stubs()
    import deploy.trainer as rtrainer
    H, W = 16, 128
    small = dict(factor_fewer_resnet_channels=8, resnet_outputs=64, unsupervised_at_start=True, inference_only=False, batch_size=2,
                 store_dataset_in_RAM=False)
    gm, gs = dict(np.load(os.path.join(HERE, "model_small.npz"))), dict(np.load(os.path.join(HERE, "step_b2.npz")))
    with tempfile.TemporaryDirectory() as tmp:
        cfg = mg.reference_config(H, W, **small)
        cfg["kitti"]["preprocessed_path"] = tmp
        cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"] = [0]
        os.makedirs(os.path.join(tmp, "00", "scans"))
        os.makedirs(os.path.join(tmp, "00", "normals"))
        scans = []
        for seed in SEEDS:
            (l1, l2), _ = mg.preprocessed_lists(seed, 16, 160, 16, 200, cfg)
            scans += [l1, l2]
        for i, (pts, nrm) in enumerate(scans):
            np.save(os.path.join(tmp, "00", "scans", f"{i:06d}.npy"), pts)
            np.save(os.path.join(tmp, "00", "normals", f"{i:06d}.npy"), nrm)
        torch.manual_seed(1234)
        trn = rtrainer.Trainer(config=copy.deepcopy(cfg))
        trn.model.load_state_dict({k[4:]: torch.from_numpy(v) for k, v in gm.items() if k.startswith("sd::")})
        dicts = [trn.dataset[i] for i in PICKS]
        raw = [{k: (mg.t2n(v).copy() if hasattr(v, "numpy") else v) for k, v in d.items()} for d in dicts]
        for j, r in enumerate(raw):                              # the very inputs of step_b2
            for k in ("scan_1", "scan_2", "normal_list_1", "normal_list_2"):
                mg.assert_same(r[k], gs[f"s{j}::{k}"], f"s{j}::{k}")
        # every argument of the projection layer, in call order: per sample scan_1, scan_2; then the transformed source of sample 0;
        # then create_images: scan_1 + normals of sample 0, the transformed pairs + normals + residuals of sample 0
        seen, layer = [], trn.img_projection
        forward = layer.forward

        def recording(input, dataset):
            seen.append(mg.t2n(input)[0, :3].astype(np.float64))
            return forward(input=input, dataset=dataset)
        layer.forward = recording
        ep = {k: 0.0 for k in ("loss_epoch", "loss_point_cloud_epoch", "loss_po2po_epoch", "loss_po2pl_epoch", "loss_pl2pl_epoch", "visible_pixels_epoch")}
        trn.optimizer.zero_grad()
        ep, T = trn.step(preprocessed_dicts=dicts, epoch_losses=ep, log_images_bool=True)
    assert len(seen) == 7, len(seen)
    mg.assert_same(mg.t2n(T), gs["T"], "T")                       # logging does not change the step
    candidates = {"log_img_1": seen[2], "log_img_2": seen[3], "log_img_2_transformed": seen[4], "log_pointwise_loss": seen[6],
                  "log_normals_target": seen[5], "log_normals_transformed_source": seen[6]}
    sensor = mg.sensor_of(cfg)
    out = dict(H=H, W=W, picks=np.asarray(PICKS), T=mg.t2n(T))
    for j, r in enumerate(raw):
        for k in ("scan_1", "scan_2", "normal_list_1", "normal_list_2"):
            out[f"s{j}::{k}"] = r[k]
    for name in IMAGES:
        img = mg.t2n(getattr(trn, name)).astype(np.float32)
        assert img.shape == (1, 4 if name == "log_img_2_transformed" else 3, H, W), (name, img.shape)
        amb = ambiguous_pixels(candidates[name], sensor)
        occ = (img[0] != 0).any(axis=0)
        share = float((amb & occ).sum()) / max(int(occ.sum()), 1)
        print(f"  {name}: occupied {int(occ.sum())}, ambiguous {int((amb & occ).sum())} ({100 * share:.2f} %)")
        assert share <= CAP, (name, share)
        out["img::" + name], out["amb::" + name] = img, amb
    path = os.path.join(HERE, "step_images_b2.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
