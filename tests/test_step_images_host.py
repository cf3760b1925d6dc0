"""The logged step on the host: ``Deployer.step(log_images_bool=True)`` fills the reference's six images through the backend's
``step_images`` (here: the CPU oracle backend extended by tests/reproject_ref.py), ``Trainer.train`` asks for them at the first and
last step of an epoch and writes the figures, and ``plot_lidar_image`` draws a PNG."""
import os

import numpy as np
import pytest
import torch

from tests import project_ref as pr
from tests import reproject_ref as rr
from tests import util
from tests.util import orc

ATTRS = ("log_img_1", "log_img_2", "log_img_2_transformed", "log_pointwise_loss", "log_normals_target", "log_normals_transformed_source")


class ImagesOracleGeometry(util.OracleStepGeometry):
    """The oracle backend plus what a logged step needs: images and normal images per sample, and ``step_images`` evaluated by the
    reference of dl_reproject's contract on brute-force correspondences."""

    def prepare(self, samples, sensor, normal_params):
        p = super().prepare(samples, sensor, normal_params)
        B, H, W = len(samples), sensor.H, sensor.W
        normals = torch.zeros((B, 2, 3, H, W))
        for b, L in enumerate(p["lists"]):
            for k, name in enumerate(("1", "2")):
                img, *_ = orc.project_to_img(torch.cat((L["scan_" + name], L["normal_list_" + name]), dim=1), p["sensor"])
                normals[b, k] = img[0, 3:6]
        p["images"], p["normals"] = p["stacked"].view(B, 2, 4, H, W), normals
        p["pr_sensor"] = pr.sensor_constants(H, W, sensor.vfov, sensor.hfov)
        return p

    def step_images(self, T, prepared, sample):
        sen = prepared["pr_sensor"]
        H, W = sen.H, sen.W
        src, srcn = prepared["images"][sample, 1].numpy(), prepared["normals"][sample, 1].numpy()
        tgt, tgtn = prepared["images"][sample, 0].numpy().reshape(4, -1), prepared["normals"][sample, 0].numpy().reshape(3, -1)
        Ts = T[sample].detach().numpy().astype(np.float32)
        s = src.reshape(4, -1)
        occ = np.nonzero(rr.occupied(s[0], s[1], s[2]))[0]
        tocc = np.nonzero(rr.occupied(tgt[0], tgt[1], tgt[2]))[0]
        q = np.stack(rr.transform(Ts, s[0, occ], s[1, occ], s[2, occ])).astype(np.float64)
        d2 = ((q[:, :, None] - tgt[:3, tocc].astype(np.float64)[:, None, :]) ** 2).sum(axis=0)
        near = tocc[np.argmin(d2, axis=1)]
        nn, match = np.full(H * W, -1, dtype=np.int32), np.zeros((6, H * W), dtype=np.float32)
        nn[occ], match[:3, occ], match[3:, occ] = near, tgt[:3, near], tgtn[:, near]
        out = rr.reproject(src[None], srcn[None], match.reshape(1, 6, H, W), nn.reshape(1, H, W), Ts[None], sen)
        return torch.from_numpy(out["moved4"]), torch.from_numpy(out["paired9"]), torch.from_numpy(out["src_pix"])


def _small_cfg(B, **over):
    gm = util.load_golden("model_small")
    opts = dict(factor_fewer_resnet_channels=int(gm["cfg::factor_fewer_resnet_channels"]), resnet_outputs=int(gm["cfg::resnet_outputs"]),
                unsupervised_at_start=True, inference_only=False, batch_size=B)
    opts.update(over)
    cfg = util.repo_config(16, 128, device="cpu", **opts)
    return cfg, {k[4:]: torch.from_numpy(v) for k, v in gm.items() if k.startswith("sd::")}


def _samples(B=2):
    g = util.load_golden("step_b2")
    return [{**{k: torch.from_numpy(g[f"s{j}::{k}"]) for k in ("scan_1", "scan_2", "normal_list_1", "normal_list_2")}, "dataset": "kitti"}
            for j in range(B)]


def _trainer(backend, **over):
    from delora_amd.deploy.trainer import Trainer
    cfg, sd = _small_cfg(2, **over)
    tr = Trainer(cfg, dataset=util.ListDataset([]), geometry_backend=backend)
    tr.raw_model.load_state_dict(sd)
    return tr


def _step(tr, log):
    tr.optimizer.zero_grad()
    return tr.step(preprocessed_dicts=[dict(s) for s in _samples()], epoch_losses=tr.new_epoch_losses(), log_images_bool=log)


# ------------------------------------------------------------------------------------------------ Deployer.step


def test_logged_step_fills_the_six_images():
    tr = _trainer(ImagesOracleGeometry())
    assert all(getattr(tr, a) == [] for a in ATTRS)                  # all start empty
    _step(tr, True)
    H, W = 16, 128
    for a in ATTRS:
        assert tuple(getattr(tr, a).shape) == (1, 4 if a == "log_img_2_transformed" else 3, H, W), a
    prepared = tr.geo.prepare(_samples(), tr.img_projection.sensor("kitti"), tr._normal_params("kitti"))
    assert torch.equal(tr.log_img_1, prepared["images"][1:2, 0, :3])      # the LAST sample's images ...
    assert torch.equal(tr.log_img_2, prepared["images"][1:2, 1, :3])
    assert not torch.equal(tr.log_img_1, prepared["images"][0:1, 0, :3])
    assert torch.equal(tr.log_normals_target, prepared["normals"][0:1, 0])  # ... everything else sample 0's
    assert not torch.equal(tr.log_normals_target, prepared["normals"][1:2, 0])
    assert tr.log_img_2_transformed.abs().sum() > 0 and tr.log_pointwise_loss.abs().sum() > 0
    # the residual image is the transformed point minus its match, and sits only where a pair won
    has = (tr.log_normals_transformed_source != 0).any(dim=1)
    assert has.any() and not (tr.log_pointwise_loss != 0).any(dim=1)[~has].any()


def test_same_step_with_and_without_logging():
    a, b = _trainer(ImagesOracleGeometry()), _trainer(ImagesOracleGeometry())
    (ep_a, T_a), (ep_b, T_b) = _step(a, False), _step(b, True)
    assert torch.equal(T_a, T_b)
    for k in ep_a:
        if torch.is_tensor(ep_a[k]):
            assert torch.equal(ep_a[k], ep_b[k]), k
    for p, q in zip(a.raw_model.parameters(), b.raw_model.parameters()):
        assert torch.equal(p, q) and torch.equal(p.grad, q.grad)


@pytest.mark.parametrize("why", ["log_images_bool False", "po2po_alone", "backend without step_images"])
def test_images_stay_untouched(why):
    over = dict(po2po_alone=True, point_to_plane_loss=False, plane_to_plane_loss=False, point_to_point_loss=True) if why == "po2po_alone" else {}
    tr = _trainer(util.OracleStepGeometry() if why.startswith("backend") else ImagesOracleGeometry(), **over)
    _step(tr, why != "log_images_bool False")
    assert all(getattr(tr, a) == [] for a in ATTRS)


# ------------------------------------------------------------------------------------------------ Trainer.train


class _Recording(ImagesOracleGeometry):
    pass


def _train(tmp_path, with_dir):
    from delora_amd.deploy.trainer import Trainer
    over = dict(checkpoint_dir=str(tmp_path), num_dataloader_workers=0, shuffle_training_data=False, checkpoint_keep_every=0)
    if with_dir:
        over["image_log_dir"] = str(tmp_path)
    cfg, sd = _small_cfg(1, **over)
    assert cfg["visualize_images"] is True                             # the shipped deployment options
    samples = _samples() + _samples() + _samples()[:1]                  # five steps per epoch
    tr = Trainer(cfg, dataset=util.ListDataset(samples), geometry_backend=_Recording())
    tr.raw_model.load_state_dict(sd)
    asked, drawn, step = [], [], Trainer.step

    def spy_step(self, preprocessed_dicts, epoch_losses=None, log_images_bool=False):
        asked.append(bool(log_images_bool))
        return step(self, preprocessed_dicts, epoch_losses, log_images_bool)

    def stub_log_image(epoch, string):
        assert tuple(tr.log_img_2_transformed.shape) == (1, 4, 16, 128)
        drawn.append((epoch, string, len(asked)))
        return ""
    tr.step = spy_step.__get__(tr)
    tr.log_image = stub_log_image
    tr.train(max_epochs=2)
    return asked, drawn


def test_trainer_logs_at_the_first_and_last_step_of_each_epoch(tmp_path):
    asked, drawn = _train(tmp_path, with_dir=True)
    assert asked == [True, False, False, False, True] * 2
    assert [(e, s) for e, s, _ in drawn] == [(0, "_start_kitti"), (0, "_image"), (1, "_image")]
    assert [n for _, _, n in drawn] == [1, 5, 10]                       # after step 0, after each epoch


def test_trainer_without_a_place_for_the_figure_never_logs(tmp_path):
    try:
        import mlflow  # noqa: F401
        pytest.skip("mlflow is importable here: image logging is on without image_log_dir")
    except ImportError:
        pass
    asked, drawn = _train(tmp_path, with_dir=False)
    assert asked == [False] * 10 and drawn == []


def test_log_image_path_and_return_value(tmp_path, monkeypatch):
    from delora_amd.utility import plotting
    tr = _trainer(ImagesOracleGeometry(), image_log_dir=str(tmp_path))
    seen = {}
    monkeypatch.setattr(plotting, "plot_lidar_image", lambda **kw: seen.update(kw))
    path = tr.log_image(epoch=3, string="_image")
    assert path == os.path.join(str(tmp_path), "test_00003_image.png") == seen["path"]
    assert len(seen["input"]) == 6 and seen["training"] is True and seen["iteration"] == (3 + 1) * tr.steps_per_epoch


# ------------------------------------------------------------------------------------------------ the figure


def test_plot_lidar_image_writes_a_png(tmp_path):
    pytest.importorskip("matplotlib")
    Image = pytest.importorskip("PIL.Image")
    from delora_amd.utility import plotting
    tr = _trainer(ImagesOracleGeometry())
    _step(tr, True)
    path = str(tmp_path / "figure.png")
    out = plotting.plot_lidar_image(input=[getattr(tr, a) for a in ATTRS], label="target", iteration=7, path=path, training=True)
    assert out == path and os.path.getsize(path) > 5000
    with Image.open(path) as im:
        assert im.format == "PNG" and im.size[0] >= 400 and im.size[1] >= 300
        px = np.asarray(im.convert("RGB"))
    assert len(np.unique(px.reshape(-1, 3), axis=0)) > 50               # six coloured rows, not a blank canvas


def test_row_colours_follow_the_reference_rules():
    matplotlib = pytest.importorskip("matplotlib")
    from delora_amd.utility import plotting
    turbo = matplotlib.colormaps["turbo"]
    img = np.zeros((3, 2, 3))
    img[:, 0, 0], img[:, 1, 2] = (3.0, 0.0, 4.0), (0.0, 1.0, 0.0)
    rgb, norm = plotting.row_colours(img, False, turbo)
    assert norm[0, 0] == 5.0 and norm[1, 2] == 1.0 and rgb.dtype == np.uint8
    assert not rgb[0, 1].any() and rgb[0, 0].any()                      # empty pixels are black
    assert tuple(rgb[0, 0]) == tuple((np.array(turbo(255)[:3]) * 255).astype(np.uint8))
    n = np.zeros((3, 1, 2))
    n[:, 0, 0] = (1.0, 0.0, -1.0)
    rgb, _ = plotting.row_colours(n, True, turbo)
    assert tuple(rgb[0, 0]) == (255, 127, 0) and not rgb[0, 1].any()     # (n + 1) / 2 as RGB; no normal: black
    t = torch.arange(24, dtype=torch.float32).view(1, 4, 2, 3)
    assert np.array_equal(plotting._as_image(t)[0], np.array([[2.0, 1.0, 0.0], [5.0, 4.0, 3.0]]))      # columns flipped
