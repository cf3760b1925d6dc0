"""The logged step on the GPU: the six images against the reference's own (tests/golden/step_images_b2.npz, written by
tests/golden/make_golden_images.py), the step's numbers with and without logging, how the images are composed, dl_reproject inside a
captured graph, ``Trainer.train`` writing the figures, and logged steps running eagerly between replayed ones under ``hip_graph: true``."""
import os

import numpy as np
import pytest
import torch

from tests import reproject_ref as rr
from tests import util

pytestmark = pytest.mark.gpu

ATTRS = ("log_img_1", "log_img_2", "log_img_2_transformed", "log_pointwise_loss", "log_normals_target", "log_normals_transformed_source")
PARITY = 1e-4                                          # the project's stated parity bound (README.md)
MASK_CAP = 0.05


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _sync():
    """A device error (not a mismatch) ends the session: nothing more is started on a GPU that has just faulted."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def _spy_on_step_images(tr):
    """Record (prepared, sample, outputs) of the backend's step_images calls."""
    calls, inner = [], tr.geo.step_images

    def spy(T, prepared, sample):
        out = inner(T, prepared, sample)
        calls.append({"prepared": prepared, "sample": sample, "T": T, "out": out})
        return out
    tr.geo.step_images = spy
    return calls


# ------------------------------------------------------------------------------------------------ (a) against the reference itself


def test_logged_images_match_the_reference():
    from delora_amd.deploy.trainer import Trainer
    dev = _dev()
    g, gm = util.load_golden("step_images_b2"), util.load_golden("model_small")
    B = len(g["picks"])
    cfg = util.repo_config(int(g["H"]), int(g["W"]), device="cuda:0", factor_fewer_resnet_channels=int(gm["cfg::factor_fewer_resnet_channels"]),
                           resnet_outputs=int(gm["cfg::resnet_outputs"]), unsupervised_at_start=True, inference_only=False, batch_size=B)
    samples = [{**{k: torch.from_numpy(g[f"s{j}::{k}"]).to(dev) for k in ("scan_1", "scan_2", "normal_list_1", "normal_list_2")}, "dataset": "kitti"}
               for j in range(B)]
    tr = Trainer(cfg, dataset=util.ListDataset(samples))
    tr.raw_model.load_state_dict({k[4:]: torch.from_numpy(v).to(dev) for k, v in gm.items() if k.startswith("sd::")})
    tr.optimizer.zero_grad()
    _, T = tr.step(preprocessed_dicts=[dict(s) for s in samples], epoch_losses=tr.new_epoch_losses(), log_images_bool=True)
    _sync()
    util.measured("step_images_b2: largest pose difference to the reference", float(np.abs(T.detach().cpu().numpy() - g["T"]).max()), bound=PARITY)
    for a in ATTRS:
        got, ref, amb = getattr(tr, a).cpu().numpy(), g["img::" + a], g["amb::" + a]
        assert got.shape == ref.shape, (a, got.shape, ref.shape)
        occ_got, occ_ref = (got[0] != 0).any(axis=0), (ref[0] != 0).any(axis=0)
        share = float((amb & occ_ref).sum()) / max(int(occ_ref.sum()), 1)
        assert share <= MASK_CAP, (a, share)                             # the generator's cap, re-asserted from the stored mask
        clean = ~amb
        wrong = int(((occ_got != occ_ref) & clean).sum())
        both = clean & occ_got & occ_ref
        worst = float(np.abs(got[0][:, both] - ref[0][:, both]).max()) if both.any() else 0.0
        print(f"[images] {a}: occupied {int(occ_ref.sum())} (reference) / {int(occ_got.sum())}, masked {100 * share:.2f} %, occupancy differs at "
              f"{wrong} clean pixels, largest difference {worst:.3g}")
        util.measured(f"step_images_b2 {a}: largest difference to the reference outside the ambiguity mask", worst)
        assert wrong == 0, f"{a}: occupancy differs at {wrong} pixels outside the ambiguity mask"
        assert worst <= PARITY, f"{a}: {worst} > {PARITY}"


# ------------------------------------------------------------------------------------------------ (b), (c) on the HIP trunk


def _hip_trunk_trainer():
    from delora_amd.data.dataset import SyntheticPairDataset
    from delora_amd.deploy.trainer import Trainer
    cfg = util.repo_config(16, 512, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=2, learning_rate=1e-5)
    ds = SyntheticPairDataset(cfg, "kitti", 2, rings=16, azimuth_steps=600)
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=ds)
    assert tr.raw_model.resnet.hip_path_takes(16, 512, batch=2)
    return tr, tr.to_device([ds[0], ds[1]])


def test_logging_changes_no_number_of_the_step_and_the_images_are_composed_as_documented():
    _dev()
    runs = {}
    for log in (False, True):
        tr, batch = _hip_trunk_trainer()
        calls = _spy_on_step_images(tr)
        tr.optimizer.zero_grad(set_to_none=True)
        ep, T = tr.step(preprocessed_dicts=[dict(b) for b in batch], epoch_losses=tr.new_epoch_losses(), log_images_bool=log)
        _sync()
        runs[log] = (tr, ep, T, calls)
    (tr0, ep0, T0, calls0), (tr1, ep1, T1, calls1) = runs[False], runs[True]
    # (b) bitwise the same step
    assert len(calls0) == 0 and all(getattr(tr0, a) == [] for a in ATTRS)
    assert torch.equal(T0, T1)
    for k in ep0:
        if torch.is_tensor(ep0[k]):
            assert torch.equal(ep0[k], ep1[k]), k
    assert torch.equal(tr0.last_step["loss_terms"], tr1.last_step["loss_terms"])
    for (n, p), q in zip(tr0.raw_model.named_parameters(), tr1.raw_model.parameters()):
        assert torch.equal(p.grad, q.grad), f"gradient of {n}"
        assert torch.equal(p, q), f"updated {n}"
    # (c) composition
    assert len(calls1) == 1 and calls1[0]["sample"] == 0
    prepared, (moved4, paired9, src_pix) = calls1[0]["prepared"], calls1[0]["out"]
    assert tuple(moved4.shape) == (1, 4, 16, 512) and tuple(paired9.shape) == (1, 9, 16, 512) and tuple(src_pix.shape) == (1, 2, 16, 512)
    assert torch.equal(tr1.log_normals_target[0], prepared["normals"][0, 0])
    assert torch.equal(tr1.log_img_1[0], prepared["images"][1, 0, :3]) and torch.equal(tr1.log_img_2[0], prepared["images"][1, 1, :3])
    assert torch.equal(tr1.log_img_2_transformed, moved4) and torch.equal(tr1.log_pointwise_loss, paired9[:, 6:9])
    assert torch.equal(tr1.log_normals_transformed_source, paired9[:, 3:6])
    same = (src_pix[0, 1] == src_pix[0, 0]) & (src_pix[0, 0] >= 0)
    assert int(same.sum()) > 100
    assert torch.equal(paired9[0, 0:3][:, same].view(torch.int32), moved4[0, 0:3][:, same].view(torch.int32))
    assert not paired9[0][:, src_pix[0, 1] < 0].any() and not moved4[0][:, src_pix[0, 0] < 0].any()
    # the residual plane is the transformed point minus the matched target point of the winner's source pixel
    w = src_pix[0, 1][same].long()
    m = prepared["match"][0, 0:3].reshape(3, -1)[:, w]
    assert torch.equal(paired9[0, 6:9][:, same], paired9[0, 0:3][:, same] - m)


# ------------------------------------------------------------------------------------------------ (d) graph replay


def test_reproject_replays_inside_a_captured_graph():
    from delora_amd import geometry
    dev = _dev()
    c = rr.case("ragged-small")
    sen = c["sen"]
    sensor = geometry.Sensor(sen.H, sen.W, sen.vfov, sen.hfov)
    src, srcn, match, nn = (torch.from_numpy(np.array(c[k])).to(dev) for k in ("src", "srcn", "match", "nn"))
    rng = np.random.default_rng(3)
    poses = [torch.from_numpy(np.stack([rr.pose(kind, rng)])).to(dev) for kind in ("small", "large", "rotation")]
    T = poses[0].clone()

    def run():
        return geometry.reproject(src, T, sensor, src_normals=srcn, match=match, nn_pix=nn)
    eager = []
    for p in poses:
        T.copy_(p)
        eager.append([t.clone() for t in run()])
    _sync()
    ref = rr.reproject(c["src"], c["srcn"], c["match"], c["nn"], poses[1].cpu().numpy(), sen)
    if all(bool(rr.pr.settled(q).all()) for q in ref["q"]):             # (a drawn pose may leave a point unsettled: then the eager call is the yardstick)
        assert np.array_equal(eager[1][0].cpu().numpy().view(np.uint32), ref["moved4"].view(np.uint32))
    T.copy_(poses[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for i in (1, 2):                                                    # two replays with a changed T
        T.copy_(poses[i])
        graph.replay()
        _sync()
        for got, exp in zip(out, eager[i]):
            assert torch.equal(got.view(torch.int32), exp.view(torch.int32)), f"replay {i}"
    assert not torch.equal(eager[1][0], eager[2][0])


# ------------------------------------------------------------------------------------------------ (e) Trainer end to end


def test_trainer_writes_the_figures(tmp_path):
    pytest.importorskip("matplotlib")
    from delora_amd.data import synthetic
    from delora_amd.data.dataset import PreprocessedPointCloudDataset
    from delora_amd.deploy.trainer import Trainer
    _dev()
    scans, _ = synthetic.make_sequence(11, 5, rings=16, azimuth_steps=160)
    synthetic.write_tree(str(tmp_path / "data"), scans, sequence=0, normals=None)
    cfg = util.repo_config(16, 128, device="cuda:0", factor_fewer_resnet_channels=8, resnet_outputs=64, batch_size=2, unsupervised_at_start=True,
                           inference_only=False, checkpoint_dir=str(tmp_path), learning_rate=1e-4, num_dataloader_workers=0,
                           shuffle_training_data=False, image_log_dir=str(tmp_path), training_run_name="t", run_name="t")
    cfg["kitti"]["preprocessed_path"] = str(tmp_path / "data")
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"] = [0]
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=PreprocessedPointCloudDataset(cfg))
    assert tr.image_logging_enabled()
    tr.train(max_epochs=2)
    _sync()
    for name in ("t_00000_start_kitti.png", "t_00000_image.png", "t_00001_image.png"):
        path = tmp_path / name
        assert path.exists() and path.stat().st_size > 5000, name
    assert sorted(p.name for p in tmp_path.glob("*.png")) == ["t_00000_image.png", "t_00000_start_kitti.png", "t_00001_image.png"]
    assert tuple(tr.log_img_2_transformed.shape) == (1, 4, 16, 128) and np.isfinite(tr.history[-1]["loss_epoch"])


def test_logged_steps_run_eagerly_between_replayed_ones(tmp_path):
    """``hip_graph: true``: every step is replayed from the captured graph except the logged ones (first and last of an epoch), which run
    eagerly, fill the images and are not counted in ``graph_steps``."""
    from delora_amd.data import synthetic
    from delora_amd.data.dataset import PreprocessedPointCloudDataset
    from delora_amd.deploy.trainer import Trainer
    _dev()
    scans, _ = synthetic.make_sequence(11, 9, rings=16, azimuth_steps=160)
    synthetic.write_tree(str(tmp_path / "data"), scans, sequence=0, normals=None)
    cfg = util.repo_config(16, 128, device="cuda:0", factor_fewer_resnet_channels=8, resnet_outputs=64, batch_size=2, unsupervised_at_start=True,
                           inference_only=False, checkpoint_dir=str(tmp_path), learning_rate=1e-4, num_dataloader_workers=0,
                           shuffle_training_data=False, image_log_dir=str(tmp_path), hip_graph=True)
    cfg["kitti"]["preprocessed_path"] = str(tmp_path / "data")
    cfg["kitti"]["data_identifiers"] = cfg["kitti"]["training_identifiers"] = [0]
    torch.manual_seed(7)
    tr = Trainer(cfg, dataset=PreprocessedPointCloudDataset(cfg))
    assert tr.graph_policy() == "on" and tr.image_logging_enabled()
    logged, drawn, step = [], [], Trainer.step

    def spy_step(self, preprocessed_dicts, epoch_losses=None, log_images_bool=False):
        assert not (log_images_bool and torch.cuda.is_current_stream_capturing())
        logged.append(bool(log_images_bool))
        return step(self, preprocessed_dicts, epoch_losses, log_images_bool)

    def stub_log_image(epoch, string):
        assert tuple(tr.log_img_2_transformed.shape) == (1, 4, 16, 128) and bool(torch.isfinite(tr.log_img_2_transformed).all())
        drawn.append((epoch, string))
        return ""
    tr.step = spy_step.__get__(tr)
    tr.log_image = stub_log_image
    tr.train(max_epochs=2)
    _sync()
    assert len(tr.dataset) == 8                                         # four steps per epoch: two logged, two replayed
    assert sum(logged) == 4 and tr._graphed.captured
    assert tr.graph_steps == 4, tr.graph_steps
    assert drawn == [(0, "_start_kitti"), (0, "_image"), (1, "_image")]
    assert all(np.isfinite(h["loss_epoch"]) and h["loss_epoch"] > 0 for h in tr.history)
