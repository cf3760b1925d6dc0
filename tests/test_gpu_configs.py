"""BASELINE.json's configurations as -m gpu parity tests: the FULL training step (HIP projection / normals / search / loss
through the C ABI, the full 11.9 M-parameter pose CNN, backward, Adam) at the configured image sizes, every sample checked
against the CPU oracle and a plain torch fp32 evaluation of the network on the host.

  config 0  64x1024, batch 1                         test_config0_64x1024_batch1_step_against_oracle
  config 1  64x2048, batch 8 (bench.py's workload)   test_config1_bench_workload_step_against_oracle,
                                                     test_config1_full_model_gradients_against_cpu_reference,
                                                     test_bench_final_loss_reproduces,
                                                     test_bench_plain_run_reports_the_headline_and_dumps_the_last_step
  config 3  128x2048, batch 8 per GPU                test_config3_128x2048_batch8_step_against_oracle
  config 4  mixed sensors in one batch               test_config4_mixed_sensor_batch_against_oracle (fp32 and autocast)

What "against the oracle" means here (reference src/deploy/deployer.py:237-375): for every checked sample the range images
the kernels produced are compared with the oracle's projection of the same raw scan (mismatching pixels counted, all of
them inside the atan2 ambiguity mask), the online normals with the oracle's, and -- on the images the GPU produced and the
poses the GPU network predicted -- the three loss terms, the pair counts and the weighted batch loss with
``oracle.step_losses`` (KD-tree correspondences, torch CPU arithmetic).  The network itself is compared with the same
module evaluated by torch on the CPU in fp32 (poses within 1e-4; parameter gradients of the whole step at B=2).
Every measured deviation is recorded (tests/util.py: measured()).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import util
from tests.util import orc

pytestmark = pytest.mark.gpu
REL = 1e-4


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _trainer(cfg, samples):
    from delora_amd.data.dataset import ListDataset
    from delora_amd.deploy.trainer import Trainer
    return Trainer(cfg, dataset=ListDataset(samples))


def _identity_state(model):
    import bench
    bench.identity_pretrained_state(model)


def _synthetic_samples(dataset, cfg, seeds, dev, rings, azimuth_steps):
    from delora_amd.data import synthetic
    vf = cfg[dataset]["vertical_field_of_view"]
    out = []
    for seed in seeds:
        s1, s2, T = synthetic.make_pair(seed, rings=rings, azimuth_steps=azimuth_steps,
                                        vfov_deg=(float(np.rad2deg(vf[0])), float(np.rad2deg(vf[1]))))
        out.append({"dataset": dataset, "scan_1": torch.from_numpy(s1).unsqueeze(0).to(dev),
                    "scan_2": torch.from_numpy(s2).unsqueeze(0).to(dev), "normal_list_1": None, "normal_list_2": None})
    return out


def _check_sample_against_oracle(trainer, sample, T_j, terms_j, counts_j, tag, check_images=True, check_normals=True):
    """One sample of a finished step: images vs the oracle's projection, normals vs the oracle's, loss terms and pair
    counts vs oracle.icp_losses on the GPU images with the GPU pose.  Returns the oracle's loss dict."""
    cfg = trainer.config
    ds = sample["dataset"]
    sensor = trainer.img_projection.sensor(ds)
    o_sensor = util.oracle_sensor(sensor.H, sensor.W, sensor.vfov, sensor.hfov)
    prepared = trainer.geo.prepare([sample], sensor, trainer._normal_params(ds))
    images, normals = prepared["images"][0].cpu(), prepared["normals"][0].cpu()
    if check_images:
        for k, name in ((0, "scan_1"), (1, "scan_2")):
            scan = sample[name][0].cpu().numpy()
            ref_img = orc.project_to_img(sample[name].cpu(), o_sensor)[0][0].numpy()
            got = images[k].numpy()
            differ = np.any(got != ref_img, axis=0)
            tainted = util.tainted_pixels(scan, o_sensor)
            assert not np.any(differ & ~tainted), f"{tag}/{name}: image differs outside the ambiguity mask"
            util.measured(f"{tag}/{name}: image pixels that differ from the oracle's projection (of {differ.size})",
                          int(differ.sum()), bound=max(2, int(np.ceil(1e-4 * differ.size))))
    if check_normals:
        a, b, eps, min_n = trainer._normal_params(ds)
        img = images[1:2]
        n_ref, has_ref, pts_ref, aux = orc.compute_normal_vectors(img.clone(), o_sensor, side=(2 * a + 1, 2 * b + 1),
                                                                  epsilon_range=eps, min_neighbors=min_n, return_aux=True)
        got = normals[1].numpy()[:, aux["v"].numpy(), aux["u"].numpy()].T
        got_has = np.any(got != 0, axis=1)
        mism = got_has != has_ref.numpy()
        util.measured(f"{tag}: has-normal mask differs from the oracle (pixels of {mism.size})", int(mism.sum()),
                      bound=max(2, int(np.ceil(1e-4 * mism.size))))
        both = got_has & has_ref.numpy()
        x, y = got[both].astype(np.float64), n_ref.numpy()[both].astype(np.float64)
        ang = np.arctan2(np.linalg.norm(np.cross(x, y), axis=1), np.sum(x * y, axis=1))
        util.measured(f"{tag}: median normal angle to the oracle [rad]", float(np.median(ang)), bound=1e-5)
    # losses on the GPU's own images / normals with the GPU's pose
    lists = {}
    for k, name in ((0, "1"), (1, "2")):
        pts, nrm, _ = util.lists_from_images(images[k], normals[k])
        lists["scan_" + name], lists["normal_list_" + name] = pts, nrm
    Tj = T_j.detach().cpu().view(1, 4, 4)
    flags = trainer_flags(cfg)
    l, aux = orc.icp_losses(orc.transform_points(Tj, lists["scan_2"]), orc.rotate_points(Tj, lists["normal_list_2"]),
                            lists["scan_1"], lists["normal_list_1"], normal_loss=cfg["normal_loss"],
                            point_to_point=bool(flags & 1), point_to_plane=bool(flags & 2), plane_to_plane=bool(flags & 4),
                            return_aux=True)
    exp = np.array([float(l["loss_po2po"]), float(l["loss_po2pl"]), float(l["loss_pl2pl"])])
    got = terms_j.detach().cpu().numpy().astype(np.float64)
    rel = np.abs(got - exp) / np.maximum(np.abs(exp), 1e-30)
    rel = np.where(exp == 0, np.abs(got), rel)
    # contract: 1e-4 (north star); the same images and pose on both sides leave only summation order: guard at 1e-5
    util.measured(f"{tag}: worst relative error of the loss terms vs the oracle", float(rel.max()), bound=0.1 * REL)
    util.measured(f"{tag}: |pair count - oracle| (oracle {aux['pairs']})", abs(int(counts_j[0]) - aux["pairs"]),
                  bound=max(1, int(1e-4 * aux["pairs"])))
    return l


def trainer_flags(cfg):
    from delora_amd import geometry
    return geometry.loss_flags(cfg)


def _cpu_model_poses(trainer, stacked):
    """The same network evaluated by torch on the CPU in fp32 (plain torch ops: the module's CPU path)."""
    from delora_amd.models.model import OdometryModel
    from delora_amd.models.model_parts import GeometryHandler
    cfg = dict(trainer.config, device=torch.device("cpu"))
    m = OdometryModel(cfg)
    m.load_state_dict({k: v.detach().cpu() for k, v in trainer.raw_model.state_dict().items()})
    t, q = m(stacked.detach().cpu())
    return m, GeometryHandler.get_transformation_matrix_quaternion(t, q, torch.device("cpu"))


def _one_step(trainer, samples):
    ep = trainer.new_epoch_losses()
    trainer.optimizer.zero_grad(set_to_none=True)
    ep, T = trainer.step(preprocessed_dicts=[dict(s) for s in samples], epoch_losses=ep)
    torch.cuda.synchronize()
    return ep, T


def _check_batch_loss(trainer, ep, per_sample_oracle, tag):
    """loss_pc with the reference's (B-j)/B weighting (deployer.py:309-312,329) from the oracle's per-sample terms."""
    cfg = trainer.config
    B = len(per_sample_oracle)
    run = {"loss_po2po": 0.0, "loss_po2pl": 0.0, "loss_pl2pl": 0.0}
    pc = 0.0
    for l in per_sample_oracle:
        run["loss_po2po"] += float(l["loss_po2po"])
        run["loss_po2pl"] += float(cfg["lambda_po2pl"]) * float(l["loss_po2pl"])
        run["loss_pl2pl"] += float(l["loss_pl2pl"])
        pc += run["loss_po2po"] + run["loss_po2pl"] + run["loss_pl2pl"]
    got = float(ep["loss_point_cloud_epoch"])
    util.measured(f"{tag}: relative error of the weighted batch loss loss_pc vs the oracle", abs(got - pc / B) / abs(pc / B), bound=1e-6)   # measured <= 7e-8


# ------------------------------------------------------------------------------------------------------------ config 0
def test_config0_64x1024_batch1_step_against_oracle():
    """BASELINE config 0's workload (64x1024, batch 1) through the GPU path with the full-size network."""
    dev = _dev()
    cfg = util.repo_config(64, 1024, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=1)
    torch.manual_seed(7)
    samples = _synthetic_samples("kitti", cfg, [1000], dev, rings=64, azimuth_steps=2250)
    trainer = _trainer(cfg, samples)
    _identity_state(trainer.raw_model)
    sensor = trainer.img_projection.sensor("kitti")
    stacked = trainer.geo.prepare(samples, sensor, trainer._normal_params("kitti"))["stacked"]
    _, T_cpu = _cpu_model_poses(trainer, stacked)
    ep, T = _one_step(trainer, samples)
    util.measured("config0: max |T_gpu - T_cpu(torch fp32)|", float((T.detach().cpu() - T_cpu.detach()).abs().max()), bound=1e-6)
    last = trainer.last_step
    l = _check_sample_against_oracle(trainer, samples[0], T[0], last["loss_terms"][0], last["pair_counts"][0], "config0 64x1024")
    _check_batch_loss(trainer, ep, [l], "config0 64x1024")
    assert all(torch.isfinite(p.grad).all() for p in trainer.raw_model.parameters())


# ------------------------------------------------------------------------------------------------------------ config 1
def _bench_setup(batch, dev, rotate=1):
    """bench.py's own workload construction (its seeds, batches, configuration and model state)."""
    import bench
    args = bench.parse(["--batch", str(batch), "--rotate", str(rotate)])
    cfg = bench.build_config(args, dev)
    torch.manual_seed(1234)
    host = bench.derived_batches(bench.make_batch(args, 0), rotate, 0, shuffled=args.point_order == "shuffled")
    batches = [bench.to_device(b, dev) for b in host]
    trainer = _trainer(cfg, [d for b in host for d in b])
    bench.identity_pretrained_state(trainer.raw_model)
    return args, cfg, (batches[0] if rotate == 1 else batches), trainer


def test_config1_bench_workload_step_against_oracle():
    """bench.py's exact workload (64x2048, batch 8, full network, its seeds and model state): first training step, every
    sample's loss terms / pair counts and the weighted batch loss against the oracle; images and normals of two samples."""
    dev = _dev()
    args, cfg, samples, trainer = _bench_setup(8, dev)
    ep, T = _one_step(trainer, samples)
    last = trainer.last_step
    per = []
    for j, s in enumerate(samples):
        per.append(_check_sample_against_oracle(trainer, s, T[j], last["loss_terms"][j], last["pair_counts"][j],
                                                f"config1 64x2048 sample {j}", check_images=j in (0, 5), check_normals=j == 3))
    _check_batch_loss(trainer, ep, per, "config1 64x2048 B=8")


def test_config1_full_model_gradients_against_cpu_reference():
    """64x2048, batch 2 of the bench batch, full 11.9 M-parameter network: poses and EVERY parameter gradient of the whole
    step (projection -> CNN -> T -> correspondences -> loss -> backward) against the same step evaluated on the host --
    torch fp32 network + oracle losses (KD-tree) with autograd through T."""
    dev = _dev()
    args, cfg, samples, trainer = _bench_setup(2, dev)
    # poses of the RANDOMLY INITIALISED full network (arbitrary rotations, every layer contributes): GPU vs torch CPU fp32
    from delora_amd.models.model_parts import GeometryHandler
    sensor = trainer.img_projection.sensor("kitti")
    stacked = trainer.geo.prepare(samples, sensor, trainer._normal_params("kitti"))["stacked"]
    torch.manual_seed(99)
    with torch.no_grad():
        for lin in (trainer.raw_model.fully_connected_rotation[-1], trainer.raw_model.fully_connected_translation[-1]):
            torch.nn.init.normal_(lin.weight, 0.0, 0.1)
            torch.nn.init.normal_(lin.bias, 0.0, 0.5)
        t, q = trainer._run_model(stacked)
        T_rand = GeometryHandler.get_transformation_matrix_quaternion(t, q, dev)
        _, T_rand_cpu = _cpu_model_poses(trainer, stacked)
    scale = float(T_rand_cpu.abs().max())
    util.measured("config1 B=2, random-init network: max |T_gpu - T_cpu| / max|T|", float((T_rand.cpu() - T_rand_cpu).abs().max()) / scale, bound=1e-5)    # measured 2.7e-7
    assert float((T_rand_cpu[:, :3, :3] - torch.eye(3)).abs().max()) > 0.05       # not the identity
    import bench
    bench.identity_pretrained_state(trainer.raw_model)
    # a state in which the pose depends on the weights of BOTH heads (the bench state zeroes the last layers)
    with torch.no_grad():
        trainer.raw_model.fully_connected_rotation[-1].weight.normal_(0, 1e-3)
        trainer.raw_model.fully_connected_translation[-1].weight.normal_(0, 1e-3)
    prepared = trainer.geo.prepare(samples, sensor, trainer._normal_params("kitti"))
    m_cpu, T_cpu = _cpu_model_poses(trainer, prepared["stacked"])
    lists = []
    for b in range(2):
        entry = {}
        for k, name in ((0, "1"), (1, "2")):
            pts, nrm, _ = util.lists_from_images(prepared["images"][b, k].cpu(), prepared["normals"][b, k].cpu())
            entry["scan_" + name], entry["normal_list_" + name] = pts, nrm
        lists.append(entry)
    out, _ = orc.step_losses(lists, T_cpu, lambda_po2pl=cfg["lambda_po2pl"], normal_loss=cfg["normal_loss"])
    out["loss_pc"].sum().backward()
    ep, T = _one_step(trainer, samples)
    util.measured("config1 B=2: max |T_gpu - T_cpu|", float((T.detach().cpu() - T_cpu.detach()).abs().max()), bound=1e-6)    # measured 2.6e-9
    util.measured("config1 B=2: relative error of loss_pc vs the host step",
                  abs(float(ep["loss_point_cloud_epoch"]) - float(out["loss_pc"])) / abs(float(out["loss_pc"])), bound=1e-6)    # measured 1e-7
    worst, worst_name = 0.0, ""
    cpu_params = dict(m_cpu.named_parameters())
    for k, p in trainer.raw_model.named_parameters():
        g_gpu, g_cpu = p.grad.detach().cpu().double(), cpu_params[k].grad.double()
        err = float((g_gpu - g_cpu).norm() / g_cpu.norm().clamp_min(1e-30))
        if err > worst:
            worst, worst_name = err, k
    # ||g_gpu - g_cpu|| / ||g_cpu|| per parameter tensor: fp32 convolutions of two different libraries (MIOpen / oneDNN)
    util.measured(f"config1 B=2: worst relative gradient error over the 30 parameter tensors ({worst_name})", worst, bound=2.5e-5)      # measured 2.5e-6


def test_config1_step_at_a_non_identity_network_pose_against_oracle():
    """The bench workload (64x2048, full network) with heads that predict a MODERATE motion (a few degrees, ~0.6 m) instead of the
    identity the other full-size tests evaluate at: the correspondence search then runs its uncertified passes (window lists,
    tile walk, seed scan) on most queries, and the loss / pair counts / weighted batch loss must still equal the oracle's
    KD-tree evaluation at the pose the GPU network produced."""
    dev = _dev()
    args, cfg, samples, trainer = _bench_setup(4, dev)
    with torch.no_grad():
        trainer.raw_model.fully_connected_rotation[-1].bias.copy_(torch.tensor([0.03, -0.02, 0.05, 1.0]))
        trainer.raw_model.fully_connected_translation[-1].bias.copy_(torch.tensor([0.5, -0.3, 0.1]))
    ep, T = _one_step(trainer, samples)
    ang = torch.rad2deg(torch.acos(((T[:, 0, 0] + T[:, 1, 1] + T[:, 2, 2] - 1) / 2).clamp(-1, 1)))
    assert float(ang.min()) > 3.0 and float(T[:, :3, 3].norm(dim=1).min()) > 0.5, "the step must not run at the identity"
    last = trainer.last_step
    per = []
    for j, s in enumerate(samples):
        per.append(_check_sample_against_oracle(trainer, s, T[j], last["loss_terms"][j], last["pair_counts"][j],
                                                f"config1 64x2048 non-identity pose sample {j}", check_images=False, check_normals=False))
    _check_batch_loss(trainer, ep, per, "config1 64x2048 B=4 non-identity pose")


def test_bench_final_loss_reproduces():
    """`python bench.py` (3 steps, no warm-up) in a subprocess reports the loss this process computes for the same three
    steps of the same workload; the JSON line carries the contract's fields."""
    dev = _dev()
    args, cfg, batches, trainer = _bench_setup(8, dev, rotate=8)
    for b in batches:                      # bench.py primes the allocator with one step per distinct batch before warm-up and timing
        _one_step(trainer, b)
    for i in range(3):
        ep, _ = _one_step(trainer, batches[i])
    mine = float(ep["loss_epoch"])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--steps", "3", "--warmup", "0", "--no-cpu-baseline",
                        "--kernel-reps", "2", "--feed-steps", "0", "--long-steps", "0", "--no-live-pmc", "--variant-steps", "2",
                        "--autocast-steps", "0", "--shipped-steps", "8", "--ddp-steps", "2"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    j = json.loads(line)
    util.measured("bench.py final_loss vs the same 3 steps in-process (relative)", abs(j["final_loss"] - mine) / abs(mine), bound=REL)
    assert j["n_gpus"] == 1 and j["steps"] == 3 and j["dtype"] == "f32" and j["config"]["global_batch"] == 8
    assert j["roofline"]["bound"] and 0 < j["roofline"]["frac"] < 1.5
    # the reference's shipped image size runs on the HIP stem + trunk too (overhanging tiles), and a run from scratch has a number
    assert j["shipped_image"]["image"] == "64x720" and "hip trunk" in j["shipped_image"]["cnn_impl"] and j["shipped_image"]["value"] > 0
    assert "random" in j["untrained_network"]["network_state"] and j["untrained_network"]["value"] > 0 and np.isfinite(j["untrained_network"]["final_loss"])
    # the reference's default operating point (unmodified YAML: 64x720, batch 1, stored lists): eager, replayed, and the product loop,
    # whose `hip_graph: auto` must have found the batch-1 step host-bound and replayed it -- from the packed feed and from the DataLoader
    sc = j["shipped_config"]
    assert "error" not in sc, sc
    b1 = sc["batch_1"]
    for leg in ("eager_resident", "graph_resident", "product_loop_packed_feed_2_workers", "product_loop_yaml_default_0_workers"):
        assert b1[leg]["ms_per_step"] > 0 and b1[leg]["value"] > 0, leg
    assert b1["graph_resident"]["eager_fallback_steps"] == 0
    for leg in ("product_loop_packed_feed_2_workers", "product_loop_yaml_default_0_workers"):
        auto = b1[leg]["hip_graph_auto"]
        assert auto["decision"].split(" ")[0] in ("graph", "eager") and auto["stream_ms"] > 0, (leg, b1[leg])
        assert b1[leg]["graph_replayed_steps"] == (b1[leg]["steps"] if auto["decision"] == "graph" else 0), (leg, b1[leg])
        assert b1[leg]["feed"] == "PackedFeed"          # 0 workers included: the consumer decodes in-process into page-locked slots
        util.measured(f"default operating point (64x720, batch 1), {leg}: step time / eager step on resident batches",
                      b1[leg]["ms_per_step"] / b1["eager_resident"]["ms_per_step"], bound=1.6)
    assert sc["batch_8"]["eager_resident"]["value"] > 0
    util.measured("default operating point (64x720, batch 1): graph replay / eager step time", b1["graph_resident"]["ms_per_step"] / b1["eager_resident"]["ms_per_step"], bound=1.1)
    # one rank under DistributedDataParallel over a one-rank RCCL group, fp32 and bf16
    dd = j["ddp_rank"]
    assert "error" not in dd, dd
    for prec in ("fp32", "bf16"):
        assert dd[prec]["ddp"]["ms_per_step"] > 0 and np.isfinite(dd[prec]["ddp"]["final_loss"]) and isinstance(dd[prec]["ddp_host_bound"], bool)


def test_bench_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    """A plain `python bench.py` (3 steps, no warm-up) prints the headline line only, and `--dump-outputs` holds what the last of its
    timed steps computed: the poses, the loss sums, the fixed sample of the updated weights and of their gradients -- the arrays this
    process computes for the same three steps of the same workload."""
    import bench
    dev = _dev()
    args, cfg, batches, trainer = _bench_setup(8, dev, rotate=8)
    for b in batches:                      # bench.py primes the allocator with one step per distinct batch before warm-up and timing
        _one_step(trainer, b)
    for i in range(3):
        ep, T = _one_step(trainer, batches[i])
    mine = bench.step_outputs(trainer, ep, T)
    del trainer
    torch.cuda.empty_cache()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["steps"] == 3 and j["warmup"] == 0 and j["unit"] == "scan-pairs/s" and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] > 0 and j["value"] == pytest.approx(8 * 1e3 / j["ms_per_step"], rel=1e-3)
    assert not {"roofline", "roofline_loss", "kernels", "long_run", "feed", "autocast", "cpu_baseline", "shipped_config", "ddp_rank"} & set(j)
    files = sorted(p.name for p in out.iterdir())
    assert files == sorted(k + ".npy" for k in mine)
    got = {k: np.load(out / (k + ".npy")) for k in mine}
    assert all(v.dtype in (np.float32, np.float64) for v in got.values()) and sum(v.nbytes for v in got.values()) <= bench.DUMP_MAX_BYTES
    assert got["transformations"].shape == (8, 4, 4) and got["weights_sample"].shape == (bench.DUMP_SAMPLE,)
    assert abs(float(got["losses_loss_epoch"][0]) - j["final_loss"]) <= 1e-6 * abs(j["final_loss"])
    util.measured("bench.py --dump-outputs poses vs the same 3 steps in-process (relative to the largest element)",
                  float(np.abs(got["transformations"] - mine["transformations"]).max() / np.abs(mine["transformations"]).max()), bound=REL)
    for k in (k for k in mine if k.startswith("losses_")):
        util.measured(f"bench.py --dump-outputs {k} vs in-process (relative)",
                      float(np.abs(got[k] - mine[k]).max() / max(float(np.abs(mine[k]).max()), 1e-12)), bound=REL)
    for k, bound in (("weights_sample", 1e-3), ("gradients_sample", 1e-2)):
        util.measured(f"bench.py --dump-outputs {k} vs in-process (relative norm of the difference)",
                      float(np.linalg.norm(got[k] - mine[k]) / np.linalg.norm(mine[k])), bound=bound)


def test_bench_measures_the_convolution_traffic_itself():
    """`bench.py`'s roofline.traffic is measured by the run: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE child passes over one launch per
    convolution kernel and layer shape.  Every Winograd row must come back, at or above the bytes the launch cannot avoid
    (input + output; the counters include L2 misses served by the Infinity Cache) and below 8x of them."""
    _dev()
    import shutil
    if not (shutil.which("rocprofv3") or os.path.exists("/opt/rocm/bin/rocprofv3")):
        pytest.skip("no rocprofv3 on this box")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    rows = bench.live_pmc_traffic("float32")
    assert rows, "the rocprofv3 child passes returned nothing"
    wino = {k: v for k, v in rows.items() if k.startswith("k_wino_conv ")}
    assert len(wino) == 4, sorted(rows)
    for name, b in wino.items():
        n, hw, c, k = name.split(" ")[2:6]
        h, w = (int(v) for v in hw.split("x"))
        compulsory = int(n[1:]) * h * w * (int(c[1:]) + int(k[1:])) * 4
        util.measured(f"live PMC traffic / (input + output bytes): {name}", b / compulsory, bound=8.0)
        assert b >= 0.9 * compulsory, (name, b, compulsory)


# ------------------------------------------------------------------------------------------------------------ config 3
def test_config3_128x2048_batch8_step_against_oracle():
    """BASELINE config 3's per-GPU share: 128-ring 128x2048 scans, batch 8, full network; one sample against the oracle."""
    dev = _dev()
    cfg = util.repo_config(128, 2048, dataset="ouster128", device="cuda:0", unsupervised_at_start=True, inference_only=False,
                           batch_size=8)
    torch.manual_seed(3)
    samples = _synthetic_samples("ouster128", cfg, [3000 + j for j in range(8)], dev, rings=128, azimuth_steps=2048)
    trainer = _trainer(cfg, samples)
    _identity_state(trainer.raw_model)
    ep, T = _one_step(trainer, samples)
    last = trainer.last_step
    assert torch.isfinite(last["loss_terms"]).all() and (last["pair_counts"][:, 0] > 100000).all()
    _check_sample_against_oracle(trainer, samples[6], T[6], last["loss_terms"][6], last["pair_counts"][6], "config3 128x2048 sample 6")
    assert all(torch.isfinite(p.grad).all() for p in trainer.raw_model.parameters())


# ------------------------------------------------------------------------------------------------------------ config 4
@pytest.mark.parametrize("amp", ["", "float16"])
def test_config4_mixed_sensor_batch_against_oracle(amp):
    """BASELINE config 4: a batch mixing kitti (64 rings, vFoV -24.5..2), darpa (64 rings, +-22.5) and the 128-ring sensor,
    each with its own image size; fp32 and the fp16-autocast CNN.  Every sample against the ORACLE (images, loss terms,
    pair counts); the batch loss against the oracle's weighting over the mixed batch."""
    dev = _dev()
    from delora_amd import config as cfgmod
    cfg = util.repo_config(64, 1024, dataset="kitti", device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=4)
    cfg["datasets"] = ["darpa", "ouster128"]
    cfgmod.degrees_to_radians(cfg)                       # repo_config converted the kitti block and the horizontal field of view
    cfg["horizontal_field_of_view"] = util.repo_config(64, 1024)["horizontal_field_of_view"]
    cfg["datasets"] = ["kitti", "darpa", "ouster128"]
    assert abs(cfg["darpa"]["vertical_field_of_view"][1] - np.deg2rad(22.5)) < 1e-9 and abs(cfg["horizontal_field_of_view"][1] - np.deg2rad(179.9)) < 1e-9
    cfg["darpa"]["vertical_cells"], cfg["darpa"]["horizontal_cells"] = 64, 512
    cfg["ouster128"]["vertical_cells"], cfg["ouster128"]["horizontal_cells"] = 128, 1024
    if amp:
        cfg["amp_dtype"] = amp
    torch.manual_seed(11)
    samples = (_synthetic_samples("kitti", cfg, [4000], dev, 64, 1100) + _synthetic_samples("ouster128", cfg, [4001], dev, 128, 1024)
               + _synthetic_samples("darpa", cfg, [4002], dev, 64, 512) + _synthetic_samples("kitti", cfg, [4003], dev, 64, 1100))
    trainer = _trainer(cfg, samples)
    _identity_state(trainer.raw_model)
    ep, T = _one_step(trainer, samples)
    last = trainer.last_step
    per = []
    for j, s in enumerate(samples):
        per.append(_check_sample_against_oracle(trainer, s, T[j], last["loss_terms"][j], last["pair_counts"][j],
                                                f"config4{'/' + amp if amp else ''} sample {j} ({s['dataset']})", check_normals=j == 1))
    _check_batch_loss(trainer, ep, per, f"config4{'/' + amp if amp else ''} mixed batch")
    assert all(torch.isfinite(p.grad).all() for p in trainer.raw_model.parameters())


# ------------------------------------------------------------------------------------------- config 2 (multi-GPU readiness)
def test_bench_eight_ranks_dry_run_on_one_gpu():
    """`python bench.py --gpus 8` end to end on a 1-GPU box: the script re-launches itself as EIGHT ranks (torch.distributed.run), all
    sharing the GPU over gloo (test hooks), at a tiny size (64x256 images, one pair per rank).  One JSON line, n_gpus = rccl_ranks = 8,
    a global batch of 8, eight per-rank step times, a finite loss -- the launch / barrier / max-over-ranks / gather path of BASELINE
    configs[2] with its real world size (no scaling number can come from one GPU)."""
    _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DELORA_BENCH_SHARE_GPU="1", DELORA_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "8", "--steps", "3", "--warmup", "1", "--batch", "1", "--width", "256",
           "--rotate", "2", "--kernel-reps", "2", "--no-live-pmc", "--no-profile"]
    # (a bounded wait: eight processes time-slicing one GPU are slow, not stuck -- but a stuck run must cost minutes, not the session)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=root, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=420)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, 9)
        out, err = proc.communicate()
        pytest.fail("bench.py --gpus 8 on one shared GPU did not finish in 420 s:\n" + err[-3000:])
    r = subprocess.CompletedProcess(cmd, proc.returncode, out, err)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly one JSON line"
    j = json.loads(lines[0])
    assert j["n_gpus"] == 8 and j["rccl_ranks"] == 8 and j["config"]["global_batch"] == 8 and j["config"]["parallelism"] == "dp8"
    rk = j["rank_ms_per_step"]
    assert len(rk["per_rank"]) == 8 and 0 < rk["min"] <= rk["max"] <= j["ms_per_step"] * 1.001 + 1e-3
    assert j["scaling"] == "weak" and j["steps"] == 3 and np.isfinite(j["final_loss"]) and j["value"] > 0
    assert "cpu_baseline" not in j and "shipped_config" not in j and "hip trunk" in j["config"]["cnn_impl"]
    # round 6: what the first real scaling run needs to explain itself -- per rank, the timeline of the gradient all-reduce
    tl = j["ddp_timeline"]
    assert tl and len(tl["per_rank"]) == 8 and sorted(r["rank"] for r in tl["per_rank"]) == list(range(8))
    for r in tl["per_rank"]:
        assert r["steps"] >= 3 and r["exposed_allreduce_ms"] is not None and r["exposed_allreduce_ms"] >= 0.0 and r["feed_wait_ms_per_step"] == 0.0
        assert 4.6e7 < r["bytes_per_step"] < 4.9e7 and len(r["buckets"]) >= 2            # the 47.5 MB of fp32 gradients in 5 MB buckets
        assert all(b["ready_ms"] is not None and b["done_ms"] is not None and b["done_ms"] >= b["ready_ms"] - 1e-3 for b in r["buckets"])
        assert r["backward_end_ms"] > 0


def test_rccl_two_gpus_bench_and_timeline():
    """BASELINE configs[2] on real links, as far as a test can go: `bench.py --gpus 2` over RCCL with one rank per GPU.  Skipped unless the
    box shows at least two GPUs (the development boxes have one; the driver's 8-GPU node runs it): n_gpus = rccl_ranks = 2, a finite loss,
    both ranks' step times, and the all-reduce timeline with its exposed part."""
    _dev()
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs (RCCL over xGMI); a 1-GPU box covers the launch path over gloo in the tests next to this one")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DELORA_BENCH_SHARE_GPU", "DELORA_BENCH_BACKEND"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "10", "--warmup", "3", "--kernel-reps", "2", "--no-live-pmc", "--no-profile"]
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=root, start_new_session=True)
    try:
        out, err = proc.communicate(timeout=900)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, 9)
        out, err = proc.communicate()
        pytest.fail("bench.py --gpus 2 over RCCL did not finish in 900 s:\n" + err[-3000:])
    assert proc.returncode == 0, (out[-1500:], err[-3000:])
    lines = [x for x in out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["collective_backend"] == "nccl" and np.isfinite(j["final_loss"])
    tl = j["ddp_timeline"]
    assert len(tl["per_rank"]) == 2 and all(r["exposed_allreduce_ms"] is not None for r in tl["per_rank"])
    util.measured("bench.py --gpus 2 over RCCL: scan-pairs/s (two ranks)", float(j["value"]))
    util.measured("bench.py --gpus 2 over RCCL: exposed all-reduce per step (ms, worst rank)", float(tl["exposed_allreduce_ms"]["max"]))


@pytest.mark.parametrize("launcher", ["torchrun", "plain"])
def test_bench_two_ranks_on_one_gpu_through_torchrun(launcher):
    """BASELINE config 2's launch path on a 1-GPU box: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`
    exactly as the driver starts it ("torchrun"), and the plain `python bench.py --gpus 2` the driver uses for N=1 ("plain": the
    script must re-launch itself as 2 ranks -- it used to run ONE rank silently), both ranks sharing the GPU over gloo (test hooks
    DELORA_BENCH_SHARE_GPU / DELORA_BENCH_BACKEND).  Checks the JSON contract of a multi-rank run: n_gpus, global batch, ranks
    seen by the process group, per-rank step times, finite loss, weak scaling label.  (RCCL itself is exercised by
    test_rccl_backend_initialises_and_reduces_on_one_rank; no scaling number can come from one GPU.)"""
    _dev()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DELORA_BENCH_SHARE_GPU="1", DELORA_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    bench_args = [os.path.join(root, "bench.py"), "--full", "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2",
                  "--rotate", "2", "--kernel-reps", "2", "--no-live-pmc"]
    if launcher == "torchrun":
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", "29533"] + bench_args
    else:
        cmd = [sys.executable] + bench_args
        # without the hook the same command must refuse: 2 ranks, 1 visible GPU
        if torch.cuda.device_count() < 2:
            refused = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root,
                                     env={k: v for k, v in env.items() if k != "DELORA_BENCH_SHARE_GPU"})
            assert refused.returncode != 0 and "GPU(s) visible" in refused.stderr and not [x for x in refused.stdout.splitlines() if x.startswith("{")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, "rank 0 prints exactly one JSON line"
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["rccl_ranks"] == 2 and j["config"]["global_batch"] == 4 and j["config"]["parallelism"] == "dp2"
    rk = j["rank_ms_per_step"]
    assert len(rk["per_rank"]) == 2 and 0 < rk["min"] <= rk["max"] <= j["ms_per_step"] * 1.001 + 1e-3
    assert j["scaling"] == "weak" and j["steps"] == 3 and np.isfinite(j["final_loss"]) and j["value"] > 0
    assert "cpu_baseline" not in j and "feed" not in j          # single-GPU legs only
    # the full-width image: the ranks run the HIP trunk, and rank 0 must not start collective steps of its own after the timed region
    assert "hip trunk" in j["config"]["cnn_impl"] and j["roofline"]["bound"] == "mfma" and "second pass" in j["roofline"]["measured_in"]


def test_ddp_wrapping_uses_small_buckets_and_bucket_views():
    """The gradient all-reduce is the path's only exchange: DDP must overlap it with backward in buckets that
    leave only the small early layers for the last, exposed all-reduce."""
    dev = _dev()
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    dist.init_process_group(backend="gloo", rank=0, world_size=1)
    try:
        from delora_amd.deploy.trainer import Trainer
        gm = util.load_golden("model_small")
        cfg = util.repo_config(16, 128, device="cuda:0", factor_fewer_resnet_channels=int(gm["cfg::factor_fewer_resnet_channels"]),
                               resnet_outputs=int(gm["cfg::resnet_outputs"]), unsupervised_at_start=True, inference_only=False, batch_size=1)
        tr = Trainer(cfg, dataset=util.ListDataset([]))
        assert tr.world_size == 1 and not isinstance(tr.model, torch.nn.parallel.DistributedDataParallel)
        tr.world_size = 2                                    # wrap as a 2-rank job would
        wrapped = Trainer._wrap_ddp(tr, tr.raw_model)
        assert isinstance(wrapped, torch.nn.parallel.DistributedDataParallel)
        assert wrapped.bucket_bytes_cap == 5 * 1024 * 1024 and wrapped.gradient_as_bucket_view
    finally:
        dist.destroy_process_group()


def test_full_size_step_replays_as_a_hip_graph():
    """The whole bench step (64x2048, B=8, HIP stem + trunk) captured once and replayed over ROTATING RAGGED batches (different scan
    lengths and contents per step, packed into the graph's static buffers): the replays must run (a memset node in the captured
    graph used to fault on the second replay: the library initialises its buffers with a kernel instead) and follow the eager
    trajectory of the same batch sequence."""
    from delora_amd.deploy.graph_step import GraphedStep
    dev = _dev()
    args, cfg, batches, tr_e = _bench_setup(8, dev, rotate=4)
    lengths = {d[k].shape[2] for b in batches for d in b for k in ("scan_1", "scan_2")}
    assert len(lengths) > 8, "the rotating batches must be ragged"
    seq = [0, 1, 2, 3, 0, 1, 2]                          # (GraphedStep's warm-up steps on batch 0 leave no trace: weights and Adam state are restored)
    eager = []
    for i in seq:
        ep, _ = _one_step(tr_e, batches[i])
        eager.append(float(ep["loss_epoch"]))
    args, cfg, batches, tr_g = _bench_setup(8, dev, rotate=4)
    gs = GraphedStep(tr_g, batches[0], warmup=3)
    assert gs.captured
    got = []
    for i in seq:
        ep, _ = gs(batches[i])
        torch.cuda.synchronize()
        got.append(float(ep["loss_epoch"]))
    assert gs.fallback_steps == 0
    print("eager", eager, "graph", got)
    util.measured("full-size graph replay over rotating ragged batches: worst relative deviation of the loss from the eager trajectory",
                  float(np.max(np.abs(np.array(got) - np.array(eager)) / np.abs(np.array(eager)))), bound=1e-3)
    # a batch that does not fit the static buffers runs eagerly instead of failing
    long_batch = [dict(d) for d in batches[1]]
    long_batch[0]["scan_1"] = torch.cat([long_batch[0]["scan_1"]] * 2, dim=2)
    ep, _ = gs(long_batch)
    assert gs.fallback_steps == 1 and np.isfinite(float(ep["loss_epoch"]))


def test_ddp_all_reduce_overlaps_the_trunk_backward():
    """The gradient all-reduce is the path's only exchange.  Under DDP the trunk is cut into three autograd Functions
    ([layer1+2] [layer3] [layer4]; ``Trainer._wrap_ddp``), so DistributedDataParallel receives layer4's and layer3's weight
    gradients (89 % of the 47.5 MB) when those segments' backward has run: their buckets must be handed to the communication hook
    BEFORE the backward of layer1 + layer2 has finished, and what is still outstanding when the last segment returns must be less
    than one 10 MB bucket.  (One Function per block would overlap more but costs the host 1.7 ms per step -- the eager step is
    only just GPU-bound; measured with bench.py --trunk-segments.)"""
    dev = _dev()
    import torch.distributed as dist
    from delora_amd.models import ring_conv
    if dist.is_initialized():
        pytest.skip("a process group is already initialised in this process")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29536")
    dist.init_process_group(backend="gloo", rank=0, world_size=1)
    try:
        from delora_amd.deploy.trainer import Trainer
        cfg = util.repo_config(16, 1024, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=2)
        tr = Trainer(cfg, dataset=util.ListDataset([]))
        tr.world_size = 2
        model = Trainer._wrap_ddp(tr, tr.raw_model)
        trace = []

        def hook(state, bucket):
            trace.append(("bucket", bucket.index(), bucket.buffer().numel() * 4))
            fut = torch.futures.Future()
            fut.set_result(bucket.buffer())
            return fut
        model.register_comm_hook(None, hook)
        ring_conv.BACKWARD_TRACE = trace
        x = torch.randn((2, 8, 16, 1024), device=dev)
        for _ in range(2):                                   # DDP rebuilds its buckets in gradient-ready order after the first pass
            del trace[:]
            model.zero_grad(set_to_none=True)
            t, q = model(x)
            (t.square().sum() + q.sum()).backward()
            torch.cuda.synchronize()
    finally:
        ring_conv.BACKWARD_TRACE = None
        dist.destroy_process_group()
    segs = [i for i, e in enumerate(trace) if e[0] == "segment"]
    assert len(segs) == 3 and [trace[i][3] for i in segs] == [2, 2, 4], trace          # layer4, layer3, layer1+2 (backward order)
    total = sum(e[2] for e in trace if e[0] == "bucket")
    after_trunk = sum(e[2] for e in trace[segs[-1]:] if e[0] == "bucket")
    # a bucket is launched when the LAST of its parameters is ready, i.e. when the segment holding it has returned
    early = sum(e[2] for e in trace[:segs[-1]] if e[0] == "bucket")               # before the backward of layer1 + layer2 has finished
    util.measured("DDP: gradient bytes handed to the all-reduce only after the last trunk segment's backward", after_trunk, bound=10 * 1024 * 1024)
    util.measured("DDP: share of the gradient bytes already in flight while layer1 + layer2 still run their backward", early / total)
    assert abs(total - 4 * sum(p.numel() for p in tr.raw_model.parameters())) < 1024
    assert early / total > 0.6


# ------------------------------------------------------- the reference's own Trainer.step at full size (full-size digests)
@pytest.mark.parametrize("name", ["step_full_64_b1", "step_full_64_b2", "step_full_64_b8", "step_full_128_b1", "step_b8_small"])
def test_step_matches_the_references_own_trainer_step(name):
    """tests/golden/step_full_*.npz hold what the REFERENCE's `Trainer.step` (src/deploy/deployer.py:237-375) produced at 64x2048
    (B=1, B=2 and B=8 = BASELINE configs[1], the bench's own batch) and 128x2048 (B=1) with the FULL 11.9 M-parameter network, and at B=8 on the small network: poses, the five loss
    scalars, the 30 per-parameter gradient norms, the Adam update, pair counts.  Inputs and weights are regenerated here from seeds
    by the portable generators and sha-checked against the fixture, so the HIP path (stored normal lists through the projection,
    HIP stem + trunk, search, loss, backward, Adam) is tied to the reference DIRECTLY at full width, not through the narrow module."""
    from delora_amd.deploy.trainer import Trainer
    dev = _dev()
    g = util.load_golden(name)
    H, W = int(g["H"]), int(g["W"])
    samples = util.portable_step_inputs(g)
    B = len(samples)
    if name == "step_b8_small":
        gm = util.load_golden("model_small")
        cfg = util.repo_config(H, W, device="cuda:0", factor_fewer_resnet_channels=int(gm["cfg::factor_fewer_resnet_channels"]),
                               resnet_outputs=int(gm["cfg::resnet_outputs"]), unsupervised_at_start=True, inference_only=False, batch_size=B)
        state = {k[4:]: torch.from_numpy(v) for k, v in gm.items() if k.startswith("sd::")}
    else:
        cfg = util.repo_config(H, W, device="cuda:0", unsupervised_at_start=True, inference_only=False, batch_size=B)
        cfg["kitti"]["vertical_field_of_view"] = [float(v) for v in g["vfov"]]
        state = util.portable_full_state(g)
    samples = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in s.items()} for s in samples]
    trainer = Trainer(cfg, dataset=util.ListDataset(samples))
    trainer.raw_model.load_state_dict({k: v.to(dev) for k, v in state.items()})
    if name != "step_b8_small":
        assert trainer.raw_model.resnet.hip_path_takes(H, W, batch=B), "the full-width network must run on the HIP stem + trunk"
    before = {k: v.detach().clone() for k, v in trainer.raw_model.state_dict().items()}
    trainer.optimizer.zero_grad()
    ep, T = trainer.step(preprocessed_dicts=[dict(s) for s in samples], epoch_losses=trainer.new_epoch_losses())
    torch.cuda.synchronize()
    T_ref = g["T"]
    util.measured(f"{name}: poses vs the reference (relative to the largest element)",
                  float(np.abs(T.detach().cpu().numpy() - T_ref).max() / np.abs(T_ref).max()), bound=REL)
    for key in ("loss_epoch", "loss_point_cloud_epoch", "loss_po2pl_epoch", "loss_pl2pl_epoch", "loss_po2po_epoch"):
        ref = float(g["ep::" + key])
        util.measured(f"{name}: {key} vs the reference (relative)", abs(float(ep[key]) - ref) / max(abs(ref), 1e-12), bound=REL)
    assert int(ep["visible_pixels_epoch"]) == int(g["ep::visible_pixels_epoch"])
    counts = trainer.last_step["pair_counts"]
    if counts is not None:
        got = counts.detach().cpu().numpy().reshape(B, -1)[:, 0].astype(np.int64)
        util.measured(f"{name}: pair counts differing from the reference's (pairs, summed over the batch)",
                      int(np.abs(got - g["pairs"]).sum()), bound=max(2, int(1e-4 * g["pairs"].sum())))
    terms = trainer.last_step["loss_terms"].detach().cpu().numpy().astype(np.float64)
    util.measured(f"{name}: per-sample loss terms vs the reference-pinned oracle (relative)",
                  float((np.abs(terms - g["terms"]) / np.maximum(np.abs(g["terms"]), 1e-12)).max()), bound=REL)
    errs = []
    for k, p in trainer.raw_model.named_parameters():
        ref = float(g["gradnorm::" + k])
        errs.append((abs(float(p.grad.double().norm()) - ref) / max(ref, 1e-12), k, ref))
    errs.sort(reverse=True)
    print(f"  {name}: largest gradient-norm deviations: " + ", ".join(f"{k} {e:.2e} (|g| {r:.3g})" for e, k, r in errs[:4]))
    worst = errs[0][0]
    slack = 0.0
    if "T64" in g:
        # The fixture also holds the reference's step with the NETWORK evaluated in float64 (make_golden.py: referee64).  At batch 8 the
        # reference's own float32 run is further from that referee than this library is (oneDNN convolves a batch of eight with other
        # algorithms than a batch of one or two: its poses move by 5e-6, its conv1 gradient by 3e-4) -- so the bar applies to the referee,
        # and the comparison with the float32 run is allowed the reference's own rounding on top.
        ref_own = max(abs(float(g["gradnorm::" + k]) - float(g["gradnorm64::" + k])) / max(float(g["gradnorm64::" + k]), 1e-12)
                      for k, _ in trainer.raw_model.named_parameters())
        ours64 = max(abs(float(p.grad.double().norm()) - float(g["gradnorm64::" + k])) / max(float(g["gradnorm64::" + k]), 1e-12)
                     for k, p in trainer.raw_model.named_parameters())
        util.measured(f"{name}: the REFERENCE's float32 gradient norms vs its own float64 evaluation (worst, relative)", ref_own)
        util.measured(f"{name}: worst relative error of the 30 gradient norms vs the reference evaluated in float64", ours64, bound=REL)
        util.measured(f"{name}: the REFERENCE's float32 poses vs its own float64 evaluation (relative to the largest element)",
                      float(np.abs(g["T"] - g["T64"]).max() / np.abs(g["T64"]).max()))
        util.measured(f"{name}: poses vs the reference evaluated in float64 (relative to the largest element)",
                      float(np.abs(T.detach().cpu().numpy() - g["T64"]).max() / np.abs(g["T64"]).max()), bound=REL)
        slack = ref_own
    util.measured(f"{name}: worst relative error of the 30 per-parameter gradient norms vs the reference ({errs[0][1]})", worst, bound=REL + slack)
    after = trainer.raw_model.state_dict()
    for k in before:                                        # Adam's first step moves every weight by ~lr*sign(grad)
        got = float((after[k].double() - before[k].double()).sum())
        n = before[k].numel()
        assert abs(got - float(g["delta::" + k])) <= 1e-5 * max(2.0, 0.005 * n), f"Adam update {k}"


def test_quaternion_kernel_against_the_references_own_quat2mat():
    """k_quat_to_T_fwd (csrc/pose.hip) against the reference-held formula `OdometryPublisher.quat2mat`
    (src/ros_utils/odometry_publisher.py:113-126; 1000 unit quaternions evaluated by the reference in make_golden.py)."""
    from delora_amd.models.model_parts import GeometryHandler
    dev = _dev()
    g = util.load_golden("quat2mat")
    q = torch.from_numpy(g["q"]).to(dev)
    T = GeometryHandler.get_transformation_matrix_quaternion(torch.zeros((len(q), 3), device=dev), q, dev)
    util.measured("quaternion -> T kernel vs the reference's quat2mat (absolute, 1000 unit quaternions)",
                  float(np.abs(T[:, :3, :3].cpu().numpy() - g["R"]).max()), bound=1e-6)


@pytest.mark.parametrize("workers", [0, 2])
def test_run_training_cli_with_the_unmodified_yaml_takes_the_hip_path_and_the_graph(tmp_path, workers):
    """The drop-in claim end to end (review item 2): `bin/run_training.py` with this repo's config/*.yaml UNMODIFIED -- the reference's
    shipped KITTI setup, 64x720 images, batch 1, identity pre-training first -- on a tree in the reference's on-disk format under the
    YAML's own relative path.  The CNN must run on the HIP stem + trunk (no "MODULE path" line), epochs must complete and a checkpoint
    with the reference's layout must appear.  With `num_dataloader_workers: 2` (the one key changed, as a user would) the batches come
    through the packed feed."""
    _dev()
    import shutil
    from delora_amd.data import synthetic
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "config"), tmp_path / "config")
    opt = tmp_path / "config" / "deployment_options.yaml"
    if workers:
        opt.write_text(opt.read_text().replace("num_dataloader_workers: 0", f"num_dataloader_workers: {workers}")
                       + "\nhip_graph: auto\n")             # the opt-in measuring policy (round 6: eager is the default) ...
    else:
        assert "hip_graph" not in opt.read_text()              # ... and the YAML exactly as shipped: eager steps
    rng = np.random.default_rng(0)
    for seq in range(9):                                               # training_identifiers 0..8 of the kitti block
        scans, _ = synthetic.make_sequence(100 + seq, 3, rings=64, azimuth_steps=200)
        normals = []
        for sc in scans:
            n = rng.normal(size=sc.shape).astype(np.float32)
            normals.append(n / np.linalg.norm(n, axis=0, keepdims=True))
        synthetic.write_tree(str(tmp_path / "datasets" / "kitti" / "preprocessed" / "sequences"), scans, sequence=seq, normals=normals)
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(root, "bin", "run_training.py"), "--training_run_name", "dropin", "--max_epochs", "2"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "MODULE path" not in r.stdout, "the unmodified YAML (64x720) must run on the HIP stem + trunk"
    assert r.stdout.count("Epoch Summary") == 2 and "nan" not in r.stdout.lower()
    # With `hip_graph: auto` added (the 2-worker run) the loop must have MEASURED the default operating point -- batch 1: ~100 launches whose
    # enqueue time is of the order of their GPU time -- and said what it decided; when it found the step host-bound, the rest of the two
    # epochs must have been replayed as a captured graph, fed from worker processes.  The YAML as shipped (0 workers) takes eager steps.
    import re
    replayed = [int(x) for x in re.findall(r"steps replayed as a HIP graph so far: (\d+)", r.stdout)]
    assert len(replayed) == 2
    if not workers:
        assert "hip_graph auto" not in r.stdout and replayed[-1] == 0, r.stdout[-3000:]
    else:
        m = re.search(r"hip_graph auto \(identity phase\): the host needs ([0-9.]+) ms per step .* the stream ([0-9.]+) ms -> the step is (host|GPU)-bound", r.stdout)
        assert m, r.stdout[-3000:]
        util.measured(f"YAML + `hip_graph: auto` through the CLI ({workers} workers): host period / stream time of the batch-1 step (>= 0.8: replayed as a graph)",
                      float(m.group(1)) / float(m.group(2)), bound=50.0)
        if m.group(3) == "host" and "capture of the step failed" not in r.stdout:
            assert "training step captured as a HIP graph: True" in r.stdout, r.stdout[-3000:]
            assert replayed[-1] >= 4 or "back to the eager step" in r.stdout, replayed
        elif m.group(3) == "GPU":
            assert replayed[-1] == 0, replayed
    ck = torch.load("/tmp/dropin_latest_checkpoint.pth", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["parameters"]["kitti"]["horizontal_cells"] == 720 and len(ck["model_state_dict"]) == 30
    for name in ("dropin_latest_checkpoint.pth", "dropin_checkpoint_epoch_0.pth"):
        if os.path.exists(os.path.join("/tmp", name)):
            os.remove(os.path.join("/tmp", name))
