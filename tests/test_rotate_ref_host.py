"""tests/rotate_ref.py on the host, and the host-side switches of the rotation augmentation (no GPU anywhere in this file):
the fp32 rotation reference is what it says it is, the float64 draws -> matrix reference has the properties the issue of the
option states, the cases of the GPU tier tell every listed defect from the contract, and the configuration gates moved exactly as
far as they should -- the packed feed takes augmented training, graph capture still does not, evaluation never draws."""
import ctypes

import numpy as np
import pytest
import torch

from tests import project_ref as pr
from tests import rotate_ref as rr
from tests import util

f32, f64 = np.float32, np.float64


def _draws(B, seed):
    return np.random.default_rng(seed).random((B, 4), dtype=f32)


# ------------------------------------------------------------------------------------------------ the fp32 rotation reference


def test_rotation_arithmetic_is_three_products_and_two_sums_rounded_to_fp32():
    """Against exact rational arithmetic with an explicit rounding after every operation, on a few hundred points."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    R = rr.rodrigues((0.3, 0.5, 0.8), 0.7).reshape(9).astype(f32)
    p = (rng.normal(size=(3, 200)) * 10.0).astype(f32)
    got = rr.rotate_points(R, p)
    rnd = pr.round_fraction_to_f32
    for i in range(p.shape[1]):
        for k in range(3):
            a, b, c = (rnd(Fraction(float(R[3 * k + j])) * Fraction(float(p[j, i]))) for j in range(3))
            ab = rnd(Fraction(float(a)) + Fraction(float(b)))
            want = rnd(Fraction(float(ab)) + Fraction(float(c)))
            assert got[k, i].view(np.uint32) == want.view(np.uint32), (i, k)


def test_identity_by_bits_passes_every_word_through():
    sen = pr.sensor(rr.SENSOR)
    scan = pr.with_aux(pr.specials(sen), 7, 1)
    assert np.signbit(scan[:3]).any() and np.isnan(scan[:3]).any() and np.isinf(scan[:3]).any()
    same = rr.rotate_scan(rr.IDENTITY9, scan)
    assert np.array_equal(same.view(np.uint32), scan.view(np.uint32))
    # the identity APPLIED would not: -0.0 * 1 + 0 * y is +0.0 and inf * 0 is NaN -- which is why the kernel must not multiply
    applied = rr.rotate_points(rr.IDENTITY9, scan[:3])
    assert not np.array_equal(applied.view(np.uint32), scan[:3].view(np.uint32))
    neg = rr.IDENTITY9.copy()
    neg[1] = -0.0
    assert rr.is_identity_bits(rr.IDENTITY9) and not rr.is_identity_bits(neg)


def test_channels_3_to_5_rotate_only_as_a_whole_vector():
    R = rr.rodrigues((0.0, 0.0, 1.0), 0.5).reshape(9).astype(f32)
    for C in (3, 4, 5, 6, 8):
        scan = pr.with_aux(pr.random_cloud(50, 10.0, 40 + C), C, C)
        out = rr.rotate_scan(R, scan)
        assert np.array_equal(out[:3], rr.rotate_points(R, scan[:3])) and not np.array_equal(out[:3], scan[:3])
        if C >= 6:
            assert np.array_equal(out[3:6], rr.rotate_points(R, scan[3:6])) and np.array_equal(out[6:], scan[6:])
        else:
            assert np.array_equal(out[3:], scan[3:])


# ------------------------------------------------------------------------------------------------ draws -> matrix


@pytest.mark.parametrize("only_yaw", [False, True])
@pytest.mark.parametrize("magnitude_deg", [4.0, 90.0, 360.0])
def test_draws_to_matrix_reference(only_yaw, magnitude_deg):
    B, mag = 64, np.deg2rad(magnitude_deg)
    d = _draws(B, 17)
    d[5, 3] = 0.5                                                   # angle 0
    d[6, :3] = 0.0                                                  # no axis
    R = rr.rotations_from_draws(d, only_yaw, mag).reshape(B, 2, 3, 3)
    eye = np.eye(3)
    assert np.array_equal(R[:, 0], np.broadcast_to(eye, (B, 3, 3))), "scan 1 is never rotated"
    assert np.array_equal(R[5, 1], eye), "angle 0 gives the identity exactly"
    if not only_yaw:
        assert np.array_equal(R[6, 1], eye)
    ang = rr.angles_from_draws(d, mag)
    assert np.all(np.abs(ang) <= f64(f32(mag)) / 2) and np.abs(ang).max() > 0.4 * mag
    # orthonormal, determinant +1, and the angle the draw asked for
    for b in range(B):
        M = R[b, 1]
        assert np.abs(M @ M.T - eye).max() < 1e-14 and abs(np.linalg.det(M) - 1.0) < 1e-14
        if not (only_yaw is False and b == 6):
            assert abs(np.arccos(np.clip((np.trace(M) - 1.0) / 2.0, -1.0, 1.0)) - abs(ang[b])) < 1e-7
    if only_yaw:
        assert np.array_equal(R[:, 1, 2, :], np.broadcast_to([0.0, 0.0, 1.0], (B, 3)))
        assert np.array_equal(R[:, 1, :, 2], np.broadcast_to([0.0, 0.0, 1.0], (B, 3)))
    else:
        # the reference's quirk, kept: every axis lies in the positive octant -- the skew part of R has the signs of +d * sin(a)
        for b in range(B):
            if b in (5, 6):
                continue
            M = R[b, 1]
            axis = np.array([M[2, 1] - M[1, 2], M[0, 2] - M[2, 0], M[1, 0] - M[0, 1]]) / (2.0 * np.sin(ang[b]))
            assert np.all(axis >= -1e-12) and abs(np.linalg.norm(axis) - 1.0) < 1e-9


# ------------------------------------------------------------------------------------------------ the cases tell the defects


def test_cases_cover_what_the_issue_lists():
    cs = rr.cases()
    assert len(cs) == len(rr.CASE_C) * len(rr.CASE_S) * len(rr.CASE_AXES) * len(rr.CASE_ANGLES_DEG) == 72
    met = {True: set(), False: set()}
    for c in cs:
        rot = rr.case_rotations(c)
        for layout in c["layouts"]:
            for s, n in enumerate(rr.case_lengths(c, layout)):
                met[not rr.is_identity_bits(rot[s])].add((c["S"], n))
    for S in rr.CASE_S:
        assert {n for (s_, n) in met[True] if s_ == S} == set(rr.CASE_LENGTHS), f"S={S}: a length never met by a rotated scan"
    assert {n for (s_, n) in met[False] if s_ == 16} == set(rr.CASE_LENGTHS)


def test_every_listed_defect_is_told_by_the_cases():
    """For each defect: the cases whose DEFECTIVE pre-rotated scans differ from the contract's -- the projection of different points
    is compared bit for bit on the GPU tier, and the staging records carry every coordinate into image4 / aux."""
    told = {d: 0 for d in rr.DEFECTS}
    for c in rr.cases():
        layout = c["layouts"][-1]
        scans, rot = rr.case_scans(c, layout), rr.case_rotations(c)
        ref = rr.rotate_scans(scans, rot)
        for d in rr.DEFECTS:
            if (d == "normals-unrotated" and c["C"] < 6) or (d == "previous-row" and c["S"] == 1):
                continue                                            # nothing to get wrong
            if d == "transposed" and c["deg"] == 180.0:
                continue                                            # a half turn is its own transpose: 2 and 90 degrees tell
            if d == "contracted" and c["axis"] == "yaw" and c["deg"] != 2.0:
                continue                                            # entries 0, +-1 and 6e-17: there is nothing left to fuse
            bad = rr.rotate_scans(scans, rot, defect=d)
            assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(ref, bad)), (c["name"], d)
            told[d] += 1
    assert told == {"transposed": 48, "previous-row": 54, "normals-unrotated": 48, "contracted": 48}, told


# ------------------------------------------------------------------------------------------------ the library's refusals (no launch)


def test_rotated_projection_refuses_before_any_launch():
    """The library loads without a GPU and every refusal comes before the first launch: dl_project's own, under the new name."""
    from delora_amd import _lib
    lib = _lib.load()
    sen = _lib.SensorStruct(16, 130, -3.0, 3.0, -0.4, 0.03)
    p = lambda v: ctypes.c_void_p(v)
    ok = dict(pts=p(4096), pts_cs=100, n_cols=100, offs=p(4096), S=2, C=6, max_n=50, sensor=ctypes.byref(sen), image4=p(4096), aux=p(4096),
              packed=p(4096), packed_aux=p(4096), pix2pt=p(4096), ws=p(4096), kept=p(0), uvr=p(0), rot=p(4096))

    def call(**kw):
        a = dict(ok, **kw)
        return lib.dl_project_rotated(a["pts"], a["pts_cs"], a["n_cols"], a["offs"], a["S"], a["C"], a["max_n"], a["sensor"], a["image4"], a["aux"],
                                      a["packed"], a["packed_aux"], a["pix2pt"], a["ws"], a["kept"], a["uvr"], a["rot"], p(0))

    for kw, text in ((dict(offs=p(0)), b"null pointer"), (dict(S=0), b"bad sizes"), (dict(n_cols=101), b"bad sizes"), (dict(C=2), b"bad sizes"),
                     (dict(aux=p(0)), b"needs an aux image"), (dict(C=5), b"packed_aux needs C >= 6"), (dict(ws=p(4096 + 8)), b"16-byte aligned"),
                     (dict(rot=p(4096 + 2)), b"rot must be 4-byte aligned")):
        rc = call(**kw)
        err = lib.dl_last_error()
        assert rc == -1 and err.startswith(b"dl_project_rotated:") and text in err, (kw, rc, err)
    assert lib.dl_rotations_from_draws(p(0), 2, 0, 0.1, p(4096), p(0)) == -1 and b"null pointer" in lib.dl_last_error()
    assert lib.dl_rotations_from_draws(p(4096), 0, 0, 0.1, p(4096), p(0)) == -1 and b"bad sizes" in lib.dl_last_error()
    assert lib.dl_rotations_from_draws(p(4096), 2, 0, float("nan"), p(4096), p(0)) == -1 and b"bad sizes" in lib.dl_last_error()
    assert lib.dl_rotations_from_draws(p(4096), 2, 0, 0.1, p(4096 + 1), p(0)) == -1 and b"4-byte aligned" in lib.dl_last_error()
    assert lib.dl_abi_version() == 10
    for name in ("dl_project_rotated", "dl_rotations_from_draws"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["dl_project_rotated"][1]) == len(_lib.SIGNATURES["dl_project"][1]) + 1


# ------------------------------------------------------------------------------------------------ the configuration gates


def test_augmented_training_keeps_the_packed_feed_and_stays_eager(tmp_path):
    from delora_amd.data import feed
    from delora_amd.data.dataset import PreprocessedPointCloudDataset
    from delora_amd.deploy.graph_step import GraphedStep
    cfg = util.repo_config(16, 128, random_point_cloud_rotations=True, normalization_scaling=False, use_jit=False)
    ds = PreprocessedPointCloudDataset.__new__(PreprocessedPointCloudDataset)       # the gate looks at the type only
    assert feed.packed_feed_applicable(ds, cfg, torch.device("cuda")), "augmented training must keep the packed feed"
    assert not feed.packed_feed_applicable(ds, cfg, torch.device("cpu"))
    assert not feed.packed_feed_applicable(ds, dict(cfg, normalization_scaling=True), torch.device("cuda"))

    class T:
        world_size, grad_scaler = 1, None
        config = cfg
    assert not GraphedStep.config_eligible(T), "an augmented step is not captured"
    T.config = dict(cfg, random_point_cloud_rotations=False)
    assert GraphedStep.config_eligible(T)


def test_only_a_training_step_draws(tmp_path, monkeypatch):
    """A Tester with the option on runs its step without a single draw (the oracle geometry backend on the CPU); a Deployer and a
    Trainer in evaluation mode ask for no rotations either, and augment_input no longer raises."""
    from delora_amd.deploy.deployer import Deployer
    from delora_amd.deploy.tester import Tester
    from delora_amd.deploy.trainer import Trainer
    from tests.test_host_logic import _samples, _small_cfg
    g = util.load_golden("step_b2")
    H, W = int(g["H"]), int(g["W"])
    cfg, sd = _small_cfg(H, W, 1, random_point_cloud_rotations=True)
    tr = Trainer(cfg, dataset=util.ListDataset([]), geometry_backend=util.OracleStepGeometry())
    tr.raw_model.load_state_dict(sd)
    ck = str(tmp_path / "m.pth")
    tr.save_checkpoint(ck, 0, 0.0)
    sample = _samples(g, 1)[0]
    assert tr.augment_input(sample) is sample

    def no_draws(*a, **k):
        raise AssertionError("an evaluation step drew random numbers")
    monkeypatch.setattr(torch, "rand", no_draws)
    cfg2, _ = _small_cfg(H, W, 1, random_point_cloud_rotations=True)
    cfg2.update(checkpoint=ck, output_dir=str(tmp_path), run_name="t", mode="testing")
    te = Tester(cfg2, dataset=util.ListDataset([]), geometry_backend=util.OracleStepGeometry())
    state = torch.get_rng_state()
    with torch.no_grad():
        ep, T = te.step(preprocessed_dicts=_samples(g, 1), epoch_losses=None)
    assert torch.equal(torch.get_rng_state(), state) and torch.isfinite(T).all()
    assert te.last_step["rotations"] is None and te.last_step["rotation_draws"] is None
    assert te.step_rotations(1) == (None, None)
    dep = Deployer(cfg, dataset=util.ListDataset([]), geometry_backend=util.OracleStepGeometry())
    assert dep.step_rotations(2) == (None, None)
    tr.training_bool = False
    assert tr.step_rotations(2) == (None, None)
    tr.training_bool = True
    with pytest.raises(AssertionError, match="drew random numbers"):
        tr.step_rotations(2)                                         # a training step does draw -- exactly here
