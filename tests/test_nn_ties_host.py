"""Host-side checks of the exact-tie scenes and the float64 referee of tests/test_gpu_nn_ties.py (no GPU needed)."""
import numpy as np
import torch

from tests import util
from tests.util import orc


def _pair_d2(q, a, b):
    """fp64 squared distances from fp32 queries to fp32 points, formed as nn.hip's dist2 does (differences of the fp32 values)."""
    da = [(q[i][:, None].double() - a[i][None].double()) for i in range(3)]
    db = [(q[i][:, None].double() - b[i][None].double()) for i in range(3)]
    return (da[0] * da[0] + da[1] * da[1] + da[2] * da[2]), (db[0] * db[0] + db[1] * db[1] + db[2] * db[2]), da


def test_mirror_pairs_tie_bit_for_bit():
    """Grid coordinates: every mirror pair's d2 is the same fp64 number for queries on the mirror plane -- under a 90-degree pose, and
    under an inexact yaw (q_z = c stays exact) -- and the fp32 differences the kernel screens with are exact."""
    tgt = torch.from_numpy(util.mirror_scene(16, 128, "ground", seed=3))
    assert torch.equal(torch.round(tgt.double() / util.GRID) * util.GRID, tgt.double()) and tgt.abs().max() < 2 ** 12
    n = tgt.shape[1] // 2
    real, mirror = tgt[:, :n], tgt[:, n:]
    assert torch.equal(mirror[2].double(), 2 * util.MIRROR_Z - real[2].double()) and torch.equal(mirror[:2], real[:2])
    src = torch.from_numpy(util.ground_sources(16, 128, seed=3))[:, ::7]
    c, s = np.cos(0.37), np.sin(0.37)
    yaw = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    for R, t, exact in ((util.exact_pose(1)[:3, :3], torch.tensor([0.5, -0.25, 0.0]), True), (yaw, torch.tensor([0.3, -0.2, 0.0]), False)):
        q = (R @ src + t[:, None]).float()
        assert torch.all(q[2] == util.MIRROR_Z)
        da, db, diffs = _pair_d2(q, real, mirror)
        assert torch.equal(da, db)
        if exact:
            assert torch.equal((q[0][:, None] - real[0][None]).double(), diffs[0])


def test_referee_breaks_ties_to_the_lower_pixel():
    q = torch.zeros((3, 2), dtype=torch.float64)
    q[0, 1] = 2.0
    pts = torch.tensor([[1.0, -1.0, 0.0, 0.0, 2.25], [0.0, 0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0, 0.0]])
    pix = torch.tensor([7, 3, 5, 1, 9])
    ref, d2, ties = util.nn_referee(q, pts, pix, chunk=1)
    assert ref.tolist() == [3, 9] and d2.tolist() == [1.0, 0.0625] and ties.tolist() == [3, 1]
    # the order of the list does not matter, only the pixel ids
    perm = torch.tensor([4, 2, 0, 3, 1])
    ref2, _, _ = util.nn_referee(q, pts[:, perm], pix[perm])
    assert torch.equal(ref, ref2)


def test_referee_distances_match_the_kdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(5)
    t = rng.normal(0, 5, size=(3, 2000)).astype(np.float32)
    q = rng.normal(0, 5, size=(3, 700)).astype(np.float32)
    ref, d2, _ = util.nn_referee(torch.from_numpy(q), torch.from_numpy(t), torch.arange(2000), chunk=128)
    dk, ik = cKDTree(t.T.astype(np.float64)).query(q.T.astype(np.float64), k=1)
    assert np.allclose(np.sqrt(d2.numpy()), dk, rtol=1e-12, atol=0)
    assert np.array_equal(ref.numpy(), ik)          # no ties in a random cloud


def test_mirror_scene_keeps_every_pair_in_the_image():
    """Every point of the scene has a pixel of its own in the reference projection, so the image holds both members of every pair."""
    vfov, hfov = util.tie_sensor_fov()
    for family in ("ground", "seam"):
        tgt = util.mirror_scene(32, 256, family, seed=1)
        img, _, _, idx, _ = orc.project_to_img(torch.from_numpy(tgt).view(1, 3, -1), util.oracle_sensor(32, 256, vfov, hfov))
        assert len(idx) == tgt.shape[1] > 2000
    src = util.ground_sources(32, 256)
    assert src.shape[1] > 2000 and np.all(src[2] == np.float32(util.MIRROR_Z))
