"""Host-side checks of the float64 normals reference of tests/test_gpu_normals.py (tests/normals_ref.py; no GPU needed): against the
oracle on the committed goldens, against planted scenes with analytic answers, and the figures of its fp32-moment model that size
the GPU file's tolerances."""
import numpy as np
import pytest
import torch

from tests import normals_ref as R
from tests import util
from tests.util import orc


# ------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("name", ["small", "mid"])
def test_reference_agrees_with_the_oracle_on_the_goldens(name):
    """Mask equal on every non-ambiguous pixel; angles by the criteria of check_normals (tests/test_gpu_geometry.py) -- the oracle's
    fp32 LAPACK solve of raw-moment covariances is the noisy side, hence the statistical form."""
    g = util.load_golden("normals_" + name)
    img = g["image"][0, :3]
    a, b = int(g["side"][0] / 2), int(g["side"][1] / 2)
    ref = R.reference(img, a, b, float(g["epsilon_range"]), int(g["min_neighbors"]))
    v, u = g["v"], g["u"]
    valid = np.zeros(img.shape[1:], dtype=bool)
    valid[v, u] = True
    assert np.array_equal(valid, ref["valid"])
    amb = ref["ambiguous"][v, u]
    util.measured(f"normals reference vs oracle ({name}): ambiguous share", amb.mean(), bound=R.AMBIGUOUS_SHARE_CAP)
    assert np.array_equal(ref["has"][v, u][~amb], g["has"][~amb])
    both = ref["has"][v, u] & g["has"]
    lam = g["eigenvalues"][both].astype(np.float64)
    gap = (lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-30)
    o = np.zeros((3,) + img.shape[1:])
    o[:, v, u] = g["normals"].T
    ang = R.angle_to_reference(o, ref)[v, u][both]
    well = gap > 1e-3
    bound = 2e-4 + 50 * 6e-8 / np.maximum(gap, 1e-12)
    util.measured(f"normals reference vs oracle ({name}): fraction of well-conditioned normals outside the conditioning bound",
                  np.mean(ang[well] > bound[well]), bound=1e-3)
    util.measured(f"normals reference vs oracle ({name}): median angle [rad]", float(np.median(ang)), bound=1e-5)


def test_reference_mask_equals_the_oracle_on_a_scan():
    """64x720 synthetic scan: the has-normal mask equals oracle.compute_normal_vectors on every non-ambiguous valid pixel, and the
    neighbour count equals the oracle's there."""
    img = R.scene("64x720")
    ref = R.reference(img, 3, 5, 0.5, 10)
    sensor = util.oracle_sensor(64, 720, *util.kitti_fov())
    t = torch.zeros(1, 4, 64, 720)
    t[0, :3] = torch.from_numpy(img)
    n, has, pts, aux = orc.compute_normal_vectors(t, sensor, return_aux=True)
    v, u = aux["v"].numpy(), aux["u"].numpy()
    assert len(v) == int(ref["valid"].sum()) > 40000
    keep = ~ref["ambiguous"][v, u]
    assert np.array_equal(ref["has"][v, u][keep], has.numpy()[keep])
    assert np.array_equal(ref["N"][v, u][keep], aux["count"].numpy()[keep].astype(np.float64))


# --------------------------------------------------------------------------------------------------- planted scenes
def test_reference_on_a_plane():
    img, n = R.plane_image()
    for a, b in ((3, 5), (0, 5), (3, 0), (1, 1)):
        ref = R.reference(img, a, b, 5.0, 3)
        need = (2 * a + 1) * (2 * b + 1) >= 3 and a > 0 and b > 0           # a single row or column of a plane is a curve, not a plane
        assert ref["has"].all()
        if need:
            ang = R.angle(ref["normal"], -n[:, None, None] * np.ones_like(ref["normal"]))
            assert ang.max() < 1e-4, (a, b, ang.max())                     # fp32 rounding of the coordinates (1e-6 m over ~0.1 m)
        assert np.all(np.sum(ref["normal"] * img, axis=0) <= 0)


def test_reference_on_two_planes_meeting_at_an_edge():
    img, n, left = R.two_planes_image()
    a, b = 3, 5
    ref = R.reference(img, a, b, 50.0, 10)
    W = img.shape[2]
    edge = int(np.argmin(left[0]))
    one_wall = np.ones(left.shape, dtype=bool)
    one_wall[:, edge - b:edge + b] = False                                  # windows that straddle the edge
    ang = R.angle(ref["normal"], -n)
    assert ref["has"].all() and 0 < edge < W and ang[one_wall].max() < 1e-4
    assert ang[:, edge - 1:edge + 1].min() > 1e-2                           # on the edge the answer is neither wall's


def test_reference_on_collinear_runs():
    img, dirs = R.collinear_image()
    ref = R.reference(img, 3, 5, 100.0, 5)
    rows = np.nonzero(np.any(dirs != 0, axis=1))[0]
    assert np.array_equal(np.nonzero(ref["has"].any(axis=1))[0], rows) and ref["has"][rows].all()
    for r in rows:
        d = dirs[r] / np.linalg.norm(dirs[r])
        assert np.abs(ref["normal"][:, r].T @ d).max() < 1e-9
        assert (ref["evals"][1, r] / ref["evals"][2, r]).max() < 1e-12     # rank 1
        assert np.allclose(np.linalg.norm(ref["normal"][:, r], axis=0), 1.0, atol=1e-12)


def test_reference_rules_on_planted_pixels():
    """The exact rules, one planted pixel each: equality keeps a neighbour, one step beyond drops it; a point with one zero coordinate
    is no centre but counts as a neighbour; an infinite coordinate empties the pixel; clamping duplicates, it does not wrap."""
    img = np.zeros((3, 1, 8), dtype=np.float32)
    img[:, 0, :4] = np.array([[2, 1, 2], [4, 2, 4], [6, 3, 6], [8 + 2.0 ** -19, 4 + 2.0 ** -20, 8 + 2.0 ** -19]],
                             dtype=np.float32).T                          # ranges 3, 6, 9 and 12 + 3 ulp: the last one step beyond eps
    ref = R.reference(img, 0, 1, 3.0, 2, exact_ranges=True)
    assert ref["N"][0, :4].tolist() == [3, 3, 2, 1]      # column 0: itself twice (clamped) and column 1 (at eps exactly)
    img2 = img.copy()
    img2[:, 0, 7] = (2, 1, 2)                                              # a wrap would hand this point to column 0
    assert R.reference(img2, 0, 1, 3.0, 2, exact_ranges=True)["N"][0, 0] == 3
    img3 = img.copy()
    img3[1, 0, 1] = 0.0                                                    # (4, 0, 4): present, not a centre
    r3 = R.reference(img3, 0, 1, 3.0, 2, exact_ranges=True)
    assert not r3["valid"][0, 1] and r3["N"][0, 0] == 3 and not r3["has"][0, 1]
    img4 = img.copy()
    img4[0, 0, 1] = np.inf
    img5 = img.copy()
    img5[:, 0, 1] = 0.0
    r4, r5 = R.reference(img4, 0, 1, 3.0, 2), R.reference(img5, 0, 1, 3.0, 2)
    assert np.array_equal(r4["N"], r5["N"]) and np.array_equal(r4["normal"], r5["normal"]) and r4["N"][0, 0] == 2


def test_gate_image_is_exact_and_has_neighbours_at_eps_and_one_step_beyond():
    img, eps = R.gate_image()
    assert R.ranges_are_exact(img)
    r = np.sqrt(np.sum(img.astype(np.float64) ** 2, axis=0))
    d = np.abs(r[:, 1:] - r[:, :-1])
    assert (d == float(eps)).sum() > 10 and (d == float(eps) + 0.125).sum() > 10
    ref = R.reference(img, 3, 5, eps, 10, exact_ranges=True)
    loose = R.reference(img, 3, 5, float(eps) - 2.0 ** -20, 10, exact_ranges=True)
    assert (ref["N"] > loose["N"]).sum() > 100            # equality keeps the neighbour: dropping it changes the counts
    assert ref["has"].any() and (~ref["has"] & ref["valid"]).any()


# ------------------------------------------------------------------------------------------- the fp32-moment model
def test_moment_model_figures_and_ambiguous_share():
    """What fp32 moments alone cost, on every case of the GPU file: recorded per case with no bound (the GPU file sizes its Rayleigh
    bound from the same figure, normals_ref.rayleigh_bound), and the ambiguous share of every case within the cap.
    Left out here for host time (a minute together): the windows (15,28) and (15,29) on both scenes and (15,31) on the 64x720 scan;
    tests/test_gpu_normals.py computes and asserts the same two figures for them inside check_case.  test_large_window_gate_choice
    below records the share that made those windows on the scan use eps = 8."""
    worst_excess, worst_scaled, worst_rel = 0.0, 0.0, 0.0
    for name, build, a, b, eps, min_n in R.natural_cases() + R.planted_cases():
        if a == 15 and (b != 31 or name.startswith("64x720")):
            continue                                      # the 31-row windows cost a minute of host time together: one of them, small
        img = build()
        exact = name == "exact gate"
        ref = R.reference(img, a, b, eps, min_n, exact_ranges=exact)
        share = ref["ambiguous"].sum() / max(1, int(ref["valid"].sum()))
        util.measured(f"normals reference: ambiguous share ({name})", share, bound=R.AMBIGUOUS_SHARE_CAP)
        mod = R.moment_model32(img, a, b, eps, min_n)
        assert np.array_equal(mod["has"], ref["has"])
        h = ref["has"]
        if not h.any():
            continue
        ang, gap = R.angle_to_reference(mod["normal"], ref)[h], ref["gap"][h]
        rel, scaled = float((ang / R.angle_bound(gap)).max()), float((ang * gap / R.EPS32).max())
        excess = float(R.rayleigh_excess(mod["normal"], ref)[h].max())
        util.measured(f"normals fp32-moment model ({name}): worst angle * gap / eps32", scaled)
        util.measured(f"normals fp32-moment model ({name}): worst Rayleigh excess", excess)
        worst_rel, worst_scaled, worst_excess = max(worst_rel, rel), max(worst_scaled, scaled), max(worst_excess, excess)
    util.measured("normals fp32-moment model: worst angle / (2e-4 + 50 eps32 / gap)", worst_rel)
    util.measured("normals fp32-moment model: worst angle * gap / eps32", worst_scaled)
    util.measured("normals fp32-moment model: worst Rayleigh excess", worst_excess)
    assert R.rayleigh_bound(0.0) == 10.0 * R.EPS32 ** 2 / R.NRM_FP32_GAP and R.rayleigh_bound(1e-9) == 1e-8


def test_boundary_counts_are_populated_on_the_64x720_scene():
    ref = R.reference(R.scene("64x720"), 3, 5, 0.5, 10)
    n = ref["N"][ref["valid"] & ~ref["ambiguous"]]
    assert (n == 10).sum() > 20 and (n == 9).sum() > 20
    gap = ref["gap"][ref["has"]]
    assert (gap < 1e-3).sum() > 100                      # the pixels no older normals test says anything about


def test_large_window_gate_choice():
    """Why the 31-row windows on the 64x720 scan use eps = 8: with eps = 0.5 the ambiguous share of (15,31) is above the cap, with
    eps = 8 well below it (recorded; about 8 s of host time)."""
    img = R.scene("64x720")
    for eps in (0.5, 8.0):
        ref = R.reference(img, 15, 31, eps, 10)
        share = ref["ambiguous"].sum() / ref["valid"].sum()
        util.measured(f"normals reference: ambiguous share (64x720 window (15,31), eps {eps})", share,
                      bound=R.AMBIGUOUS_SHARE_CAP if eps == 8.0 else None)
