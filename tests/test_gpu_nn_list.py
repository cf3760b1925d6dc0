"""Exact tree search between free-form point lists (geometry.PointTree = dl_nn_list_build / dl_nn_list_query).

Referee: geometry.nn_bruteforce (dl_nn_bruteforce, the exhaustive fp64 kernel) on the same device tensors.  Comparison: torch.equal
on the index vectors -- no mismatch is allowed anywhere.  Every input is made on the host in numpy fp32 and uploaded.  The inputs
that come from seeds were checked on the CPU to be free of near-ties (tools/nn_list_tie_check.py: smallest relative gap between the
nearest and the second nearest squared distance 6.4e-10, six orders above fp64 rounding), so the exact index is unambiguous; the
inputs with exact ties are built from bit-identical copies, which tie in any arithmetic.
"""
import warnings

import numpy as np
import pytest
import torch

from delora_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _geo():
    from delora_amd import geometry
    return geometry


def _up(a, dev):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32 and a.ndim == 2 and a.shape[0] == 3
    return torch.from_numpy(a).to(dev)


def _tilt(s):
    R = syn._rot_zyx(0.3, -0.1, 0.05).astype(np.float32)
    return (R @ s + np.array([[30.0], [2.0], [0.5]], np.float32)).astype(np.float32)


def _poses(seed, s1, s2):
    rng = np.random.default_rng(seed)
    Rr = syn._rot_zyx(*rng.uniform(-3.1, 3.1, 3)).astype(np.float32)
    tr = rng.normal(size=(3, 1)).astype(np.float32)
    return {"identity": s2, "tilted": _tilt(s2), "random": (Rr @ s2 + tr).astype(np.float32), "self": s1}


def _agree(src, tgt, what, tree=None):
    """Tree answer == referee answer on device tensors; returns the answer."""
    geo = _geo()
    tree = tree if tree is not None else geo.PointTree(tgt)
    got = tree.query(src)
    ref = geo.nn_bruteforce(src, tgt)
    assert got.dtype == torch.int32 and got.shape == ref.shape
    bad = int((got != ref).sum())
    print(f"{what}: Ms {src.shape[1]} Mt {tgt.shape[1]} mismatches {bad}")
    assert torch.equal(got, ref), f"{what}: {bad} of {src.shape[1]} indices differ from the exhaustive search"
    return got


CASES = [(seed, n) for n in (1, 63, 64, 65, 1000, 32768, 131072) for seed in (9101, 9102)] + [(9101, 262144)]


@pytest.mark.parametrize("seed,n", CASES)
def test_portable_pairs_in_four_poses(seed, n):
    dev = _dev()
    p = syn.portable_pair(seed, n)
    tgt = _up(p["scan_1"], dev)
    tree = _geo().PointTree(tgt)
    for name, src in _poses(seed, p["scan_1"], p["scan_2"]).items():
        got = _agree(_up(src, dev), tgt, f"pair {seed} n={n} {name}", tree)
        if name == "self":                                             # no duplicate targets: every point is its own neighbour
            assert torch.equal(got, torch.arange(n, dtype=torch.int32, device=dev))


def test_ragged_lists_and_column_strides():
    dev = _dev()
    p, q = syn.portable_pair(9101, 70001), syn.portable_pair(9102, 1000)
    for name, (src, tgt) in {"1000 vs 70001": (q["scan_2"], p["scan_1"]), "70001 vs 1000": (p["scan_2"], q["scan_1"])}.items():
        s, t = _up(src, dev), _up(tgt, dev)
        dense = _agree(s, t, "ragged " + name)
        # the same lists as views into larger tensors: column strides above the counts
        big_s = torch.full((3, s.shape[1] + 37), 7.5, device=dev)
        big_t = torch.full((3, t.shape[1] + 101), -3.25, device=dev)
        big_s[:, :s.shape[1]] = s
        big_t[:, :t.shape[1]] = t
        vs, vt = big_s[:, :s.shape[1]], big_t[:, :t.shape[1]]
        assert vs.stride(0) > vs.shape[1] and vt.stride(0) > vt.shape[1]
        tree = _geo().PointTree(vt)
        assert tree._cs == vt.stride(0) and tree.tgt.data_ptr() == big_t.data_ptr()          # really the view, not a dense copy
        assert torch.equal(tree.query(vs), dense), "strided " + name


def test_uniform_cloud_and_scale_mixture():
    dev = _dev()
    n = 131072
    rng = np.random.default_rng(5)
    u_t = rng.uniform(-50, 50, (3, n)).astype(np.float32)
    u_s = rng.uniform(-60, 60, (3, n)).astype(np.float32)                  # queries outside the target box
    _agree(_up(u_s, dev), _up(u_t, dev), "uniform cloud")
    core = rng.normal(0, 0.01, (3, n // 2)).astype(np.float32)
    far = (rng.normal(0, 1, (3, n // 2)) * 5000).astype(np.float32)
    mix = np.concatenate([core, far], 1)
    src = (mix[:, rng.permutation(n)] * np.float32(1.001)).astype(np.float32)
    _agree(_up(src, dev), _up(mix, dev), "scale mixture")                  # the ordering grid is useless here; the answer is not


def test_degenerate_lists():
    dev = _dev()
    geo = _geo()
    rng = np.random.default_rng(11)
    src = _up(rng.normal(0, 3, (3, 777)).astype(np.float32), dev)
    # all targets identical: every answer is index 0
    same = np.repeat(np.array([[1.5], [-2.25], [0.125]], np.float32), 1000, axis=1)
    got = _agree(src, _up(same, dev), "identical targets")
    assert int(got.abs().max()) == 0
    # all points in one cell of the ordering grid but distinct (spread 1e-3 around a point at 1e4: a few ulp apart)
    cell = (np.array([[1e4], [1e4], [1e4]], np.float32) + rng.integers(-4, 5, (3, 500)).astype(np.float32) * np.float32(2 ** -10)).astype(np.float32)
    _agree(_up(cell[:, ::-1].copy() + np.float32(2 ** -11), dev), _up(cell, dev), "one cell")
    # targets on a line
    k = np.arange(1000, dtype=np.float32)
    line = np.stack([np.float32(0.5) + k * np.float32(0.25), np.float32(-1.0) + k * np.float32(0.125), np.float32(2.0) - k * np.float32(0.0625)])
    _agree(src, _up(line, dev), "collinear targets")
    _agree(_up(line[:, ::3].copy(), dev), _up(line, dev), "collinear both")
    # a span from 1e-3 to 1e4 m
    span = (rng.normal(0, 1, (3, 4000)) * (10.0 ** rng.uniform(-3, 4, (1, 4000)))).astype(np.float32)
    _agree(_up((span[:, :2000] * np.float32(1.01)).astype(np.float32), dev), _up(span, dev), "1e-3 .. 1e4")
    # tiny lists
    pts = rng.normal(0, 3, (3, 2)).astype(np.float32)
    for mt in (0, 1, 2):
        got = _agree(src, _up(pts[:, :mt], dev), f"Mt={mt}")
        if mt == 0:
            assert bool((got == -1).all())
        assert geo.PointTree(_up(pts[:, :mt], dev)).query(src[:, :0]).shape == (0,)         # Ms = 0
    assert _agree(src[:, :1].contiguous(), _up(line, dev), "Ms=1").shape == (1,)


def test_tie_rule_lowest_index_of_a_duplicate_group():
    dev = _dev()
    base = syn.portable_pair(9101, 32768)["scan_1"]
    n, c = base.shape[1], 4096
    pts = np.concatenate([base[:, n - c:], base, base[:, :c]], 1)          # copies of the LAST points in front, of the FIRST behind
    assert pts.shape[1] == n + 2 * c == 40960
    tgt = _up(pts, dev)
    got = _agree(tgt, tgt, "ties, self query")
    j = np.arange(n + 2 * c)
    b = j - c                                                           # index into base of the middle part
    expect = np.where(j < c, j, np.where(j >= c + n, j - n, np.where(b >= n - c, b - (n - c), j)))
    assert np.array_equal(got.cpu().numpy(), expect.astype(np.int32))     # the lowest index of every duplicate group
    _agree(_up(_tilt(pts), dev), tgt, "ties, tilted query")


def test_non_finite_queries_and_targets():
    dev = _dev()
    p = syn.portable_pair(9102, 1000)
    tgt_h, src_h = p["scan_1"], _tilt(p["scan_2"])
    tgt = _up(tgt_h, dev)
    clean = _agree(_up(src_h, dev), tgt, "clean")
    bad_q = src_h.copy()
    rows = np.arange(0, 1000, 7)
    for i, col in enumerate(rows):
        bad_q[i % 3, col] = (np.nan, np.inf, -np.inf)[(i // 3) % 3]
    got = _agree(_up(bad_q, dev), tgt, "non-finite queries")
    mask = torch.zeros(1000, dtype=torch.bool, device=dev)
    mask[torch.from_numpy(rows).to(dev)] = True
    assert bool((got[mask] == -1).all()) and torch.equal(got[~mask], clean[~mask])          # and the neighbours are not disturbed
    # non-finite targets, a few and then the majority: never returned
    for every, name in ((9, "few"), (1, "most")):
        bad_t = tgt_h.copy()
        cols = np.array([k for k in range(1000) if (k % every == 0 and k % 10 != 3)])
        for i, col in enumerate(cols):
            bad_t[i % 3, col] = (np.inf, np.nan, -np.inf)[(i // 3) % 3]
        got = _agree(_up(src_h, dev), _up(bad_t, dev), f"non-finite targets ({name}: {len(cols)} of 1000)")
        assert not np.isin(got.cpu().numpy(), cols).any() and int(got.min()) >= 0
    none = np.full((3, 200), np.nan, np.float32)
    none[1] = 1.0
    got = _agree(_up(src_h, dev), _up(none, dev), "no finite target")
    assert bool((got == -1).all())


def test_deterministic_and_a_tree_serves_many_queries():
    dev = _dev()
    geo = _geo()
    p = syn.portable_pair(9101, 32768)
    tgt, a, b = _up(p["scan_1"], dev), _up(_tilt(p["scan_2"]), dev), _up(p["scan_2"][:, :20001].copy(), dev)
    tree = geo.PointTree(tgt)
    first = tree.query(a).clone()
    assert torch.equal(tree.query(a), first)
    x = torch.randn((1024, 1024), device=dev)
    (x @ x).sum().item()                                                # other work on the stream in between
    assert torch.equal(tree.query(a), first)
    on_b = tree.query(b).clone()
    assert torch.equal(tree.query(a), first)                            # ... and after a query of another size
    assert torch.equal(geo.PointTree(tgt).query(a), first) and torch.equal(geo.PointTree(tgt).query(b), on_b)
    assert torch.equal(first, geo.nn_bruteforce(a, tgt)) and torch.equal(on_b, geo.nn_bruteforce(b, tgt))


def test_permuting_the_targets_permutes_the_answers():
    dev = _dev()
    p = syn.portable_pair(9102, 32768)
    src, tgt_h = _up(_tilt(p["scan_2"]), dev), p["scan_1"]
    perm = np.random.default_rng(3).permutation(tgt_h.shape[1])
    nn = _agree(src, _up(tgt_h, dev), "in order")
    nn_p = _agree(src, _up(tgt_h[:, perm].copy(), dev), "permuted")
    assert torch.equal(torch.from_numpy(perm).to(dev)[nn_p.long()].int(), nn)


def test_against_ckdtree_on_the_host():
    from scipy.spatial import cKDTree
    dev = _dev()
    p = syn.portable_pair(9101, 131072)
    src_h, tgt_h = _tilt(p["scan_2"]), p["scan_1"]
    _, ref = cKDTree(tgt_h.T.astype(np.float64)).query(src_h.T.astype(np.float64), k=1, workers=16)
    got = _geo().PointTree(_up(tgt_h, dev)).query(_up(src_h, dev))
    assert np.array_equal(got.cpu().numpy().astype(np.int64), ref.astype(np.int64))


def test_build_and_query_replay_from_a_captured_graph():
    dev = _dev()
    geo = _geo()
    p1, p2 = syn.portable_pair(9101, 32768), syn.portable_pair(9102, 32768)
    tgt_s, src_s = _up(p1["scan_1"], dev), _up(_tilt(p1["scan_2"]), dev)       # static operands of the graph
    out = torch.full((src_s.shape[1],), -7, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tree = geo.PointTree(tgt_s)
        tree.query(src_s, out=out)                                      # warm-up: the workspace exists before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager1 = out.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                           # one stream, one linear chain of launches
        tree.rebuild()
        tree.query(src_s, out=out)
    for pair in (p2, p1):
        tgt_s.copy_(_up(pair["scan_1"], dev))
        src_s.copy_(_up(_tilt(pair["scan_2"]), dev))
        out.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        fresh = geo.PointTree(tgt_s.clone()).query(src_s.clone())
        assert torch.equal(out, fresh) and torch.equal(out, geo.nn_bruteforce(src_s, tgt_s))
    assert torch.equal(out, eager1)


def _same(a, b):
    a, b = a.detach(), b.detach()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


@pytest.mark.parametrize("p2p", [True, False])
@pytest.mark.parametrize("drop_normals", [False, True])
def test_icp_losses_on_full_size_lists(p2p, drop_normals, monkeypatch):
    """The list module on 131 072-point lists: losses, T.grad and the pair count equal, bit for bit, those of the same module forced
    onto the exhaustive kernel (same indices, same torch arithmetic), and the tree path raises no RuntimeWarning.
    drop_normals: additionally every 5th source and every 7th target normal zeroed, so that the point-to-point branch has pairs."""
    from delora_amd.losses.icp_losses import ICPLosses
    dev = _dev()
    p = syn.portable_pair(9101, 131072)
    R = syn._rot_zyx(0.3, -0.1, 0.05).astype(np.float32)
    n1, n2 = p["normal_list_1"].copy(), p["normal_list_2"].copy()
    if drop_normals:
        n2[:, ::5] = 0.0
        n1[:, ::7] = 0.0
    tgt, tgt_n = _up(p["scan_1"], dev).view(1, 3, -1), _up(n1, dev).view(1, 3, -1)
    src, src_n = _up(p["scan_2"], dev).view(1, 3, -1), _up(n2, dev).view(1, 3, -1)
    cfg = {"normal_loss": "squared", "po2po_alone": False, "point_to_point_loss": p2p, "point_to_plane_loss": True,
           "plane_to_plane_loss": True}
    mod = ICPLosses(cfg)

    def run():
        T = torch.eye(4, device=dev).view(1, 4, 4).clone()
        T[0, :3, :3] = torch.from_numpy(R).to(dev)
        T[0, :3, 3] = torch.tensor([30.0, 2.0, 0.5], device=dev)
        T.requires_grad_(True)
        s_t = T[:, :3, :3].matmul(src) + T[:, :3, 3].view(-1, 3, 1)
        n_t = T[:, :3, :3].matmul(src_n)
        losses, plotting = mod(source_point_cloud_transformed=s_t, source_normal_list_transformed=n_t, target_point_cloud=tgt,
                               target_normal_list=tgt_n, compute_pointwise_loss_bool=False)
        total = 2.0 * losses["loss_po2pl"] + 0.5 * losses["loss_pl2pl"]
        if p2p and drop_normals:
            total = total + losses["loss_po2po"]
        total.sum().backward()
        return losses, T.grad.clone(), int(plotting["scan_2_transformed"].shape[2])

    monkeypatch.setattr(ICPLosses, "_warned_quadratic", False)
    assert ICPLosses._wants_tree(131072, 131072)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                  # the tree path must not warn
        l_tree, g_tree, pairs_tree = run()
    assert ICPLosses._warned_quadratic is False
    monkeypatch.setattr(ICPLosses, "tree_min_pairs", 1 << 62)           # the same module on the exhaustive kernel
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        l_bf, g_bf, pairs_bf = run()
    assert ICPLosses._warned_quadratic is True                           # ... which does say so
    for k in ("loss_po2po", "loss_po2pl", "loss_pl2pl"):
        assert _same(l_tree[k], l_bf[k]), (k, l_tree[k], l_bf[k])
    assert bool(torch.isfinite(l_tree["loss_po2pl"]).all()) and bool(torch.isfinite(l_tree["loss_pl2pl"]).all())
    assert _same(g_tree, g_bf) and bool(torch.isfinite(g_tree).all())
    assert pairs_tree == pairs_bf > 0
