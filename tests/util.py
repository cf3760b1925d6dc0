"""Shared helpers of the test-suite (the only place besides bench.py's cpu_baseline leg and
__graft_entry__.smoke() that touches oracle/)."""
import os

import numpy as np
import torch

from oracle import delora_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Measured deviations (mismatch counts, worst relative errors) recorded by the parity tests: printed as a table at the end
# of the session and written to gpurun_out/parity_measured.json (tests/conftest.py), so that a regression inside a
# tolerance is still visible as a number.
MEASURED = {}


def measured(name, value, bound=None):
    """Record (and print) a measured deviation; with ``bound`` also assert value <= bound."""
    MEASURED[name] = {"value": float(value), "bound": None if bound is None else float(bound)}
    print(f"[measured] {name} = {float(value):.6g}" + (f"  (bound {float(bound):.6g})" if bound is not None else ""))
    if bound is not None:
        assert float(value) <= float(bound), f"{name}: measured {float(value):.6g} exceeds the bound {float(bound):.6g}"


def load_golden(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def oracle_sensor(H, W, vfov, hfov):
    return orc.Sensor(int(H), int(W), [float(v) for v in vfov], [float(h) for h in hfov])


def kitti_fov():
    return ((-24.5 * (np.pi / 180.0), 2.0 * (np.pi / 180.0)), (-179.9 * (np.pi / 180.0), 179.9 * (np.pi / 180.0)))


def reference_pixels(xyz, sensor):
    """Per-point (pixel index or -1, u, v) as the reference computes them: fp32 torch ops of
    compute_2D_coordinates + round-half-even + FoV test (elementwise, so input order is irrelevant)."""
    pc = torch.from_numpy(np.ascontiguousarray(xyz[:3])).view(1, 3, -1)
    u, v = orc.compute_2d_coordinates(pc, sensor)
    ru, rv = torch.round(u[0]), torch.round(v[0])
    inside = (ru <= sensor.W - 1) & (ru >= 0) & (rv <= sensor.H - 1) & (rv >= 0)
    pix = torch.where(inside, rv.long() * sensor.W + ru.long(), torch.full_like(ru, -1).long())
    return pix.numpy(), u[0].numpy(), v[0].numpy()


def ambiguity_mask(xyz, sensor, tol=2e-3):
    """Points whose exact (fp64) image coordinate lies within tol px of a rounding boundary: the only points
    whose pixel may differ between two correct fp32 evaluations of atan2."""
    p = np.asarray(xyz[:3], dtype=np.float64)
    u = (np.arctan2(p[1], p[0]) - sensor.hfov[0]) / (sensor.hfov[1] - sensor.hfov[0]) * (sensor.W - 1)
    v = (np.arctan2(p[2], np.hypot(p[0], p[1])) - sensor.vfov[0]) / (sensor.vfov[1] - sensor.vfov[0]) * (sensor.H - 1)
    fu = np.abs(u - np.floor(u) - 0.5)
    fv = np.abs(v - np.floor(v) - 0.5)
    return (fu < tol) | (fv < tol)


def lists_from_images(image4, normals):
    """Raster-order point / normal lists ``[1,3,M]`` (CPU) of the occupied pixels of one image, plus the pixel ids."""
    img = image4.detach().cpu()
    occ = ~((img[0] == 0) & (img[1] == 0) & (img[2] == 0))
    pix = torch.nonzero(occ.reshape(-1)).reshape(-1)
    pts = img[:3].reshape(3, -1)[:, pix].contiguous().view(1, 3, -1)
    nrm = normals.detach().cpu().reshape(3, -1)[:, pix].contiguous().view(1, 3, -1)
    return pts, nrm, pix


def tainted_pixels(xyz, sensor, tol=2e-3):
    """Pixels an ambiguous point (see ambiguity_mask) may or may not land in: both rounding candidates in u and v.
    Two correct fp32 evaluations of the projection (different CPUs' Sleef paths, or the GPU's) can only differ there."""
    p = np.asarray(xyz[:3], dtype=np.float64)
    amb = ambiguity_mask(xyz, sensor, tol)
    u = (np.arctan2(p[1], p[0]) - sensor.hfov[0]) / (sensor.hfov[1] - sensor.hfov[0]) * (sensor.W - 1)
    v = (np.arctan2(p[2], np.hypot(p[0], p[1])) - sensor.vfov[0]) / (sensor.vfov[1] - sensor.vfov[0]) * (sensor.H - 1)
    t = np.zeros((sensor.H, sensor.W), dtype=bool)
    ua, va = u[amb], v[amb]
    for du in (-tol * 2, tol * 2):
        for dv in (-tol * 2, tol * 2):
            uu, vv = np.rint(ua + du).astype(np.int64), np.rint(va + dv).astype(np.int64)
            ok = (uu >= 0) & (uu < sensor.W) & (vv >= 0) & (vv < sensor.H)
            t[vv[ok], uu[ok]] = True
    return t


def repo_config(H, W, dataset="kitti", device="cpu", **over):
    """The flat run config built from THIS repo's config/*.yaml the way bin/run_training.py builds it."""
    import copy
    from delora_amd import config as cfgmod
    from tests.conftest import ROOT
    cfg = cfgmod.load_yaml_config(os.path.join(ROOT, "config"))
    cfg["datasets"] = [dataset]
    cfgmod.degrees_to_radians(cfg)
    cfg[dataset]["data_identifiers"] = cfg[dataset]["training_identifiers"]
    cfg[dataset]["vertical_cells"], cfg[dataset]["horizontal_cells"] = int(H), int(W)
    cfg["device"] = torch.device(device)
    cfg["checkpoint"] = None
    cfg["training_run_name"] = cfg["run_name"] = "test"
    cfg["mode"] = "training"
    cfg.update(over)
    return copy.deepcopy(cfg)


class ListDataset(torch.utils.data.Dataset):
    def __init__(self, samples):
        self.samples = samples

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        return dict(self.samples[i])


class OracleStepGeometry:
    """Test-only geometry backend with the interface of delora_amd.deploy.step_geometry.HipStepGeometry, evaluated by
    the CPU oracle.  It lets the host logic of the step (loss weighting, DDP, optimiser) be exercised without a GPU;
    the product never constructs it (Deployer defaults to the HIP backend and fails without the library)."""

    def prepare(self, samples, sensor, normal_params):
        o_sensor = orc.Sensor(sensor.H, sensor.W, sensor.vfov, sensor.hfov)
        stacked, lists = [], []
        a, b, eps, min_n = normal_params
        for s in samples:
            entry, imgs = {}, []
            for k in ("1", "2"):
                scan = s["scan_" + k].detach().cpu()
                img, _, _, idx, _ = orc.project_to_img(scan, o_sensor)
                imgs.append(img[0])
                if s.get("normal_list_" + k) is not None:
                    entry["scan_" + k] = scan[:, :, idx]
                    entry["normal_list_" + k] = s["normal_list_" + k].detach().cpu()[:, :, idx]
                else:
                    n, has, pts = orc.compute_normal_vectors(img.clone(), o_sensor, side=(2 * a + 1, 2 * b + 1),
                                                             epsilon_range=eps, min_neighbors=min_n)
                    entry["scan_" + k] = pts.t().contiguous().view(1, 3, -1)
                    entry["normal_list_" + k] = n.t().contiguous().view(1, 3, -1)
            stacked.append(torch.cat(imgs, dim=0))
            lists.append(entry)
        return {"stacked": torch.stack(stacked), "lists": lists, "sensor": o_sensor}

    def losses(self, T, prepared, flags, need_without_normals):
        rows, vis = [], []
        for j, L in enumerate(prepared["lists"]):
            Tj = T[j:j + 1]
            s_t = orc.transform_points(Tj, L["scan_2"])
            l = orc.icp_losses(s_t, orc.rotate_points(Tj, L["normal_list_2"]), L["scan_1"], L["normal_list_1"],
                               normal_loss="linear" if flags & 8 else "squared", point_to_point=bool(flags & 1),
                               point_to_plane=bool(flags & 2), plane_to_plane=bool(flags & 4), po2po_alone=bool(flags & 16))
            rows.append(torch.stack([l["loss_po2po"].reshape(()), l["loss_po2pl"].reshape(()), l["loss_pl2pl"].reshape(())]))
            vis.append(orc.visible_pixels(s_t, prepared["sensor"]))
        return torch.stack(rows), None, torch.tensor(vis)


def portable_step_inputs(g):
    """Regenerate the inputs of a `step_full_*` / `step_b8_small` fixture from its seeds (delora_amd.data.synthetic's portable generators)
    and prove by sha256 that they are the arrays the reference ran on.  Returns the list of sample dicts ([1,3,n] CPU tensors)."""
    from delora_amd.data import synthetic
    pairs = [synthetic.portable_pair(int(sd), int(g["n_points"])) for sd in g["seeds"]]
    got = synthetic.digest([p[k] for p in pairs for k in ("scan_1", "normal_list_1", "scan_2", "normal_list_2")])
    assert got == str(g["input_sha"]), "the portable generator does not reproduce the fixture's inputs on this machine"
    return [{**{k: torch.from_numpy(p[k]).unsqueeze(0) for k in ("scan_1", "scan_2", "normal_list_1", "normal_list_2")}, "dataset": "kitti"}
            for p in pairs]


def portable_full_state(g):
    """The full network's state_dict of a `step_full_*` fixture, regenerated and sha-checked."""
    from delora_amd.data import synthetic
    shapes = {k[len("shape::"):]: tuple(int(d) for d in v) for k, v in g.items() if k.startswith("shape::")}
    state = synthetic.portable_state_dict(int(g["state_seed"]), shapes)
    assert synthetic.digest([state[k] for k in shapes]) == str(g["state_sha"]), "portable weights differ from the fixture's"
    return {k: torch.from_numpy(v) for k, v in state.items()}


# ------------------------------------------------------------------------------------ scenes with exact distance ties
# Every coordinate is a multiple of 2^-10 m below 2^12 m in magnitude: a fp32 difference of two of them is exact, so are its
# square and the sum of three squares in fp64 -- the search kernel's distances and a float64 torch referee are then the SAME
# numbers, and two targets placed symmetrically about a plane through the query are an exact tie.
GRID = 2.0 ** -10
MIRROR_Z = -1.75                 # the mirror plane z = c of the ground family (a ground plane below the sensor)
TIE_VFOV_DEG = (-40.0, 15.0)     # far enough below the horizon for the reflections to land in the image
ROOM = (18.0, 11.0)              # half extents of the room in x and y


def on_grid(a):
    return np.round(np.asarray(a, dtype=np.float64) / GRID) * GRID


def tie_sensor_fov():
    return (TIE_VFOV_DEG[0] * np.pi / 180.0, TIE_VFOV_DEG[1] * np.pi / 180.0), kitti_fov()[1]


def _room_surfaces(rng, n):
    """About n points on the room above the ground plane z = MIRROR_Z (walls, boxes, pillars), none on the plane itself."""
    c, (X, Y) = MIRROR_Z, ROOM
    z0, z1 = c + 1.0 / 32.0, c + 4.5
    pts = []
    nw = int(n * 0.55)
    s = rng.uniform(-1.0, 1.0, nw)
    side = rng.integers(0, 4, nw)
    z = rng.uniform(z0, z1, nw)
    x = np.where(side < 2, np.where(side == 0, -X, X), s * X)
    y = np.where(side < 2, s * Y, np.where(side == 2, -Y, Y))
    pts.append(np.stack([x, y, z]))
    boxes = [(-9.0, -5.0, 2.0, 1.0, 1.5), (7.5, 4.0, 1.25, 2.5, 0.75), (3.0, -6.5, 0.75, 0.75, 2.25), (-4.0, 6.0, 1.5, 1.0, 1.0),
             (12.0, -2.0, 1.0, 1.75, 2.5), (-13.5, 3.5, 0.5, 2.0, 0.5)]
    nb = int(n * 0.3) // len(boxes)
    for (bx, by, hx, hy, hz) in boxes:
        f = rng.integers(0, 5, nb)                   # faces -x, +x, -y, +y and the top
        u, w, v = rng.uniform(-1.0, 1.0, nb), rng.uniform(-1.0, 1.0, nb), rng.uniform(0.0, 1.0, nb)
        xx = np.where(f == 0, bx - hx, np.where(f == 1, bx + hx, bx + u * hx))
        yy = np.where(f == 2, by - hy, np.where(f == 3, by + hy, by + w * hy))
        zz = np.where(f == 4, c + hz, z0 + v * (c + hz - z0))
        pts.append(np.stack([xx, np.where(f < 2, by + u * hy, yy), zz]))
    pillars = [(-2.0, -2.5), (5.0, 1.5), (-7.0, 2.0), (10.0, 6.5)]
    npl = (n - sum(p.shape[1] for p in pts)) // len(pillars)
    for (px, py) in pillars:
        a = rng.uniform(-np.pi, np.pi, npl)
        pts.append(np.stack([px + 0.25 * np.cos(a), py + 0.25 * np.sin(a), rng.uniform(z0, z1, npl)]))
    return np.concatenate(pts, axis=1)


def _pixels(p, H, W, vfov, hfov):
    """Pixel index (or -1) of fp32 points as the reference projects them, -1 also for points within 0.05 px of a rounding
    boundary (a GPU evaluation of atan2 may round those the other way)."""
    s = oracle_sensor(H, W, vfov, hfov)
    pix, _, _ = reference_pixels(p.astype(np.float32), s)
    return np.where(ambiguity_mask(p, s, tol=0.05), -1, pix)


def mirror_scene(H, W, family="ground", seed=0, n=None):
    """Target cloud [3,N] fp32 of exact mirror pairs (one pixel each, no two points sharing a pixel in the image of an
    (H, W) sensor with tie_sensor_fov()).  family "ground": the room and its reflection z -> 2c - z about z = MIRROR_Z;
    "seam": the room's half y > 0 and its reflection y -> -y (the partners sit on either side of the azimuth seam for queries
    on y = 0 with x < 0)."""
    vfov, hfov = tie_sensor_fov()
    rng = np.random.default_rng(seed)
    p = on_grid(_room_surfaces(rng, n or 3 * H * W))
    if family == "ground":
        m = p.copy()
        m[2] = 2.0 * MIRROR_Z - p[2]
    else:
        p = p[:, p[1] >= 1.0 / 32.0]
        m = p.copy()
        m[1] = -p[1]
    pa, pb = _pixels(p, H, W, vfov, hfov), _pixels(m, H, W, vfov, hfov)
    keep = (pa >= 0) & (pb >= 0)
    idx = np.nonzero(keep)[0]
    # one point per pixel: the first pair wins a pixel, a pair that lost either of its pixels goes entirely
    for arr in (pa, pb):
        _, first = np.unique(arr[idx], return_index=True)
        idx = idx[np.sort(first)]
    idx = idx[~np.isin(pa[idx], pb[idx]) & ~np.isin(pb[idx], pa[idx])]
    return np.concatenate([p[:, idx], m[:, idx]], axis=1).astype(np.float32)


def ground_sources(H, W, seed=0):
    """Source cloud [3,M] fp32: ground hits at z = MIRROR_Z exactly (one per pixel below the horizon, inside the room), x and y
    on the grid."""
    vfov, hfov = tie_sensor_fov()
    rng = np.random.default_rng(seed + 1)
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    v = rows.reshape(-1) + rng.uniform(-0.3, 0.3, H * W)
    u = cols.reshape(-1) + rng.uniform(-0.3, 0.3, H * W)
    el = vfov[0] + v / (H - 1) * (vfov[1] - vfov[0])
    az = hfov[0] + u / (W - 1) * (hfov[1] - hfov[0])
    ok = el < -0.02
    r = MIRROR_Z / np.tan(el[ok])
    x, y = on_grid(r * np.cos(az[ok])), on_grid(r * np.sin(az[ok]))
    ins = (np.abs(x) < ROOM[0] - 0.25) & (np.abs(y) < ROOM[1] - 0.25)
    p = np.stack([x[ins], y[ins], np.full(int(ins.sum()), MIRROR_Z)])
    return p[:, _pixels(p, H, W, vfov, hfov) >= 0].astype(np.float32)


def exact_pose(quarter_turns=0, t=(0.0, 0.0, 0.0), about="z"):
    """4x4 float32 rigid motion whose rotation entries are 0 / +-1 (a multiple of 90 degrees about z, or about x), t on the grid:
    the kernel's fmaf chain and a float64 product give the same transformed point, bit for bit."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    T = np.eye(4)
    if about == "z":
        T[:2, :2] = [[c, -s], [s, c]]
    else:
        T[1:3, 1:3] = [[c, -s], [s, c]]
    T[:3, 3] = on_grid(t)
    return torch.tensor(T, dtype=torch.float32)


def nn_referee(q, tgt_pts, tgt_pix, chunk=256):
    """Nearest target of every query with the tie rule written out: the smallest (d2, pixel index), lexicographically.
    q [3,M], tgt_pts [3,N] (any float dtype; evaluated in float64 with explicit differences, not the matmul form of cdist),
    tgt_pix [N] pixel ids.  Returns (pixel [M] int64, d2 [M] float64, ties [M] int64 = targets at that minimum)."""
    q = q.double()
    t = tgt_pts.double()
    pix = tgt_pix.long().to(t.device)
    big = torch.iinfo(torch.int64).max
    out_pix, out_d2, out_ties = [], [], []
    for i in range(0, q.shape[1], chunk):
        qc = q[:, i:i + chunk, None]
        dx, dy, dz = qc[0] - t[0][None], qc[1] - t[1][None], qc[2] - t[2][None]
        d2 = dx * dx + dy * dy + dz * dz
        m = d2.min(dim=1).values
        at = d2 == m[:, None]
        out_pix.append(torch.where(at, pix[None], torch.full_like(d2, 0, dtype=torch.int64) + big).min(dim=1).values)
        out_d2.append(m)
        out_ties.append(at.sum(dim=1))
    if not out_pix:
        e = torch.zeros(0, dtype=torch.int64, device=t.device)
        return e, e.double(), e
    return torch.cat(out_pix), torch.cat(out_d2), torch.cat(out_ties)
