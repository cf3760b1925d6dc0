"""Batched geometry of the DeLORA training step on MI355X: thin torch wrappers over the C ABI.

Every function takes/returns CUDA(HIP) tensors, allocates outputs with torch's caching allocator,
passes raw device pointers plus torch's *current stream* to libdelora_hip.so, and never
synchronises.  Layouts are those of include/delora_hip.h: planar fp32 range images
``[S,4,H,W]`` (x,y,z,range) and normals ``[S,3,H,W]`` for everything that is streamed, packed
``[S,H,W,4]`` twins ((x,y,z,range) / (nx,ny,nz,0)) for everything that is gathered from, int32 pixel maps.
"""
import ctypes

import torch

from . import _lib

LOSS_POINT_TO_POINT, LOSS_POINT_TO_PLANE, LOSS_PLANE_TO_PLANE, LOSS_NORMAL_LINEAR, LOSS_PO2PO_ALONE = 1, 2, 4, 8, 16


class Sensor:
    """Projection parameters of one dataset, resolved once from the reference's flat config
    (``config[dataset]["vertical_cells"|"horizontal_cells"|"vertical_field_of_view"]`` and
    ``config["horizontal_field_of_view"]``, radians; reference src/utility/projection.py:16,50-52)."""

    def __init__(self, height, width, vfov, hfov):
        self.H, self.W = int(height), int(width)
        self.vfov = (float(vfov[0]), float(vfov[1]))
        self.hfov = (float(hfov[0]), float(hfov[1]))
        self.struct = _lib.SensorStruct(self.H, self.W, self.hfov[0], self.hfov[1], self.vfov[0], self.vfov[1])

    @classmethod
    def from_config(cls, config, dataset):
        d = config[dataset]
        return cls(d["vertical_cells"], d["horizontal_cells"], d["vertical_field_of_view"],
                   config["horizontal_field_of_view"])

    def key(self):
        return (self.H, self.W, self.vfov, self.hfov)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.DeloraHipError("delora_amd geometry needs tensors on the GPU (no CPU implementation)")


def _planar(t, channels):
    """(data_ptr tensor, scan stride) of a ``[S,channels,H,W]`` tensor whose inner three dims are dense."""
    S, C, H, W = t.shape
    if C < channels or t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or t.dtype != torch.float32:
        raise ValueError(f"expected planar fp32 [S,>={channels},H,W] with dense inner dims, got {tuple(t.shape)} / {t.stride()}")
    return t, t.stride(0)


def project(points, offsets, max_points, sensor, want_uv=False, want_kept=True, want_packed=True, rotations=None):
    """Range images of S scans.  points ``[C,sumN]`` fp32 (rows 0..2 = xyz), offsets ``[S+1]`` int32 (device).
    ``rotations``: None, or ``[S,9]`` / ``[S,3,3]`` fp32 on the device -- scan s is projected as R_s p (stored normals as R_s n) inside
    the vote (``dl_project_rotated``); an identity row leaves its scan bit-identical, ``points`` is never written.
    Returns dict(image4 [S,4,H,W], aux [S,C-3,H,W]|None, packed [S,H,W,4]|None, packed_aux [S,H,W,4]|None (C >= 6: the
    stored normals), pix2pt [S,H,W] int32, kept [S] int32|None, uv [3,sumN]|None = u, v and range of every point)."""
    lib = _lib.load()
    _require_cuda(points, offsets)
    if points.dtype != torch.float32 or points.dim() != 2 or points.stride(1) != 1:
        raise ValueError("points must be fp32 [C,sumN] with unit inner stride")
    if offsets.dtype != torch.int32:
        raise ValueError("offsets must be int32")
    C, S = points.shape[0], offsets.numel() - 1
    H, W, dev = sensor.H, sensor.W, points.device
    image4 = torch.empty((S, 4, H, W), dtype=torch.float32, device=dev)
    aux = torch.empty((S, C - 3, H, W), dtype=torch.float32, device=dev) if C > 3 else None
    packed = torch.empty((S, H, W, 4), dtype=torch.float32, device=dev) if want_packed else None
    packed_aux = torch.empty((S, H, W, 4), dtype=torch.float32, device=dev) if (want_packed and C >= 6) else None
    pix2pt = torch.empty((S, H, W), dtype=torch.int32, device=dev)
    kept = torch.empty((S,), dtype=torch.int32, device=dev) if want_kept else None
    n_cols = points.shape[1]
    ws = torch.empty((lib.dl_project_workspace_bytes(S, H, W, n_cols, C) // 8,), dtype=torch.int64, device=dev)
    uv = torch.empty((3, points.shape[1]), dtype=torch.float32, device=dev) if want_uv else None
    if uv is not None and points.stride(0) != uv.stride(0):
        raise ValueError("want_uv needs a dense points buffer")
    if rotations is None:
        _lib.check(lib.dl_project(_ptr(points), points.stride(0), n_cols, _ptr(offsets), S, C, int(max_points),
                                  ctypes.byref(sensor.struct), _ptr(image4), _ptr(aux), _ptr(packed), _ptr(packed_aux),
                                  _ptr(pix2pt), _ptr(ws), _ptr(kept), _ptr(uv), _stream()), "dl_project")
    else:
        _require_cuda(rotations)
        if rotations.dtype != torch.float32 or rotations.numel() != 9 * S or not rotations.is_contiguous():
            raise ValueError(f"rotations must be contiguous fp32 [S,9] with S = {S}, got {tuple(rotations.shape)}")
        _lib.check(lib.dl_project_rotated(_ptr(points), points.stride(0), n_cols, _ptr(offsets), S, C, int(max_points),
                                          ctypes.byref(sensor.struct), _ptr(image4), _ptr(aux), _ptr(packed), _ptr(packed_aux),
                                          _ptr(pix2pt), _ptr(ws), _ptr(kept), _ptr(uv), _ptr(rotations), _stream()), "dl_project_rotated")
    return {"image4": image4, "aux": aux, "packed": packed, "packed_aux": packed_aux, "pix2pt": pix2pt, "kept": kept,
            "uv": uv}


def rotations_from_draws(draws, only_yaw, magnitude_rad):
    """The rotations of one augmented training step (``dl_rotations_from_draws``): draws ``[B,4]`` fp32 uniform in [0, 1) on the device
    (0..2 the direction, 3 the angle) -> ``[2B,9]`` fp32: row 2b the exact identity (scan 1), row 2b+1 Rodrigues' matrix of the axis
    ((0, 0, 1) when ``only_yaw``, else the normalised draws) and the angle (u - 0.5) * ``magnitude_rad``.  One launch, no host sync."""
    lib = _lib.load()
    _require_cuda(draws)
    if draws.dtype != torch.float32 or draws.dim() != 2 or draws.shape[1] != 4 or not draws.is_contiguous():
        raise ValueError("draws must be contiguous fp32 [B,4]")
    B = draws.shape[0]
    rot = torch.empty((2 * B, 9), dtype=torch.float32, device=draws.device)
    _lib.check(lib.dl_rotations_from_draws(_ptr(draws), B, 1 if only_yaw else 0, float(magnitude_rad), _ptr(rot), _stream()),
               "dl_rotations_from_draws")
    return rot


def record_layout(point_step, offsets, filter=0, min_range=0.0):
    """A ``_lib.RecordLayout``: fp32 x, y, z at byte ``offsets`` of ``point_step``-byte records; ``filter`` = ``_lib.RECORDS_*`` bits."""
    ox, oy, oz = (int(o) for o in offsets)
    return _lib.RecordLayout(int(point_step), ox, oy, oz, int(filter), float(min_range))


def project_records(records, offsets, max_points, sensor, layout, want_kept=True, want_packed=True):
    """Range images of S scans given as raw point records (``dl_project_records``), the layout's filter applied inside the vote.
    records: 1-D ``uint8`` or ``float32`` CUDA tensor holding whole records; offsets ``[S+1]`` int32 (device), in records.
    Returns the dict of ``project`` (aux / packed_aux / uv None; pix2pt holds RECORD indices) plus n_pass ``[S]`` int32: the records
    that took part."""
    lib = _lib.load()
    _require_cuda(records, offsets)
    if records.dtype not in (torch.uint8, torch.float32) or records.dim() != 1 or not records.is_contiguous():
        raise ValueError("records must be a contiguous 1-D uint8 or float32 tensor")
    if offsets.dtype != torch.int32:
        raise ValueError("offsets must be int32")
    nbytes = records.numel() * records.element_size()
    if layout.point_step <= 0 or nbytes % layout.point_step:
        raise ValueError(f"{nbytes} bytes are not whole records of {layout.point_step} bytes")
    S, H, W, dev = offsets.numel() - 1, sensor.H, sensor.W, records.device
    image4 = torch.empty((S, 4, H, W), dtype=torch.float32, device=dev)
    packed = torch.empty((S, H, W, 4), dtype=torch.float32, device=dev) if want_packed else None
    pix2pt = torch.empty((S, H, W), dtype=torch.int32, device=dev)
    kept = torch.empty((S,), dtype=torch.int32, device=dev) if want_kept else None
    n_pass = torch.empty((S,), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.dl_project_records_workspace_bytes(S, H, W) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.dl_project_records(_ptr(records), nbytes // layout.point_step, ctypes.byref(layout), _ptr(offsets), S, int(max_points),
                                      ctypes.byref(sensor.struct), _ptr(image4), _ptr(packed), _ptr(pix2pt), _ptr(ws), _ptr(kept),
                                      _ptr(n_pass), _stream()), "dl_project_records")
    return {"image4": image4, "aux": None, "packed": packed, "packed_aux": None, "pix2pt": pix2pt, "kept": kept, "uv": None,
            "n_pass": n_pass}


def normals(image4, half_rows=3,half_cols=5, epsilon_range=0.5, min_neighbors=10, want_packed=False):
    """Normals ``[S,3,H,W]`` of range images ``[S,>=3,H,W]`` (zero vector = no normal); with ``want_packed`` also the
    packed twin ``[S,H,W,4]`` -> (planar, packed)."""
    lib = _lib.load()
    _require_cuda(image4)
    t, ss = _planar(image4, 3)
    S, _, H, W = t.shape
    out = torch.empty((S, 3, H, W), dtype=torch.float32, device=t.device)
    pk = torch.empty((S, H, W, 4), dtype=torch.float32, device=t.device) if want_packed else None
    _lib.check(lib.dl_normals(_ptr(t), ss, S, H, W, int(half_rows), int(half_cols), float(epsilon_range),
                              int(min_neighbors), _ptr(out), _ptr(pk), _stream()), "dl_normals")
    return (out, pk) if want_packed else out


def pack_image(planar):
    """Packed twin ``[S,H,W,4]`` of a planar ``[S,3|4,H,W]`` tensor (torch ops; for callers that did not get it from
    project()/normals())."""
    S, C, H, W = planar.shape
    out = torch.zeros((S, H, W, 4), dtype=torch.float32, device=planar.device)
    out[..., :min(C, 4)] = planar[:, :4].permute(0, 2, 3, 1)
    return out


def _packed(t):
    S, H, W, C = t.shape
    if C != 4 or t.stride(3) != 1 or t.stride(2) != 4 or t.stride(1) != 4 * W or t.dtype != torch.float32:
        raise ValueError(f"expected packed fp32 [S,H,W,4] with dense inner dims, got {tuple(t.shape)} / {t.stride()}")
    return t, t.stride(0)


def nn_workspace_bytes(B, H, W):
    """Size of the exact search's workspace for B images of H x W pixels."""
    return int(_lib.load().dl_nn_workspace_bytes(int(B), int(H), int(W)))


def nn_correspond(src_image4, src_normals, tgt_packed, tgt_normals_packed, T, sensor, need_without_normals=False,
                  want_visible=True, want_match=True, workspace=None):
    """Exact nearest target pixel of every transformed source point (source planar, target packed ``[B,H,W,4]``).
    Returns (nn_pix [B,H,W] int32, visible [B]|None, match [B,6,H,W]|None): ``match`` holds, per SOURCE pixel, the matched
    target point (planes 0..2) and normal (planes 3..5) -- the operand stream of icp_loss().
    ``workspace``: an optional caller-owned int64 device tensor of at least nn_workspace_bytes(B, H, W) bytes; the search's
    work lists and their counters are left in it (tests read them to see which regime served a query)."""
    lib = _lib.load()
    _require_cuda(src_image4, tgt_packed, T)
    s, s_ss = _planar(src_image4, 3)
    t, t_ss = _packed(tgt_packed)
    tn, tn_ss = _packed(tgt_normals_packed) if tgt_normals_packed is not None else (None, 0)
    n, n_ss = _planar(src_normals, 3) if src_normals is not None else (None, 0)
    B, H, W = s.shape[0], sensor.H, sensor.W
    Tc = T.detach().contiguous().float()
    nn = torch.empty((B, H, W), dtype=torch.int32, device=s.device)
    match = torch.empty((B, 6, H, W), dtype=torch.float32, device=s.device) if want_match else None
    vis = torch.empty((B,), dtype=torch.int32, device=s.device) if want_visible else None
    if workspace is None:
        ws = torch.empty((lib.dl_nn_workspace_bytes(B, H, W) // 8 + 1,), dtype=torch.int64, device=s.device)
    else:
        ws = workspace
        if ws.dtype != torch.int64 or ws.device != s.device or not ws.is_contiguous() or ws.numel() * 8 < lib.dl_nn_workspace_bytes(B, H, W):
            raise ValueError(f"workspace must be a contiguous int64 tensor on {s.device} of at least nn_workspace_bytes({B}, {H}, {W}) bytes")
    _lib.check(lib.dl_nn_correspond(_ptr(s), s_ss, _ptr(n), n_ss, _ptr(t), t_ss, _ptr(tn), tn_ss, _ptr(Tc), B,
                                    ctypes.byref(sensor.struct), int(bool(need_without_normals)), _ptr(nn),
                                    _ptr(match), _ptr(vis), _ptr(ws), _stream()), "dl_nn_correspond")
    return nn, vis, match


def reproject(src_image4, T, sensor, src_normals=None, match=None, nn_pix=None, want_paired=True, want_src_pix=True):
    """Range images of the TRANSFORMED source image (dl_reproject): the pictures of a logged step.  ``src_image4 [B,>=3,H,W]``
    planar, ``T [B,4,4]``; ``src_normals [B,3,H,W]``, ``match [B,6,H,W]`` and ``nn_pix [B,H,W]`` (from nn_correspond) are given
    together or not at all.  Returns (moved4 [B,4,H,W], paired9 [B,9,H,W]|None, src_pix [B,2,H,W] int32|None)."""
    lib = _lib.load()
    _require_cuda(src_image4, T, src_normals, match, nn_pix)
    s, s_ss = _planar(src_image4, 3)
    given = [t is not None for t in (src_normals, match, nn_pix)]
    if any(given) and not all(given):
        raise ValueError("src_normals, match and nn_pix are given together or not at all")
    n, n_ss = _planar(src_normals, 3) if given[0] else (None, 0)
    mt, mt_ss = _planar(match, 6) if given[1] else (None, 0)
    if given[2] and (nn_pix.dtype != torch.int32 or not nn_pix.is_contiguous()):
        raise ValueError("nn_pix must be a contiguous int32 [B,H,W] tensor")
    B, H, W, dev = s.shape[0], sensor.H, sensor.W, s.device
    if tuple(s.shape[2:]) != (H, W):
        raise ValueError(f"the image is {tuple(s.shape[2:])}, the sensor {(H, W)}")
    Tc = T.detach().contiguous().float()
    moved4 = torch.empty((B, 4, H, W), dtype=torch.float32, device=dev)
    paired9 = torch.empty((B, 9, H, W), dtype=torch.float32, device=dev) if (want_paired and all(given)) else None
    src_pix = torch.empty((B, 2, H, W), dtype=torch.int32, device=dev) if want_src_pix else None
    ws = torch.empty((lib.dl_reproject_workspace_bytes(B, H, W) // 8,), dtype=torch.int64, device=dev)
    _lib.check(lib.dl_reproject(_ptr(s), s_ss, _ptr(n), n_ss, _ptr(mt), mt_ss, _ptr(nn_pix), _ptr(Tc), B,
                                ctypes.byref(sensor.struct), _ptr(moved4), _ptr(paired9), _ptr(src_pix), _ptr(ws), _stream()),
               "dl_reproject")
    return moved4, paired9, src_pix


# bench.py sets this to a callable returning a fresh timer handle (LossTimers.new): the streaming loss kernel of every
# training step is then launched with its own begin/end timestamps attached, so that its duration can be measured
# inside real steps (dl_icp_loss_partial_timed)
LOSS_TIMER_FACTORY = None


class LossTimers:
    """A pool of dl_timer handles; ``new()`` hands one to each launch, ``elapsed_ms()`` reads them all back."""

    def __init__(self, reserve=0):
        """``reserve`` timers are created up front: creating the HIP events of a timer while the stream is busy costs the host
        milliseconds (measured: a 5 ms autocast step became a 10.6 ms step with one timer created per step)."""
        self.lib = _lib.load()
        self.handles = []
        self.used = 0
        for _ in range(int(reserve)):
            self._create()

    def _create(self):
        h = ctypes.c_void_p()
        _lib.check(self.lib.dl_timer_create(ctypes.byref(h)), "dl_timer_create")
        self.handles.append(h)

    def new(self):
        if self.used == len(self.handles):
            self._create()
        self.used += 1
        return self.handles[self.used - 1]

    def elapsed_ms(self):
        out = []
        for h in self.handles[:self.used]:
            ms = ctypes.c_float()
            _lib.check(self.lib.dl_timer_elapsed_ms(h, ctypes.byref(ms)), "dl_timer_elapsed_ms")
            out.append(ms.value)
        return out

    def close(self):
        for h in self.handles:
            self.lib.dl_timer_destroy(h)
        self.handles = []
        self.used = 0


class _IcpLoss(torch.autograd.Function):
    """loss_terms[B,3] = (po2po, po2pl, pl2pl) as a differentiable function of T[B,4,4]; the
    correspondences are constants, exactly as the gather indices are in the reference."""

    @staticmethod
    def forward(ctx, T, src_image4, src_normals, match, nn_pix, flags):
        lib = _lib.load()
        s, s_ss = _planar(src_image4, 3)
        sn, sn_ss = _planar(src_normals, 3)
        mt, mt_ss = _planar(match, 6)
        B, _, H, W = s.shape
        dev = s.device
        Tc = T.detach().contiguous().float()
        loss_terms = torch.empty((B, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((B, 2), dtype=torch.int32, device=dev)
        grad_terms = torch.empty((B, 3, 12), dtype=torch.float32, device=dev)
        ws = torch.empty((lib.dl_icp_loss_workspace_bytes(B, H, W) // 4,), dtype=torch.float32, device=dev)
        if LOSS_TIMER_FACTORY is None:
            _lib.check(lib.dl_icp_loss_partial(_ptr(s), s_ss, _ptr(sn), sn_ss, _ptr(mt), mt_ss, _ptr(nn_pix), _ptr(Tc),
                                               B, H, W, int(flags), _ptr(ws), _stream()), "dl_icp_loss_partial")
        else:                                                           # bench.py: the same launch with timestamps attached
            _lib.check(lib.dl_icp_loss_partial_timed(_ptr(s), s_ss, _ptr(sn), sn_ss, _ptr(mt), mt_ss, _ptr(nn_pix), _ptr(Tc),
                                                     B, H, W, int(flags), _ptr(ws), LOSS_TIMER_FACTORY(), _stream()),
                       "dl_icp_loss_partial_timed")
        _lib.check(lib.dl_icp_loss_reduce(_ptr(ws), B, H, W, int(flags), _ptr(loss_terms), _ptr(counts),
                                          _ptr(grad_terms), _stream()), "dl_icp_loss_reduce")
        ctx.save_for_backward(grad_terms)
        ctx.mark_non_differentiable(counts)
        return loss_terms, counts

    @staticmethod
    def backward(ctx, g_terms, _g_counts):
        lib = _lib.load()
        (grad_terms,) = ctx.saved_tensors
        B = grad_terms.shape[0]
        g = g_terms.contiguous().float()
        grad_T = torch.empty((B, 4, 4), dtype=torch.float32, device=g.device)
        _lib.check(lib.dl_icp_loss_bwd(_ptr(grad_terms), _ptr(g), B, _ptr(grad_T), _stream()), "dl_icp_loss_bwd")
        return grad_T, None, None, None, None, None


def icp_loss(T, src_image4, src_normals, match, nn_pix, flags):
    """(loss_terms [B,3], pair_counts [B,2]); loss_terms is differentiable with respect to T.  Source planes
    ``[B,>=3,H,W]`` / ``[B,3,H,W]``, ``match`` ``[B,6,H,W]`` and ``nn_pix`` from nn_correspond()."""
    _require_cuda(T, src_image4, src_normals, match, nn_pix)
    return _IcpLoss.apply(T, src_image4, src_normals, match, nn_pix, flags)


def icp_information(T, src_image4, src_normals, match, nn_pix, workspace=None):
    """Point-to-plane normal equations of the matched pairs at the pose ``T [B,4,4]`` (``dl_icp_information``): the operands of
    ``icp_loss``.  Returns a dict of float64 tensors: ``information [B,6,6]`` = sum J J^T and ``rhs [B,6]`` = sum J r with
    J = (n, q x n) -- a left perturbation, translation first --, ``sum_r2 [B]``, ``pairs [B]``, ``covariance [B,6,6]`` =
    sum_r2 / (pairs - 6) * information^-1 (zeros unless status is 0) and ``status [B]`` int32 (``_lib.INFO_*``).  Nothing is refined:
    T is only read.  ``workspace``: an optional caller-owned fp32 device tensor of ``dl_icp_information_workspace_bytes`` bytes."""
    lib = _lib.load()
    _require_cuda(T, src_image4, src_normals, match, nn_pix)
    s, s_ss = _planar(src_image4, 3)
    sn, sn_ss = _planar(src_normals, 3)
    mt, mt_ss = _planar(match, 6)
    if nn_pix.dtype != torch.int32 or not nn_pix.is_contiguous():
        raise ValueError("nn_pix must be a contiguous int32 [B,H,W] tensor")
    B, _, H, W = s.shape
    dev = s.device
    Tc = T.detach().contiguous().float()
    info = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    rhs = torch.empty((B, 6), dtype=torch.float64, device=dev)
    stats = torch.empty((B, 2), dtype=torch.float64, device=dev)
    cov = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    need = int(lib.dl_icp_information_workspace_bytes(B, H, W))
    if not need:
        raise _lib.DeloraHipError((lib.dl_last_error() or b"").decode())
    ws = workspace if workspace is not None else torch.empty((need // 4,), dtype=torch.float32, device=dev)
    if ws.numel() * ws.element_size() < need or not ws.is_contiguous():
        raise ValueError(f"workspace needs {need} contiguous bytes")
    _lib.check(lib.dl_icp_information(_ptr(s), s_ss, _ptr(sn), sn_ss, _ptr(mt), mt_ss, _ptr(nn_pix), _ptr(Tc), B, H, W, _ptr(info), _ptr(rhs),
                                      _ptr(stats), _ptr(cov), _ptr(status), _ptr(ws), _stream()), "dl_icp_information")
    return {"information": info, "rhs": rhs, "sum_r2": stats[:, 0], "pairs": stats[:, 1], "covariance": cov, "status": status}


def loss_flags(config):
    """Flag word of dl_icp_loss_fwd from the reference's hyper-parameters (config/hyperparameters.yaml:14-19).

    ``po2po_alone`` (src/losses/icp_losses.py:36-45) pairs EVERY source point with its nearest target and keeps the
    point-to-point term only; the reference defines no pair lists for the normal-based terms in that branch and dies
    with an UnboundLocalError when one of them is enabled as well (:135-146) -- made explicit here."""
    f = 0
    if config.get("po2po_alone", False):
        if config["point_to_plane_loss"] or config["plane_to_plane_loss"]:
            raise Exception("po2po_alone needs point_to_plane_loss and plane_to_plane_loss switched off "
                            "(the reference fails for this combination, icp_losses.py:36-45,135-146).")
        f |= LOSS_PO2PO_ALONE
    if config["point_to_point_loss"]:
        f |= LOSS_POINT_TO_POINT
    if config["point_to_plane_loss"]:
        f |= LOSS_POINT_TO_PLANE
    if config["plane_to_plane_loss"]:
        f |= LOSS_PLANE_TO_PLANE
    if config["normal_loss"] == "linear":
        f |= LOSS_NORMAL_LINEAR
    elif config["normal_loss"] != "squared":
        raise Exception("The normal loss which is defined here is not admissible.")
    return f


def need_without_normals(config):
    """Whether the search must also answer source points WITHOUT a normal: the point-to-point term uses them
    (icp_losses.py:85-100), and po2po_alone uses every source point (:36-45)."""
    return bool(config["point_to_point_loss"]) or bool(config.get("po2po_alone", False))


def nn_bruteforce(src, tgt):
    """Exact NN index into ``tgt [3,Mt]`` for every column of ``src [3,Ms]`` (free-form lists)."""
    lib = _lib.load()
    _require_cuda(src, tgt)
    src, tgt = src.detach().contiguous().float(), tgt.detach().contiguous().float()
    Ms, Mt = src.shape[1], tgt.shape[1]
    nn = torch.empty((Ms,), dtype=torch.int32, device=src.device)
    _lib.check(lib.dl_nn_bruteforce(_ptr(src), max(Ms, 1), Ms, _ptr(tgt), max(Mt, 1), Mt, _ptr(nn), _stream()),
               "dl_nn_bruteforce")
    return nn


def _list(t):
    """Dense fp32 ``[3,M]`` view of a point list (a view into a larger tensor keeps its column stride)."""
    t = t.detach()
    if t.dim() != 2 or t.shape[0] != 3:
        raise ValueError(f"expected a [3,M] point list, got {tuple(t.shape)}")
    if t.dtype != torch.float32 or (t.shape[1] > 0 and (t.stride(1) != 1 or t.stride(0) < t.shape[1])):
        t = t.contiguous().float()
    return t, (t.stride(0) if t.shape[1] > 0 else 1)


class PointTree:
    """Exact nearest-neighbour tree over a free-form target list ``tgt [3,Mt]`` (dl_nn_list_build): what the reference builds
    with ``scipy.spatial.cKDTree``.  ``query(src [3,Ms])`` returns the int32 index of the nearest target for every column, the
    same index ``nn_bruteforce`` returns (lowest index among exact ties, -1 where there is no finite answer).  The tree owns its
    buffer and a reference to the target tensor; build and queries run on the current stream."""

    def __init__(self, tgt):
        lib = _lib.load()
        _require_cuda(tgt)
        self.tgt, self._cs = _list(tgt)
        self.Mt = int(self.tgt.shape[1])
        self.device = self.tgt.device
        self._tree = torch.empty((lib.dl_nn_list_tree_bytes(self.Mt),), dtype=torch.uint8, device=self.device)
        self._ws = None
        self.rebuild()

    def rebuild(self):
        """Build again from the current contents of the target tensor, into the same buffer (a target list refreshed in place,
        e.g. between replays of a captured graph)."""
        _lib.check(_lib.load().dl_nn_list_build(_ptr(self.tgt), self._cs, self.Mt, _ptr(self._tree), _stream()), "dl_nn_list_build")
        return self

    def query(self, src, out=None):
        lib = _lib.load()
        _require_cuda(src)
        src, cs = _list(src)
        if src.device != self.device:
            raise ValueError(f"PointTree on {self.device} queried with points on {src.device}")
        Ms = int(src.shape[1])
        nn = out if out is not None else torch.empty((Ms,), dtype=torch.int32, device=self.device)
        if nn.dtype != torch.int32 or nn.shape != (Ms,) or not nn.is_contiguous() or nn.device != self.device:
            raise ValueError("out must be a contiguous int32 [Ms] tensor on the tree's device")
        need = lib.dl_nn_list_query_workspace_bytes(Ms)
        if self._ws is None or self._ws.numel() < need:          # kept between queries (stream-ordered reuse, as torch's own allocator)
            self._ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
        _lib.check(lib.dl_nn_list_query(_ptr(src), cs, Ms, _ptr(self.tgt), self._cs, self.Mt, _ptr(self._tree), _ptr(nn),
                                        _ptr(self._ws), _stream()), "dl_nn_list_query")
        return nn


def probe_stream_read(src_image4, src_normals, match, nn_pix):
    """Launch the read-only twin of the loss kernel on the same operands (measurement aid, see dl_probe_stream_read)."""
    lib = _lib.load()
    s, s_ss = _planar(src_image4, 3)
    sn, sn_ss = _planar(src_normals, 3)
    mt, mt_ss = _planar(match, 6)
    B, _, H, W = s.shape
    ws = torch.empty((lib.dl_icp_loss_workspace_bytes(B, H, W) // 4,), dtype=torch.float32, device=s.device)
    _lib.check(lib.dl_probe_stream_read(_ptr(s), s_ss, _ptr(sn), sn_ss, _ptr(mt), mt_ss, _ptr(nn_pix), B, H, W, _ptr(ws),
                                        _stream()), "dl_probe_stream_read")
