"""Inference through the C ABI alone: the pose network as ``dl_pose_net`` (include/delora_hip.h, csrc/infer.hip) and its weight file.

``NativePoseNet`` binds an ``OdometryModel`` to ``dl_pose_net_prepare`` / ``dl_pose_net_forward``: the parameters are viewed in place
(as ``ring_conv.weight_storage`` does), the Winograd-domain weights are produced once and the workspace is allocated once, so a
forward pass is ONE library call that allocates nothing but its three small outputs.  torch is only the allocator here; a C or C++
program does the same with ``hipMalloc`` (tools/odometry_demo.hip) from the file ``export_pose_net`` writes -- the counterpart of
the reference's scripts/convert_pytorch_models.py, which re-saves a checkpoint for its inference node.

Weight file (little-endian; INTEGRATION.md section C has the same description for non-Python readers):

    bytes 0..7    magic  b"DLPOSNET"
    bytes 8..11   uint32 format version (1)
    bytes 12..15  uint32 n = length of the JSON header in bytes
    bytes 16..    the JSON header (UTF-8), zero padding up to the next multiple of 256 = ``data_offset``
    data_offset.. ``data_bytes`` bytes of raw fp32 arrays, each starting at a multiple of 256 relative to ``data_offset``

    header = {"format": 1, "activation": "tanh" | "relu", "F": .., "R": .., "Hd": ..,
              "blocks": [{"cin": .., "cout": .., "stride": [sh, sw], "has_downsample": true | false}, ...],
              "sensor": {"H": .., "W": .., "hfov": [rad, rad], "vfov": [rad, rad]} | null,
              "data_offset": .., "data_bytes": ..,
              "arrays": {name: {"offset": bytes from data_offset, "shape": [...]}}}

Array names and layouts (the C layouts of ``dl_pose_net``): ``conv1_w`` [64][3][3][8]; ``blocks.<i>.w1`` [cout][3][3][cin], ``blocks.<i>.w2``
[cout][3][3][cout], ``blocks.<i>.wd`` [cout][1][1][cin]; ``heads.fc_w`` [R][F], ``heads.fc_b`` [R], ``heads.r1_w`` [Hd][R], ``heads.r1_b``,
``heads.r3_w`` [4][Hd], ``heads.r3_b``, ``heads.t1_w`` [Hd][R], ``heads.t1_b``, ``heads.t3_w`` [3][Hd], ``heads.t3_b``.
"""
import ctypes
import json
import struct

import numpy as np
import torch

from .. import _lib
from ..models import ring_conv

MAGIC = b"DLPOSNET"
FORMAT_VERSION = 1
ALIGN = 256
MAX_BATCH = 16
HEAD_NAMES = ("fc_w", "fc_b", "r1_w", "r1_b", "r3_w", "r3_b", "t1_w", "t1_b", "t3_w", "t3_b")


def _align(n):
    return (int(n) + ALIGN - 1) // ALIGN * ALIGN


def why_unsupported(model, H, W, B=1):
    """None when ``dl_pose_net`` serves this model on ``[B,8,H,W]`` inputs, else the reason (the C side's scope, restated on the
    model's config so that a caller hears it before anything is built)."""
    cfg = model.config
    if cfg.get("pre_feature_extraction"):
        return "pre_feature_extraction (the per-image feature tower) is not served by dl_pose_net"
    if cfg.get("use_single_mlp_at_output"):
        return "use_single_mlp_at_output is not served by dl_pose_net (two-MLP heads only)"
    if not 1 <= int(B) <= MAX_BATCH:
        return f"a batch of {B} is not served (1 <= B <= {MAX_BATCH})"
    resnet = model.resnet
    blocks, _ = resnet._trunk_blocks()
    C0 = resnet.conv1.out_channels
    if resnet.conv1.in_channels != 8 or C0 != 64 or any(cin % 64 or cout % 64 for (cin, cout, _, _) in blocks):
        return "narrow networks (factor_fewer_resnet_channels > 1) are not served by dl_pose_net: channel counts must be multiples of 64"
    if len(blocks) > _lib.POSE_NET_MAX_BLOCKS:
        return f"{len(blocks)} residual blocks are not served (at most {_lib.POSE_NET_MAX_BLOCKS})"
    if any(has_ds == (tuple(stride) == (1, 1)) or (not has_ds and cin != cout) for (cin, cout, stride, has_ds) in blocks):
        return "a 1x1 shortcut on a stride-1 block (or none on a strided one) is not served by dl_pose_net"
    if not ring_conv.stem_supported((B, 8, H, W), C0) or not ring_conv.supported((B, H, W // 4, C0), blocks):
        return f"a {H}x{W} image is not served (a width that is a multiple of 4, activations below 2^31 elements)"
    return None


def _head_tensors(model):
    fr, ft = model.fully_connected_rotation, model.fully_connected_translation
    return (model.resnet.fc.weight, model.resnet.fc.bias, fr[1].weight, fr[1].bias, fr[3].weight, fr[3].bias, ft[1].weight, ft[1].bias,
            ft[3].weight, ft[3].bias)


def _arrays(model):
    """name -> tensor in the C layout, views of the parameters wherever their memory already has that layout (conv1 keeps torch's default
    layout and is re-laid out; the trunk's weights are views after ``trunk_weights_channels_last``)."""
    out = {"conv1_w": ring_conv.weight_storage(model.resnet.conv1.weight.detach())}
    blocks, weights = model.resnet._trunk_blocks()
    wi = 0
    for i, (_, _, _, has_ds) in enumerate(blocks):
        out[f"blocks.{i}.w1"] = ring_conv.weight_storage(weights[wi].detach())
        out[f"blocks.{i}.w2"] = ring_conv.weight_storage(weights[wi + 1].detach())
        if has_ds:
            out[f"blocks.{i}.wd"] = ring_conv.weight_storage(weights[wi + 2].detach())
        wi += 3 if has_ds else 2
    for name, t in zip(HEAD_NAMES, _head_tensors(model)):
        out["heads." + name] = t.detach().contiguous()
    return blocks, out


def fill_pose_net(net, act, blocks, sizes, address):
    """Fill a ``_lib.PoseNet``: act 1 / 2, blocks = (cin, cout, stride, has_downsample) tuples, sizes = (F, R, Hd), ``address(name)`` = the
    device address of an array by its weight-file name."""
    net.act, net.n_blocks = int(act), len(blocks)
    net.conv1_w = address("conv1_w")
    for i, (cin, cout, stride, has_ds) in enumerate(blocks):
        b = net.blocks[i]
        b.cin, b.cout, b.stride_h, b.stride_w, b.has_downsample = int(cin), int(cout), int(stride[0]), int(stride[1]), int(bool(has_ds))
        b.w1, b.w2 = address(f"blocks.{i}.w1"), address(f"blocks.{i}.w2")
        b.wd = address(f"blocks.{i}.wd") if has_ds else None
    for name in HEAD_NAMES:
        setattr(net.heads, name, address("heads." + name))
    net.F, net.R, net.Hd = (int(v) for v in sizes)
    return net


class NativePoseNet(object):
    """An ``OdometryModel`` behind ``dl_pose_net_forward`` for inputs ``[B,4,H,W]`` + ``[B,4,H,W]``.

    The struct points INTO the model's parameters (conv1, whose parameter keeps torch's default layout, is the one copy): an in-place
    weight update is seen by the stem, the strided and 1x1 layers and the heads at the next forward pass, and by the Winograd layers
    after the next ``prepare()``.  ``prepared`` / ``workspace``: optional caller-owned fp32 / uint8 CUDA tensors of at least
    ``prepared_bytes`` / ``workspace_bytes`` bytes, 256-byte aligned (tests carve them out of a poisoned arena).

    ``dtype``: ``torch.bfloat16`` / ``torch.float16`` bind the half-precision family (``dl_pose_net_prepare_h`` / ``dl_pose_net_forward_h``):
    the trunk runs on the kernels of ``torch.autocast`` training, with EVERY trunk weight converted once by ``prepare()`` into
    ``prepared`` (a uint8 buffer of ``prepared_bytes``) -- the model's eval forward inside ``torch.autocast(dtype=...)``, bit for bit,
    without its per-call weight conversion.  Images, parameters and outputs stay fp32."""

    def __init__(self, model, B, H, W, prepared=None, workspace=None, own_workspace=True, dtype=torch.float32):
        if dtype != torch.float32 and dtype not in ring_conv.DTYPE_CODE:
            raise ValueError(f"NativePoseNet: dtype {dtype} is not served (torch.float32, torch.bfloat16, torch.float16)")
        self.dtype = dtype
        self.dtype_code = ring_conv.DTYPE_CODE.get(dtype, 0)         # (0 = DL_DTYPE_F32: the family without _h)
        self._h = ("_h", (self.dtype_code,)) if self.dtype_code else ("", ())
        why = why_unsupported(model, H, W, B)
        if why is not None:
            raise ValueError("NativePoseNet: " + why)
        self.lib = _lib.load()
        self.B, self.H, self.W = int(B), int(H), int(W)
        self.device = model.resnet.conv1.weight.device
        if self.device.type != "cuda":
            raise _lib.DeloraHipError("NativePoseNet needs the model on the GPU (no CPU implementation)")
        blocks, self._tensors = _arrays(model)                       # (kept: the struct holds raw addresses)
        act = ring_conv.ACT["relu" if model.config["activation_fct"] == "relu" else "tanh"]
        heads = _head_tensors(model)
        self.net = fill_pose_net(_lib.PoseNet(), act, blocks, (heads[0].shape[1], heads[0].shape[0], heads[2].shape[0]),
                                 lambda name: self._tensors[name].data_ptr())
        self._net_p = ctypes.cast(ctypes.pointer(self.net), ctypes.c_void_p)
        self.prepared_bytes = self._size("dl_pose_net_prepared_bytes")
        self.workspace_bytes = self._size("dl_pose_net_workspace_bytes")
        if prepared is None and self.dtype_code:
            prepared = torch.empty((self.prepared_bytes,), dtype=torch.uint8, device=self.device)
        self.prepared = prepared if prepared is not None else torch.empty((self.prepared_bytes // 4,), dtype=torch.float32, device=self.device)
        if workspace is None and own_workspace:
            workspace = torch.empty((self.workspace_bytes,), dtype=torch.uint8, device=self.device)
        self.workspace = workspace                                   # (None: ``forward`` is not used, the owner calls the library itself)
        for name, t, need in (("prepared", self.prepared, self.prepared_bytes), ("workspace", self.workspace, self.workspace_bytes)):
            if t is not None and (t.numel() * t.element_size() < need or not t.is_contiguous()):
                raise ValueError(f"NativePoseNet: {name} needs {need} contiguous bytes")
        self.prepare()

    def _size(self, fn):
        fn += self._h[0]
        n = int(getattr(self.lib, fn)(self._net_p, self.B, self.H, self.W, *self._h[1]))
        if not n:
            raise _lib.DeloraHipError(f"{fn}: {(self.lib.dl_last_error() or b'').decode()}")
        return n

    @staticmethod
    def supported(model, H, W, B=1):
        return why_unsupported(model, H, W, B) is None

    def prepare(self):
        """The Winograd-domain weights of the stride-1 3x3 layers -- in half precision: the converted weights of every trunk layer --
        from the parameters as they are NOW (one launch)."""
        fn = "dl_pose_net_prepare" + self._h[0]
        _lib.check(getattr(self.lib, fn)(self._net_p, self.B, self.H, self.W, *self._h[1], ring_conv._ptr(self.prepared), ring_conv._stream()), fn)

    def forward(self, image_prev, image_cur, out=None):
        """Two planar fp32 images ``[B,4,H,W]`` (dense inner dims, any scan stride) -> (translation [B,3], quaternion [B,4], T [B,4,4]);
        ``out``: those three as caller-owned contiguous fp32 tensors (nothing is allocated then)."""
        if self.workspace is None:
            raise _lib.DeloraHipError("NativePoseNet was built without a workspace")
        ptrs = []
        for t in (image_prev, image_cur):
            if (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (self.B, 4, self.H, self.W) or t.stride(3) != 1
                    or t.stride(2) != self.W or t.stride(1) != self.H * self.W):
                raise ValueError(f"expected planar fp32 CUDA [{self.B},4,{self.H},{self.W}] with dense inner dims, got {tuple(t.shape)} / {t.stride()}")
            ptrs += [ring_conv._ptr(t), t.stride(0) if self.B > 1 else 4 * self.H * self.W]
        if out is None:
            out = tuple(torch.empty((self.B,) + s, dtype=torch.float32, device=self.device) for s in ((3,), (4,), (4, 4)))
        translation, quaternion, T = out
        for t, s in zip(out, ((3,), (4,), (4, 4))):
            if not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (self.B,) + s or not t.is_contiguous():
                raise ValueError(f"out: expected contiguous fp32 CUDA {(self.B,) + s}, got {tuple(t.shape)}")
        fn = "dl_pose_net_forward" + self._h[0]
        _lib.check(getattr(self.lib, fn)(self._net_p, ring_conv._ptr(self.prepared), *ptrs, self.B, self.H, self.W, *self._h[1],
                                         ring_conv._ptr(self.workspace), ring_conv._ptr(translation), ring_conv._ptr(quaternion), ring_conv._ptr(T),
                                         ring_conv._stream()), fn)
        return translation, quaternion, T


class NativeOdometry(object):
    """``dl_odometry_push`` with its buffers: two ping-pong images, the offsets vector, the workspace (grown when a larger scan
    arrives) and the three outputs.  ``push(points [3,N])`` returns None for the first scan, then (translation [1,3], quaternion [1,4],
    T [1,4,4]) -- tensors that the next push overwrites.  ``image_t_1`` / ``image_t`` are the images of the last pair.
    ``push_records(records, layout)`` is the same from raw point records (``dl_odometry_push_records``); the two may be mixed.
    ``dtype``: as ``NativePoseNet`` (``torch.bfloat16`` / ``torch.float16``: ``dl_odometry_push_h`` / ``dl_odometry_push_records_h``).
    ``quality``: every push is followed by ``dl_odometry_quality`` with ``normal_params`` = (half_rows, half_cols, epsilon_range,
    min_neighbors), what ``NormalsComputer._params`` returns: the object owns the two ``dl_scan_geometry`` records beside the two
    images, and from the second scan on ``quality_out`` holds float64 device tensors ``information [6,6]``, ``rhs [6]``, ``stats [2]``
    (sum of squared residuals, pairs), ``covariance [6,6]`` and ``status [1]`` int32 of the last pair.  The first push fills the record
    of its image only.  The poses do not change by a bit."""

    def __init__(self, model, sensor, max_points=1 << 17, dtype=torch.float32, quality=False, normal_params=None):
        self.pose = NativePoseNet(model, 1, sensor.H, sensor.W, own_workspace=False, dtype=dtype)     # (the forward's workspace is the head of this one's)
        self._h = self.pose._h
        self.lib, self.sensor, dev = self.pose.lib, sensor, self.pose.device
        self.images = torch.zeros((2, 4, sensor.H, sensor.W), dtype=torch.float32, device=dev)
        self.offs = torch.zeros((2,), dtype=torch.int32, device=dev)
        self.translation = torch.empty((1, 3), dtype=torch.float32, device=dev)
        self.quaternion = torch.empty((1, 4), dtype=torch.float32, device=dev)
        self.T = torch.empty((1, 4, 4), dtype=torch.float32, device=dev)
        self.max_points, self.workspace = 0, None
        self._reserve(max_points)
        self.cur, self.count = 0, 0
        # push_records from the host: two alternating page-locked staging buffers with the event behind their last transfer, one device buffer
        self._stage, self._stage_np, self._stage_event, self._stage_next, self._records = [None, None], [None, None], [None, None], 0, None
        self.quality, self.quality_out = bool(quality), None
        if self.quality:
            if normal_params is None or len(normal_params) != 4:
                raise ValueError("NativeOdometry(quality=True) needs normal_params = (half_rows, half_cols, epsilon_range, min_neighbors)")
            self.normal_params = (int(normal_params[0]), int(normal_params[1]), float(normal_params[2]), int(normal_params[3]))
            H, W = sensor.H, sensor.W
            self.normals = torch.zeros((2, 3, H, W), dtype=torch.float32, device=dev)
            self.packed_images = torch.zeros((2, H, W, 4), dtype=torch.float32, device=dev)
            self.packed_normals = torch.zeros((2, H, W, 4), dtype=torch.float32, device=dev)
            self._records_geometry = [_lib.ScanGeometry(self.normals[i].data_ptr(), self.packed_images[i].data_ptr(), self.packed_normals[i].data_ptr())
                                      for i in range(2)]
            nbytes = int(self.lib.dl_odometry_quality_workspace_bytes(ctypes.byref(sensor.struct), H, W))
            if not nbytes:
                raise _lib.DeloraHipError(f"dl_odometry_quality_workspace_bytes: {(self.lib.dl_last_error() or b'').decode()}")
            self.quality_workspace = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            self._quality_buffers = {"information": torch.zeros((6, 6), dtype=torch.float64, device=dev), "rhs": torch.zeros((6,), dtype=torch.float64, device=dev),
                                     "stats": torch.zeros((2,), dtype=torch.float64, device=dev), "covariance": torch.zeros((6, 6), dtype=torch.float64, device=dev),
                                     "status": torch.zeros((1,), dtype=torch.int32, device=dev)}

    def _quality(self, prev):
        """``dl_odometry_quality`` on the pair the push has just served (``prev`` None: the first scan, the record alone)."""
        p, q = ring_conv._ptr, self._quality_buffers
        a, b, eps, min_n = self.normal_params
        geometry_prev = ctypes.byref(self._records_geometry[1 - self.cur]) if prev is not None else None
        _lib.check(self.lib.dl_odometry_quality(ctypes.byref(self.sensor.struct), p(prev), geometry_prev, p(self.images[self.cur]),
                                                ctypes.byref(self._records_geometry[self.cur]), p(self.T), a, b, eps, min_n, p(self.quality_workspace),
                                                p(q["information"]), p(q["rhs"]), p(q["stats"]), p(q["covariance"]), p(q["status"]),
                                                ring_conv._stream()), "dl_odometry_quality")
        self.quality_out = q if prev is not None else None

    def _reserve(self, n_points):
        if self.workspace is not None and n_points <= self.max_points:
            return
        self.max_points = max(int(n_points), 2 * self.max_points)
        fn = "dl_odometry_workspace_bytes" + self._h[0]
        nbytes = int(getattr(self.lib, fn)(self.pose._net_p, ctypes.byref(self.sensor.struct), self.max_points, self.sensor.H, self.sensor.W, *self._h[1]))
        if not nbytes:
            raise _lib.DeloraHipError(f"{fn}: {(self.lib.dl_last_error() or b'').decode()}")
        self.workspace = torch.empty((nbytes,), dtype=torch.uint8, device=self.pose.device)

    @property
    def image_t(self):
        return self.images[self.cur]

    @property
    def image_t_1(self):
        return self.images[1 - self.cur]

    def push(self, points):
        if not points.is_cuda or points.dtype != torch.float32 or points.dim() != 2 or points.shape[0] < 3 or points.stride(1) != 1:
            raise ValueError("points must be fp32 CUDA [>=3,N] with unit inner stride")
        n = int(points.shape[1])
        self._reserve(n)
        if self.count:
            self.cur = 1 - self.cur                                  # the swap of the two image buffers
        prev = self.images[1 - self.cur] if self.count else None
        p = ring_conv._ptr
        fn = "dl_odometry_push" + self._h[0]
        _lib.check(getattr(self.lib, fn)(self.pose._net_p, p(self.pose.prepared), ctypes.byref(self.sensor.struct), p(points), points.stride(0), n,
                                         p(self.offs), p(prev), p(self.images[self.cur]), *self._h[1], p(self.workspace), p(self.translation),
                                         p(self.quaternion), p(self.T), ring_conv._stream()), fn)
        if self.quality:
            self._quality(prev)
        self.count += 1
        return (self.translation, self.quaternion, self.T) if prev is not None else None

    def _upload(self, host):
        """The bytes of a contiguous host array -> the kept device buffer, through one of two alternating page-locked staging buffers:
        the host copy of message k+1 overlaps the transfer (and the push) of message k, and a staging buffer is overwritten only after
        the event behind its last transfer (a single reused pinned buffer once let the next message overwrite a transfer
        in flight).  Buffers grow on demand and are kept: nothing is allocated per push once they have grown."""
        flat = host.reshape(-1).view(np.uint8)
        n = int(flat.shape[0])
        k = self._stage_next
        self._stage_next = 1 - k
        if self._stage[k] is None or self._stage[k].numel() < n:
            if self._stage_event[k] is not None:
                self._stage_event[k].synchronize()
            self._stage[k] = torch.empty((max(n, 2 * (0 if self._stage[k] is None else self._stage[k].numel())),), dtype=torch.uint8, pin_memory=True)
            self._stage_np[k] = self._stage[k].numpy()
            self._stage_event[k] = torch.cuda.Event()
        else:
            self._stage_event[k].synchronize()
        if self._records is None or self._records.numel() < n:
            # (the old buffer goes back to the caching allocator, which keeps it for this stream's later work: stream-ordered reuse)
            self._records = torch.empty((max(n, 2 * (0 if self._records is None else self._records.numel())),), dtype=torch.uint8,
                                        device=self.pose.device)
        np.copyto(self._stage_np[k][:n], flat)
        self._records[:n].copy_(self._stage[k][:n], non_blocking=True)
        self._stage_event[k].record()
        return self._records, n

    def push_records(self, records, layout):
        """``push`` from raw point records (``dl_odometry_push_records``): ``layout`` is a ``_lib.RecordLayout``, filter included.
        records: a CUDA 1-D ``uint8`` / ``float32`` tensor goes to the library as it is; a contiguous host ``numpy`` array -- any dtype
        whose itemsize is ``point_step`` (a structured message), ``[N,C]`` fp32 with ``4*C == point_step``, or raw bytes -- is staged
        and copied asynchronously.  Nothing is filtered, compacted or transposed on the host."""
        why = why_layout_unsupported(layout)
        if why is not None:
            raise ValueError("push_records: " + why)
        if torch.is_tensor(records):
            if not records.is_cuda or records.dtype not in (torch.uint8, torch.float32) or records.dim() != 1 or not records.is_contiguous():
                raise ValueError("records must be a contiguous 1-D uint8 or float32 CUDA tensor (or a host numpy array)")
            buf, nbytes = records, records.numel() * records.element_size()
        else:
            if not isinstance(records, np.ndarray) or not records.flags.c_contiguous:
                raise ValueError("records must be a C-contiguous numpy array (or a CUDA tensor)")
            buf, nbytes = self._upload(records)
        if nbytes % layout.point_step:
            raise ValueError(f"{nbytes} bytes are not whole records of {layout.point_step} bytes")
        if self.count:
            self.cur = 1 - self.cur
        prev = self.images[1 - self.cur] if self.count else None
        p = ring_conv._ptr
        fn = "dl_odometry_push_records" + self._h[0]
        _lib.check(getattr(self.lib, fn)(self.pose._net_p, p(self.pose.prepared), ctypes.byref(self.sensor.struct), p(buf),
                                         nbytes // layout.point_step, ctypes.byref(layout), p(self.offs), p(prev), p(self.images[self.cur]),
                                         *self._h[1], p(self.workspace), p(self.translation), p(self.quaternion), p(self.T), ring_conv._stream()), fn)
        if self.quality:
            self._quality(prev)
        self.count += 1
        return (self.translation, self.quaternion, self.T) if prev is not None else None


def why_layout_unsupported(layout):
    """None when ``dl_project_records`` serves this ``_lib.RecordLayout``, else the reason (the C side's rule restated, so that a
    caller can choose the host route before anything is copied)."""
    step, offs = layout.point_step, (layout.off_x, layout.off_y, layout.off_z)
    if step % 4 or not 12 <= step <= 256:
        return f"point_step={step} is not a multiple of 4 in 12..256"
    if any(o < 0 or o % 4 or o + 4 > step for o in offs) or len(set(offs)) != 3:
        return f"offsets {offs} are not three distinct multiples of 4 inside a {step}-byte record"
    if layout.filter & _lib.RECORDS_MIN_RANGE and not np.isfinite(layout.min_range):
        return "min_range is not finite"
    return None


# ---------------------------------------------------------------------------------------------------------------------
def export_pose_net(model, path, sensor=None):
    """Write the model's weights as the flat file described at the top of this module; ``sensor``: a ``geometry.Sensor`` (or None).
    Works for a model on any device.  Returns the header."""
    why = why_unsupported(model, 4, 4)                               # (the smallest image: the file does not depend on the image size)
    if why is not None:
        raise ValueError("export_pose_net: " + why)
    blocks, tensors = _arrays(model)
    heads = _head_tensors(model)
    arrays, off, blobs = {}, 0, []
    for name, t in tensors.items():
        a = np.ascontiguousarray(t.detach().cpu().numpy().astype("<f4", copy=False))
        arrays[name] = {"offset": off, "shape": list(a.shape)}
        blobs.append((off, a))
        off = _align(off + a.nbytes)
    header = {"format": FORMAT_VERSION, "activation": "relu" if model.config["activation_fct"] == "relu" else "tanh",
              "F": int(heads[0].shape[1]), "R": int(heads[0].shape[0]), "Hd": int(heads[2].shape[0]),
              "blocks": [{"cin": int(cin), "cout": int(cout), "stride": [int(s[0]), int(s[1])], "has_downsample": bool(ds)} for (cin, cout, s, ds) in blocks],
              "sensor": None if sensor is None else {"H": sensor.H, "W": sensor.W, "hfov": list(sensor.hfov), "vfov": list(sensor.vfov)},
              "data_offset": 0, "data_bytes": off, "arrays": arrays}
    # the header names its own padded length: settle it with the widest plausible number, then pad the text to that length
    header["data_offset"] = _align(16 + len(json.dumps(header).encode()) + 16)
    text = json.dumps(header).encode()
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<II", FORMAT_VERSION, len(text)) + text)
        f.write(b"\0" * (header["data_offset"] - 16 - len(text)))
        pos = 0
        for o, a in blobs:
            f.write(b"\0" * (o - pos))
            f.write(a.tobytes())
            pos = o + a.nbytes
        f.write(b"\0" * (off - pos))
    return header


def load_pose_net_blob(path):
    """Read a weight file back: (header, {name: fp32 numpy array}).  A wrong magic, an unknown format version, a header that does not
    parse and a file shorter than its header announces are ``ValueError``."""
    with open(path, "rb") as f:
        raw = f.read()
    if len(raw) < 16 or raw[:8] != MAGIC:
        raise ValueError(f"{path}: not a pose-network weight file (magic {raw[:8]!r})")
    version, n = struct.unpack("<II", raw[8:16])
    if version != FORMAT_VERSION:
        raise ValueError(f"{path}: format version {version}, this reader knows {FORMAT_VERSION}")
    if len(raw) < 16 + n:
        raise ValueError(f"{path}: truncated inside the header ({len(raw)} bytes, the header ends at {16 + n})")
    try:
        header = json.loads(raw[16:16 + n].decode())
        base, nbytes = int(header["data_offset"]), int(header["data_bytes"])
        entries = {name: (int(e["offset"]), tuple(int(d) for d in e["shape"])) for name, e in header["arrays"].items()}
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError(f"{path}: the header does not parse: {e}") from e
    if base < 16 + n or base % ALIGN or len(raw) < base + nbytes:
        raise ValueError(f"{path}: truncated ({len(raw)} bytes, the header announces {base + nbytes})")
    arrays = {}
    for name, (off, shape) in entries.items():
        count = int(np.prod(shape, dtype=np.int64))
        if off % ALIGN or off < 0 or off + 4 * count > nbytes:
            raise ValueError(f"{path}: array {name} lies outside the data section")
        arrays[name] = np.frombuffer(raw, dtype="<f4", count=count, offset=base + off).reshape(shape).copy()
    return header, arrays
