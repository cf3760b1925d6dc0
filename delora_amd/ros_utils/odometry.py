"""Scan-to-scan odometry on a stream of raw LiDAR scans: the ROS-free core of the reference's inference node.

``ScanToScanOdometry`` is what ``OdometryPublisher.subscriber_callback`` / ``predict_and_publish`` do between receiving
a PointCloud2 message and filling the Odometry message (reference src/ros_utils/odometry_publisher.py:93-172), and
``TrajectoryIntegrator`` is ``OdometryIntegrator.update_transformation`` (src/ros_utils/odometry_integrator.py:79-93);
the ROS plumbing around them (publishers, TF, message conversion) is out of scope and not built.  Both scans of a pair are projected by ONE launch of the
HIP projection (``geometry.project``), the network runs on the stacked pair, nothing else touches the points.

``quaternion_from_matrix`` / ``quaternion_matrix`` restate the two ``tf.transformations`` functions the node calls
(:151, odometry_integrator.py:82,86; ROS ``tf`` is third party and absent here: restated from the published algorithm of
transformations.py as shipped with ROS tf, quaternions in (x, y, z, w) order; checked against scipy's Rotation in
tests/test_host_logic.py -- parity with the ROS package itself is unpinned).
"""
import math

import numpy as np
import torch

from .. import _lib, geometry
from ..models import model as model_module
from ..models import model_parts
from ..preprocessing.normal_computation import NormalsComputer


def quaternion_from_matrix(matrix):
    """(x, y, z, w) of the rotation part of a 4x4 homogeneous matrix (tf.transformations.quaternion_from_matrix)."""
    M = np.asarray(matrix, dtype=np.float64)[:4, :4]
    q = np.empty((4,), dtype=np.float64)
    t = np.trace(M)
    if t > M[3, 3]:
        q[3] = t
        q[2] = M[1, 0] - M[0, 1]
        q[1] = M[0, 2] - M[2, 0]
        q[0] = M[2, 1] - M[1, 2]
    else:
        i, j, k = 0, 1, 2
        if M[1, 1] > M[0, 0]:
            i, j, k = 1, 2, 0
        if M[2, 2] > M[i, i]:
            i, j, k = 2, 0, 1
        t = M[i, i] - (M[j, j] + M[k, k]) + M[3, 3]
        q[i] = t
        q[j] = M[i, j] + M[j, i]
        q[k] = M[k, i] + M[i, k]
        q[3] = M[k, j] - M[j, k]
    q *= 0.5 / math.sqrt(t * M[3, 3])
    return q


def quaternion_matrix(quaternion):
    """4x4 homogeneous rotation matrix of an (x, y, z, w) quaternion (tf.transformations.quaternion_matrix)."""
    q = np.array(quaternion[:4], dtype=np.float64, copy=True)
    nq = np.dot(q, q)
    if nq < np.finfo(float).eps * 4.0:
        return np.identity(4)
    q *= math.sqrt(2.0 / nq)
    q = np.outer(q, q)
    return np.array((
        (1.0 - q[1, 1] - q[2, 2], q[0, 1] - q[2, 3], q[0, 2] + q[1, 3], 0.0),
        (q[0, 1] + q[2, 3], 1.0 - q[0, 0] - q[2, 2], q[1, 2] - q[0, 3], 0.0),
        (q[0, 2] - q[1, 3], q[1, 2] + q[0, 3], 1.0 - q[0, 0] - q[1, 1], 0.0),
        (0.0, 0.0, 0.0, 1.0)), dtype=np.float64)


class TrajectoryIntegrator(object):
    """Accumulated sensor pose ``T_0_t`` as the product of the scan-to-scan transforms (odometry_integrator.py:45,79-86)."""

    def __init__(self):
        self.T_0_t = np.expand_dims(np.eye(4), axis=0)

    def update_transformation(self, quaternion, translation):
        T_t_1_t = np.zeros((1, 4, 4))
        T_t_1_t[0] = quaternion_matrix(quaternion)
        T_t_1_t[0, :3, 3] = translation
        self.T_0_t = np.matmul(self.T_0_t, T_t_1_t)
        return self.T_0_t[0, :3, 3].copy(), quaternion_from_matrix(self.T_0_t[0])


def filter_scans(scan):
    """``[1,C,N]`` numpy scan without the points that have an exactly-zero x, y or z or lie within 0.3 m of the sensor
    (odometry_publisher.py:93-102)."""
    scan = np.asarray(scan)
    xyz = scan[0, :3]
    keep = (xyz[0] != 0.0) & (xyz[1] != 0.0) & (xyz[2] != 0.0)
    keep &= np.linalg.norm(xyz, axis=0) > 0.3
    return scan[:, :, keep]


def record_layout(dtype_or_step, offsets=None, filter=_lib.RECORDS_DROP_ZERO | _lib.RECORDS_MIN_RANGE, min_range=0.3):
    """The ``_lib.RecordLayout`` of a message: a numpy structured dtype with fp32 fields ``x``, ``y``, ``z`` (what ``ros_numpy.numpify``
    returns for a PointCloud2: its itemsize is the message's point_step), or ``(point_step, (off_x, off_y, off_z))`` in bytes.  The
    default filter is the node's (odometry_publisher.py:95-97): exactly-zero coordinates and ranges within 0.3 m are dropped."""
    if offsets is None:
        dtype = np.dtype(dtype_or_step)
        if dtype.fields is None or any(name not in dtype.fields for name in "xyz"):
            raise ValueError(f"record_layout: {dtype} is not a structured dtype with fields x, y, z")
        for name in "xyz":
            if dtype.fields[name][0] != np.dtype("<f4"):
                raise ValueError(f"record_layout: field {name} is {dtype.fields[name][0]}, only little-endian float32 is served")
        dtype_or_step, offsets = dtype.itemsize, tuple(dtype.fields[name][1] for name in "xyz")
    return geometry.record_layout(dtype_or_step, offsets, filter, min_range)


def unpack_records(message, layout):
    """``[1,3,N]`` fp32 from a message's raw records on the host (any point_step and offsets, unaligned ones included)."""
    raw = np.ascontiguousarray(message).reshape(-1).view(np.uint8)
    if raw.size % layout.point_step:
        raise ValueError(f"{raw.size} bytes are not whole records of {layout.point_step} bytes")
    raw = raw.reshape(-1, layout.point_step)
    xyz = [np.ascontiguousarray(raw[:, o:o + 4]).view("<f4")[:, 0] for o in (layout.off_x, layout.off_y, layout.off_z)]
    return np.stack(xyz, axis=0)[None].astype(np.float32, copy=False)


def _project_pair_hip(previous, current, sensor):
    """Both scans through one launch of the HIP projection -> ``[2,4,H,W]`` (x, y, z, range)."""
    pts = torch.cat((previous[0, :3], current[0, :3]), dim=1).contiguous().float()
    n0, n1 = previous.shape[2], current.shape[2]
    offs = torch.tensor([0, n0, n0 + n1], dtype=torch.int32, device=pts.device)
    return geometry.project(pts, offs, max(n0, n1), sensor)["image4"]


class ScanToScanOdometry(object):
    """Feed raw scans with ``push``; from the second scan on every call returns the motion since the previous scan.

    config: the dict of ``bin/run_rosnode.py`` (the training config plus ``checkpoint``, ``datasets=[name]``,
    ``integrate_odometry``).  ``model`` / ``project_pair`` can be injected (tests run the core on the CPU with the
    oracle's projection); by default the model is built from the config and loaded from ``config["checkpoint"]`` and
    the projection is the HIP one.

    ``engine``: "torch" (default) runs the model's modules on the stacked pair; "native" drives ``dl_odometry_push`` (the torch-free
    C ABI of include/delora_hip.h, through ``deploy.native_infer.NativeOdometry``) with two ping-pong images -- the same kernels on the
    same operands, so the same numbers, for the configs that path serves: the 8-channel full-width network with two-MLP heads and no
    ``normalization_scaling``; anything else raises ``ValueError`` at construction.

    ``push_records`` takes a message as the driver delivers it (raw point records); on the native engine the node's filter runs inside
    the library's projection (``dl_odometry_push_records``) and the host never touches the points.

    ``precision``: "float32" (default), "bfloat16" or "float16" -- how a network trained under ``amp_dtype`` is served as it was trained.
    Engine "torch" wraps the model call in ``torch.autocast("cuda", dtype=...)`` and takes ``.float()`` of its outputs; engine "native"
    binds the half-precision family (``NativeOdometry(dtype=...)``: every trunk weight converted once).  ``config["amp_dtype"]`` is
    deliberately NOT read: a caller who passes a training config gets fp32, as ever.  ``config["amp_stem"]`` IS followed by engine
    "torch" in half precision (the model is built from the config: conv1 then runs on rounded operands as in training); engine "native"
    keeps conv1 in fp32 whatever the key says.

    ``quality=True``: every result dict gains how well the pair constrains the returned motion, from the point-to-plane normal equations
    of the matched pairs at that motion (``geometry.icp_information``; nothing is refined, the pose is the network's):
    ``covariance`` [6,6] float64, row-major (x, y, z, rot X, rot Y, rot Z) -- the layout of ``nav_msgs/Odometry.pose.covariance`` --, the
    covariance of the scan-to-scan transform under a left perturbation, in the previous scan's frame (zeros unless ``quality_status`` is
    0, which is what the reference publishes); ``information`` [6,6]; ``residual_rms`` = sqrt(sum r^2 / pairs); ``pairs``;
    ``quality_status`` (0 fine, 1 at most six pairs, 2 unobservable along some axis); ``information_eigenvalues`` [6], ascending, of the
    information matrix scaled to a unit diagonal (NaN where a diagonal entry is not positive).  Engine "torch" chains
    ``geometry.normals`` (both images, one launch), ``geometry.nn_correspond`` and ``geometry.icp_information``; engine "native" calls
    ``dl_odometry_quality`` -- the same kernels on the same operands.  The normal parameters are ``NormalsComputer._params`` of the config.
    Not served together with ``normalization_scaling`` (the clouds are rescaled per pair).  Propagating the covariance into the
    integrated pose ``T_0_t`` is left to the caller.  ``quality=False`` (default): today's keys, nothing new is launched."""

    PRECISIONS = {"float32": torch.float32, "bfloat16": torch.bfloat16, "float16": torch.float16}

    def __init__(self, config, model=None, project_pair=None, engine="torch", precision="float32", quality=False):
        if engine not in ("torch", "native"):
            raise ValueError(f"engine must be 'torch' or 'native', got {engine!r}")
        self.quality = bool(quality)
        if self.quality and config["normalization_scaling"]:
            raise ValueError("quality=True does not serve normalization_scaling: it rescales both clouds per pair, so the covariance would "
                             "not be in metres and the previous scan's normals could not be reused")
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be 'float32', 'bfloat16' or 'float16', got {precision!r}")
        self.precision, self.dtype = precision, self.PRECISIONS[precision]
        self.engine = engine
        self.config = config
        self.device = config["device"]
        self.dataset = config["datasets"][0]                       # "Assumes the dataset in config['datasets'][0]" (:26)
        self.sensor = geometry.Sensor.from_config(config, self.dataset)
        self.normal_params = NormalsComputer(config, self.dataset)._params() if self.quality else None
        if model is None:
            model = model_module.OdometryModel(config=config).to(self.device)
            if config.get("checkpoint"):
                state = torch.load(config["checkpoint"], map_location=self.device, weights_only=False)
                model.load_state_dict(state["model_state_dict"])
        self.model = model.eval()
        self.geometry_handler = model_parts.GeometryHandler(config=config)
        self.project_pair = project_pair if project_pair is not None else _project_pair_hip
        self.integrator = TrajectoryIntegrator() if config.get("integrate_odometry", True) else None
        self.scaling_factor = 1.0
        self.point_cloud_t_1 = None
        self.native = None
        if engine == "native":
            # scan -> pose through dl_odometry_push alone (include/delora_hip.h): only the new scan is projected, the Winograd-domain
            # weights are prepared once, nothing is allocated per push
            from ..deploy import native_infer
            if project_pair is not None:
                raise ValueError("engine 'native' projects inside the library: project_pair cannot be injected")
            if config["normalization_scaling"]:
                raise ValueError("engine 'native' does not serve normalization_scaling: it rescales both clouds per pair, so the previous "
                                 "scan's image cannot be reused")
            why = native_infer.why_unsupported(self.model, self.sensor.H, self.sensor.W)
            if why is not None:
                raise ValueError("engine 'native': " + why)
            self.native = native_infer.NativeOdometry(self.model, self.sensor, dtype=self.dtype, quality=self.quality, normal_params=self.normal_params)

    @staticmethod
    def _quality_result(information, sum_r2, pairs, covariance, status):
        """The quality keys of a result dict from the device outputs of one sample."""
        info = information.cpu().numpy().astype(np.float64).reshape(6, 6)
        sum_r2, pairs = float(sum_r2), float(pairs)
        d = np.diag(info)
        if np.all(np.isfinite(info)) and np.all(d > 0):
            s = 1.0 / np.sqrt(d)
            eig = np.linalg.eigvalsh((info * s[:, None]) * s[None, :])
        else:
            eig = np.full((6,), np.nan)
        return {"covariance": covariance.cpu().numpy().astype(np.float64).reshape(6, 6), "information": info,
                "residual_rms": math.sqrt(sum_r2 / pairs) if pairs > 0 and sum_r2 >= 0 else float("nan"), "pairs": int(pairs),
                "quality_status": int(status), "information_eigenvalues": eig}

    def _native_result(self, out):
        if out is None:
            return None
        result = self._result(out[2], out[0])
        if self.quality:
            q = self.native.quality_out
            result.update(self._quality_result(q["information"], q["stats"][0], q["stats"][1], q["covariance"], q["status"][0]))
        return result

    def _result(self, T, translation_1):
        """The returned dict from ``T [1,4,4]`` and ``translation [1,3]`` (odometry_publisher.py:151-172)."""
        quaternion = quaternion_from_matrix(T[0].double().cpu().numpy())
        translation = translation_1[0].double().cpu().numpy() * self.scaling_factor
        transformation = T[0].double().cpu().numpy().copy()
        transformation[:3, 3] = translation
        result = {"translation": translation, "quaternion": quaternion, "transformation": transformation}
        if self.integrator is not None:
            gt, gq = self.integrator.update_transformation(quaternion=quaternion, translation=translation)
            result.update(global_translation=gt, global_quaternion=gq, T_0_t=self.integrator.T_0_t[0].copy())
        return result

    def normalize_input(self, input_1, input_2):
        """Both clouds divided by the mean range over all their points, in place (odometry_publisher.py:104-113)."""
        mean_range = torch.mean(torch.cat((torch.norm(input_1, dim=1), torch.norm(input_2, dim=1)), dim=1))
        input_1 /= mean_range
        input_2 /= mean_range
        return float(mean_range)

    @torch.no_grad()
    def push(self, scan):
        """scan: ``[1,C>=3,N]`` (x, y, z first); a numpy array is filtered with ``filter_scans`` as the node does with every
        message, a tensor is taken as is.  Returns None for the first scan, then a dict with
        ``translation`` [3], ``quaternion`` (x,y,z,w), ``transformation`` [4,4] (previous -> current, metres) and, when
        integrating, ``global_translation`` / ``global_quaternion`` / ``T_0_t``."""
        if not torch.is_tensor(scan):
            scan = torch.from_numpy(filter_scans(np.asarray(scan, dtype=np.float32)))
        current = scan[:, :3].to(self.device).float().clone()
        result = None
        if self.native is not None:
            return self._native_result(self.native.push(current[0].contiguous()))     # (a filtered numpy scan arrives with transposed strides)
        if self.point_cloud_t_1 is not None:
            previous = self.point_cloud_t_1
            if self.config["normalization_scaling"]:
                self.scaling_factor = self.normalize_input(input_1=current, input_2=previous)
            images = self.project_pair(previous, current, self.sensor)
            stacked = torch.cat((images[0:1], images[1:2]), dim=1)                # image_1 = previous, image_2 = current (:143)
            if self.dtype == torch.float32:
                translation_1, rot_repr_1 = self.model(stacked)
            else:
                with torch.autocast("cuda", dtype=self.dtype):
                    translation_1, rot_repr_1 = self.model(stacked)
                translation_1, rot_repr_1 = translation_1.float(), rot_repr_1.float()
            T = self.geometry_handler.get_transformation_matrix_quaternion(
                translation=translation_1, quaternion=rot_repr_1, device=self.device)
            quaternion = quaternion_from_matrix(T[0].double().cpu().numpy())
            translation = translation_1[0].double().cpu().numpy() * self.scaling_factor
            transformation = T[0].double().cpu().numpy().copy()
            transformation[:3, 3] = translation
            result = {"translation": translation, "quaternion": quaternion, "transformation": transformation}
            if self.integrator is not None:
                gt, gq = self.integrator.update_transformation(quaternion=quaternion, translation=translation)
                result.update(global_translation=gt, global_quaternion=gq, T_0_t=self.integrator.T_0_t[0].copy())
            if self.quality:
                # source = the current scan, target = the previous one: the direction of T
                a, b, eps, min_n = self.normal_params
                nrm, nrm_packed = geometry.normals(images, a, b, eps, min_n, want_packed=True)
                nn_pix, _, match = geometry.nn_correspond(images[1:2], nrm[1:2], geometry.pack_image(images[0:1]), nrm_packed[0:1], T, self.sensor,
                                                          need_without_normals=False, want_visible=False)
                q = geometry.icp_information(T, images[1:2], nrm[1:2], match, nn_pix)
                result.update(self._quality_result(q["information"][0], q["sum_r2"][0], q["pairs"][0], q["covariance"][0], q["status"][0]))
        self.point_cloud_t_1 = current * self.scaling_factor                    # undo the in-place scaling (:172)
        return result

    @torch.no_grad()
    def push_records(self, message, layout=None):
        """``push`` for a message as the driver delivers it: a numpy structured array (``layout`` defaults to ``record_layout`` of its
        dtype), a ``[N,C]`` fp32 array (a KITTI .bin file: x, y, z first) or raw bytes with an explicit ``layout``.  The node's filter
        always applies.  Engine "native" hands the records to ``dl_odometry_push_records``: filter, projection and network in the
        library, no host pass over the points.  Engine "torch", and any layout the library refuses (a 22-byte record), unpacks on the
        host into ``[1,3,N]`` and goes through ``push`` -- the reference's route.  Returns what ``push`` returns."""
        message = np.asarray(message)
        if layout is None:
            if message.dtype.fields is not None:
                layout = record_layout(message.dtype)
            elif message.dtype == np.float32 and message.ndim == 2 and message.shape[1] >= 3:
                layout = record_layout(4 * message.shape[1], (0, 4, 8))
            else:
                raise ValueError("push_records: a layout is needed for anything but a structured array or [N,C>=3] float32")
        layout = geometry.record_layout(layout.point_step, (layout.off_x, layout.off_y, layout.off_z),
                                        _lib.RECORDS_DROP_ZERO | _lib.RECORDS_MIN_RANGE, 0.3)
        if self.native is not None and message.flags.c_contiguous:
            from ..deploy import native_infer
            if native_infer.why_layout_unsupported(layout) is None:
                return self._native_result(self.native.push_records(message, layout))
        return self.push(unpack_records(message, layout))
