/*
 * delora_hip.h -- C ABI of libdelora_hip.so: the MI355X (gfx950) kernels of DeLORA -- the geometry of the
 * per-scan-pair training step (projection, normals, exact search, losses), the pose CNN's convolutions,
 * pooling and heads, and on top of them the torch-free inference path scan -> pose (dl_pose_net_*,
 * dl_odometry_push).
 *
 * The reference (leggedrobotics/delora) has no native layer; its boundary for this path is the
 * Python module API.  Each entry point below replaces the torch-op sequence of one reference
 * function (file:line into the reference tree) and is what a ctypes binding of the reference would
 * call (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, strides in ELEMENTS; no torch/HIP types in signatures
 *     (dl_stream is the hipStream_t handle passed as void*, e.g. torch's current stream).
 *   - the caller owns every buffer; the library allocates nothing and keeps no mutable global state (the one exception is
 *     the opt-in launch profiler at the end of this header), never synchronises the device: all work is enqueued on the given
 *     stream (graph-capturable).
 *   - return 0 on success, negative dl_status otherwise; dl_last_error() (thread-local) has the text.
 *   - data layout: a batch of S scans is a planar fp32 buffer pts[C][sumN] + CSR offsets offs[S+1];
 *     a range image is planar fp32 [S][4][H][W] = (x, y, z, range), empty pixels are all-zero;
 *     normals are planar fp32 [S][3][H][W], the zero vector meaning "no normal"; pixel indices are
 *     int32 row-major v*W+u, -1 = none.  Row 0 is the lowest elevation, column 0 azimuth hfov[0].
 *     Planar images are what is STREAMED (network input, source side of the loss); images that are
 *     GATHERED from (the target side of correspondence search and loss) additionally exist in a packed
 *     form [S][H][W][4] fp32 -- (x,y,z,range) and (nx,ny,nz,0) -- so that one pixel is one 16-byte load.
 *   - results are deterministic: no floating-point atomics, order-independent integer atomics only.
 */
#ifndef DELORA_HIP_H
#define DELORA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DL_ABI_VERSION 10   /* 10: dl_conv_plan_describe (additive), the narrow convolution family dl_tower_* (purely additive: the number stays), its strided / 1x1 / residual members for narrow pose networks dl_narrow_* (purely additive: the number stays),dl_reproject / dl_reproject_workspace_bytes (purely additive: the number stays), inference without Python: dl_pose_net_* / dl_odometry_* (purely additive: the number stays), projection and streaming odometry from raw point records: dl_project_records / dl_odometry_push_records (purely additive: the number stays), rotation augmentation inside the projection: dl_project_rotated / dl_rotations_from_draws (purely additive: the number stays); 9: exact tree search between free-form point lists (dl_nn_list_*; additive); 8: dropout on the HIP path (dl_dropout_scale_f32, dl_stem_input_nhwc_drop_f32, dl_channel_scale_*_nhwc_t, dl_heads_*_drop; additive); 7: the Winograd-domain weights are an opaque operand (blocked LDS-image layout); 6: dl_project takes n_cols and ONE workspace (key plane + staging records of the vote), dl_wino_conv3x3_nhwc_f32 an optional split-K workspace; 5: batched weight gradients (dl_conv2d_wgrad_batch_*); 4: free image sizes in the convolution family (the strided input gradients take the INPUT image size and a seam workspace); 3: half-precision convolutions, launch profiler */

typedef void* dl_stream;

typedef enum {
  DL_OK = 0,
  DL_ERR_INVALID_ARGUMENT = -1,
  DL_ERR_LAUNCH = -2,
  DL_ERR_UNSUPPORTED = -3
} dl_status;

/* Projection model of one sensor (radians).  The fp64 fields are the exact config values; the
 * kernels derive the fp32 constants the reference's torch expression uses from them:
 * fp32(f0) and fp32(f1 - f0), the difference formed in fp64 (src/utility/projection.py:23-30). */
typedef struct {
  int32_t H;          /* vertical_cells   (config/config_datasets.yaml:20)  */
  int32_t W;          /* horizontal_cells (config/config_datasets.yaml:21)  */
  double hfov0, hfov1; /* horizontal_field_of_view (config_datasets.yaml:3, after deg->rad) */
  double vfov0, vfov1; /* <dataset>.vertical_field_of_view (config_datasets.yaml:19)        */
} dl_sensor;

/* Flags of dl_icp_loss_fwd (config/hyperparameters.yaml:14-19). */
#define DL_LOSS_POINT_TO_POINT 1u   /* point_to_point_loss */
#define DL_LOSS_POINT_TO_PLANE 2u   /* point_to_plane_loss */
#define DL_LOSS_PLANE_TO_PLANE 4u   /* plane_to_plane_loss */
#define DL_LOSS_NORMAL_LINEAR  8u   /* normal_loss == "linear" (default "squared") */
#define DL_LOSS_PO2PO_ALONE   16u   /* po2po_alone (hyperparameters.yaml:19, src/losses/icp_losses.py:36-45): EVERY matched
                                       source point takes part in point-to-point, no normal masks; excludes flags 2 and 4
                                       (the reference fails for that combination) */

int dl_abi_version(void);
const char* dl_last_error(void);

/* Bytes of scratch dl_project needs for S scans of H x W pixels whose points lie in columns [0, n_cols) of a C-channel buffer:
 * the uint64 key plane [S][H*W] followed by one 16-byte staging record per column (two when C > 3). */
size_t dl_project_workspace_bytes(int32_t S, int32_t H, int32_t W, int64_t n_cols, int32_t C);

/*
 * Spherical projection of S scans into range images, nearest point per pixel.
 * Replaces ImageProjectionLayer.project_to_img (src/utility/projection.py:48-106): range channel
 * (:55-60), argsort by range + sequential first-wins dedup on the host (:63-67, :34-43, :80-91)
 * and the index scatter (:98-103) become one atomicMin pass over (range_bits << 32 | point_index)
 * keys -- which also leaves (x,y,z,range) of every point behind as one 16-byte record -- plus one resolve pass
 * (one 16-byte gather per occupied pixel); u,v follow compute_2D_coordinates (:21-31) with round-half-even.
 *   pts      [C][pts_cs]   planar fp32, channels 0..2 = x,y,z; scan s owns columns offs[s]..offs[s+1)
 *   n_cols                 number of columns in use (offs[S] <= n_cols <= pts_cs): sizes the staging records
 *   offs     [S+1]         int32 CSR offsets (device); max_n = largest scan length (host value)
 *   image4   [S][4][H][W]  out: x,y,z,range of the winning point, zeros elsewhere
 *   aux      [S][C-3][H][W] out (may be NULL when C == 3): the remaining channels of the winner
 *   packed   [S][H][W][4]  out (may be NULL): x,y,z,range of the winner, pixel-interleaved
 *   packed_aux [S][H][W][4] out (may be NULL; needs C >= 6): channels 3..5 of the winner + 0 (stored normals)
 *   pix2pt   [S][H][W]     out: index of the winning point relative to its scan start, -1 if empty
 *   workspace dl_project_workspace_bytes(S,H,W,n_cols,C) bytes of scratch, 16-byte aligned (a misaligned one is refused
 *                          with DL_ERR_INVALID_ARGUMENT before any launch)
 *   kept     [S]           out (may be NULL): number of occupied pixels per scan
 *   uvr      [3][pts_cs]   out (may be NULL): fp32 u, v and range of EVERY input point, input order; only the columns
 *                          offs[0]..offs[S]) of each plane are written
 * The contract, bit for bit (tests/project_ref.py is its plain restatement):
 *   range = sqrt(fma(z,z, fma(y,y, x*x))) and norm2 = sqrt(fma(y,y, x*x)), every step correctly rounded to fp32; a point whose
 *     squares overflow has range +inf: it still votes and loses to every finite point of its pixel;
 *   a = fp32(atan2(y, x)), e = fp32(atan2(z, norm2)) evaluated in fp64 and rounded once; u = ((a - fp32(hfov0)) / fp32(hfov1 - hfov0))
 *     * fp32(W-1) in fp32, v likewise; the pixel is rint() of them, half to even;
 *   a point is inside iff 0 <= rint(u) <= W-1 and 0 <= rint(v) <= H-1: a coordinate that rounds to -0.0 counts as pixel 0, a NaN
 *     coordinate is outside;
 *   the winner of a pixel is the point with the smallest (uint32 bit pattern of the range, index within the scan);
 *   empty pixels hold +0.0 in every image and -1 in pix2pt; packed_aux.w is +0.0;
 *   max_n only sizes the grid: any value >= the largest scan length gives the same result.
 */
int dl_project(const float* pts, int64_t pts_cs, int64_t n_cols, const int32_t* offs, int32_t S, int32_t C,
               int32_t max_n, const dl_sensor* sensor, float* image4, float* aux, float* packed,
               float* packed_aux, int32_t* pix2pt, void* workspace, int32_t* kept, float* uvr,
               dl_stream stream);

/*
 * dl_project with a rotation per scan applied INSIDE the vote (additive: the ABI number stays) -- the training-time augmentation
 * `random_point_cloud_rotations` (src/deploy/deployer.py:205-218, dead in the reference behind its raise at :203-204) without a
 * pass of its own and without writing the caller's point buffer.  Every argument of dl_project, plus
 *   rot      [S][9]        fp32 row-major 3x3 matrices (device), or NULL: exactly dl_project.
 * The contract, bit for bit (tests/rotate_ref.py is its plain restatement):
 *   a scan whose nine words are the bit pattern of the identity (1.0f on the diagonal, +0.0f elsewhere) is NOT multiplied: every
 *     output of that scan is dl_project's, -0.0, inf and NaN coordinates included;
 *   any other scan is projected as dl_project projects the points p' = R p, one coordinate being (r0*x + r1*y) + r2*z with every
 *     operation rounded to fp32 and nothing fused; image4, packed, uvr and the winner follow from p' alone (pix2pt still indexes
 *     the input columns);
 *   with C >= 6 channels 3..5 (the stored normals) are rotated by the same matrix in the same arithmetic; with C = 4 or 5 they
 *     pass through, as channels 6 and above always do.
 * Workspace: dl_project_workspace_bytes, unchanged.  Refusals are dl_project's, before any launch.
 */
int dl_project_rotated(const float* pts, int64_t pts_cs, int64_t n_cols, const int32_t* offs, int32_t S, int32_t C,
                       int32_t max_n, const dl_sensor* sensor, float* image4, float* aux, float* packed,
                       float* packed_aux, int32_t* pix2pt, void* workspace, int32_t* kept, float* uvr,
                       const float* rot, dl_stream stream);

/*
 * The rotations of one augmented training step from uniform draws, one tiny launch (additive: the ABI number stays).
 *   draws [B][4] fp32 in [0, 1) (device): 0..2 the direction, 3 the angle;  rot [2B][9] out, the layout dl_project_rotated reads for a
 *   batch stored as b0.scan_1, b0.scan_2, b1.scan_1, ...
 * Row 2b is the exact identity (scan 1 is never rotated).  Row 2b+1 is Rodrigues' matrix cos(a) I + sin(a) [d]x + (1 - cos(a)) d d^T of
 * the unit axis d = (0, 0, 1) when only_yaw, else draws 0..2 normalised (the reference draws them in [0, 1): every axis lies in the
 * positive octant -- kept), and the angle a = (draw 3 - 0.5) * magnitude_rad, so |a| <= magnitude_rad / 2.  a == 0 (and three zero
 * draws: no axis) give the exact identity; only_yaw writes row and column 2 as exact 0 / 1.  Entries are within 1e-6 of the float64
 * evaluation (a dozen fp32 operations on values <= 1, sinf / cosf at a few ulp).
 */
int dl_rotations_from_draws(const float* draws, int32_t B, int32_t only_yaw, float magnitude_rad, float* rot, dl_stream stream);

/*
 * The same projection from RAW POINT RECORDS, with the reference node's filter applied inside the vote (additive: the ABI number
 * stays).  A sensor driver delivers a scan as n records of point_step bytes with fp32 x, y, z at byte offsets -- a KITTI .bin file is
 * point_step 16, offsets 0, 4, 8; a PointCloud2 message names its own -- and the reference's node (src/ros_utils/
 * odometry_publisher.py:91-100) drops every point with an exactly zero coordinate or within 0.3 m on the host before it projects.
 *   records  n_records records (device), 4-byte aligned; scan s owns records offs[s]..offs[s+1)
 *   layout   passed by value semantics (read on the host during the call)
 *   offs     [S+1] int32 CSR offsets in records (device); max_n >= the largest scan length (host value, sizes the grid only);
 *            a record index outside [0, n_records) gives no load and no vote
 *   image4 [S][4][H][W], packed [S][H][W][4] (may be NULL), pix2pt [S][H][W], kept [S] (may be NULL): as dl_project, pix2pt holding
 *            the winner's RECORD index within its scan;  n_pass [S] out (may be NULL): records that took part
 *   workspace dl_project_records_workspace_bytes(S,H,W) = S*H*W*8 rounded up to 16 bytes, 16-byte aligned: the key plane ONLY.
 *            There are no staging records: resolve gathers x, y, z of the one winning record per occupied pixel from `records`
 *            and takes the range from the winning key's upper word, the bits the vote computed.
 * The contract, bit for bit (tests/records_ref.py is its plain restatement):
 *   x, y, z are the fp32 words at the three offsets of record i; no other byte of a record influences anything;
 *   a record takes part iff (!(filter & DL_RECORDS_DROP_ZERO) or (x != 0 and y != 0 and z != 0): -0.0 counts as zero, NaN does not)
 *     and (!(filter & DL_RECORDS_MIN_RANGE) or range_np > min_range), range_np = sqrt((x*x + y*y) + z*z) with every operation
 *     rounded to fp32 and NOTHING fused -- what numpy.linalg.norm(xyz, axis=0) computes, NOT dl_project's fused range: near 0.3 m
 *     the two disagree about the threshold for ~1 % of the points within a few ulp of it.  A NaN comparison is false;
 *   a record that takes part is projected exactly as dl_project projects a point (the fused range in the key, the image and the
 *     packed image included), its index being the record index within its scan.
 *   Hence image4, packed and kept equal dl_project on the host-filtered, compacted, transposed list, pix2pt equals its pix2pt mapped
 *   through the list of surviving record indices, and n_pass is that list's length.
 * Layouts served: point_step a multiple of 4 in 12..256; the three offsets multiples of 4, distinct, off + 4 <= point_step; records
 * 4-byte aligned; min_range finite under DL_RECORDS_MIN_RANGE.  Any other layout is DL_ERR_UNSUPPORTED with a text naming the field
 * (a 22-byte record has to be unpacked by the caller: no misaligned device loads).  A null pointer, an unknown filter bit, bad
 * sizes or a misaligned workspace are DL_ERR_INVALID_ARGUMENT.  Every refusal happens before any launch.  16-byte records on a
 * 16-byte aligned base are read with one 16-byte load per record, every other layout with three 4-byte loads at the record stride.
 */
#define DL_RECORDS_DROP_ZERO 1u   /* drop a record whose x, y or z is exactly zero (odometry_publisher.py:95) */
#define DL_RECORDS_MIN_RANGE 2u   /* drop a record unless range_np > min_range (:96-97) */
typedef struct { int32_t point_step, off_x, off_y, off_z; uint32_t filter; float min_range; } dl_record_layout;
size_t dl_project_records_workspace_bytes(int32_t S, int32_t H, int32_t W);
int dl_project_records(const void* records, int64_t n_records, const dl_record_layout* layout, const int32_t* offs, int32_t S, int32_t max_n,
                       const dl_sensor* sensor, float* image4, float* packed, int32_t* pix2pt, void* workspace, int32_t* kept, int32_t* n_pass,
                       dl_stream stream);

/*
 * Per-pixel surface normals of S range images.
 * Replaces NormalsComputer.compute_normal_vectors + covariance_eigen_decomposition + linalg.cov
 * (src/preprocessing/normal_computation.py:89-122, :53-87; src/utility/linalg.py:33-56): the
 * (2a+1)x(2b+1) clamped-neighbour gather, range gate, masked covariance, n >= min_n gate, CPU
 * symeig and viewpoint flip become one LDS-tiled kernel with an in-register 3x3 eigen solve.
 *   image4  [S][4][H][W] in (scan stride image_ss elements, channel stride H*W)
 *   normals [S][3][H][W] out (scan stride 3*H*W), zeros where no normal
 *   packed_normals [S][H][W][4] out (may be NULL): (nx,ny,nz,0), pixel-interleaved
 * A pixel is processed iff x != 0 && y != 0 && z != 0 (normal_computation.py:35); a neighbour counts iff any of its components is
 * non-zero, its range is finite and |range - centre range| <= epsilon_range (fp32; equality keeps it); window coordinates are
 * clamped to the image (edge pixels are duplicated, no wrap); a normal needs min_neighbors such neighbours (the centre included).
 * min_neighbors < 2 is accepted but leaves the covariance of a single neighbour undefined.
 *   half_rows 0..15, half_cols 0..31 (a = half_rows, b = half_cols: the window is (2a+1) x (2b+1)); anything else, S, H or W <= 0
 *   or a null image4 / normals is DL_ERR_INVALID_ARGUMENT before any launch.  Every window in that range runs: the tile staged in
 *   LDS is (4+2a)(64+2b) pixels of 16 bytes, up to 68 544 B at (15,31), and the entry point raises the kernel's dynamic-LDS limit
 *   where that exceeds 64 KiB (a device that refuses the raise is DL_ERR_INVALID_ARGUMENT as well, before the launch).
 *   "Range" is the fp32 value sqrt(fma(z, z, fma(y, y, x * x))): a finite point whose squares overflow fp32 (|coordinate| above
 *   ~1.8e19) has an infinite range and is an empty pixel.
 */
int dl_normals(const float* image4, int64_t image_ss, int32_t S, int32_t H, int32_t W,
               int32_t half_rows, int32_t half_cols, float epsilon_range, int32_t min_neighbors,
               float* normals, float* packed_normals, dl_stream stream);

/* Bytes of scratch dl_nn_correspond needs (list counters, the record lists of the uncertified queries, the two-level pyramid of the
 * target tiles, packet descriptors; ~85 B per pixel of the batch). */
size_t dl_nn_workspace_bytes(int32_t B, int32_t H, int32_t W);

/*
 * Exact 3-D nearest target point of every transformed source point (k=1, Euclidean, fp64 distances).
 * Replaces the CPU cKDTree build + queries of ICPLosses.forward (src/losses/icp_losses.py:24-26,
 * :34, :63-80) together with the source transform of Deployer.step (src/deploy/deployer.py:294-296).
 * Target points are the occupied pixels of the target image (given in packed form, as produced by dl_project
 * with THE SAME sensor: the search relies on every stored point lying in the pixel it projects to), source
 * points those of src_image4.
 *   tgt_packed [B][H][W][4] packed target image (scan stride tgt_ss elements)
 *   tgt_normals_packed [B][H][W][4] packed target normals (may be NULL: matched normals are then zero)
 *   T          [B][4][4]  fp32 row-major source->target transforms
 *   match      [B][6][H][W] out (may be NULL): per SOURCE pixel the matched target point (planes 0..2) and its
 *                         normal (planes 3..5), zeros where nn_pix is -1 -- what dl_icp_loss_* streams
 *   nn_pix     [B][H][W]  out: target pixel index of the nearest target point per source pixel
 *                         (-1 for empty source pixels or an empty target image); written twice for some pixels (the first
 *                         pass hands its best candidate to the second through it): read it after the call, on `stream`
 *   visible    [B]        out (may be NULL): number of source points with round(v) < H and v > 0 in the
 *                         target frame (the visible_pixels metric, deployer.py:349-352,365-367)
 *   src_normals may be NULL; when given and need_without_normals == 0, source pixels without a normal
 *   are skipped (their correspondences are only used by the point-to-point term).
 */
int dl_nn_correspond(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss,
                     const float* tgt_packed, int64_t tgt_ss, const float* tgt_normals_packed, int64_t tgtn_ss,
                     const float* T, int32_t B, const dl_sensor* sensor, int32_t need_without_normals,
                     int32_t* nn_pix, float* match, int32_t* visible, void* workspace, dl_stream stream);

/* Bytes of scratch dl_reproject needs: exactly the two uint64 key planes [B][2][H*W], rounded up to 16 bytes; 0 for a
 * non-positive size. */
size_t dl_reproject_workspace_bytes(int32_t B, int32_t H, int32_t W);

/*
 * Re-projection of the TRANSFORMED source image: the range images of the logged step figure.
 * Replaces, for Deployer.log_image (src/deploy/deployer.py:73-100), the host-side pair lists and the three project_to_img calls
 * of a logged step (deployer.py:80-89, :317-320; src/losses/icp_losses.py:196-206): a vote pass over the source pixels (up to two
 * 64-bit atomicMin per occupied pixel) and a resolve pass over the output pixels that recomputes the winner's values from its
 * source pixel.  The inputs are the tensors of dl_icp_loss_fwd:
 *   src_image4 [B][4][H][W] planar source image (scan stride src_ss elements, >= 3*H*W; planes 0..2 are read)
 *   src_normals [B][3][H][W] source normals (scan stride srcn_ss >= 3*H*W)
 *   match      [B][6][H][W] from dl_nn_correspond (scan stride match_ss >= 6*H*W)
 *   nn_pix     [B][H][W]   its map; only the sign is used
 *   T          [B][4][4]   fp32 row-major source->target transforms
 *   moved4     [B][4][H][W] out: x', y', z', range' of the winning transformed source point, the winner taken over ALL occupied
 *                          source pixels (the reference's image_2_transformed, deployer.py:317-320)
 *   paired9    [B][9][H][W] out (may be NULL): the winner taken over the PAIRS WITH NORMALS only; planes 0..2 the transformed
 *                          point, 3..5 the rotated source normal R n, 6..8 the residual vector d = s' - m (m = match planes 0..2)
 *                          (image_2_transformed_and_normals_and_pointwise_loss, channels 0..8: deployer.py:80-89)
 *   src_pix    [B][2][H][W] int32 out (may be NULL): the source pixel index of the winner of moved4 (plane 0) and of paired9
 *                          (plane 1), -1 where there is none
 *   workspace  dl_reproject_workspace_bytes(B, H, W) bytes, 16-byte aligned
 * src_normals, match and nn_pix may be NULL only together; paired9 must then be NULL as well.  When paired9 is NULL, plane 1 of
 * src_pix is still written, all -1.  Every element of every output is written on every call; empty pixels hold +0.0 (-1 in src_pix).
 * The contract, bit for bit (tests/reproject_ref.py is its plain restatement; it builds on dl_project's):
 *   a source pixel is occupied iff !(x == 0 && y == 0 && z == 0) (the rule of dl_nn_correspond);
 *   the transformed point is q = fma(m2, z, fma(m1, y, m0 * x)) + m3 per row of T (the operations of dl_icp_loss_fwd), the rotated
 *     normal the same chain without the addition, d = q - m, all in fp32;
 *   range, u, v, half-to-even rounding and the inside test of q are dl_project's: a NaN coordinate is outside, an infinite range
 *     still votes and loses to every finite one;
 *   the winner of a pixel is the smallest (uint32 bit pattern of range', source pixel index);
 *   a source pixel is PAIRED iff it is occupied, nn_pix >= 0, its source normal is not the zero vector and the normal in match
 *     planes 3..5 is not the zero vector (the pair set of icp_losses.py:48-52,110-121);
 *   a non-finite T[b] stays in sample b: every other sample's output is the same to the bit.
 * DL_ERR_INVALID_ARGUMENT before any launch: a null src_image4 / T / sensor / moved4 / workspace; B <= 0, H < 2 or W < 2;
 * 2*B*H*W beyond 2^31 - 1; the pair inputs given in part; paired9 without them; a scan stride below the dense size; a workspace
 * that is not 16-byte aligned.  The call is three kernels on `stream` (key fill, vote, resolve): no synchronisation, allocation,
 * read-back or floating-point atomic, capturable into a HIP graph.
 */
int dl_reproject(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss, const float* match,
                 int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, const dl_sensor* sensor, float* moved4,
                 float* paired9, int32_t* src_pix, void* workspace, dl_stream stream);

/* Bytes of scratch dl_icp_loss_fwd needs (per-block partial sums). */
size_t dl_icp_loss_workspace_bytes(int32_t B, int32_t H, int32_t W);

/*
 * Fused source transform + point-to-plane / plane-to-plane / point-to-point residuals + reduction,
 * and the moments of the analytic gradient with respect to T.
 * Replaces Deployer.step's R@p+t, R@n (src/deploy/deployer.py:294-299) and
 * KDPointToPlaneLoss / KDPlaneToPlaneLoss / KDPointToPointLoss (src/losses/icp_losses.py:196-206,
 * :224-240, :168-179) with the pair selection of ICPLosses.forward (:48-60, :102-121).
 *   src_image4 / src_normals   planar source planes; match [B][6][H][W] from dl_nn_correspond; nn_pix its map
 *                          (only the sign is used: validity).  All thirteen planes are streamed once.
 *   loss_terms [B][3]      out: loss_po2po, loss_po2pl, loss_pl2pl (means; 0 for disabled terms,
 *                          NaN when an enabled term has no pairs, as torch's MSELoss of an empty set)
 *   pair_counts[B][2]      out: pairs with normals (K), pairs without normals (K', po2po)
 *   grad_terms [B][3][12]  out: d loss_term / d T[:3,:4] (row-major 3x4), correspondences held fixed
 * Masking is MULTIPLICATIVE: every pixel's residuals are formed and then multiplied by 0 or 1 (nn_pix < 0, a missing normal on
 * either side and po2po_alone select the factor), so that no load waits for a branch.  The operands at pixels that do not count
 * -- all thirteen planes where nn_pix < 0, the normals of a pair whose partner has none -- must therefore be FINITE: an inf or
 * NaN there turns the sample's sums into NaN (0 * inf), any finite value contributes an exact zero.  dl_nn_correspond writes zeros
 * into match where it writes nn_pix = -1, and dl_project / dl_normals write zeros into empty source pixels.  A ragged last chunk
 * re-reads pixel 0 of every plane under a zero factor, so pixel 0 must be finite as well.  T itself may be anything: a non-finite
 * pose stays in its own sample, the other samples' outputs do not change by a bit.
 *   workspace              dl_icp_loss_workspace_bytes(B, H, W) bytes, 16-byte aligned whatever H*W is (the reduction reads the partial
 *                          rows with 16-byte loads); a workspace that is not is DL_ERR_INVALID_ARGUMENT before any launch
 */
int dl_icp_loss_fwd(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss,
                    const float* match, int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, int32_t H, int32_t W,
                    uint32_t flags, float* loss_terms, int32_t* pair_counts, float* grad_terms,
                    void* workspace, dl_stream stream);

/* The two launches of dl_icp_loss_fwd as separate entry points (same arguments): the streaming pass that leaves one
 * partial row per workgroup in the workspace, and the per-sample fp64 reduction of those rows. */
int dl_icp_loss_partial(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss,
                        const float* match, int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, int32_t H, int32_t W, uint32_t flags,
                        void* workspace, dl_stream stream);
int dl_icp_loss_reduce(const void* workspace, int32_t B, int32_t H, int32_t W, uint32_t flags, float* loss_terms,
                       int32_t* pair_counts, float* grad_terms, dl_stream stream);

/* Measurement aid: dl_icp_loss_partial with the kernel's own begin/end timestamps attached to a timer (two HIP events
 * filled by hipExtLaunchKernelGGL), so that its duration can be read inside real training steps; timer may be NULL.
 * dl_timer_elapsed_ms waits for the kernel to finish.  Not graph-capturable when a timer is given. */
int dl_timer_create(void** timer);
int dl_timer_destroy(void* timer);
int dl_timer_elapsed_ms(void* timer, float* ms);
int dl_icp_loss_partial_timed(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss,
                              const float* match, int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B,
                              int32_t H, int32_t W, uint32_t flags, void* workspace, void* timer, dl_stream stream);

/* Measurement aid: reads exactly the operand streams of dl_icp_loss_partial (same grid, same 16-byte loads) and does
 * no arithmetic -- the time the memory system needs for this transfer.  workspace as for dl_icp_loss_fwd. */
int dl_probe_stream_read(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss,
                         const float* match, int64_t match_ss, const int32_t* nn_pix, int32_t B, int32_t H, int32_t W,
                         void* workspace, dl_stream stream);

/*
 * Backward of dl_icp_loss_fwd: grad_T[b][:3,:4] = sum_k grad_loss_terms[b][k] * grad_terms[b][k]
 * (row 3 of grad_T is zero).  grad_T is [B][4][4].
 */
int dl_icp_loss_bwd(const float* grad_terms, const float* grad_loss_terms, int32_t B, float* grad_T,
                    dl_stream stream);

/*
 * Point-to-plane normal equations of the matched pairs (csrc/info.hip; additive, ABI 10 as it stands): how well the pairs constrain
 * the pose T, as an information matrix and a covariance.  The reference's node publishes a nav_msgs/Odometry whose 6x6
 * pose.covariance it never sets (src/ros_utils/odometry_publisher.py:128-172); this is the quantity that belongs there.  It is NOT a
 * refinement: no Gauss-Newton step is taken or returned.
 * The inputs are exactly those of dl_icp_loss_fwd (thirteen planes streamed once, 52 B per source pixel).  Per source pixel, in fp32
 * unless said otherwise:
 *   q = fma(m2, z, fma(m1, y, m0 * x)) + m3 per row of T (the chain of dl_icp_loss_fwd and dl_reproject), used for the moment arm;
 *   the residual, the one quantity that cancels (centimetres on coordinates of tens of metres near a converged pose), is formed in
 *   FP64 from the fp32 operands and rounded ONCE to fp32:  d = (fma(m2, z, fma(m1, y, m0 * x)) + m3) - p_t per row,
 *   r = (float) fma(dz, n_z, fma(dy, n_y, dx * n_x)) with n the MATCHED TARGET normal (match planes 3..5; it is not normalised
 *   here) -- its error is relative to |r|, not to |q|; on small-integer data it is the value of the fp32 chain, bit for bit;
 *   a = q x n:  a_x = fma(q_y, n_z, -(q_z * n_y)),  a_y = fma(q_z, n_x, -(q_x * n_z)),  a_z = fma(q_x, n_y, -(q_y * n_x)),
 *   J = (n_x, n_y, n_z, a_x, a_y, a_z): the derivative of r under the LEFT perturbation q <- q + omega x q + v with respect to
 *       (v, omega) -- translation first, the order of pose.covariance (x, y, z, rotation about X, Y, Z), in the TARGET frame,
 *   w = 1 iff nn_pix >= 0, the source normal is not the zero vector and the matched normal is not the zero vector (the point-to-plane
 *       pair set of dl_icp_loss_fwd), else 0.  Masking is multiplicative, with dl_icp_loss_fwd's contract: the operands of pixels that
 *       do not count must be FINITE (then they contribute an exact zero), pixel 0 included where H*W is not a multiple of 256.
 * Outputs per sample, all fp64 (the fp32 per-lane sums are added per workgroup in fp32 and across workgroups in fp64, fixed order):
 *   info       [B][6][6]  sum w J J^T (the 21 unique sums are accumulated once, both triangles written)
 *   rhs        [B][6]     sum w J r   (half the gradient of sum w r^2 under the perturbation)
 *   stats      [B][2]     sum w r^2,  K = sum w
 *   covariance [B][6][6]  sigma^2 info^-1 with sigma^2 = sum w r^2 / (K - 6) where status is DL_INFO_OK, else all +0.0 (what the
 *                         reference publishes today)
 *   status     [B] int32  DL_INFO_TOO_FEW_PAIRS if K <= 6; else DL_INFO_UNOBSERVABLE if a diagonal entry of info is not > 0 or, with
 *                         D = diag(info) and Ah = D^-1/2 info D^-1/2 (Ah_ij = (info_ij * s_i) * s_j, s_i = 1 / sqrt(info_ii)), a
 *                         pivot of the Cholesky factorisation of Ah -- the remainder Ah_jj - sum_c L_jc^2 before its square root -- is not
 *                         > DL_INFO_MIN_PIVOT; else DL_INFO_OK.  The test is scale free (metres or millimetres, ten pairs or a million:
 *                         Ah has a unit diagonal), and the constant is part of this contract.  "not >" makes a NaN -- a non-finite
 *                         T[b] -- unobservable; such a pose stays in sample b, the other samples' outputs do not change by a bit.
 *   workspace  dl_icp_information_workspace_bytes(B, H, W) bytes (host arithmetic: one row of 32 floats per workgroup), 16-byte aligned
 * DL_ERR_INVALID_ARGUMENT before any launch, the text naming the entry point: a null pointer; B, H or W <= 0, H*W above 2^30 or
 * B above 65535 (the size function then returns 0); a scan stride below the dense size (src_ss, srcn_ss >= 3*H*W, match_ss >= 6*H*W);
 * where H*W is a multiple of 4, planes or strides that are not 16-byte aligned; a workspace that is not 16-byte aligned.
 * Two launches on `stream`; no floating-point atomic, synchronisation, allocation or read-back: the same inputs give the same bits
 * on every run, and the call is capturable into a HIP graph.  tests/information_ref.py is the plain float64 restatement.
 */
#define DL_INFO_OK 0
#define DL_INFO_TOO_FEW_PAIRS 1
#define DL_INFO_UNOBSERVABLE 2
#define DL_INFO_MIN_PIVOT 1e-10
size_t dl_icp_information_workspace_bytes(int32_t B, int32_t H, int32_t W);
int dl_icp_information(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss, const float* match,
                       int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, int32_t H, int32_t W, double* info,
                       double* rhs, double* stats, double* covariance, int32_t* status, void* workspace, dl_stream stream);

/*
 * Exact nearest neighbour between two free-form point lists (no range-image structure), fp64
 * distances, LDS-tiled brute force.  Backs the list-based ICPLosses.forward signature
 * (src/losses/icp_losses.py:28-33) when the caller has lists rather than images.
 *   src [3][ms_cs], tgt [3][mt_cs] planar fp32; nn [Ms] out (index into tgt, -1 if Mt == 0)
 */
int dl_nn_bruteforce(const float* src, int64_t ms_cs, int32_t Ms, const float* tgt, int64_t mt_cs,
                     int32_t Mt, int32_t* nn, dl_stream stream);

/*
 * The same search through a tree: exact nearest neighbour between two free-form point lists in O(M log M), what the
 * reference does with scipy.spatial.cKDTree (src/losses/icp_losses.py:24-34: one tree over the target list, one query per
 * source list; called once per sample from src/deploy/deployer.py:302-307).  Built once per target list, queried any
 * number of times.  The answer is dl_nn_bruteforce's on every input: the target that minimises dx*dx + dy*dy + dz*dz in fp64
 * on the fp32 coordinates, the LOWEST target index among exact ties, -1 for a query with a non-finite coordinate or when no
 * target is finite (Mt == 0 included); a target with a non-finite coordinate is never returned.  Bitwise reproducible.
 *   tgt [3][mt_cs], src [3][ms_cs] planar fp32 (column strides >= the counts); nn [Ms] out, index into tgt in the caller's order
 *   Ms, Mt free, 0 included, at most 2^30 (DL_ERR_UNSUPPORTED beyond: indices are 32-bit)
 *   tree       caller-owned, 16-byte aligned, dl_nn_list_tree_bytes(Mt) bytes:
 *                8192 + 40 * P + 32 * nodes + 1024 * ceil(Mt / 2048),  P = Mt rounded up to a multiple of 64 (the leaf size),
 *                nodes = P/64 leaves + ceil(leaves/64) + ... down to the first level of at most 64 nodes
 *              (per point: 16 B packed record + 2 x 8 B sort keys + 2 x 4 B sort indices, ~0.5 B of boxes, 0.5 B of digit counts)
 *              It holds its own copy of the coordinates: the target list may change after the build without affecting queries.
 *   workspace  caller-owned, 16-byte aligned, dl_nn_list_query_workspace_bytes(Ms) bytes:
 *                24 * Q + 1024 * ceil(Ms / 2048),  Q = Ms rounded up to a multiple of 64.  One query at a time per workspace.
 *   The size functions return 0 for a negative count or one above 2^30.  tgt / mt_cs of the query are accepted for symmetry
 *   with dl_nn_bruteforce and may be NULL / 0 (the tree is self-contained); Mt must be the count the tree was built with.
 * Neither call synchronises, allocates or reads back: both can be captured into a HIP graph (a linear chain of kernels).
 */
size_t dl_nn_list_tree_bytes(int32_t Mt);
size_t dl_nn_list_query_workspace_bytes(int32_t Ms);
int dl_nn_list_build(const float* tgt, int64_t mt_cs, int32_t Mt, void* tree, dl_stream stream);
int dl_nn_list_query(const float* src, int64_t ms_cs, int32_t Ms, const float* tgt, int64_t mt_cs, int32_t Mt,
                     const void* tree, int32_t* nn, void* workspace, dl_stream stream);

/*
 * Fused elementwise glue of the pose CNN: out[r][pad + w] = act(x[r][w] + res[r][w]) plus, for pad == 1, the two
 * wrap-around columns out[r][0] = out[r][W], out[r][W+1] = out[r][1]  (rows r = n*C*H + c*H + h).
 * Replaces the separate activation, residual add and F.pad(..., (1,1,0,0), 'circular') calls of the reference's
 * ResNet (src/models/resnet_modified.py:95-120, :159-177).
 *   x    [rows][W] dense;  res (may be NULL) rows of width W at pitch res_pitch starting at element res_off
 *   act  0 none, 1 tanh, 2 relu;  pad 0 or 1;  out [rows][W + 2*pad]
 * Backward: grad_x[r][w] = (grad_out[r][pad+w] + folded wrap columns) * act'(y), y = the saved forward output;
 * grad_res_padded (may be NULL) [rows][W+2] receives grad_x in its interior and zeros in its border columns.
 */
int dl_ring_act_pad_fwd(const float* x, const float* res, int64_t res_pitch, int64_t res_off, int64_t rows,
                        int32_t W, int32_t pad, int32_t act, float* out, dl_stream stream);
int dl_ring_act_pad_bwd(const float* grad_out, const float* y, int64_t rows, int32_t W, int32_t pad, int32_t act,
                        float* grad_x, float* grad_res_padded, dl_stream stream);

/* Stem of the pose CNN in one pass: activation, wrap-around padding, 3x3 max-pooling with stride (1,2) and H padding 1
 * (torch.nn.MaxPool2d arg-max rule), wrap-around padding of the pooled map.  Replaces reference
 * src/models/resnet_modified.py:100-102 (act, F.pad circular, self.maxpool) and the F.pad of the next convolution.
 *   x [planes][H][W] dense, planes = N*C;  out [planes][H][Wo+2], Wo = (W-1)/2 + 1;  win [planes][H][Wo] int8: position
 *   0..8 of each maximum inside its window (saved for the backward).  act as in dl_ring_act_pad_fwd. */
int dl_ring_act_pool_pad_fwd(const float* x, int64_t planes, int32_t H, int32_t W, int32_t act, float* out, int8_t* win,
                             dl_stream stream);
/* grad_out, y [planes][H][Wo+2] (y = forward output); grad_x [planes][H][W] = dL/dx. */
int dl_ring_act_pool_pad_bwd(const float* grad_out, const float* y, const int8_t* win, int64_t planes, int32_t H,
                             int32_t W, int32_t act, float* grad_x, dl_stream stream);

/* Storage types of the *_t / *_h entry points. */
#define DL_DTYPE_F32  0
#define DL_DTYPE_F16  1
#define DL_DTYPE_BF16 2

/* The same four entry points for fp16 / bf16 storage (autocast): dtype 0 fp32, 1 fp16, 2 bf16 for every tensor argument;
 * the arithmetic is fp32 and every stored element is rounded once, as the separate torch ops would. */
int dl_ring_act_pad_fwd_t(const void* x, const void* res, int64_t res_pitch, int64_t res_off, int64_t rows, int32_t W, int32_t pad,
                          int32_t act, int32_t dtype, void* out, dl_stream stream);
int dl_ring_act_pad_bwd_t(const void* grad_out, const void* y, int64_t rows, int32_t W, int32_t pad, int32_t act, int32_t dtype,
                          void* grad_x, void* grad_res_padded, dl_stream stream);
int dl_ring_act_pool_pad_fwd_t(const void* x, int64_t planes, int32_t H, int32_t W, int32_t act, int32_t dtype, void* out, int8_t* win,
                               dl_stream stream);
int dl_ring_act_pool_pad_bwd_t(const void* grad_out, const void* y, const int8_t* win, int64_t planes, int32_t H, int32_t W,
                               int32_t act, int32_t dtype, void* grad_x, dl_stream stream);

/*
 * Convolutions of the pose CNN on 360-degree range images, channels-last fp32 on the fp32 matrix cores (exact fp32
 * products, v_mfma_f32_32x32x2_f32), with the wrap-around width padding as addressing and the elementwise tail fused.
 * Replaces F.pad(x, (1,1,0,0), 'circular') + Conv2d(kernel 3, padding (1,0)) [+ residual add] + tanh/relu and the
 * 1x1 strided down-sampling convolution of the reference's ResNet (src/models/resnet_modified.py:97-98, :101-102,
 * :150-177; torch Conv2d there) and their autograd.
 *   x    [N][H][W][C]  input (channels-last);  y [N][H/stride_h][W/stride_w][K] output
 *   w    transposed == 0: [K][ksize][ksize][C] (the torch parameter [K,C,k,k] in channels_last memory format)
 *        transposed == 1: [C][ksize][ksize][K] -- the FORWARD weight of the layer whose input gradient is wanted: the
 *                         kernel reads it with flipped taps and swapped channel roles (stride 1, 3x3 only)
 *   3x3: rows -1 and H read zeros, columns -1 and W read columns W-1 and 0; 1x1: no padding.
 *   epilogue (flags, applied in this order on the fp32 accumulator v of output element (pixel, k)):
 *     1 DL_CONV_ADD   v += add[pixel][k]
 *     2 DL_CONV_ACT   v  = act(v)                      act: 0 none, 1 tanh, 2 relu
 *     4 DL_CONV_DACT  v *= act'(dsrc[pixel][k])        dsrc = saved OUTPUT of the activation (tanh' = 1 - y^2)
 *   add, dsrc: [N][Ho][Wo][K] or NULL.  Ho = ceil(H / stride_h), Wo = ceil(W / stride_w) (the reference's padded convolution:
 *   floor((X - 1) / stride) + 1).  The IMAGE SIZE IS FREE (ABI 4): tiles hang over the right / lower edge of images that do not
 *   divide -- the reference's shipped 64x720 image has feature maps 180, 90, 45 and 23 pixels wide (config/config_datasets.yaml:21)
 *   -- odd sizes included.  Channels must tile: K % 64 == 0, C % 8 == 0 (DL_ERR_UNSUPPORTED otherwise; the caller then uses its
 *   library convolution).  Only the strided 3x3 layers and, below 256 channels, the stride-1 images that divide into 256-pixel tiles
 *   (Wo % 128 == 0 with even Ho, or Wo % 64 == 0 with Ho % 4 == 0) reduce in chunks of 8 channels; every other launch needs C % 16 == 0 and refuses the
 *   rest the same way (the Winograd entry point below takes any C % 8 == 0 on any image).
 *   ALIGNMENT (every entry point of the convolution families, fp32, Winograd and half precision alike): each tensor, weight, seam and
 *   workspace pointer must be 16-byte aligned -- operands move as 16-byte vectors (four fp32 / eight half values; the LDS DMA copies
 *   16 bytes per lane) and the channel counts above keep every pixel's row of channels a multiple of 16 bytes, so an aligned base
 *   keeps every access aligned.  Nothing more is assumed: a base 16 bytes past a 256-byte boundary is as good as an allocator's.
 *   The kernels write only inside the tensors they are given (overhanging tiles are masked in the epilogue) and read only inside them.
 */
#define DL_CONV_ADD  1u
#define DL_CONV_ACT  2u
#define DL_CONV_DACT 4u
int dl_conv2d_nhwc_f32(const float* x, const float* w, float* y, const float* add, const float* dsrc, int32_t N,
                       int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w,
                       int32_t transposed, int32_t act, uint32_t epilogue, dl_stream stream);

/* Input gradient of the STRIDED layers (3x3 stride (1,2) / (2,2), 1x1 stride (1,2) / (2,2)), torch autograd of
 * Conv2d(stride) in the reference.  One pass per stride phase over the output-gradient grid, each with exactly the taps
 * whose phase matches (no zero-stuffing).  H, W = the size of the layer's INPUT image (ABI 4; the gradient grid is Ho = ceil(H /
 * stride_h) x Wo = ceil(W / stride_w)): g [N][Ho][Wo][K] (K = the layer's output channels), w = the layer's FORWARD weight
 * [K][ksize][ksize][C], dx [N][H][W][C].
 *   dense != 0 (1x1 layers): only phase (0,0) receives gradient; the result is written densely as [N][Ho][Wo][C] and is
 *                            meant to be handed to the 3x3 layer's call as add_grid.
 *   epilogue flags: 8 DL_CONV_ADD_GRID  v += add_grid[n][ho][wo][c] on the phase-(0,0) pixels (the down-sampling
 *                   branch's gradient), 4 DL_CONV_DACT  v *= act'(dsrc[pixel][c]) with dsrc at full resolution.
 *   seam_ws: fp32 scratch of N*H*2*C floats, REQUIRED when W is odd, stride_w == 2, ksize == 3 and dense == 0 (else may be NULL):
 *            on an odd width the stride phases do not close under the wrap-around (column 2 wo + s - 1 mod W changes parity at the
 *            seam); the two terms that cross it are summed into seam_ws first and added by the phase that owns columns 0 and W-1. */
#define DL_CONV_ADD_GRID 8u
int dl_conv2d_dgrad_strided_nhwc_f32(const float* g, const float* w, float* dx, const float* add_grid, const float* dsrc,
                                     int32_t N, int32_t H, int32_t W, int32_t K, int32_t C, int32_t ksize,
                                     int32_t stride_h, int32_t stride_w, int32_t dense, int32_t act, uint32_t epilogue,
                                     float* seam_ws, dl_stream stream);

/* Weight gradient of the same convolutions: dw[k][tap][c] = sum over output pixels of g[pixel][k] * x[pixel + tap][c]
 * (wrap-around / zero-row addressing as above), slab-wise partial sums added in a fixed order (deterministic).
 *   x [N][H][W][C], g [N][Ho][Wo][K] (Ho, Wo = ceil), dw [K][ksize][ksize][C];  workspace: dl_conv2d_wgrad_workspace_bytes(...) bytes.
 *   Any image size; channels must tile: K % 64 == 0, C % 64 == 0. */
size_t dl_conv2d_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize,
                                       int32_t stride_h, int32_t stride_w);
int dl_conv2d_wgrad_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W,
                             int32_t C, int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, dl_stream stream);

/*
 * The NARROW family (csrc/tower.hip): the same 3x3, stride-1 ring convolution -- rows -1 and H read zeros, columns -1 and W read
 * columns W-1 and 0, as addressing -- for FEW channels, on v_mfma_f32_16x16x4_f32 (exact fp32).  It serves the per-image feature
 * tower of `pre_feature_extraction` (reference src/models/model.py:30-54: 4 -> 8 -> 16 -> 24 -> 32 -> 40 channels at full image
 * resolution) and its autograd.  Channel domain: C % 4 == 0, K % 8 == 0, 4 <= C <= 64, 8 <= K <= 64 (DL_ERR_UNSUPPORTED otherwise).
 * Any H >= 1 and W >= 1: tiles of 4 rows x 64 columns hang over the edges.
 *
 * VIEWS.  x, y, dsrc (and g of the weight gradient) are addressed through a view = three int32 {pitch, offset, group}:
 *   element (image n, pixel p = h * W + w, channel c)  =  base[((n / group) * H * W + p) * pitch + offset + (n % group) * CH + c]
 * with CH the tensor's own channel count (C for x; K for y, dsrc, g).  A dense [N][H][W][CH] tensor is {CH, 0, 1}.  {128, 0, 2}
 * with K = 40 makes images 2b and 2b + 1 write channels 0..39 and 40..79 of pixel row b of a [N/2][H][W][128] buffer: the
 * concatenation of the two towers of a sample is never a copy, and the backward reads its slices the same way.  Required:
 * group >= 1, N % group == 0, pitch % 4 == 0, offset % 4 == 0, offset + group * CH <= pitch (DL_ERR_INVALID_ARGUMENT otherwise);
 * (N / group) * H * W * pitch < 2^31 per view (DL_ERR_UNSUPPORTED beyond: 32-bit offsets).  Bases 16-byte aligned, as above.
 * Only the CH channels of a view are read / written; the rest of a pixel's pitch is never touched.
 *
 *   dl_tower_conv3x3_nhwc_f32   y = epilogue(conv(x, w)).  w: transposed == 0: [K][3][3][C]; transposed == 1: [C][3][3][K], the
 *       FORWARD weight of the layer whose input gradient is wanted (x = the output gradient), read with flipped taps, as
 *       dl_conv2d_nhwc_f32 does.  epilogue: DL_CONV_ACT (v = act(v)) and / or DL_CONV_DACT (v *= act'(dsrc), dsrc = saved output of
 *       the activation) with act 0 none, 1 tanh, 2 relu; any other flag, a bad act, a null x / w / y / x_view / y_view, or DACT
 *       without dsrc and dsrc_view is DL_ERR_INVALID_ARGUMENT.  dsrc / dsrc_view may be NULL without DACT.
 *   dl_tower_wgrad3x3_nhwc_f32  dw [K][3][3][C] = sum over pixels of g[pixel][k] * x[pixel + tap][c].  Every workgroup adds its four
 *       waves in a fixed order and writes one partial dW to `workspace` (dl_tower_wgrad_workspace_bytes(N, H, W, C, K) bytes; the
 *       query returns 0 for shapes the launch refuses); a second launch sums the partials in slab order.  No float atomics: the
 *       result is bit-identical from run to run.  The workspace need not be initialised.  A null x / g / dw / workspace / view is
 *       DL_ERR_INVALID_ARGUMENT.
 * Both refuse through dl_last_error before any launch; no synchronisation, launches go to the caller's stream.
 */
int dl_tower_conv3x3_nhwc_f32(const float* x, const float* w, float* y, const float* dsrc, int32_t N, int32_t H, int32_t W,
                              int32_t C, int32_t K, const int32_t* x_view, const int32_t* y_view, const int32_t* dsrc_view,
                              int32_t transposed, int32_t act, uint32_t epilogue, dl_stream stream);
size_t dl_tower_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K);
int dl_tower_wgrad3x3_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W,
                               int32_t C, int32_t K, const int32_t* x_view, const int32_t* g_view, dl_stream stream);

/*
 * The narrow family for NARROW POSE NETWORKS (csrc/narrow.hip; factor_fewer_resnet_channels 2 and 4 of the reference's
 * config/hyperparameters.yaml: widths 32/64/128/256 and 16/32/64/128): the layers whose channel counts are not multiples of 64 -- the
 * stem's conv1, layer1, and the first layers of layer2 (and of layer3 at factor 4).  Same arithmetic, channel domain (C % 4 == 0,
 * K % 8 == 0, 4 <= C <= 64, 8 <= K <= 64 for the LAYER's input / output channels), ring addressing and free image size as above, on
 * DENSE tensors, plus what a residual network needs: ksize 3 or 1 (1x1: unpadded), stride (1,1) or (1,2) (output width
 * Wo = ceil(W / 2)), a residual-add epilogue and the strided layers' input gradient.  N * H * W * 64 < 2^31 (DL_ERR_UNSUPPORTED beyond).
 *
 *   dl_narrow_conv2d_nhwc_f32         y [N][H][Wo][K] = epilogue(conv(x [N][H][W][C], w)), arguments and epilogue (DL_CONV_ADD, DL_CONV_ACT,
 *       DL_CONV_DACT, in this order; add, dsrc [N][H][Wo][K]) as dl_conv2d_nhwc_f32.  transposed == 1 (stride (1,1) only): w is the FORWARD
 *       weight [C'][ksize][ksize][K'] of the layer whose input gradient is wanted, x its output gradient (C = K', K = C').  At stride
 *       (1,2) a workgroup's tile is 4 rows x 32 output columns (half the stride-1 tile: the staged halo and the LDS budget stay the
 *       same, two workgroups per CU).
 *   dl_narrow_dgrad_strided_nhwc_f32  input gradient of a stride-(1,2) layer, arguments as dl_conv2d_dgrad_strided_nhwc_f32 without the
 *       seam workspace: H, W = the layer's INPUT image, g [N][H][ceil(W/2)][K], w the forward weight [K][ksize][ksize][C], dx [N][H][W][C].
 *       The gradient is read as if zeros stood between its columns (addressing only) and the stride-1 transposed convolution runs on
 *       that ring: exact on any width, twice the MFMA work of a phase-split form.  epilogue: DL_CONV_ADD_GRID (v += add_grid
 *       [n][h][w / 2][c] on the even columns), then DL_CONV_DACT (dsrc [N][H][W][C]).  dense != 0 (ksize 1, no epilogue): the 1x1
 *       layer's gradient on the grid, [N][H][ceil(W/2)][C], meant as add_grid of the 3x3 layer's call.
 *   dl_narrow_wgrad_nhwc_f32          dw [K][ksize][ksize][C] from x [N][H][W][C] and g [N][H][Wo][K]: partial sums per workgroup in
 *       `workspace` (dl_narrow_wgrad_workspace_bytes(...) bytes; 0 for shapes the launch refuses; need not be initialised), summed in
 *       a fixed order by a second launch.  No float atomics: bit-identical from run to run.
 * Refusals -- a null x / w / y / g / dx / dw / workspace, an unknown epilogue flag, a bad act, a flag without its operand
 * (DL_ERR_INVALID_ARGUMENT); channels outside the domain, another ksize or stride, transposed with a stride
 * (DL_ERR_UNSUPPORTED) -- happen before any launch, through dl_last_error.  No synchronisation, no allocation; launches go to the
 * caller's stream (capturable).
 */
int dl_narrow_conv2d_nhwc_f32(const float* x, const float* w, float* y, const float* add, const float* dsrc, int32_t N, int32_t H,
                              int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t transposed,
                              int32_t act, uint32_t epilogue, dl_stream stream);
int dl_narrow_dgrad_strided_nhwc_f32(const float* g, const float* w, float* dx, const float* add_grid, const float* dsrc, int32_t N,
                                     int32_t H, int32_t W, int32_t K, int32_t C, int32_t ksize, int32_t stride_h, int32_t stride_w,
                                     int32_t dense, int32_t act, uint32_t epilogue, dl_stream stream);
size_t dl_narrow_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h,
                                       int32_t stride_w);
int dl_narrow_wgrad_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W, int32_t C,
                             int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, dl_stream stream);

/*
 * The same stride-1 3x3 convolution (forward and, with the backward weight set, input gradient) as fused Winograd
 * F(2x2,3x3) on the fp32 matrix cores: 2.25x fewer multiplications; input transform, 16 batched GEMMs, output transform and
 * the epilogue of dl_conv2d_nhwc_f32 in one launch (the transformed tensors never reach HBM).
 *   dl_wino_weights_f32: w [K][3][3][C] -> u_fwd and/or u_bwd (each 16*K*C floats = dl_wino_weights_floats; either may be NULL).
 *                        Run once per optimiser step.  Layout (an OPAQUE operand of dl_wino_conv3x3_nhwc_f32 since ABI 7): reduction
 *                        channels in chunks of 8, output rows (k of u_fwd, c of u_bwd) in blocks of 64, and per (chunk, block) the
 *                        16 planes as [16][64 rows][8] with the 16-byte halves of a row swapped where bit 3 of the row is set --
 *                        the bytes the kernel's LDS DMA copies linearly.  Row counts that are not multiples of 64 (no convolution
 *                        entry point consumes them) keep [chunk][16][rows][8].
 *   dl_wino_conv3x3_nhwc_f32: x [N][H][W][C], u = u_fwd of the layer -> y [N][H][W][K]; for the input gradient pass the
 *                        output gradient as x, u = u_bwd and swap C and K.  epilogue / act / add / dsrc as above.
 *   Shapes: any image size (a workgroup takes 64 tiles as 2x32, 4x16, 8x8 or 16x4, whichever wastes the fewest; tile groups hang over
 *   the edges of images that do not divide, odd sizes end in partial tiles); C % 8 == 0; K % 64 == 0.
 */
size_t dl_wino_weights_floats(int32_t K, int32_t C);
int dl_wino_weights_f32(const float* w, float* u_fwd, float* u_bwd, int32_t K, int32_t C, dl_stream stream);
/* The same transform for up to DL_WINO_BATCH layers in one launch (the trunk's 13 stride-1 layers: one launch per autograd segment
 * instead of one per layer).  A layer's u_fwd or u_bwd may be null. */
#define DL_WINO_BATCH 16
typedef struct {
  const float* w;      /* [K][3][3][C] */
  float* u_fwd;        /* 16*K*C floats (layout above) or null */
  float* u_bwd;        /* 16*K*C floats or null */
  int32_t K, C;
} dl_wino_layer;
int dl_wino_weights_batch_f32(const dl_wino_layer* layers, int32_t n, dl_stream stream);
/* Scratch of dl_wino_conv3x3_nhwc_f32: 0 for launches that fill the chip; for SMALL launches (few tile groups: the reference's
 * default batch size 1) the bytes of the partial sums of a split over the input channels -- the launch then runs its channel ranges on
 * otherwise idle CUs and a second, elementwise launch adds them up and applies the epilogue.  workspace may be NULL (no split). */
size_t dl_wino_conv3x3_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K);
int dl_wino_conv3x3_nhwc_f32(const float* x, const float* u, float* y, const float* add, const float* dsrc, int32_t N,
                             int32_t H, int32_t W, int32_t C, int32_t K, int32_t act, uint32_t epilogue, void* workspace,
                             dl_stream stream);

/*
 * Stride-(1,2) 3x3 layers (wrap-around columns, zero rows) on the same fused Winograd kernel.  With an even width the layer is a
 * stride-1 3x3 convolution of the same memory read as [N][H][W/2][2C] (a pixel pair = one pixel with 2C channels) whose kernel has no
 * tap in its third column: a quarter of the Winograd planes is identically zero and is neither fetched nor multiplied (12 instead of
 * the direct form's 18 multiply-adds per output and (c, k) pair).  H, W, C, K always describe the LAYER: x [N][H][W][C], y and g
 * [N][H][W/2][K], w [K][3][3][C].
 *   dl_wino_strided_takes:        1 when the dispatch should take the layer (stride (1,2); H even, W % 4 == 0; C, K multiples of 64; the
 *                                 pair view divides into 2x32 or 4x16 tile groups; enough tile groups that the stride-1 dispatch would not
 *                                 split the channels at `cu_count` CUs), else 0.  cu_count > 0 answers without a GPU; <= 0: this device.
 *   dl_wino_strided_weights_f32:  w -> u_fwd and/or u_bwd, dl_wino_strided_weights_floats (= 16 K 2C) floats each, once per step.
 *   dl_wino_strided_conv3x3_nhwc_f32:  forward; epilogue 0 or the activation bit (2).
 *   dl_wino_strided_dgrad3x3_nhwc_f32: input gradient dx [N][H][W][C]; epilogue bits as dl_conv2d_dgrad_strided_nhwc_f32: 8 adds
 *                                 add_grid, the compact [N][H][W/2][C] gradient of the 1x1 down-sampling branch, onto the even pixels;
 *                                 4 multiplies by act'(dsrc), dsrc [N][H][W][C].
 * The two convolutions run every shape that tiles, whatever dl_wino_strided_takes answers.  Other shapes: DL_ERR_UNSUPPORTED.
 */
int dl_wino_strided_takes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride_h, int32_t stride_w, int32_t cu_count);
size_t dl_wino_strided_weights_floats(int32_t K, int32_t C, int32_t stride_h, int32_t stride_w);
int dl_wino_strided_weights_f32(const float* w, float* u_fwd, float* u_bwd, int32_t K, int32_t C, int32_t stride_h, int32_t stride_w,
                                dl_stream stream);
int dl_wino_strided_conv3x3_nhwc_f32(const float* x, const float* u_fwd, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K,
                                     int32_t stride_h, int32_t stride_w, int32_t act, uint32_t epilogue, dl_stream stream);
int dl_wino_strided_dgrad3x3_nhwc_f32(const float* g, const float* u_bwd, float* dx, const float* add_grid, const float* dsrc, int32_t N,
                                      int32_t H, int32_t W, int32_t K, int32_t C, int32_t stride_h, int32_t stride_w, int32_t act,
                                      uint32_t epilogue, dl_stream stream);

/*
 * Weight gradient of a stride-1 3x3 layer in the Winograd domain (2.25x fewer multiplications than
 * dl_conv2d_wgrad_nhwc_f32; partial sums in a fixed order): x [N][H][W][C], g [N][H][W][K] -> dw [K][3][3][C].
 * Any image size (partial 2x2 tiles at odd edges, overhanging chunks of 8 tiles); C and K multiples of 64;
 * dl_wino_wgrad_workspace_bytes returns 0 for other channel counts.
 */
size_t dl_wino_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K);
int dl_wino_wgrad3x3_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W,
                              int32_t C, int32_t K, dl_stream stream);

/*
 * Weight gradients of SEVERAL layers in one call (round 4).  One layer has 1-64 output tiles; filling 256 CUs with it takes 4-512
 * pixel slabs per tile, and every slab writes a full fp32 copy of its tile -- ~70 MB of partial sums per layer whatever its size,
 * written and read back.  The weight gradients of a run of layers do not depend on each other, so the trunk defers them to the end
 * of the run (x and g stay alive until then) and hands them over together: layers that share a kernel instantiation run in ONE
 * launch with 1-8 slabs each, layers that end up with a single slab write dw directly, and one launch sums what was split.
 * Results equal the single-layer entry points up to the summation order of the slabs (fixed for a given set of layers).
 *   dl_wino_wgrad3x3_batch_nhwc_f32   stride-1 3x3 layers in the Winograd domain (ksize / stride fields must be 3 / 1 / 1)
 *   dl_conv2d_wgrad_batch_nhwc_f32    the direct kernel: ksize 1 or 3, strides 1 or 2
 *   dl_conv2d_wgrad_batch_nhwc_h      half-precision x / g (declared with the half-precision family below)
 * The *_workspace_bytes functions return 0 when a layer is not supported.
 */
#define DL_WGRAD_BATCH 24
typedef struct dl_wgrad_layer {
  const void* x;        /* [N][H][W][C] */
  const void* g;        /* [N][ceil(H/stride_h)][ceil(W/stride_w)][K] */
  float* dw;            /* [K][ksize][ksize][C] fp32 */
  int32_t N, H, W, C, K, ksize, stride_h, stride_w;
} dl_wgrad_layer;
/* The slab plan of such a merged launch, for inspection and tests (host only, no GPU needed): n layers with tiles[i] output tiles and
 * chunks[i] equal-cost pixel chunks per tile, `slots` workgroups running at a time, every slab beyond a tile's only one costing
 * `partial_cost` chunks' worth of time -> nslabs[i]; returns the simulated makespan in chunks (workgroups dispatched by decreasing
 * slab size, each to the first free slot), or a negative status. */
int64_t dl_wgrad_batch_plan(const int32_t* tiles, const int32_t* chunks, int32_t n, int32_t slots, int32_t partial_cost, int32_t* nslabs);
size_t dl_wino_wgrad3x3_batch_workspace_bytes(const dl_wgrad_layer* layers, int32_t n);
int dl_wino_wgrad3x3_batch_nhwc_f32(const dl_wgrad_layer* layers, int32_t n, void* workspace, dl_stream stream);
size_t dl_conv2d_wgrad_batch_workspace_bytes(const dl_wgrad_layer* layers, int32_t n);
int dl_conv2d_wgrad_batch_nhwc_f32(const dl_wgrad_layer* layers, int32_t n, void* workspace, dl_stream stream);
/*
 * Weight gradients of stride-(1,2) 3x3 layers in the Winograd domain, on the pixel-pair view of dl_wino_strided_* above: x read as
 * [N][H][W/2][2C] and g [N][H][W/2][K] are a stride-1 problem whose kernel [K][3][3][2C] has no third tap column and, for the even-pixel
 * channels, a middle column only.  dW = G^T dU G then needs 12 of the 16 planes of dU for the odd-pixel channel blocks and 8 for the
 * even-pixel ones: 5 C K multiply-adds per output pixel instead of the direct kernel's 9 C K.  The dead planes are neither multiplied nor
 * transformed, accumulated or stored.  The table holds layers with ksize 3, strides (1,2); H, W, C, K describe the LAYER, dw is its own
 * [K][3][3][C].  Slab partials are summed in a fixed order (no atomics): results are deterministic.
 *   dl_wino_strided_wgrad_takes:  1 for stride (1,2), H even, W % 32 == 0, C and K multiples of 64, the pair view below 2^31 elements
 *                                 (2^30 per sample); else 0.  Host only.
 *   *_workspace_bytes:            0 when a layer is not one the query takes (dl_last_error names the field).
 */
int dl_wino_strided_wgrad_takes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride_h, int32_t stride_w);
size_t dl_wino_strided_wgrad3x3_batch_workspace_bytes(const dl_wgrad_layer* layers, int32_t n);
int dl_wino_strided_wgrad3x3_batch_nhwc_f32(const dl_wgrad_layer* layers, int32_t n, void* workspace, dl_stream stream);

/*
 * The same convolutions in HALF precision (dtype DL_DTYPE_F16 or DL_DTYPE_BF16 for every activation / gradient tensor,
 * fp32 accumulation on v_mfma_f32_32x32x16_f16 / _bf16): the network's autocast mode (torch.autocast around
 * src/models/resnet_modified.py:95-120 in a reference run with mixed precision; BASELINE.json configs[4]).  Operands reach
 * LDS by DMA; every stored element is rounded to the storage type once; epilogue arithmetic is fp32 (csrc/convh.hip).
 *   dl_conv_weights_h     the fp32 parameter w [K][taps][C] (taps = ksize^2) -> w_fwd [taps][K][C] and / or w_bwd [taps][C][K] in
 *                         half precision (either may be NULL); once per optimiser step.
 *   dl_conv2d_nhwc_h      as dl_conv2d_nhwc_f32 with x, y, add, dsrc in half precision; w = w_fwd of the layer
 *                         (transposed == 0) or w_bwd of the layer whose input gradient is wanted (transposed == 1, stride 1,
 *                         3x3 only; x is then the output gradient and C / K swap roles).  Any image size; K % 64 == 0, C % 32 == 0.
 *   dl_conv2d_dgrad_strided_nhwc_h   as dl_conv2d_dgrad_strided_nhwc_f32; w = w_bwd of the layer.
 *   dl_cast_f32_to_h      n fp32 values -> half precision (n % 8 == 0).
 */
int dl_conv_weights_h(const float* w, void* w_fwd, void* w_bwd, int32_t K, int32_t taps, int32_t C, int32_t dtype, dl_stream stream);
/* The same conversion for up to DL_CONVH_BATCH layers in one launch (all convolutions of an autograd segment of the trunk). */
#define DL_CONVH_BATCH 32
typedef struct {
  const float* w;      /* [K][taps][C] fp32 parameter (channels-last storage) */
  void* w_fwd;         /* [taps][K][C] half precision, or null */
  void* w_bwd;         /* [taps][C][K] half precision, or null */
  int32_t K, taps, C;
} dl_convh_layer;
int dl_conv_weights_batch_h(const dl_convh_layer* layers, int32_t n, int32_t dtype, dl_stream stream);
int dl_conv2d_nhwc_h(const void* x, const void* w, void* y, const void* add, const void* dsrc, int32_t N, int32_t H, int32_t W,
                     int32_t C, int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t transposed, int32_t dtype,
                     int32_t act, uint32_t epilogue, dl_stream stream);
int dl_conv2d_dgrad_strided_nhwc_h(const void* g, const void* w, void* dx, const void* add_grid, const void* dsrc, int32_t N,
                                   int32_t H, int32_t W, int32_t K, int32_t C, int32_t ksize, int32_t stride_h, int32_t stride_w,
                                   int32_t dense, int32_t dtype, int32_t act, uint32_t epilogue, float* seam_ws, dl_stream stream);
int dl_cast_f32_to_h(const float* src, void* dst, int64_t n, int32_t dtype, dl_stream stream);
/* Global average pooling of a half-precision channels-last map x [N][P][C] -> y [N][C] fp32 (fixed summation order), and its
 * backward fused with the activation derivative of the layer that produced x:
 * grad_pre[n][p][c] = grad_y[n][c] / P * act'(x[n][p][c]) in half precision (act 0 none, 1 tanh: 1 - x^2, 2 relu).  C % 8 == 0. */
int dl_mean_hw_nhwc_h(const void* x, int32_t N, int32_t P, int32_t C, int32_t dtype, float* y, dl_stream stream);
int dl_mean_hw_bwd_act_h(const float* grad_y, const void* x, int32_t N, int32_t P, int32_t C, int32_t act, int32_t dtype,
                         void* grad_pre, dl_stream stream);
/* Weight gradient from half-precision x [N][H][W][C] and g [N][Ho][Wo][K]: dw [K][ksize][ksize][C] in FP32 (the layout and type of
 * the parameter's gradient), fp32 accumulation, slab partials summed in a fixed order.  Fragments are built by the transposing
 * LDS read (ds_read_b64_tr_b16).  C % 64 == 0, K % 64 == 0, any image size; workspace bytes from the first function
 * (0 = shape not supported). */
size_t dl_conv2d_wgrad_h_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h,
                                         int32_t stride_w);
int dl_conv2d_wgrad_nhwc_h(const void* x, const void* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W, int32_t C,
                           int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t dtype, dl_stream stream);

/* The weight gradients of up to DL_WGRAD_BATCH layers in one call (see dl_wgrad_layer above). */
typedef dl_wgrad_layer dl_wgrad_h_layer;
size_t dl_conv2d_wgrad_batch_h_workspace_bytes(const dl_wgrad_h_layer* layers, int32_t n);      /* 0 = a layer is not supported */
int dl_conv2d_wgrad_batch_nhwc_h(const dl_wgrad_h_layer* layers, int32_t n, void* workspace, int32_t dtype, dl_stream stream);

/*
 * The stem's max-pooling on channels-last activations (reference src/models/resnet_modified.py:100-102: F.pad(circular) +
 * MaxPool2d(kernel 3, stride (1,2), padding (1,0)) after conv1 + activation), between the convolution kernels above:
 *   dl_pool3x3s12_nhwc_fwd: a [N][H][W][C] (activated conv1 output) -> y [N][H][W/2][C], win [N][H][W/2][C] int8 = position
 *                           0..8 of each maximum, row-major in the window (torch's rule: rows first, the first strictly
 *                           greater value wins, NaN propagates; the column left of column 0 is column W-1)
 *   dl_pool3x3s12_nhwc_bwd: g [N][H][W/2][C], a, win -> g_conv [N][H][W][C] = act'(a) * (sum of g over the windows that
 *                           selected the element); act: 0 none, 1 tanh (1 - a^2), 2 relu (a > 0)
 *   W even, C % 4 == 0.  The forward takes any a: a window of -inf gives -inf at its first in-range position (0, or 3 in row 0),
 *   the LAST NaN of a window wins, of equal zeros the first keeps its sign.  The backward (and dl_stem_wgrad_f32 below) needs a
 *   FINITE a: relu' is evaluated as "0 where a <= 0, else 1", which agrees with a > 0 on every finite value and on +-0 but lets
 *   the gradient through at a NaN.  g may hold anything: a gradient reaches only the element its window selected.
 */
int dl_pool3x3s12_nhwc_fwd(const float* a, int32_t N, int32_t H, int32_t W, int32_t C, float* y, int8_t* win, dl_stream stream);
/* The forward for inference in half precision: the same a -> y [N][H][W/2][C] in DL_DTYPE_F16 / DL_DTYPE_BF16 and NO window plane; equal,
 * bit for bit, to dl_pool3x3s12_nhwc_fwd followed by dl_cast_f32_to_h (the same window rule, the same conversion).  W even, C % 8 == 0,
 * fewer than 2^32 elements in a; any other dtype is DL_ERR_UNSUPPORTED. */
int dl_pool3x3s12_nhwc_fwd_h(const float* a, int32_t N, int32_t H, int32_t W, int32_t C, int32_t dtype, void* y, dl_stream stream);
int dl_pool3x3s12_nhwc_bwd(const float* g, const float* a, const int8_t* win, int32_t N, int32_t H, int32_t W, int32_t C,
                           int32_t act, float* g_conv, dl_stream stream);

/* Weight gradient of conv1 (3x3, stride (1,2), 8 -> 64 channels; reference src/models/resnet_modified.py:40-42, :97-98) fused with
 * the pooling backward and the activation derivative: g_pooled [N][H][W/4][64] (gradient of the pooled map), a [N][H][W/2][64] and
 * win (forward outputs of conv1 + activation and of dl_pool3x3s12_nhwc_fwd), x8 [N][H][W][8] (the channels-last network input)
 * -> dw [64][8][3][3] (the parameter's default layout).  The 134 MB gradient with respect to conv1's pre-activation is built
 * tile by tile in LDS and never written.  W % 4 == 0; workspace bytes from the first function (0 = not supported). */
size_t dl_stem_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W);
int dl_stem_wgrad_f32(const float* g_pooled, const float* a, const int8_t* win, const float* x8, int32_t N, int32_t H, int32_t W,
                      int32_t act, void* workspace, float* dw, dl_stream stream);

/*
 * The same stem in half precision (csrc/stemh.hip; the config key amp_stem under amp_dtype).  dtype is DL_DTYPE_F16 or DL_DTYPE_BF16,
 * h(v) the round-to-nearest-even conversion of an fp32 value to it (the conversion of dl_cast_f32_to_h, torch's .to(dtype)).
 *   dl_stem_input_nhwc_h  x_nchw [N][8][H][W] fp32 -> x8h [N][H][W][8] = h(x): the channels-last image, 16 bytes per pixel.
 *   dl_stem_conv1_h       a [N][H][W/2][64] = h(act(sum over (r, s, c) of h(w1[k][r][s][c]) * x8h[n][y + r - 1][(2 wc + s - 1) mod W][c])):
 *                         rows outside the image contribute zero, the width wraps around, the sum is accumulated in fp32 (every product
 *                         of two half values is an fp32 number), act: 0 none, 1 tanh, 2 relu (the epilogue arithmetic of
 *                         dl_conv2d_nhwc_h).  w1 is the RAW fp32 parameter in its channels-last storage [64][3][3][8], converted inside
 *                         the kernel: no prepared buffer.
 *   dl_stem_pool_fwd_h    a [N][H][Wc][C] half -> y [N][H][Wc/2][C] half and win int8, by the window rule of dl_pool3x3s12_nhwc_fwd
 *                         (rows first, the first strictly greater value wins, the wrapped left column, its NaN / zero / infinity
 *                         rules) on the half values: equal bit for bit, win included, to that pooling of float(a) followed by
 *                         dl_cast_f32_to_h.  Wc even, C % 8 == 0.
 *   dl_stem_wgrad_h       g_pooled [N][H][W/4][64] half, a, win (the two forward outputs), x8h -> dw [64][8][3][3] fp32 (the parameter's
 *                         default layout) = sum over the pixels of gc * x8h with gc = h(act'(a) * (sum of g over the windows that
 *                         selected the element, fp32)) built tile by tile in LDS and never written; fp32 accumulation, slab and wave
 *                         sums in a fixed order, no atomics: the same bits from run to run.  a must be finite (as dl_stem_wgrad_f32).
 *                         The workspace holds one [64][72] fp32 partial per slab: 64-pixel chunks of the W/2-wide rows, at most 512
 *                         slabs -- the plan of dl_stem_wgrad_f32; bytes from dl_stem_wgrad_h_workspace_bytes (0 = shape refused).
 * Refusals, before any launch, with dl_last_error naming the entry point and the field: a NULL pointer, a pointer that is not aligned
 * (16 bytes for the half tensors, w1 and the workspace, 8 for win, 4 for x_nchw and dw), a non-positive size or an act outside 0..2
 * are DL_ERR_INVALID_ARGUMENT; any other dtype, W % 4 != 0 (Wc odd, C % 8 != 0 for the pooling) and 2^31 or more elements in the
 * largest tensor of the call are DL_ERR_UNSUPPORTED.  No call synchronises or copies to the host; every launch goes to `stream`.
 */
int dl_stem_input_nhwc_h(const float* x_nchw, int32_t N, int32_t H, int32_t W, int32_t dtype, void* x8h, dl_stream stream);
int dl_stem_conv1_h(const void* x8h, const float* w1, int32_t N, int32_t H, int32_t W, int32_t act, int32_t dtype, void* a, dl_stream stream);
int dl_stem_pool_fwd_h(const void* a, int32_t N, int32_t H, int32_t Wc, int32_t C, int32_t dtype, void* y, int8_t* win, dl_stream stream);
size_t dl_stem_wgrad_h_workspace_bytes(int32_t N, int32_t H, int32_t W);
int dl_stem_wgrad_h(const void* g_pooled, const void* a, const int8_t* win, const void* x8h, int32_t N, int32_t H, int32_t W, int32_t act,
                    int32_t dtype, void* workspace, float* dw, dl_stream stream);

/*
 * The pose heads in seven launches (csrc/heads.hip): fc -> the two two-layer MLPs -> whole-batch quaternion norm, forward and backward
 * (reference src/models/resnet_modified.py:118-120, src/models/model.py:74-83, :114; torch autograd through them).  fp32.
 *   x [B][F] pooled feature; fc [R][F]; first layers [Hd][R]; last layers [4][Hd] (rotation), [3][Hd] (translation); 1 <= B <= 16;
 *   act: 0 none, 1 tanh, 2 relu (applied to the fc output and to the hidden layers, as the reference's `[act, Linear, act, Linear]`).
 *   dl_heads_fwd  -> a1 [B][R] = act(fc(x)), a2 [B][2][Hd] = act(hidden), rot_raw [B][4], translation [B][3],
 *                    rotation [B][4] = rot_raw / ||rot_raw||_F (ONE norm over the whole batch), norm [1]   (a1, a2, rot_raw, norm: saved)
 *   dl_heads_bwd  -> the ten parameter gradients (`grads`: same struct, pointers to writable buffers of the parameters' shapes) and
 *                    grad_x [B][F]; workspace: dl_heads_bwd_workspace_bytes.  Deterministic (fixed summation orders).
 */
typedef struct {
  const float *fc_w, *fc_b;   /* [R][F], [R] */
  const float *r1_w, *r1_b;   /* rotation head, first layer [Hd][R], [Hd] */
  const float *r3_w, *r3_b;   /* rotation head, last layer [4][Hd], [4] */
  const float *t1_w, *t1_b;   /* translation head, first layer [Hd][R], [Hd] */
  const float *t3_w, *t3_b;   /* translation head, last layer [3][Hd], [3] */
} dl_heads_params;
int dl_heads_fwd(const float* x, const dl_heads_params* params, int32_t B, int32_t F, int32_t R, int32_t Hd, int32_t act, float* a1,
                 float* a2, float* rot_raw, float* translation, float* rotation, float* norm, dl_stream stream);
size_t dl_heads_bwd_workspace_bytes(int32_t B, int32_t F, int32_t R, int32_t Hd);
int dl_heads_bwd(const float* x, const dl_heads_params* params, int32_t B, int32_t F, int32_t R, int32_t Hd, int32_t act, const float* a1,
                 const float* a2, const float* rot_raw, const float* norm, const float* grad_translation, const float* grad_rotation,
                 const dl_heads_params* grads, float* grad_x, void* workspace, dl_stream stream);

/* The same two calls with dropout on the fc output (reference src/models/resnet_modified.py:118: `dropout_values(fc(x))`): fc_scale
 * [B][R] holds 0 or 1 / (1 - p) per element (dl_dropout_scale_f32, site 3), or is NULL.  Forward: a1 = act((fc(x) + bias) * fc_scale);
 * backward: the gradient with respect to the fc output additionally times fc_scale.  With fc_scale == NULL they ARE dl_heads_fwd /
 * dl_heads_bwd (one implementation). */
int dl_heads_fwd_drop(const float* x, const dl_heads_params* params, int32_t B, int32_t F, int32_t R, int32_t Hd, int32_t act,
                      const float* fc_scale, float* a1, float* a2, float* rot_raw, float* translation, float* rotation, float* norm,
                      dl_stream stream);
int dl_heads_bwd_drop(const float* x, const dl_heads_params* params, int32_t B, int32_t F, int32_t R, int32_t Hd, int32_t act,
                      const float* fc_scale, const float* a1, const float* a2, const float* rot_raw, const float* norm,
                      const float* grad_translation, const float* grad_rotation, const dl_heads_params* grads, float* grad_x,
                      void* workspace, dl_stream stream);

/*
 * The single-MLP head (`use_single_mlp_at_output`; reference src/models/model.py:59-72, :106-114) on the same kernels' pattern: fc, then
 * [act, Linear] five times down to 7 outputs; rotation = y[:, :4] / ||y[:, :4]||_F (ONE norm over the whole batch of raw quaternions),
 * translation = y[:, 4:].  fp32, 1 <= B <= 16, act as above.  Layer l = 0..5 has w[l] [n_{l+1}][n_l] and b[l] [n_{l+1}] with the widths
 * n = (F, R, H1, H2, H3, H4, 7); the reference's are (512, resnet_outputs, 512, 512, 256, 64, 7).  Any widths from 1 to 2^20 are
 * served; the kernels are laid out for widths of a few thousand at most (the last layer and its backward are ONE workgroup whose
 * threads walk H4 serially: correct, but slow for a very wide H4).
 *   dl_heads_single_fwd  -> acts = the five activated layer outputs back to back, [B][R] | [B][H1] | [B][H2] | [B][H3] | [B][H4], the
 *                           first one act((fc(x) + bias) * fc_scale) when fc_scale [B][R] is not NULL (the dropout mask of the fc output,
 *                           dl_dropout_scale_f32 site 3); rot_raw [B][4], translation [B][3], rotation [B][4], norm [1].  Six launches.
 *                           (acts, rot_raw, norm: saved for the backward)
 *   dl_heads_single_bwd  -> the twelve parameter gradients (`grads`: same struct, writable buffers of the parameters' shapes) and grad_x
 *                           [B][F]; fc_scale as in the forward or NULL; workspace: dl_heads_single_bwd_workspace_bytes (0 = sizes
 *                           refused).  Eleven launches, fixed summation orders, no atomics.
 */
typedef struct {
  const float* w[6];   /* fc, then the five Linear layers: [n_{l+1}][n_l] */
  const float* b[6];   /* [n_{l+1}] */
} dl_heads_single_params;
int dl_heads_single_fwd(const float* x, const dl_heads_single_params* params, int32_t B, int32_t F, int32_t R, int32_t H1, int32_t H2,
                        int32_t H3, int32_t H4, int32_t act, const float* fc_scale, float* acts, float* rot_raw, float* translation,
                        float* rotation, float* norm, dl_stream stream);
size_t dl_heads_single_bwd_workspace_bytes(int32_t B, int32_t F, int32_t R, int32_t H1, int32_t H2, int32_t H3, int32_t H4);
int dl_heads_single_bwd(const float* x, const dl_heads_single_params* params, int32_t B, int32_t F, int32_t R, int32_t H1, int32_t H2,
                        int32_t H3, int32_t H4, int32_t act, const float* fc_scale, const float* acts, const float* rot_raw,
                        const float* norm, const float* grad_translation, const float* grad_rotation,
                        const dl_heads_single_params* grads, float* grad_x, void* workspace, dl_stream stream);

/*
 * Dropout of the pose CNN (csrc/dropout.hip; reference src/models/resnet_modified.py:33-38, :95-118: p = 0.2, training mode only).
 * The random stream is this library's own and has a contract a host program can replay:
 *   generator   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85)
 *   counter     (i >> 2, i >> 34, site, 0) for decision index i; key = (seed & 0xffffffff, seed >> 32); decision i reads word i & 3
 *   site        1 = the stacked input image, 2 = the channels of layer3's output, 3 = the fc output
 *   decision    dropped iff word < round(p * 2^32) (p = 0.2: 0x33333333), else multiplied by 1.0f / (1.0f - (float)p);
 *               p = 0 keeps everything with a scale of exactly 1.0f.  0 <= p < 1.
 *   index i     the flat index of the element in the tensor the kernel writes: [N][H][W][C] channels-last for the input (a pixel's C
 *               channels are C / 4 generator calls), n * C + c for the channels, b * R + j for fc.  It does not depend on the storage type.
 *   seed        ONE 64-bit value read FROM DEVICE MEMORY by the kernel (a replayed graph sees the value its replay wrote).
 *
 *   dl_dropout_scale_f32         scale[i] = 0 or 1 / (1 - p) for the n decisions of a site (the two small masks; any site's, for tests)
 *   dl_stem_input_nhwc_drop_f32  x_nchw [N][C][H][W] planar -> x_nhwc [N][H][W][C] times the site-1 mask: the transposing copy in front
 *                                of the stem's convolution with the dropout applied on the way (no extra pass, no stored mask).  C % 4 == 0.
 *   dl_channel_scale_nhwc_t      y[n][p][c] = x[n][p][c] * scale[n][c] on a channels-last map [N][P][C] (P = H * W pixels) of dtype
 *                                DL_DTYPE_F32 / _F16 / _BF16; fp32 arithmetic, one rounding.  C % 4 == 0 (fp32) / C % 8 == 0 (half).
 *   dl_channel_scale_bwd_act_nhwc_t   g_pre[n][p][c] = g[n][p][c] * scale[n][c] * act'(x[n][p][c]) in ONE pass, x = the activated,
 *                                UN-dropped map (act 0 none, 1 tanh: 1 - x^2, 2 relu: x > 0): the gradient with respect to the
 *                                pre-activation of the layer that produced x, as the trunk's segments exchange it.
 */
int dl_dropout_scale_f32(const uint64_t* seed, uint32_t site, double p, int64_t n, float* scale, dl_stream stream);
int dl_stem_input_nhwc_drop_f32(const float* x_nchw, int32_t N, int32_t C, int32_t H, int32_t W, const uint64_t* seed, double p,
                                float* x_nhwc, dl_stream stream);
int dl_channel_scale_nhwc_t(const void* x, const float* scale, int32_t N, int32_t P, int32_t C, int32_t dtype, void* y, dl_stream stream);
int dl_channel_scale_bwd_act_nhwc_t(const void* g, const void* x, const float* scale, int32_t N, int32_t P, int32_t C, int32_t act,
                                    int32_t dtype, void* g_pre, dl_stream stream);

/* Site 1 behind the feature tower (`use_dropout` with `pre_feature_extraction`; reference src/models/resnet_modified.py:95-97: the
 * element-wise dropout hits the 80 concatenated tower channels).  Decision index i = ((b H + h) W + w) * 2 CH + c in the LOGICAL
 * channels-last [B][H][W][2 CH] tensor, c < CH image 1's tower, c >= CH image 2's; the pitch does not enter.  CH % 4 == 0, pitch % 4 == 0,
 * 2 CH <= pitch, B H W pitch < 2^31.
 *   dl_tower_wide_drop_f32      y5 [2B][H][W][CH] (compact, UN-dropped layer-5 output, image n = 2 b + k) -> xw [B][H][W][pitch]:
 *                               xw[b,h,w,k CH + c] = y5[n,h,w,c] * s(i); channels 2 CH .. pitch - 1 are written as zeros.
 *   dl_tower_wide_drop_bwd_f32  gx [B][H][W][pitch] (the true dL/dxw; channels 2 CH .. are not read) ->
 *                               g5[n,h,w,c] = (gx[b,h,w,k CH + c] * s(i)) * act'(y5[n,h,w,c]): the gradient of layer 5's pre-activation,
 *                               the mask regenerated from the seed (no mask tensor exists). */
int dl_tower_wide_drop_f32(const float* y5, const uint64_t* seed, double p, int32_t B, int32_t H, int32_t W, int32_t CH, int32_t pitch,
                           float* xw, dl_stream stream);
int dl_tower_wide_drop_bwd_f32(const float* gx, const float* y5, const uint64_t* seed, double p, int32_t act, int32_t B, int32_t H, int32_t W,
                               int32_t CH, int32_t pitch, float* g5, dl_stream stream);

/* Quaternion (x,y,z,w) + translation -> T [B][4][4] = [[R, t], [0, 1]] and its backward (reference src/models/model_parts.py:
 * 24-44; R = kornia 0.3.0 quaternion_to_rotation_matrix: normalise with eps, then the element-wise formula):
 *   dl_quat_to_T_fwd: translation [B][3], quaternion [B][4] -> T
 *   dl_quat_to_T_bwd: quaternion, grad_T [B][4][4] -> grad_translation [B][3], grad_quaternion [B][4] */
int dl_quat_to_T_fwd(const float* translation, const float* quaternion, int32_t B, float eps, float* T, dl_stream stream);
int dl_quat_to_T_bwd(const float* quaternion, const float* grad_T, int32_t B, float eps, float* grad_translation,
                     float* grad_quaternion, dl_stream stream);

/* Global average pooling of a channels-last feature map (reference resnet_modified.py: avgpool + flatten before fc):
 * x [N][P][C] (P = H*W pixels) -> y [N][C]; fixed summation order; C % 4 == 0. */
int dl_mean_hw_nhwc_f32(const float* x, int32_t N, int32_t P, int32_t C, float* y, dl_stream stream);

/*
 * INFERENCE WITHOUT PYTHON (csrc/infer.hip; additive, ABI 10 as it stands): scan -> pose on the entry points above, for a C or C++ caller that has no torch.
 * Replaces the layer walk of the reference's inference node (src/ros_utils/odometry_publisher.py:104-172: project both scans, stack,
 * model forward, quaternion -> T; bin/run_rosnode.py) and is what delora_amd/models/ring_conv.py (RingStem, RingSegment.forward) and
 * model_parts.FusedHeads do in eval mode -- the SAME launches with the same operands in the same order, hence the same bits.
 *
 * dl_pose_net describes the network as the reference builds it (src/models/resnet_modified.py, src/models/model.py:74-83); every
 * pointer is a DEVICE pointer to the RAW fp32 parameter, 16-byte aligned, in the layout the matching entry point takes:
 *   conv1_w            [64][3][3][8]   (dl_conv2d_nhwc_f32; the torch parameter [64,8,3,3] in channels_last memory format)
 *   blocks[i].w1 / w2  [cout][3][3][cin] / [cout][3][3][cout];  blocks[i].wd [cout][1][1][cin] when has_downsample, else NULL
 *   heads              dl_heads_params for fc [R][F] and the two heads ([Hd][R], [4][Hd], [3][Hd]);  F = the last block's cout
 * Scope: fp32, 8 input channels (two planar 4-channel range images), full-width channel counts (multiples of 64, the first block
 * reading conv1's 64), strides (1,1), (1,2) or (2,2) with has_downsample exactly on the strided blocks (and cin == cout on the
 * others), act 1 (tanh) or 2 (relu), the two-MLP heads, 1 <= B <= 16, H >= 1, W a multiple of 4, every activation below 2^31 elements.
 * Anything else is DL_ERR_UNSUPPORTED with a text that names the offending field; null or misaligned pointers and non-positive sizes
 * are DL_ERR_INVALID_ARGUMENT.  Everything is refused before any launch, through dl_last_error, the text naming the entry point.
 *
 * PREPARED WEIGHTS.  Every stride-1 3x3 layer runs as fused Winograd (dl_wino_conv3x3_nhwc_f32); its Winograd-domain forward weights
 * are produced ONCE by dl_pose_net_prepare (dl_wino_weights_batch_f32, no backward weights) into the caller's `prepared` buffer of
 * dl_pose_net_prepared_bytes bytes (the sum of dl_wino_weights_floats over those layers, in block order; 256-byte aligned) and stay
 * valid until a weight changes.  A forward pass with stale prepared weights runs the Winograd layers on the OLD weights and the
 * strided / 1x1 / stem / head layers, which read the raw parameters, on the new ones: prepare again after every weight update.
 *
 * FORWARD.  dl_pose_net_forward(image_prev, image_cur) enqueues: the input interleave (two planar [B][4][H][W] images with element
 * scan strides prev_ss / cur_ss >= 4*H*W, channel stride H*W -> [B][H][W][8], channels 0..3 = image_prev: a bit copy, what
 * torch.cat(dim=1).permute(0,2,3,1).contiguous() does), conv1 + activation, the pooling, per block conv (+ activation), the 1x1
 * shortcut, conv (+ shortcut + activation), dl_mean_hw_nhwc_f32, dl_heads_fwd and dl_quat_to_T_fwd with eps 1e-12.
 *   translation [B][3], quaternion [B][4] (x,y,z,w; divided by the norm over the whole batch, as the reference's model.py:114),
 *   T [B][4][4] out.  workspace: dl_pose_net_workspace_bytes bytes, 256-byte aligned, need not be initialised: four rotating
 *   activation slots (a block's input, y1, shortcut and y2; the stem's interleaved input, conv1 output and pooled map use the same
 *   slots first), the pooling's int8 window plane, the largest split-K scratch of dl_wino_conv3x3_workspace_bytes, the pooled
 *   feature and the heads' saved activations -- each carved at a 256-byte boundary.  Both size functions are host arithmetic (no GPU
 *   needed) and return 0 with a text in dl_last_error for a refused net or shape.
 *
 * STREAMING ODOMETRY.  dl_odometry_push projects ONLY the new scan (dl_project, S = 1: pts [3][pts_cs] planar fp32, n_points columns
 * in use) into image_cur [4][H][W] and runs the forward on (image_prev, image_cur) with B = 1; the caller swaps the two image
 * buffers between calls, the library keeps no state.  image_prev == NULL only projects (the first scan; translation, quaternion and T
 * may then be NULL and are not written).  offs is a caller-owned int32 [2] device vector the call overwrites (the CSR offsets {0,
 * n_points}, written by a kernel on `stream`).  workspace: dl_odometry_workspace_bytes(net, sensor, max_points, H, W) bytes, 256-byte
 * aligned, H and W being the sensor's; every push needs 0 <= n_points <= max_points (the projection's staging records are the tail of
 * the workspace).  The reference's normalization_scaling rescales both clouds per pair and is not served: the previous image could
 * not be reused.
 *
 * dl_odometry_push_records is dl_odometry_push with the projection swapped for dl_project_records (S = 1): the new scan arrives as
 * n_records raw records (device) with a dl_record_layout, filter included, and nothing has to be filtered, compacted or transposed
 * first.  The same image_prev == NULL first-scan rule, the same offs [2] vector written on the stream, the same forward, the same
 * refusals (plus the layout's, before any launch).  Its workspace is dl_odometry_workspace_bytes(net, sensor, 0, H, W) bytes for ANY
 * n_records: the records path keeps no staging records, so nothing in the workspace grows with the scan.
 */
#define DL_POSE_ACT_TANH 1
#define DL_POSE_ACT_RELU 2
#define DL_POSE_NET_MAX_BLOCKS 16
typedef struct {
  int32_t cin, cout;             /* channels of the block's input / of its two convolutions' outputs */
  int32_t stride_h, stride_w;    /* stride of the first convolution and of the shortcut */
  int32_t has_downsample;        /* 1: the shortcut is the strided 1x1 convolution wd */
  const float *w1, *w2, *wd;
} dl_pose_block;
typedef struct {
  int32_t act;                   /* DL_POSE_ACT_TANH / DL_POSE_ACT_RELU (config activation_fct) */
  int32_t n_blocks;              /* 1..DL_POSE_NET_MAX_BLOCKS (the reference: 8) */
  const float* conv1_w;
  dl_pose_block blocks[DL_POSE_NET_MAX_BLOCKS];
  dl_heads_params heads;
  int32_t F, R, Hd;              /* pooled feature width, resnet_outputs, hidden width of the heads (the reference: 512, 1000, 100) */
} dl_pose_net;
size_t dl_pose_net_prepared_bytes(const dl_pose_net* net, int32_t B, int32_t H, int32_t W);
int dl_pose_net_prepare(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, void* prepared, dl_stream stream);
size_t dl_pose_net_workspace_bytes(const dl_pose_net* net, int32_t B, int32_t H, int32_t W);
int dl_pose_net_forward(const dl_pose_net* net, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur,
                        int64_t cur_ss, int32_t B, int32_t H, int32_t W, void* workspace, float* translation, float* quaternion, float* T,
                        dl_stream stream);
size_t dl_odometry_workspace_bytes(const dl_pose_net* net, const dl_sensor* sensor, int32_t max_points, int32_t H, int32_t W);
int dl_odometry_push(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const float* pts, int64_t pts_cs,
                     int32_t n_points, int32_t* offs, const float* image_prev, float* image_cur, void* workspace, float* translation,
                     float* quaternion, float* T, dl_stream stream);
int dl_odometry_push_records(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const void* records, int32_t n_records,
                             const dl_record_layout* layout, int32_t* offs, const float* image_prev, float* image_cur, void* workspace,
                             float* translation, float* quaternion, float* T, dl_stream stream);

/*
 * THE SAME IN HALF PRECISION (additive, ABI 10 as it stands): the *_h family serves a network trained under amp_dtype with the kernels it was
 * trained on.  dtype is DL_DTYPE_F16 or DL_DTYPE_BF16 (anything else: DL_ERR_UNSUPPORTED, size functions 0); dl_pose_net, its fp32
 * parameters, the scope, the refusals and every other argument are those of the fp32 family above.  The walk is what the Python eval
 * path does inside torch.autocast (ResNetModified.pooled_features_drop, half branch, + OdometryModel._fused), the same launches on the
 * same operands, hence the same bits: the interleave and conv1 + activation in fp32, dl_pool3x3s12_nhwc_fwd_h (fp32 -> half; the
 * Python path pools in fp32 and casts, the same values), per block dl_conv2d_nhwc_h (+ activation), the 1x1 dl_conv2d_nhwc_h shortcut,
 * dl_conv2d_nhwc_h (+ shortcut + activation), dl_mean_hw_nhwc_h to the fp32 feature, dl_heads_fwd and dl_quat_to_T_fwd in fp32.  Half
 * precision has ONE kernel family for every layer, so the native and the Python walk agree at every shape.
 *   PREPARED WEIGHTS: dl_pose_net_prepare_h converts EVERY trunk weight once (dl_conv_weights_batch_h, forward layout only) into
 *   w_fwd [taps][K][C] arrays in weight order (w1, w2, wd per block), each at a 256-byte boundary of `prepared`
 *   (dl_pose_net_prepared_bytes_h bytes = the sum of taps*K*C*2, each rounded up to 256).  conv1 and the heads keep reading the fp32
 *   parameters.  Stale prepared weights run the whole trunk on the OLD weights: prepare again after every weight update.
 *   WORKSPACE: dl_pose_net_workspace_bytes_h bytes: the four rotating slots (the two stem slots sized for fp32, everything behind the
 *   pooling for half), the pooled feature and the heads' saved activations.  No fp32 pooled map, no window plane, no split-K scratch.
 *   dl_odometry_workspace_bytes_h / dl_odometry_push_h / dl_odometry_push_records_h: the streaming calls on that forward; images,
 *   points, records and outputs stay fp32.  Nothing is allocated per call, nothing synchronises, every call is capturable.
 */
size_t dl_pose_net_prepared_bytes_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype);
int dl_pose_net_prepare_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype, void* prepared, dl_stream stream);
size_t dl_pose_net_workspace_bytes_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype);
int dl_pose_net_forward_h(const dl_pose_net* net, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur,
                          int64_t cur_ss, int32_t B, int32_t H, int32_t W, int32_t dtype, void* workspace, float* translation,
                          float* quaternion, float* T, dl_stream stream);
size_t dl_odometry_workspace_bytes_h(const dl_pose_net* net, const dl_sensor* sensor, int32_t max_points, int32_t H, int32_t W,
                                     int32_t dtype);
int dl_odometry_push_h(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const float* pts, int64_t pts_cs,
                       int32_t n_points, int32_t* offs, const float* image_prev, float* image_cur, int32_t dtype, void* workspace,
                       float* translation, float* quaternion, float* T, dl_stream stream);
int dl_odometry_push_records_h(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const void* records,
                               int32_t n_records, const dl_record_layout* layout, int32_t* offs, const float* image_prev,
                               float* image_cur, int32_t dtype, void* workspace, float* translation, float* quaternion, float* T,
                               dl_stream stream);

/*
 * POSE QUALITY BEHIND A PUSH (csrc/info.hip; additive, ABI 10 as it stands): dl_odometry_quality is called after dl_odometry_push / _push_records
 * (either family: it reads only the two fp32 images and T, never the network) and answers how well the pair constrains T.
 * The library keeps no state: beside each of the two ping-pong images the caller owns one dl_scan_geometry record
 *   normals [3][H][W] planar, packed_image [H][W][4] = (x, y, z, range), packed_normals [H][W][4] = (nx, ny, nz, 0), 16-byte aligned,
 * swapped together with the images.  The call
 *   1. fills the record of image_cur: dl_normals (S = 1) with the caller's half_rows, half_cols, epsilon_range, min_neighbors, and the
 *      packed twin of the image (a bit copy);
 *   2. when image_prev and geometry_prev (filled by the previous call) are given: dl_nn_correspond with source = current, target =
 *      previous -- the direction of T in dl_odometry_push --, need_without_normals = 0, nn_pix and match in the workspace;
 *   3. dl_icp_information with B = 1: info [6][6], rhs [6], stats [2], covariance [6][6] (fp64) and status [1] as documented there.
 *      The covariance is that of the scan-to-scan transform T under a left perturbation, in the PREVIOUS scan's frame, row-major in
 *      the order (x, y, z, rotation about X, Y, Z) of nav_msgs/Odometry's pose.covariance.
 * image_prev == NULL (the first scan) only fills the record; T, workspace and the outputs may then be NULL and are not written.
 *   workspace  dl_odometry_quality_workspace_bytes(sensor, H, W) bytes (H, W the sensor's; host arithmetic, 0 with a text for a refused
 *              sensor), 256-byte aligned: nn_pix | match | the search's scratch | the partial rows.
 * Null or misaligned pointers, a bad sensor and a window outside dl_normals' range are DL_ERR_INVALID_ARGUMENT before any launch.
 * Nothing is allocated, nothing synchronises, the call is capturable.  normalization_scaling is not served, as in dl_odometry_push.
 */
typedef struct {
  float* normals;          /* [3][H][W] */
  float* packed_image;     /* [H][W][4] */
  float* packed_normals;   /* [H][W][4] */
} dl_scan_geometry;
size_t dl_odometry_quality_workspace_bytes(const dl_sensor* sensor, int32_t H, int32_t W);
int dl_odometry_quality(const dl_sensor* sensor, const float* image_prev, const dl_scan_geometry* geometry_prev, const float* image_cur,
                        const dl_scan_geometry* geometry_cur, const float* T, int32_t half_rows, int32_t half_cols, float epsilon_range,
                        int32_t min_neighbors, void* workspace, double* info, double* rhs, double* stats, double* covariance,
                        int32_t* status, dl_stream stream);

/*
 * What the convolution dispatch would launch (for tests and tools; host only, nothing is enqueued): runs the matching entry point's
 * own code -- argument checks, tile choice, slab / split plans -- with every launch replaced by a record, and writes one line per
 * launch into buf:   <kernel instantiation> grid=<x>x<y>x<z> block=<threads>[ slabs=<n> ...][ splits=<n>]
 * e.g. "k_wino_conv<32, false, true> grid=64x1x1 block=512 splits=4".  The instantiation is the compiler's own spelling of the
 * template the launch names, so the text cannot drift from the dispatch.
 *   op      DL_PLAN_*: CONV (dl_conv2d_nhwc_f32 / _h; mode = transposed), DGRAD_STRIDED (dl_conv2d_dgrad_strided_nhwc_f32 / _h; mode =
 *           dense; H, W = the layer's input image, C its input and K its output channels), WINO_CONV (dl_wino_conv3x3_nhwc_f32;
 *           mode 0 = with a workspace, 1 = workspace NULL), WGRAD / WGRAD_BATCH (dl_conv2d_wgrad_nhwc_f32 / _h and a one-layer
 *           dl_conv2d_wgrad_batch_*), WINO_WGRAD / WINO_WGRAD_BATCH (dl_wino_wgrad3x3_nhwc_f32 and its one-layer batch form)
 *   dtype   DL_DTYPE_F32 selects the fp32 entry point, _F16 / _BF16 the half-precision one (the Winograd ops are fp32 only)
 *   cu_count > 0 stands in for the device's CU count (the Winograd split plan depends on it): the query then needs no GPU;
 *           0 asks the current device (256 where there is none).
 * Returns the entry point's own status (dl_last_error has its text), DL_ERR_INVALID_ARGUMENT when buf is too small.
 */
#define DL_PLAN_CONV 0
#define DL_PLAN_DGRAD_STRIDED 1
#define DL_PLAN_WINO_CONV 2
#define DL_PLAN_WGRAD 3
#define DL_PLAN_WGRAD_BATCH 4
#define DL_PLAN_WINO_WGRAD 5
#define DL_PLAN_WINO_WGRAD_BATCH 6
int dl_conv_plan_describe(int32_t op, int32_t dtype, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize,
                          int32_t stride_h, int32_t stride_w, int32_t mode, int32_t cu_count, char* buf, size_t buf_bytes);

/* Measurement aid (bench.py, tools/): between dl_profile_begin and dl_profile_end every launch of the convolution families
 * (fp32 direct / Winograd / weight gradient, half-precision forward / weight gradient) carries its own begin / end timestamps
 * (two HIP events filled by hipExtLaunchKernelGGL on the launch stream), so that a kernel's duration can be read inside real
 * training steps.  dl_profile_end returns one row per (kernel, pass, shape): launches, summed kernel time [ms], the
 * floating-point operations the algorithm issued on the matrix cores (Winograd: 16 multiply-adds per 2x2 tile and (c,k) pair,
 * a direct convolution: 36) and the compulsory HBM bytes (operands once + result once).  One profile at a time (mutex-guarded;
 * the only mutable process-wide state of the library); only_kernel restricts the timing to one kernel family (an event-carrying
 * launch costs the host a few microseconds more); launches beyond max_launches are counted in *untimed; not
 * graph-capturable while a profile is open.  capacity < the number of rows: the first `capacity` rows are written, *count is
 * the full number. */
typedef struct {
  char name[96];     /* "<kernel> <pass> N<n> <H>x<W> C<c> K<k>" */
  int32_t launches;
  double ms, flop, bytes;
} dl_profile_row;
int dl_profile_begin(int32_t max_launches, const char* only_kernel /* NULL: all; else one kernel family, e.g. "k_wino_conv" */);
/* While paused (paused != 0) launches pass without events and are not counted: bench.py times every fourth step of its timed
 * region only -- an event-carrying launch costs the host ~0.25 ms, and 26 of them per step made a fresh box host-bound. */
int dl_profile_pause(int32_t paused);
int dl_profile_end(dl_profile_row* rows, int32_t capacity, int32_t* count, int32_t* untimed);

#ifdef __cplusplus
}
#endif
#endif /* DELORA_HIP_H */
