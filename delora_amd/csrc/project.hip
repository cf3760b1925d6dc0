// Spherical projection: points -> range image, nearest point per pixel.
//
// Replaces ImageProjectionLayer.project_to_img (reference src/utility/projection.py:48-106).  The
// reference sorts the scan by range, copies u/v to the host, runs a sequential first-wins loop and
// copies the result back (:63-67, :80-91).  Here every point votes with an order-independent 64-bit
// atomicMin on key = range_bits << 32 | point_index (range >= 0, so the fp32 bit pattern orders like
// the value; the index breaks exact ties toward the earlier point, which is what a stable sort gives),
// and a second pass turns winning keys into image channels.  No sort, no host round trip, and the
// result does not depend on the execution order of the atomics.
//
// What bounds the vote (tools/exp/scatter_probe.hip, 16 scans x 141k points): the arithmetic + loads take 17 us; the
// atomics alone take 89 us when the points arrive in random order (every vote moves another 64-byte line of the key
// plane into the voting XCD's L2: 2.3 M line transfers) and 23 us when they arrive in sensor / raster order, as the
// reference's stored scans do (8 neighbouring keys share a line).  Tried and dropped: one XCD per key plane with
// dynamically claimed scans (4x slower: the claim protocol serialises), 32-bit keys (same line traffic).
//
// HBM traffic per scan (N points, P = H*W pixels, fp32): the vote reads 12 B*N and writes a 16-byte staging record (x,y,z,range) per
// point (+16 B for channels 3..5 when the scan carries stored normals), the 8-byte atomics stay in the L2 for a 1 MiB key plane;
// resolve reads 8 B*P keys, gathers ONE 16-byte record per occupied pixel (two with normals) and writes 16 B*P planar + 16 B*P
// packed image + 4 B*P map: algorithmic 12N + 36P bytes.
//
// Round 5, what the counters said (profiles/r04_geometry_pmc.json: resolve fetched 253 MB for 42 MB of useful bytes):
//   * the winner's x, y, z came from THREE planes at a random column -- three 64-byte lines for 12 useful bytes.  The vote has
//     x, y, z and the range in registers anyway: it now leaves them behind as one float4 per point (coalesced 16-byte stores),
//     and a winner is ONE 16-byte load;
//   * the grid was (pixel blocks, scans) with the pixel blocks fastest: consecutive workgroups go to consecutive XCDs, so every one
//     of the eight L2s pulled every scan's point buffer and key plane.  The grid is now one-dimensional and maps workgroup b to
//     scan 8*(b / 8 / G) + (b % 8): all workgroups of a scan land on the same XCD (workgroups are dealt round-robin over the XCDs),
//     one L2 holds a scan's keys and staging records, and the vote's atomics on a key plane come from ONE L2.  The mapping is a
//     performance hint only: the result does not depend on where a workgroup runs.
#include "common.h"

// workgroup -> (scan, chunk): see above.  S < 8 scans keep the plain mapping (an XCD-per-scan split would idle most of the chip);
// G < 0 selects the plain mapping too (DL_PROJECT_PLAIN_GRID=1: A/B measurements).
__device__ __forceinline__ bool project_block(int S, int G, int& s, int& chunk) {
  const int b = blockIdx.x;
  if (G > 0 && S >= 8) {
    const int q = b >> 3;
    s = (q / G) * 8 + (b & 7);
    chunk = q % G;
  } else {
    if (G < 0) G = -G;
    s = b / G;
    chunk = b % G;
  }
  return s < S;
}

static inline bool project_plain_grid() {
  static const bool plain = [] { const char* e = getenv("DL_PROJECT_PLAIN_GRID"); return e && e[0] == '1'; }();
  return plain;
}
static inline int project_grid(int S, int G) { return (S >= 8 && !project_plain_grid()) ? 8 * G * ((S + 7) / 8) : S * G; }
static inline int project_garg(int S, int G) { return (S >= 8 && project_plain_grid()) ? -G : G; }

__global__ __launch_bounds__(DL_BLOCK) void k_project_scatter(
    const float* __restrict__ pts, int64_t cs, const int32_t* __restrict__ offs, int S, int C, int G, SensorK sen,
    unsigned long long* __restrict__ keys, float4* __restrict__ stage0, float4* __restrict__ stage1, float* __restrict__ uvr, int64_t n_cols) {
  int s, chunk;
  if (!project_block(S, G, s, chunk)) return;
  const int n0 = offs[s];
  const int n = offs[s + 1] - n0;
  unsigned long long* kp = keys + (size_t)s * sen.HW;
  const int stride = (G < 0 ? -G : G) * DL_BLOCK;
  for (int i = chunk * DL_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t g = (int64_t)n0 + i;
    const float x = pts[g], y = pts[cs + g], z = pts[2 * cs + g];
    const float r = norm3f(x, y, z);
    // The pixel is rint() of the reference's fp32 expression on a correctly rounded atan2 (coord_u / coord_v: fp64
    // evaluation, ~600 instructions per coordinate).  atan2f gives the same pixel unless the coordinate lies within
    // tol of k + 1/2; only those points (0.3 % of them, ~20 % of the waves) and callers that ask for the coordinates
    // themselves take the fp64 evaluation.
    float u = coord_u_fast(x, y, sen);
    float v = coord_v_fast(x, y, z, sen);
    if (uvr || near_rounding_boundary(u, sen.tol_u) || near_rounding_boundary(v, sen.tol_v)) {
      u = coord_u(x, y, sen);
      v = coord_v(x, y, z, sen);
    }
    if (uvr) { uvr[g] = u; uvr[cs + g] = v; uvr[2 * cs + g] = r; }
    if (g >= n_cols) continue;                  // offsets that disagree with the sized workspace: no store, no vote
    stage0[g] = make_float4(x, y, z, r);
    if (stage1)
      stage1[g] = make_float4(pts[3 * cs + g], C > 4 ? pts[4 * cs + g] : 0.f, C > 5 ? pts[5 * cs + g] : 0.f, 0.f);
    const float ru = rintf(u), rv = rintf(v);   // torch.round: half to even
    if (ru <= sen.wm1f && ru >= 0.0f && rv <= sen.hm1f && rv >= 0.0f) {   // projection.py:74-75
      const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned int)i;
      atomicMin(&kp[(int)rv * sen.W + (int)ru], key);
    }
  }
}

__global__ __launch_bounds__(DL_BLOCK) void k_project_resolve(
    const float* __restrict__ pts, int64_t cs, const int32_t* __restrict__ offs, int S, int C, int G, SensorK sen,
    const unsigned long long* __restrict__ keys, const float4* __restrict__ stage0, const float4* __restrict__ stage1,
    float* __restrict__ image4, float* __restrict__ aux, float4* __restrict__ packed, float4* __restrict__ packed_aux,
    int32_t* __restrict__ pix2pt, int32_t* __restrict__ kept) {
  int s, chunk;
  if (!project_block(S, G, s, chunk)) return;
  const int px = chunk * DL_BLOCK + threadIdx.x;
  const int HW = sen.HW;
  bool occupied = false;
  if (px < HW) {
    const unsigned long long key = keys[(size_t)s * HW + px];
    float* img = image4 + (size_t)s * 4 * HW + px;
    occupied = key != ~0ull;
    if (occupied) {
      const int idx = (int)(unsigned int)(key & 0xffffffffu);
      const int64_t g = (int64_t)offs[s] + idx;
      const float4 p = stage0[g];               // x, y, z and the range the vote computed (bit-equal to the key's upper half)
      img[0] = p.x; img[HW] = p.y; img[2 * HW] = p.z; img[3 * HW] = p.w;
      if (packed) packed[(size_t)s * HW + px] = p;
      if (C > 3) {
        const float4 a = stage1[g];
        const float a3[3] = {a.x, a.y, a.z};
        for (int c = 3; c < C; ++c)
          aux[((size_t)s * (C - 3) + (c - 3)) * HW + px] = c < 6 ? a3[c - 3] : pts[c * cs + g];
        if (packed_aux) packed_aux[(size_t)s * HW + px] = make_float4(a.x, a.y, a.z, 0.f);
      }
      pix2pt[(size_t)s * HW + px] = idx;
    } else {
      img[0] = 0.f; img[HW] = 0.f; img[2 * HW] = 0.f; img[3 * HW] = 0.f;
      if (packed) packed[(size_t)s * HW + px] = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c = 3; c < C; ++c) aux[((size_t)s * (C - 3) + (c - 3)) * HW + px] = 0.f;
      if (packed_aux) packed_aux[(size_t)s * HW + px] = make_float4(0.f, 0.f, 0.f, 0.f);
      pix2pt[(size_t)s * HW + px] = -1;
    }
  }
  if (kept) {   // optional statistic: one atomic per workgroup (the training step passes NULL)
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const unsigned long long m = __ballot(occupied);
    if ((threadIdx.x & (DL_WAVE - 1)) == 0 && m) atomicAdd(&s_cnt, (int)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&kept[s], s_cnt);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rotation augmentation inside the vote (dl_project_rotated): scan s is replaced by R_s p (and R_s n for stored normals) where x, y,
// z are in registers anyway -- no extra pass over the points and no write to the caller's buffer.  One row of a rotated point is
// (r0*x + r1*y) + r2*z, every operation rounded to fp32, nothing contracted (the pragma holds under any -ffp-contract setting), so
// that a numpy fp32 expression reproduces it bit for bit.
__device__ __forceinline__ float rot_row(float r0, float r1, float r2, float x, float y, float z) {
#pragma clang fp contract(off)
  const float a = r0 * x;
  const float b = r1 * y;
  const float c = r2 * z;
  const float ab = a + b;
  return ab + c;
}

// The vote of k_project_scatter (kept there word for word: its code is not touched) on the rotated point.  rot [S][9] row-major; a
// scan whose nine words are the bit pattern of the identity is NOT multiplied (x * 1 + y * 0 would turn -0.0 into +0.0 and inf into
// NaN): the decision depends on the scan alone, so it is uniform per workgroup.  Everything downstream -- range, coordinates, uvr,
// the staging records k_project_resolve gathers from -- sees the rotated values only.
__global__ __launch_bounds__(DL_BLOCK) void k_project_scatter_rot(
    const float* __restrict__ pts, int64_t cs, const int32_t* __restrict__ offs, int S, int C, int G, SensorK sen,
    unsigned long long* __restrict__ keys, float4* __restrict__ stage0, float4* __restrict__ stage1, float* __restrict__ uvr, int64_t n_cols,
    const float* __restrict__ rot) {
  int s, chunk;
  if (!project_block(S, G, s, chunk)) return;
  const int n0 = offs[s];
  const int n = offs[s + 1] - n0;
  float R[9];
  bool rotate = false;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    R[k] = rot[(size_t)s * 9 + k];
    rotate |= __float_as_uint(R[k]) != ((k & 3) == 0 ? 0x3f800000u : 0u);
  }
  unsigned long long* kp = keys + (size_t)s * sen.HW;
  const int stride = (G < 0 ? -G : G) * DL_BLOCK;
  for (int i = chunk * DL_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t g = (int64_t)n0 + i;
    float x = pts[g], y = pts[cs + g], z = pts[2 * cs + g];
    if (rotate) {
      const float px = x, py = y, pz = z;
      x = rot_row(R[0], R[1], R[2], px, py, pz);
      y = rot_row(R[3], R[4], R[5], px, py, pz);
      z = rot_row(R[6], R[7], R[8], px, py, pz);
    }
    const float r = norm3f(x, y, z);
    float u = coord_u_fast(x, y, sen);
    float v = coord_v_fast(x, y, z, sen);
    if (uvr || near_rounding_boundary(u, sen.tol_u) || near_rounding_boundary(v, sen.tol_v)) {
      u = coord_u(x, y, sen);
      v = coord_v(x, y, z, sen);
    }
    if (uvr) { uvr[g] = u; uvr[cs + g] = v; uvr[2 * cs + g] = r; }
    if (g >= n_cols) continue;                  // offsets that disagree with the sized workspace: no store, no vote
    stage0[g] = make_float4(x, y, z, r);
    if (stage1) {
      float a = pts[3 * cs + g], b = C > 4 ? pts[4 * cs + g] : 0.f, c = C > 5 ? pts[5 * cs + g] : 0.f;
      if (rotate && C > 5) {                    // channels 3..5 are a vector (the stored normals) only when all three are there
        const float pa = a, pb = b, pc = c;
        a = rot_row(R[0], R[1], R[2], pa, pb, pc);
        b = rot_row(R[3], R[4], R[5], pa, pb, pc);
        c = rot_row(R[6], R[7], R[8], pa, pb, pc);
      }
      stage1[g] = make_float4(a, b, c, 0.f);
    }
    const float ru = rintf(u), rv = rintf(v);   // torch.round: half to even
    if (ru <= sen.wm1f && ru >= 0.0f && rv <= sen.hm1f && rv >= 0.0f) {   // projection.py:74-75
      const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned int)i;
      atomicMin(&kp[(int)rv * sen.W + (int)ru], key);
    }
  }
}

// Rotations of one training step from uniform draws (the reference's dead branch, src/deploy/deployer.py:205-214, per sample):
// row 2b is the exact identity (scan 1 is never rotated), row 2b+1 is Rodrigues' matrix of the unit axis d and the angle
// a = (u3 - 0.5) * magnitude: R = cos(a) I + sin(a) [d]x + (1 - cos(a)) d d^T.  The axis is (0, 0, 1) with only_yaw, else the three
// draws normalised (all in [0, 1): the reference's positive-octant quirk).  a == 0, or three zero draws (no axis), give the exact
// identity; only_yaw writes row and column 2 as exact 0 / 1.
__global__ void k_rotations_from_draws(const float* __restrict__ draws, int B, int only_yaw, float magnitude, float* __restrict__ rot) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float* I = rot + (size_t)b * 18;
  float* R = I + 9;
#pragma unroll
  for (int k = 0; k < 9; ++k) I[k] = (k & 3) == 0 ? 1.f : 0.f;
  const float a = (draws[4 * b + 3] - 0.5f) * magnitude;
  float dx = 0.f, dy = 0.f, dz = 1.f;
  bool none = a == 0.f;
  if (!only_yaw) {
    dx = draws[4 * b]; dy = draws[4 * b + 1]; dz = draws[4 * b + 2];
    const float len = norm3f(dx, dy, dz);
    none |= !(len > 0.f);
    dx /= len; dy /= len; dz /= len;
  }
  if (none) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k & 3) == 0 ? 1.f : 0.f;
    return;
  }
  const float sn = sinf(a), cn = cosf(a), t = 1.f - cn;
  if (only_yaw) {
    R[0] = cn; R[1] = -sn; R[2] = 0.f;
    R[3] = sn; R[4] = cn; R[5] = 0.f;
    R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
    return;
  }
  R[0] = cn + t * dx * dx; R[1] = t * dx * dy - sn * dz; R[2] = t * dx * dz + sn * dy;
  R[3] = t * dx * dy + sn * dz; R[4] = cn + t * dy * dy; R[5] = t * dy * dz - sn * dx;
  R[6] = t * dx * dz - sn * dy; R[7] = t * dy * dz + sn * dx; R[8] = cn + t * dz * dz;
}

// (advisor, round 5) the staging records behind the key plane are read and written as float4: the plane's size is rounded up to 16 bytes
// (S*H*W odd would leave them 8-byte aligned); the vote's staging stores are guarded by the record count the workspace was sized for
static inline size_t project_keys_bytes(int32_t S, int32_t H, int32_t W) { return (((size_t)S * H * W * sizeof(uint64_t)) + 15) & ~(size_t)15; }

extern "C" size_t dl_project_workspace_bytes(int32_t S, int32_t H, int32_t W, int64_t n_cols, int32_t C) {
  if (S <= 0 || H <= 0 || W <= 0 || n_cols < 0 || C < 3) return 0;
  return project_keys_bytes(S, H, W) + (size_t)n_cols * 16 * (C > 3 ? 2 : 1);
}

// dl_project (rot == NULL: the launches it always made) and dl_project_rotated behind one set of refusals
static int project_impl(const char* who, const float* pts, int64_t pts_cs, int64_t n_cols, const int32_t* offs, int32_t S, int32_t C,
                        int32_t max_n, const dl_sensor* sensor, float* image4, float* aux, float* packed,
                        float* packed_aux, int32_t* pix2pt, void* workspace, int32_t* kept, float* uvr, const float* rot,
                        dl_stream stream) {
  if ((!pts && max_n > 0) || !offs || !sensor || !image4 || !pix2pt || !workspace)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
  if (S <= 0 || C < 3 || sensor->H < 2 || sensor->W < 2 || max_n < 0 || n_cols < 0 || n_cols > pts_cs)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes S=%d C=%d H=%d W=%d max_n=%d n_cols=%lld pts_cs=%lld", who, S, C,
                   sensor->H, sensor->W, max_n, (long long)n_cols, (long long)pts_cs);
  if (C > 3 && !aux) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: C=%d needs an aux image", who, C);
  if (packed_aux && C < 6) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: packed_aux needs C >= 6 (got %d)", who, C);
  // the staging records behind the key plane are read and written as float4
  if ((uintptr_t)workspace & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  const SensorK sen = make_sensor(sensor);
  // workspace = key plane [S][H*W] uint64 | staging records [n_cols] float4 (x,y,z,range) | [n_cols] float4 (channels 3..5) if C > 3
  unsigned long long* keys = (unsigned long long*)workspace;
  float4* stage0 = (float4*)((char*)workspace + project_keys_bytes(S, sen.H, sen.W));
  float4* stage1 = C > 3 ? stage0 + n_cols : nullptr;
  // the key plane and the counters are initialised by a kernel on the same stream (dl_fill_words: a kernel node, not a
  // memset node, when the step is captured into a HIP graph); a launch failure is reported by dl_check_launch below
  dl_fill_words(keys, 0xffffffffu, (size_t)S * sen.HW * 2, st);
  if (kept) dl_fill_words(kept, 0u, (size_t)S, st);
  if (max_n > 0) {
    int G = (max_n + DL_BLOCK - 1) / DL_BLOCK;
    if (G > 1024) G = 1024;
    if (rot)
      hipLaunchKernelGGL(k_project_scatter_rot, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, pts, pts_cs, offs, S, C, project_garg(S, G),
                         sen, keys, stage0, stage1, uvr, n_cols, rot);
    else
      hipLaunchKernelGGL(k_project_scatter, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, pts, pts_cs, offs, S, C, project_garg(S, G),
                         sen, keys, stage0, stage1, uvr, n_cols);
  }
  const int G = (sen.HW + DL_BLOCK - 1) / DL_BLOCK;
  hipLaunchKernelGGL(k_project_resolve, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, pts, pts_cs, offs, S, C, project_garg(S, G), sen,
                     (const unsigned long long*)keys, (const float4*)stage0, (const float4*)stage1, image4, aux,
                     (float4*)packed, (float4*)packed_aux, pix2pt, kept);
  return dl_check_launch(who);
}

extern "C" int dl_project(const float* pts, int64_t pts_cs, int64_t n_cols, const int32_t* offs, int32_t S, int32_t C,
                          int32_t max_n, const dl_sensor* sensor, float* image4, float* aux, float* packed,
                          float* packed_aux, int32_t* pix2pt, void* workspace, int32_t* kept, float* uvr,
                          dl_stream stream) {
  return project_impl("dl_project", pts, pts_cs, n_cols, offs, S, C, max_n, sensor, image4, aux, packed, packed_aux, pix2pt, workspace, kept,
                      uvr, nullptr, stream);
}

extern "C" int dl_project_rotated(const float* pts, int64_t pts_cs, int64_t n_cols, const int32_t* offs, int32_t S, int32_t C,
                                  int32_t max_n, const dl_sensor* sensor, float* image4, float* aux, float* packed,
                                  float* packed_aux, int32_t* pix2pt, void* workspace, int32_t* kept, float* uvr,
                                  const float* rot, dl_stream stream) {
  if ((uintptr_t)rot & 3) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_project_rotated: rot must be 4-byte aligned");
  return project_impl("dl_project_rotated", pts, pts_cs, n_cols, offs, S, C, max_n, sensor, image4, aux, packed, packed_aux, pix2pt,
                      workspace, kept, uvr, rot, stream);
}

extern "C" int dl_rotations_from_draws(const float* draws, int32_t B, int32_t only_yaw, float magnitude_rad, float* rot, dl_stream stream) {
  if (!draws || !rot) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_rotations_from_draws: null pointer argument");
  if (B <= 0 || !(fabsf(magnitude_rad) <= 3.402823466e38f))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_rotations_from_draws: bad sizes B=%d magnitude_rad=%g", B, (double)magnitude_rad);
  if (((uintptr_t)draws | (uintptr_t)rot) & 3) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_rotations_from_draws: draws and rot must be 4-byte aligned");
  hipLaunchKernelGGL(k_rotations_from_draws, dim3((B + DL_WAVE - 1) / DL_WAVE), dim3(DL_WAVE), 0, (hipStream_t)stream, draws, B, only_yaw ? 1 : 0,
                     magnitude_rad, rot);
  return dl_check_launch("dl_rotations_from_draws");
}

// ---------------------------------------------------------------------------------------------------------------------
// Records flavour: the scan as a sensor or a driver delivers it -- n records of point_step bytes with fp32 x, y, z at byte offsets
// (a KITTI .bin file: 16 / 0, 4, 8; a PointCloud2 message: its point_step and field offsets) -- and the reference node's filter
// (src/ros_utils/odometry_publisher.py:95-97) applied inside the vote.  The winner of a pixel is the smallest (range bits, index
// within the scan): a record that does not vote leaves every other record's key as it is, so skipping it gives the image that
// compacting the list first gives, with record indices in pix2pt instead of list positions.  No compaction pass, and no staging
// records either: the upper half of a winning key IS the range the vote computed, and resolve gathers x, y, z of the one winning
// record per occupied pixel from the record buffer itself (they share a 64-byte line for every step the layout check admits below
// 64).  HBM traffic per scan: the vote reads point_step * N bytes where the planar vote reads 12 N and writes 16 N.
// image coordinates of one point, the expressions of k_project_scatter (kept there word for word: its code is not touched): atan2f
// unless a coordinate lies near a rounding boundary
__device__ __forceinline__ void project_uv(float x, float y, float z, const SensorK& sen, float& u, float& v) {
  u = coord_u_fast(x, y, sen);
  v = coord_v_fast(x, y, z, sen);
  if (near_rounding_boundary(u, sen.tol_u) || near_rounding_boundary(v, sen.tol_v)) {
    u = coord_u(x, y, sen);
    v = coord_v(x, y, z, sen);
  }
}

// the vote of k_project_scatter: point i (index within its scan) with range r at coordinates (u, v) on its scan's key plane
__device__ __forceinline__ void project_vote(float u, float v, float r, int i, const SensorK& sen, unsigned long long* __restrict__ kp) {
  const float ru = rintf(u), rv = rintf(v);   // torch.round: half to even
  if (ru <= sen.wm1f && ru >= 0.0f && rv <= sen.hm1f && rv >= 0.0f) {   // projection.py:74-75
    const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned int)i;
    atomicMin(&kp[(int)rv * sen.W + (int)ru], key);
  }
}

struct RecordK {
  int step, wx, wy, wz;     // record length in bytes, x / y / z as dword offsets within a record
  unsigned int filter;
  float min_range;
};

// np.linalg.norm(xyz, axis=0) of the reference's filter: sqrt((x*x + y*y) + z*z), every operation rounded to fp32, nothing fused.
// NOT norm3f: near the 0.3 m threshold the two fall on different sides for ~1 % of the points within a few ulp of it.  The pragma keeps the three
// operations apart under any -ffp-contract setting; sqrtf is correctly rounded (common.h: __fsqrt_rn is not, it lowers to the
// native approximation here, and __fmul_rn / __fadd_rn are plain operators that a contracting build would fuse all the same).
__device__ __forceinline__ float range_np(float x, float y, float z) {
#pragma clang fp contract(off)
  const float xx = x * x;
  const float yy = y * y;
  const float zz = z * z;
  const float s2 = xx + yy;
  const float s3 = s2 + zz;
  return sqrtf(s3);
}

// does a record take part?  -0.0 counts as zero, NaN does not; a NaN range or a NaN comparison drops the record
__device__ __forceinline__ bool record_passes(float x, float y, float z, const RecordK& lay) {
  if ((lay.filter & DL_RECORDS_DROP_ZERO) && !(x != 0.0f && y != 0.0f && z != 0.0f)) return false;
  if ((lay.filter & DL_RECORDS_MIN_RANGE) && !(range_np(x, y, z) > lay.min_range)) return false;
  return true;
}

// word k of a 16-byte record (k is uniform: three selects, no indexed register file)
__device__ __forceinline__ float record_word(const float4& q, int k) { return k == 0 ? q.x : k == 1 ? q.y : k == 2 ? q.z : q.w; }

// VEC16: 16-byte records on a 16-byte aligned base, one dwordx4 load per lane; else three dword loads at the record stride
template <bool VEC16>
__global__ __launch_bounds__(DL_BLOCK) void k_project_records_scatter(
    const float* __restrict__ rec, int64_t n_records, RecordK lay, const int32_t* __restrict__ offs, int S, int G, SensorK sen,
    unsigned long long* __restrict__ keys, int32_t* __restrict__ n_pass) {
  int s, chunk;
  if (!project_block(S, G, s, chunk)) return;
  const int n0 = offs[s];
  const int n = offs[s + 1] - n0;
  unsigned long long* kp = keys + (size_t)s * sen.HW;
  const int stride = (G < 0 ? -G : G) * DL_BLOCK;
  const int64_t step_w = lay.step >> 2;
  int passed = 0;
  for (int i = chunk * DL_BLOCK + threadIdx.x; i < n; i += stride) {
    const int64_t g = (int64_t)n0 + i;
    if (g < 0 || g >= n_records) continue;      // offsets that disagree with the record count: no load, no vote
    float x, y, z;
    if (VEC16) {
      const float4 q = reinterpret_cast<const float4*>(rec)[g];
      x = record_word(q, lay.wx); y = record_word(q, lay.wy); z = record_word(q, lay.wz);
    } else {
      const float* p = rec + g * step_w;
      x = p[lay.wx]; y = p[lay.wy]; z = p[lay.wz];
    }
    if (!record_passes(x, y, z, lay)) continue;
    ++passed;
    const float r = norm3f(x, y, z);            // the key's range is dl_project's (fused), whatever the filter compared
    float u, v;
    project_uv(x, y, z, sen, u, v);
    project_vote(u, v, r, i, sen, kp);
  }
  if (n_pass) {   // optional statistic: one atomic per workgroup
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
#pragma unroll
    for (int o = DL_WAVE / 2; o > 0; o >>= 1) passed += __shfl_xor(passed, o, DL_WAVE);
    if ((threadIdx.x & (DL_WAVE - 1)) == 0 && passed) atomicAdd(&s_cnt, passed);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&n_pass[s], s_cnt);
  }
}

__global__ __launch_bounds__(DL_BLOCK) void k_project_records_resolve(
    const float* __restrict__ rec, RecordK lay, const int32_t* __restrict__ offs, int S, int G, SensorK sen,
    const unsigned long long* __restrict__ keys, float* __restrict__ image4, float4* __restrict__ packed, int32_t* __restrict__ pix2pt,
    int32_t* __restrict__ kept) {
  int s, chunk;
  if (!project_block(S, G, s, chunk)) return;
  const int px = chunk * DL_BLOCK + threadIdx.x;
  const int HW = sen.HW;
  bool occupied = false;
  if (px < HW) {
    const unsigned long long key = keys[(size_t)s * HW + px];
    float* img = image4 + (size_t)s * 4 * HW + px;
    occupied = key != ~0ull;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    int idx = -1;
    if (occupied) {
      idx = (int)(unsigned int)(key & 0xffffffffu);
      const float* q = rec + ((int64_t)offs[s] + idx) * (int64_t)(lay.step >> 2);   // a record that voted: inside the buffer
      p = make_float4(q[lay.wx], q[lay.wy], q[lay.wz], __uint_as_float((unsigned int)(key >> 32)));
    }
    img[0] = p.x; img[HW] = p.y; img[2 * HW] = p.z; img[3 * HW] = p.w;
    if (packed) packed[(size_t)s * HW + px] = p;
    pix2pt[(size_t)s * HW + px] = idx;
  }
  if (kept) {   // optional statistic: one atomic per workgroup
    __shared__ int s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const unsigned long long m = __ballot(occupied);
    if ((threadIdx.x & (DL_WAVE - 1)) == 0 && m) atomicAdd(&s_cnt, (int)__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(&kept[s], s_cnt);
  }
}

/* see common.h */
int dl_record_layout_check(const char* who, const void* records, const dl_record_layout* layout) {
  if (!layout) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null layout", who);
  if (layout->filter & ~(DL_RECORDS_DROP_ZERO | DL_RECORDS_MIN_RANGE))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: unknown bit in layout.filter=0x%x", who, layout->filter);
  const int step = layout->point_step;
  if (step < 12 || step > 256 || (step & 3))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: layout.point_step=%d is not a multiple of 4 in 12..256", who, step);
  const int off[3] = {layout->off_x, layout->off_y, layout->off_z};
  const char* name[3] = {"off_x", "off_y", "off_z"};
  for (int k = 0; k < 3; ++k) {
    if (off[k] < 0 || (off[k] & 3) || off[k] + 4 > step)
      return dl_fail(DL_ERR_UNSUPPORTED, "%s: layout.%s=%d is not a multiple of 4 in 0..point_step-4 (point_step=%d)", who, name[k], off[k], step);
    for (int j = 0; j < k; ++j)
      if (off[j] == off[k]) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layout.%s=%d repeats layout.%s", who, name[k], off[k], name[j]);
  }
  if ((layout->filter & DL_RECORDS_MIN_RANGE) && !(fabsf(layout->min_range) <= 3.402823466e38f))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: layout.min_range is not finite", who);
  if ((uintptr_t)records & 3) return dl_fail(DL_ERR_UNSUPPORTED, "%s: records must be 4-byte aligned (no misaligned device loads)", who);
  return DL_OK;
}

extern "C" size_t dl_project_records_workspace_bytes(int32_t S, int32_t H, int32_t W) {
  if (S <= 0 || H <= 0 || W <= 0) return 0;
  return project_keys_bytes(S, H, W);
}

extern "C" int dl_project_records(const void* records, int64_t n_records, const dl_record_layout* layout, const int32_t* offs, int32_t S,
                                  int32_t max_n, const dl_sensor* sensor, float* image4, float* packed, int32_t* pix2pt, void* workspace,
                                  int32_t* kept, int32_t* n_pass, dl_stream stream) {
  const char* who = "dl_project_records";
  if ((!records && n_records > 0) || !layout || !offs || !sensor || !image4 || !pix2pt || !workspace)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
  if (S <= 0 || sensor->H < 2 || sensor->W < 2 || max_n < 0 || n_records < 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes S=%d H=%d W=%d max_n=%d n_records=%lld", who, S, sensor->H, sensor->W, max_n,
                   (long long)n_records);
  if ((uintptr_t)workspace & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  if (int rc = dl_record_layout_check(who, records, layout)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const SensorK sen = make_sensor(sensor);
  const RecordK lay = {layout->point_step, layout->off_x >> 2, layout->off_y >> 2, layout->off_z >> 2, layout->filter, layout->min_range};
  const float* rec = (const float*)records;
  unsigned long long* keys = (unsigned long long*)workspace;   // the workspace is the key plane [S][H*W] uint64 and nothing else
  dl_fill_words(keys, 0xffffffffu, (size_t)S * sen.HW * 2, st);
  if (kept) dl_fill_words(kept, 0u, (size_t)S, st);
  if (n_pass) dl_fill_words(n_pass, 0u, (size_t)S, st);
  if (max_n > 0 && n_records > 0) {
    int G = (max_n + DL_BLOCK - 1) / DL_BLOCK;
    if (G > 1024) G = 1024;
    if (lay.step == 16 && !((uintptr_t)records & 15))
      hipLaunchKernelGGL(k_project_records_scatter<true>, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, rec, n_records, lay, offs, S,
                         project_garg(S, G), sen, keys, n_pass);
    else
      hipLaunchKernelGGL(k_project_records_scatter<false>, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, rec, n_records, lay, offs, S,
                         project_garg(S, G), sen, keys, n_pass);
  }
  const int G = (sen.HW + DL_BLOCK - 1) / DL_BLOCK;
  hipLaunchKernelGGL(k_project_records_resolve, dim3(project_grid(S, G)), dim3(DL_BLOCK), 0, st, rec, lay, offs, S, project_garg(S, G), sen,
                     (const unsigned long long*)keys, image4, (float4*)packed, pix2pt, kept);
  return dl_check_launch(who);
}
