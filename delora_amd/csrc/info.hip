// Point-to-plane normal equations of a scan pair: how well the matched pairs constrain the pose the network returned.
//
// The reference's inference node fills a nav_msgs/Odometry whose 6x6 pose.covariance it never sets
// (src/ros_utils/odometry_publisher.py:128-172).  Everything such a covariance needs is already on the device after the exact
// search: with the correspondences held fixed (as the loss holds them), a left perturbation q <- q + omega x q + v of the
// transformed source point q = R p + t changes the point-to-plane residual r = n . (q - p_t) by J . (v, omega) with
//     J = (n_x, n_y, n_z, a_x, a_y, a_z),   a = q x n   (translation first: the order of pose.covariance),
// so that  info = sum w J J^T  is the Gauss-Newton Hessian of 1/2 sum w r^2,  rhs = sum w J r  its gradient, and
// sigma^2 info^-1 with sigma^2 = sum w r^2 / (K - 6) the covariance of the pose under that perturbation, in the target frame.
// NO step is taken or returned: the pose stays the network's.
//
// Pass 1 streams the thirteen planes dl_icp_loss_fwd streams (52 B per source pixel, icp_stream.h) and keeps 29 sums per lane in
// packed fp32 (58 VGPRs; the residual alone is formed in fp64 and rounded once, see accumulate_info2): the 21 unique entries of J J^T, the 6 of J r, r^2 and the pair count; the workgroup reduction of
// loss.hip leaves one partial row (pitch 32) per workgroup.  Pass 2, one workgroup per sample, adds the rows in fp64 in a fixed
// order and one thread finishes the sample in fp64: Jacobi scaling, Cholesky, status, covariance.  No floating-point atomics, no
// synchronisation, allocation or read-back; the same inputs give the same bits on every run.
#include "common.h"
#include "icp_stream.h"

#define INFO_NA 29           // 0-20 J J^T (upper triangle, row-major), 21-26 J r, 27 r^2, 28 K
#define INFO_PITCH 32        // floats per partial row
#define INFO_SLICES (DL_BLOCK / INFO_PITCH)

static inline size_t info_rows(int HW) { return (size_t)loss_blocks(HW); }

// Two matched pairs, branch-free (multiplicative masking, the contract of dl_icp_loss_fwd): per pixel the sequence of operations of
// the scalar form in include/delora_hip.h.
__device__ __forceinline__ void accumulate_info2(f2 (&acc)[INFO_NA], const float (&m)[12], bool valid0, bool valid1, f2 x, f2 y, f2 z,
                                                 f2 nx, f2 ny, f2 nz, f2 tx, f2 ty, f2 tz, f2 tnx, f2 tny, f2 tnz) {
  const bool hs0 = (nx.x != 0.f) || (ny.x != 0.f) || (nz.x != 0.f);
  const bool hs1 = (nx.y != 0.f) || (ny.y != 0.f) || (nz.y != 0.f);
  const bool ht0 = (tnx.x != 0.f) || (tny.x != 0.f) || (tnz.x != 0.f);
  const bool ht1 = (tnx.y != 0.f) || (tny.y != 0.f) || (tnz.y != 0.f);
  const f2 w = {(valid0 && hs0 && ht0) ? 1.f : 0.f, (valid1 && hs1 && ht1) ? 1.f : 0.f};
  const f2 qx = pk_fma(m[2], z, pk_fma(m[1], y, pk_mul(m[0], x))) + m[3];
  const f2 qy = pk_fma(m[6], z, pk_fma(m[5], y, pk_mul(m[4], x))) + m[7];
  const f2 qz = pk_fma(m[10], z, pk_fma(m[9], y, pk_mul(m[8], x))) + m[11];
  // The residual is the one quantity that cancels: near a converged pose |r| is centimetres on coordinates of tens of metres, and an
  // fp32 q would leave every r with an absolute error of a few ulp of |q| whatever its own size -- the sum J r would then be off by
  // more than its terms' own rounding.  So d = R p + t - p_t and r = n . d are evaluated in fp64 from the fp32 operands (products of
  // two floats are exact there) and r is rounded ONCE to fp32; on small-integer data this is the fp32 chain's value, bit for bit.
  f2 r;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const double xd = x[e], yd = y[e], zd = z[e];
    const double ddx = fma((double)m[2], zd, fma((double)m[1], yd, (double)m[0] * xd)) + (double)m[3] - (double)tx[e];
    const double ddy = fma((double)m[6], zd, fma((double)m[5], yd, (double)m[4] * xd)) + (double)m[7] - (double)ty[e];
    const double ddz = fma((double)m[10], zd, fma((double)m[9], yd, (double)m[8] * xd)) + (double)m[11] - (double)tz[e];
    r[e] = (float)fma(ddz, (double)tnz[e], fma(ddy, (double)tny[e], ddx * (double)tnx[e]));
  }
  // J, and w J: columns 0..2 the matched normal, 3..5 the moment arm q x n
  f2 J[6] = {tnx, tny, tnz, pk_fma(qy, tnz, -(qz * tny)), pk_fma(qz, tnx, -(qx * tnz)), pk_fma(qx, tny, -(qy * tnx))};
  f2 Jw[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) Jw[i] = w * J[i];
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j, ++k) acc[k] = pk_fma(Jw[i], J[j], acc[k]);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = pk_fma(Jw[i], r, acc[21 + i]);
  acc[27] = pk_fma(w * r, r, acc[27]);
  acc[28] += w;
}

__global__ __launch_bounds__(DL_BLOCK) void k_icp_information(
    const float* __restrict__ src, int64_t src_ss, const float* __restrict__ srcn, int64_t srcn_ss,
    const float* __restrict__ match, int64_t match_ss, const int32_t* __restrict__ nn_pix,
    const float* __restrict__ T, int HW, float* __restrict__ partials) {
  constexpr int CHUNK = DL_WAVE * LOSS_PX;                       // 256 pixels
  const int b = blockIdx.y;
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = T[b * 16 + i];
  f2 acc[INFO_NA];
#pragma unroll
  for (int i = 0; i < INFO_NA; ++i) acc[i] = (f2){0.f, 0.f};
  const float* sp = src + (size_t)b * src_ss;
  const float* sn = srcn + (size_t)b * srcn_ss;
  const float* mt = match + (size_t)b * match_ss;
  const int32_t* nn = nn_pix + (size_t)b * HW;
  const int lane = threadIdx.x & (DL_WAVE - 1), wv = threadIdx.x / DL_WAVE;
  const int waves = gridDim.x * (DL_BLOCK / DL_WAVE);
  const int gw = blockIdx.x * (DL_BLOCK / DL_WAVE) + wv;
  const int nchunks = (HW + CHUNK - 1) / CHUNK;
  const int q4 = HW / 4;
  const bool vec = (HW & 3) == 0;
  for (int c = gw; c < nchunks; c += waves) {
    if (vec && c * CHUNK + CHUNK <= HW) {
      const StreamRegs cur = load_stream(nn, sp, sn, mt, q4, c * DL_WAVE + lane);
#define DL_LO(V) ((f2){cur.V.x, cur.V.y})
#define DL_HI(V) ((f2){cur.V.z, cur.V.w})
      accumulate_info2(acc, m, cur.j.x >= 0, cur.j.y >= 0, DL_LO(x), DL_LO(y), DL_LO(z), DL_LO(a), DL_LO(b), DL_LO(c), DL_LO(tx),
                       DL_LO(ty), DL_LO(tz), DL_LO(ta), DL_LO(tb), DL_LO(tc));
      accumulate_info2(acc, m, cur.j.z >= 0, cur.j.w >= 0, DL_HI(x), DL_HI(y), DL_HI(z), DL_HI(a), DL_HI(b), DL_HI(c), DL_HI(tx),
                       DL_HI(ty), DL_HI(tz), DL_HI(ta), DL_HI(tb), DL_HI(tc));
#undef DL_LO
#undef DL_HI
    } else {                                                     // ragged tail / unaligned image: scalar loads
      for (int k = 0; k < LOSS_PX; k += 2) {
        const int p0 = c * CHUNK + lane * LOSS_PX + k, p1 = p0 + 1;
        const bool i0 = p0 < HW, i1 = p1 < HW;
        const int a0 = i0 ? p0 : 0, a1 = i1 ? p1 : 0;            // out-of-range pixels read pixel 0 and are masked
#define DL_PL(P, O) ((f2){P[(size_t)(O) * HW + a0], P[(size_t)(O) * HW + a1]})
        accumulate_info2(acc, m, i0 && nn[a0] >= 0, i1 && nn[a1] >= 0, DL_PL(sp, 0), DL_PL(sp, 1), DL_PL(sp, 2), DL_PL(sn, 0),
                         DL_PL(sn, 1), DL_PL(sn, 2), DL_PL(mt, 0), DL_PL(mt, 1), DL_PL(mt, 2), DL_PL(mt, 3), DL_PL(mt, 4), DL_PL(mt, 5));
#undef DL_PL
      }
    }
  }
  __shared__ float red[(DL_BLOCK / 16) * INFO_PITCH];
  wg_reduce_row<INFO_NA, INFO_PITCH>(acc, red, partials + ((size_t)b * gridDim.x + blockIdx.x) * INFO_PITCH);
}

struct InfoOut {
  double *info, *rhs, *stats, *covariance;
  int32_t* status;
};

// Second (tiny) launch, one workgroup per sample: thread t owns column t % 32 and every 8th row; the eight slices meet in LDS and
// are added in a fixed order.  Thread 0 then finishes the sample (include/delora_hip.h has the rule).
__global__ __launch_bounds__(DL_BLOCK) void k_icp_information_reduce(const float* __restrict__ partials, int nrows, InfoOut out) {
  __shared__ double tot[INFO_SLICES * INFO_PITCH];
  __shared__ double A[36], L[36], Li[36];
  const int b = blockIdx.x, t = threadIdx.x;
  const float* rows = partials + (size_t)b * nrows * INFO_PITCH;
  {
    const int col = t % INFO_PITCH, slice = t / INFO_PITCH;
    double s = 0.0;
    for (int i = slice; i < nrows; i += INFO_SLICES) s += (double)rows[(size_t)i * INFO_PITCH + col];
    tot[slice * INFO_PITCH + col] = s;
  }
  __syncthreads();
  if (t < INFO_PITCH) {
    double s = 0.0;
#pragma unroll
    for (int p = 0; p < INFO_SLICES; ++p) s += tot[p * INFO_PITCH + t];
    tot[t] = s;                  // (thread t reads column t of every slice and writes column t of slice 0: no other thread touches them)
  }
  __syncthreads();
  if (t != 0) return;
  double* info = out.info + (size_t)b * 36;
  double* cov = out.covariance + (size_t)b * 36;
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j, ++k) A[i * 6 + j] = A[j * 6 + i] = tot[k];
  for (int i = 0; i < 36; ++i) info[i] = A[i];
  for (int i = 0; i < 6; ++i) out.rhs[(size_t)b * 6 + i] = tot[21 + i];
  const double sum_r2 = tot[27], K = tot[28];
  out.stats[(size_t)b * 2 + 0] = sum_r2;
  out.stats[(size_t)b * 2 + 1] = K;
  // status (comparisons written so that a NaN -- a non-finite pose -- is "unobservable", never a covariance)
  int status = DL_INFO_OK;
  double s[6];
  if (K <= 6.0) {
    status = DL_INFO_TOO_FEW_PAIRS;
  } else {
    for (int i = 0; i < 6; ++i)
      if (!(A[i * 6 + i] > 0.0)) status = DL_INFO_UNOBSERVABLE;
  }
  if (status == DL_INFO_OK) {
    for (int i = 0; i < 6; ++i) s[i] = 1.0 / sqrt(A[i * 6 + i]);
    // Cholesky of the scaled matrix Ah = D^-1/2 A D^-1/2 (unit diagonal): Ah = L L^T; a pivot is the remainder of the diagonal
    // entry BEFORE its square root
    for (int j = 0; j < 6 && status == DL_INFO_OK; ++j) {
      double p = (A[j * 6 + j] * s[j]) * s[j];
      for (int c = 0; c < j; ++c) p -= L[j * 6 + c] * L[j * 6 + c];
      if (!(p > DL_INFO_MIN_PIVOT)) { status = DL_INFO_UNOBSERVABLE; break; }
      const double d = sqrt(p);
      L[j * 6 + j] = d;
      for (int i = j + 1; i < 6; ++i) {
        double v = (A[i * 6 + j] * s[i]) * s[j];
        for (int c = 0; c < j; ++c) v -= L[i * 6 + c] * L[j * 6 + c];
        L[i * 6 + j] = v / d;
      }
    }
  }
  if (status == DL_INFO_OK) {
    // Li = L^-1 (lower triangular, forward substitution per column), Ah^-1 = Li^T Li, covariance = sigma^2 D^-1/2 Ah^-1 D^-1/2
    for (int c = 0; c < 6; ++c) {
      for (int i = 0; i < 6; ++i) {
        if (i < c) { Li[i * 6 + c] = 0.0; continue; }
        double v = i == c ? 1.0 : 0.0;
        for (int j = c; j < i; ++j) v -= L[i * 6 + j] * Li[j * 6 + c];
        Li[i * 6 + c] = v / L[i * 6 + i];
      }
    }
    const double sigma2 = sum_r2 / (K - 6.0);
    for (int i = 0; i < 6; ++i) {
      for (int j = i; j < 6; ++j) {
        double v = 0.0;
        for (int c = j; c < 6; ++c) v += Li[c * 6 + i] * Li[c * 6 + j];
        v = sigma2 * ((v * s[i]) * s[j]);
        cov[i * 6 + j] = v;
        cov[j * 6 + i] = v;
      }
    }
  } else {
    for (int i = 0; i < 36; ++i) cov[i] = 0.0;
  }
  out.status[b] = status;
}

// the shapes both entry points and the size function serve: positive, H*W small enough for the kernels' int pixel arithmetic
static int info_sizes(const char* who, int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 30) || B > 65535)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes B=%d H=%d W=%d (all positive, H*W <= 2^30, B <= 65535)", who, B, H, W);
  return DL_OK;
}

/* see include/delora_hip.h */
extern "C" size_t dl_icp_information_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (info_sizes("dl_icp_information_workspace_bytes", B, H, W)) return 0;
  return (size_t)B * info_rows(H * W) * INFO_PITCH * sizeof(float);   // one partial row per workgroup
}

/* see include/delora_hip.h */
extern "C" int dl_icp_information(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss, const float* match,
                                  int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, int32_t H, int32_t W, double* info,
                                  double* rhs, double* stats, double* covariance, int32_t* status, void* workspace, dl_stream stream) {
  const char* who = "dl_icp_information";
  if (!src_image4 || !src_normals || !match || !nn_pix || !T || !info || !rhs || !stats || !covariance || !status || !workspace)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
  if (int rc = info_sizes(who, B, H, W)) return rc;
  const int64_t HW = (int64_t)H * W;
  if (src_ss < 3 * HW || srcn_ss < 3 * HW || match_ss < 6 * HW)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: a scan stride is below the dense size (src_ss=%lld srcn_ss=%lld >= %lld, match_ss=%lld >= %lld)", who,
                   (long long)src_ss, (long long)srcn_ss, (long long)(3 * HW), (long long)match_ss, (long long)(6 * HW));
  if (HW % 4 == 0 && ((src_ss | srcn_ss | match_ss) % 4 ||
                      (((uintptr_t)src_image4 | (uintptr_t)src_normals | (uintptr_t)match | (uintptr_t)nn_pix) & 15)))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: planes and nn_pix must be 16-byte aligned", who);
  if ((uintptr_t)workspace & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 16-byte aligned", who);
  if (((uintptr_t)info | (uintptr_t)rhs | (uintptr_t)stats | (uintptr_t)covariance) & 7 || ((uintptr_t)status & 3))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: outputs must be aligned to their element size", who);
  hipStream_t st = (hipStream_t)stream;
  float* partials = (float*)workspace;
  const int nrows = (int)info_rows((int)HW);
  hipLaunchKernelGGL(k_icp_information, dim3(nrows, B), dim3(DL_BLOCK), 0, st, src_image4, src_ss, src_normals, srcn_ss, match, match_ss,
                     nn_pix, T, (int)HW, partials);
  if (int rc = dl_check_launch(who)) return rc;
  const InfoOut out{info, rhs, stats, covariance, status};
  hipLaunchKernelGGL(k_icp_information_reduce, dim3(B), dim3(DL_BLOCK), 0, st, (const float*)partials, nrows, out);
  return dl_check_launch(who);
}

// ---------------------------------------------------------------------------------------------------------------------
// dl_odometry_quality: the chain normals -> exact search -> normal equations behind a streaming push.

// planar [4][H][W] -> packed [H][W][4], a bit copy (what dl_project writes as its packed twin)
typedef uint32_t u32x4q __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(DL_BLOCK) void k_pack_image(const uint32_t* __restrict__ planar, uint32_t HW, u32x4q* __restrict__ packed) {
  const uint32_t p = blockIdx.x * DL_BLOCK + threadIdx.x;
  if (p >= HW) return;
  packed[p] = (u32x4q){planar[p], planar[HW + p], planar[2 * (size_t)HW + p], planar[3 * (size_t)HW + p]};
}

// (own names: tools/odometry_demo.hip compiles this file and infer.hip as one translation unit)
namespace {
constexpr size_t kQualityAlign = 256;
inline size_t quality_align(size_t n) { return (n + kQualityAlign - 1) / kQualityAlign * kQualityAlign; }

int quality_sensor(const char* who, const dl_sensor* sensor) {
  if (!sensor) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null sensor", who);
  if (sensor->H < 2 || sensor->W < 2 || (int64_t)sensor->H * sensor->W > (1 << 30))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sensor H=%d W=%d", who, sensor->H, sensor->W);
  return DL_OK;
}
}  // namespace

/* see include/delora_hip.h */
extern "C" size_t dl_odometry_quality_workspace_bytes(const dl_sensor* sensor, int32_t H, int32_t W) {
  const char* who = "dl_odometry_quality_workspace_bytes";
  if (quality_sensor(who, sensor)) return 0;
  if (H != sensor->H || W != sensor->W) {
    dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d must be the sensor's %dx%d", who, H, W, sensor->H, sensor->W);
    return 0;
  }
  const size_t HW = (size_t)H * W;
  // nn_pix [H*W] int32 | match [6][H*W] | the search's scratch | the partial rows
  return quality_align(HW * 4) + quality_align(HW * 24) + quality_align(dl_nn_workspace_bytes(1, H, W)) + quality_align(dl_icp_information_workspace_bytes(1, H, W));
}

/* see include/delora_hip.h */
extern "C" int dl_odometry_quality(const dl_sensor* sensor, const float* image_prev, const dl_scan_geometry* geometry_prev, const float* image_cur,
                                   const dl_scan_geometry* geometry_cur, const float* T, int32_t half_rows, int32_t half_cols, float epsilon_range,
                                   int32_t min_neighbors, void* workspace, double* info, double* rhs, double* stats, double* covariance,
                                   int32_t* status, dl_stream stream) {
  const char* who = "dl_odometry_quality";
  if (int rc = quality_sensor(who, sensor)) return rc;
  const int H = sensor->H, W = sensor->W;
  const size_t HW = (size_t)H * W;
  if (!image_cur || !geometry_cur || !geometry_cur->normals || !geometry_cur->packed_image || !geometry_cur->packed_normals)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument (image_cur, geometry_cur and its three buffers)", who);
  if (((uintptr_t)image_cur | (uintptr_t)geometry_cur->normals | (uintptr_t)geometry_cur->packed_image | (uintptr_t)geometry_cur->packed_normals) & 15)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: image_cur and the buffers of geometry_cur must be 16-byte aligned", who);
  if (half_rows < 0 || half_rows > 15 || half_cols < 0 || half_cols > 31)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad window a=%d b=%d (half_rows 0..15, half_cols 0..31)", who, half_rows, half_cols);
  if (image_prev) {
    if (!geometry_prev || !geometry_prev->normals || !geometry_prev->packed_image || !geometry_prev->packed_normals || !T || !workspace || !info ||
        !rhs || !stats || !covariance || !status)
      return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument (with image_prev: geometry_prev and its buffers, T, workspace, the five outputs)", who);
    if (((uintptr_t)workspace & (kQualityAlign - 1))) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 256-byte aligned", who);
    if (((uintptr_t)geometry_prev->packed_image | (uintptr_t)geometry_prev->packed_normals) & 15)
      return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: the buffers of geometry_prev must be 16-byte aligned", who);
    if (((uintptr_t)info | (uintptr_t)rhs | (uintptr_t)stats | (uintptr_t)covariance) & 7 || ((uintptr_t)status & 3) || ((uintptr_t)T & 3))
      return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: T and the outputs must be aligned to their element size", who);
  }
  hipStream_t st = (hipStream_t)stream;
  // the record of the current image: normals (planar + packed) and the packed image
  if (int rc = dl_normals(image_cur, (int64_t)4 * HW, 1, H, W, half_rows, half_cols, epsilon_range, min_neighbors, geometry_cur->normals,
                          geometry_cur->packed_normals, stream))
    return rc;
  hipLaunchKernelGGL(k_pack_image, dim3((unsigned)((HW + DL_BLOCK - 1) / DL_BLOCK)), dim3(DL_BLOCK), 0, st, (const uint32_t*)image_cur, (uint32_t)HW,
                     (u32x4q*)geometry_cur->packed_image);
  if (int rc = dl_check_launch(who)) return rc;
  if (!image_prev) return DL_OK;
  char* ws = (char*)workspace;
  int32_t* nn_pix = (int32_t*)ws;
  float* match = (float*)(ws + quality_align(HW * 4));
  void* nn_ws = ws + quality_align(HW * 4) + quality_align(HW * 24);
  void* info_ws = (char*)nn_ws + quality_align(dl_nn_workspace_bytes(1, H, W));
  // source = the current scan, target = the previous one: the direction of T in dl_odometry_push
  if (int rc = dl_nn_correspond(image_cur, (int64_t)4 * HW, geometry_cur->normals, (int64_t)3 * HW, geometry_prev->packed_image, (int64_t)4 * HW,
                                geometry_prev->packed_normals, (int64_t)4 * HW, T, 1, sensor, 0, nn_pix, match, nullptr, nn_ws, stream))
    return rc;
  return dl_icp_information(image_cur, (int64_t)4 * HW, geometry_cur->normals, (int64_t)3 * HW, match, (int64_t)6 * HW, nn_pix, T, 1, H, W, info, rhs,
                            stats, covariance, status, info_ws, stream);
}
