// Dropout of the pose CNN on the HIP path (reference src/models/resnet_modified.py:33-38, :95-118: element-wise Dropout on the stacked
// input image and on the fc output, Dropout2d on the output of layer3; p = 0.2, training mode only).
//
// The masks come from a counter-based stream with a written contract (include/delora_hip.h), so that a test can recompute every
// decision on the host: Philox4x32-10, counter = (i >> 2, i >> 34, site, 0) for decision index i, key = the 64-bit seed, decision i
// reads output word i & 3.  A value is dropped iff word < round(p 2^32), else multiplied by 1.0f / (1.0f - p).  The seed is READ FROM
// DEVICE MEMORY by every kernel: the Python side draws it with torch's generator per forward pass, and a captured graph that replays
// these launches sees the fresh value its replay wrote.
//
// All kernels here are element-wise HBM streams: 16-byte accesses, one thread per vector, no LDS.
#include "convh_common.h"

#define DR_M0 0xD2511F53u
#define DR_M1 0xCD9E8D57u
#define DR_W0 0x9E3779B9u
#define DR_W1 0xBB67AE85u

struct DrWords { uint32_t w[4]; };

__device__ __forceinline__ DrWords dr_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(DR_M0, c0), lo0 = DR_M0 * c0;
    const uint32_t hi1 = __umulhi(DR_M1, c2), lo1 = DR_M1 * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += DR_W0; k1 += DR_W1;
  }
  return DrWords{{c0, c1, c2, c3}};
}
// the four decisions 4q .. 4q+3 of a site as scale factors
__device__ __forceinline__ f32x4 dr_scales4(uint64_t quad, uint32_t site, uint64_t seed, uint32_t thresh, float keep) {
  const DrWords r = dr_philox((uint32_t)quad, (uint32_t)(quad >> 32), site, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  f32x4 s;
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = r.w[j] < thresh ? 0.f : keep;
  return s;
}

__global__ __launch_bounds__(256) void k_dropout_scale(const uint64_t* __restrict__ seed, uint32_t site, uint32_t thresh, float keep, long n,
                                                       float* __restrict__ scale) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q * 4 >= n) return;
  const f32x4 s = dr_scales4((uint64_t)q, site, seed[0], thresh, keep);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (q * 4 + j < n) scale[q * 4 + j] = s[j];
}

// x [N][C][H][W] planar -> y [N][H][W][C] channels-last, times the site-1 mask.  One thread per pixel: a wave reads 64 consecutive
// columns of every plane (256 contiguous bytes per load instruction) and each lane writes its pixel's C channels as 16-byte stores.
// Decision index = the flat index of the element in y, so the C/4 channel quads of a pixel are C/4 Philox calls.
__global__ __launch_bounds__(256) void k_stem_input_nhwc_drop(const float* __restrict__ x, int C, long HW, long pixels, const uint64_t* __restrict__ seed,
                                                              uint32_t thresh, float keep, float* __restrict__ y) {
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= pixels) return;
  const long n = pix / HW, p = pix % HW;
  const float* __restrict__ src = x + (size_t)n * C * HW + p;
  const uint64_t sd = seed[0];
  const int quads = C >> 2;
  for (int q = 0; q < quads; ++q) {
    const f32x4 s = dr_scales4((uint64_t)pix * quads + q, 1u, sd, thresh, keep);
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = src[(size_t)(q * 4 + j) * HW] * s[j];
    *(f32x4*)(y + (size_t)pix * C + q * 4) = v;
  }
}

// y[n][p][c] = x[n][p][c] * scale[n][c]; T = 0 fp32 (4 values per thread), 1 fp16, 2 bf16 (8 values per thread); arithmetic in fp32
template <int T>
__global__ __launch_bounds__(256) void k_channel_scale(const void* __restrict__ x, const float* __restrict__ scale, long vecs_per_sample, int cvecs,
                                                       int C, long total, void* __restrict__ y) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const long n = v / vecs_per_sample;
  const int c0 = (int)(v % cvecs) * (T == 0 ? 4 : 8);
  const float* __restrict__ s = scale + n * C + c0;
  if constexpr (T == 0) {
    const f32x4 a = ((const f32x4*)x)[v], sc = *(const f32x4*)s;
    ((f32x4*)y)[v] = a * sc;
  } else {
    const u16x8 a = ((const u16x8*)x)[v];
    const f32x4 s0 = *(const f32x4*)s, s1 = *(const f32x4*)(s + 4);
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = ch_f2h<T == 1>(ch_h2f<T == 1>(a[j]) * (j < 4 ? s0[j] : s1[j - 4]));
    ((u16x8*)y)[v] = o;
  }
}

// g_pre[n][p][c] = g[n][p][c] * scale[n][c] * act'(x[n][p][c]), act' from the ACTIVATED value x (the un-dropped map)
template <int T>
__global__ __launch_bounds__(256) void k_channel_scale_bwd_act(const void* __restrict__ g, const void* __restrict__ x, const float* __restrict__ scale,
                                                               long vecs_per_sample, int cvecs, int C, int act, long total, void* __restrict__ g_pre) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const long n = v / vecs_per_sample;
  const int c0 = (int)(v % cvecs) * (T == 0 ? 4 : 8);
  const float* __restrict__ s = scale + n * C + c0;
  if constexpr (T == 0) {
    const f32x4 gv = ((const f32x4*)g)[v], a = ((const f32x4*)x)[v], sc = *(const f32x4*)s;
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (gv[j] * sc[j]) * ch_dact(a[j], act);
    ((f32x4*)g_pre)[v] = o;
  } else {
    const u16x8 gv = ((const u16x8*)g)[v], a = ((const u16x8*)x)[v];
    const f32x4 s0 = *(const f32x4*)s, s1 = *(const f32x4*)(s + 4);
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      o[j] = ch_f2h<T == 1>((ch_h2f<T == 1>(gv[j]) * (j < 4 ? s0[j] : s1[j - 4])) * ch_dact(ch_h2f<T == 1>(a[j]), act));
    ((u16x8*)g_pre)[v] = o;
  }
}

// Site 1 behind the feature tower: y5 [2B][H][W][CH] (the compact, UN-dropped layer-5 output; image n = 2 b + k) -> xw [B][H][W][pitch], the
// stem's wide input: channels k CH .. k CH + CH - 1 hold image k's tower times the mask, channels 2 CH .. pitch - 1 are written as zeros.  One
// thread per 16-byte vector of xw.  Decision index = the flat index in the LOGICAL [B][H][W][2 CH] tensor (the pitch does not enter);
// CH % 4 == 0, so a vector never straddles the two images and is one Philox call.
__global__ __launch_bounds__(256) void k_tower_wide_drop(const float* __restrict__ y5, const uint64_t* __restrict__ seed, uint32_t thresh, float keep, long HW,
                                                         int CH, int pq /* pitch / 4 */, long total, float* __restrict__ xw) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const long pix = v / pq;
  const int q = (int)(v % pq), dq = CH >> 1;                // dq: data vectors (= Philox calls) per pixel
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  if (q < dq) {
    const int c = q * 4, k = c >= CH ? 1 : 0;
    const long b = pix / HW, hw = pix % HW;
    const f32x4 a = *(const f32x4*)(y5 + (size_t)((2 * b + k) * HW + hw) * CH + (c - k * CH));
    o = a * dr_scales4((uint64_t)pix * dq + q, 1u, seed[0], thresh, keep);
  }
  ((f32x4*)xw)[v] = o;
}

// backward of k_tower_wide_drop: g5[n][h][w][c] = (gx[b][h][w][k CH + c] * s(i)) * act'(y5[n][h][w][c]), the mask regenerated from the seed.
// One thread per 16-byte vector of g5; channels 2 CH .. pitch - 1 of gx are never read.
__global__ __launch_bounds__(256) void k_tower_wide_drop_bwd(const float* __restrict__ gx, const float* __restrict__ y5, const uint64_t* __restrict__ seed,
                                                             uint32_t thresh, float keep, int act, long HW, int CH, int pitch, long total,
                                                             float* __restrict__ g5) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= total) return;
  const int cq = CH >> 2, q = (int)(v % cq);
  const long np = v / cq, n = np / HW, hw = np % HW;        // np: pixel of the compact tensor
  const long pix = (n >> 1) * HW + hw;
  const int k = (int)(n & 1);
  const f32x4 g = *(const f32x4*)(gx + (size_t)pix * pitch + k * CH + q * 4), a = ((const f32x4*)y5)[v];
  const f32x4 s = dr_scales4((uint64_t)pix * (CH >> 1) + k * cq + q, 1u, seed[0], thresh, keep);
  f32x4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = (g[j] * s[j]) * ch_dact(a[j], act);
  ((f32x4*)g5)[v] = o;
}

// round(p 2^32) and 1.0f / (1.0f - p); p in [0, 1)
static int dr_params(const char* who, double p, uint32_t* thresh, float* keep) {
  if (!(p >= 0.0) || !(p < 1.0)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: p must lie in [0, 1)", who);
  const double t = p * 4294967296.0 + 0.5;
  *thresh = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
  *keep = 1.0f / (1.0f - (float)p);
  return DL_OK;
}

/* see include/delora_hip.h */
extern "C" int dl_dropout_scale_f32(const uint64_t* seed, uint32_t site, double p, int64_t n, float* scale, dl_stream stream) {
  if (!seed || !scale || n <= 0 || site == 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_dropout_scale_f32: null pointer, n <= 0 or site 0");
  uint32_t thresh; float keep;
  if (int rc = dr_params("dl_dropout_scale_f32", p, &thresh, &keep)) return rc;
  const long quads = (n + 3) / 4;
  if ((quads + 255) / 256 > 0x7fffffffL) return dl_fail(DL_ERR_UNSUPPORTED, "dl_dropout_scale_f32: n too large for one launch");
  hipLaunchKernelGGL(k_dropout_scale, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, site, thresh, keep, (long)n, scale);
  return dl_check_launch("dl_dropout_scale_f32");
}

/* see include/delora_hip.h */
extern "C" int dl_stem_input_nhwc_drop_f32(const float* x_nchw, int32_t N, int32_t C, int32_t H, int32_t W, const uint64_t* seed, double p,
                                           float* x_nhwc, dl_stream stream) {
  if (!x_nchw || !seed || !x_nhwc || N <= 0 || C <= 0 || C % 4 || H <= 0 || W <= 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_stem_input_nhwc_drop_f32: null pointer or bad size (C %% 4 == 0)");
  uint32_t thresh; float keep;
  if (int rc = dr_params("dl_stem_input_nhwc_drop_f32", p, &thresh, &keep)) return rc;
  const long HW = (long)H * W, pixels = (long)N * HW;
  if (pixels * C >= (1L << 40)) return dl_fail(DL_ERR_UNSUPPORTED, "dl_stem_input_nhwc_drop_f32: tensor too large");
  hipLaunchKernelGGL(k_stem_input_nhwc_drop, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_nchw, (int)C, HW, pixels, seed,
                     thresh, keep, x_nhwc);
  return dl_check_launch("dl_stem_input_nhwc_drop_f32");
}

static int dr_channel_check(const char* who, const void* a, const void* b, const void* c, int N, int P, int C, int dtype) {
  if (!a || !b || !c || N <= 0 || P <= 0 || C <= 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer or bad size", who);
  if (dtype != DL_DTYPE_F32 && dtype != DL_DTYPE_F16 && dtype != DL_DTYPE_BF16) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: dtype must be DL_DTYPE_F32 / _F16 / _BF16", who);
  if (C % (dtype == DL_DTYPE_F32 ? 4 : 8)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: C must be a multiple of 4 (fp32) / 8 (half precision)", who);
  if ((long)N * P * C >= (1L << 40)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: tensor too large", who);
  return DL_OK;
}

/* see include/delora_hip.h */
extern "C" int dl_channel_scale_nhwc_t(const void* x, const float* scale, int32_t N, int32_t P, int32_t C, int32_t dtype, void* y, dl_stream stream) {
  if (int rc = dr_channel_check("dl_channel_scale_nhwc_t", x, scale, y, N, P, C, dtype)) return rc;
  const int vec = dtype == DL_DTYPE_F32 ? 4 : 8, cvecs = C / vec;
  const long per = (long)P * cvecs, total = per * N;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DL_DTYPE_F32) hipLaunchKernelGGL(k_channel_scale<0>, grid, dim3(256), 0, st, x, scale, per, cvecs, (int)C, total, y);
  else if (dtype == DL_DTYPE_F16) hipLaunchKernelGGL(k_channel_scale<1>, grid, dim3(256), 0, st, x, scale, per, cvecs, (int)C, total, y);
  else hipLaunchKernelGGL(k_channel_scale<2>, grid, dim3(256), 0, st, x, scale, per, cvecs, (int)C, total, y);
  return dl_check_launch("dl_channel_scale_nhwc_t");
}

/* see include/delora_hip.h */
extern "C" int dl_channel_scale_bwd_act_nhwc_t(const void* g, const void* x, const float* scale, int32_t N, int32_t P, int32_t C, int32_t act,
                                               int32_t dtype, void* g_pre, dl_stream stream) {
  if (int rc = dr_channel_check("dl_channel_scale_bwd_act_nhwc_t", g, scale, g_pre, N, P, C, dtype)) return rc;
  if (!x || act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_channel_scale_bwd_act_nhwc_t: null x or act outside 0..2");
  const int vec = dtype == DL_DTYPE_F32 ? 4 : 8, cvecs = C / vec;
  const long per = (long)P * cvecs, total = per * N;
  const dim3 grid((unsigned)((total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DL_DTYPE_F32) hipLaunchKernelGGL(k_channel_scale_bwd_act<0>, grid, dim3(256), 0, st, g, x, scale, per, cvecs, (int)C, (int)act, total, g_pre);
  else if (dtype == DL_DTYPE_F16) hipLaunchKernelGGL(k_channel_scale_bwd_act<1>, grid, dim3(256), 0, st, g, x, scale, per, cvecs, (int)C, (int)act, total, g_pre);
  else hipLaunchKernelGGL(k_channel_scale_bwd_act<2>, grid, dim3(256), 0, st, g, x, scale, per, cvecs, (int)C, (int)act, total, g_pre);
  return dl_check_launch("dl_channel_scale_bwd_act_nhwc_t");
}

static int dr_tower_check(const char* who, const void* a, const void* b, const void* c, const void* d, int B, int H, int W, int CH, int pitch) {
  if (!a || !b || !c || !d) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument", who);
  if (B <= 0 || H <= 0 || W <= 0 || CH <= 0 || CH % 4 || pitch % 4 || 2 * (long)CH > pitch)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad size (CH %% 4 == 0, pitch %% 4 == 0, 2 CH <= pitch): B=%d H=%d W=%d CH=%d pitch=%d", who, B, H, W, CH, pitch);
  if ((long)B * H * W * pitch >= (1L << 31)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: the wide buffer would pass 2^31 elements", who);
  return DL_OK;
}

/* see include/delora_hip.h */
extern "C" int dl_tower_wide_drop_f32(const float* y5, const uint64_t* seed, double p, int32_t B, int32_t H, int32_t W, int32_t CH, int32_t pitch,
                                      float* xw, dl_stream stream) {
  if (int rc = dr_tower_check("dl_tower_wide_drop_f32", y5, seed, xw, xw, B, H, W, CH, pitch)) return rc;
  uint32_t thresh; float keep;
  if (int rc = dr_params("dl_tower_wide_drop_f32", p, &thresh, &keep)) return rc;
  const long HW = (long)H * W, total = (long)B * HW * (pitch / 4);
  hipLaunchKernelGGL(k_tower_wide_drop, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y5, seed, thresh, keep, HW, (int)CH,
                     (int)(pitch / 4), total, xw);
  return dl_check_launch("dl_tower_wide_drop_f32");
}

/* see include/delora_hip.h */
extern "C" int dl_tower_wide_drop_bwd_f32(const float* gx, const float* y5, const uint64_t* seed, double p, int32_t act, int32_t B, int32_t H, int32_t W,
                                          int32_t CH, int32_t pitch, float* g5, dl_stream stream) {
  if (int rc = dr_tower_check("dl_tower_wide_drop_bwd_f32", gx, y5, seed, g5, B, H, W, CH, pitch)) return rc;
  if (act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_wide_drop_bwd_f32: act outside 0..2");
  uint32_t thresh; float keep;
  if (int rc = dr_params("dl_tower_wide_drop_bwd_f32", p, &thresh, &keep)) return rc;
  const long HW = (long)H * W, total = 2L * B * HW * (CH / 4);
  hipLaunchKernelGGL(k_tower_wide_drop_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gx, y5, seed, thresh, keep,
                     (int)act, HW, (int)CH, (int)pitch, total, g5);
  return dl_check_launch("dl_tower_wide_drop_bwd_f32");
}
