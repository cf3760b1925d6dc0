// Re-projection of the transformed source IMAGE: the range images behind the logged step figure.
//
// Replaces, for the figure of Deployer.log_image (reference src/deploy/deployer.py:73-100), the three project_to_img calls of a
// logged step (deployer.py:80-89, :317-320): the reference gathers the matched pairs into lists on the host, argsorts them by range
// and runs the sequential first-wins loop of projection.py three times.  Here the source side already IS an image and the pairs
// are the match planes of dl_nn_correspond, so one vote pass over the source pixels and one resolve pass over the output pixels
// do all of it:
//   vote     every occupied source pixel transforms its point (the loss kernel's operations, loss.hip / nn.hip transform_point),
//            projects it (dl_project's rules: norm3f, coord_* behind the atan2f screen, half-to-even, the inside test) and votes
//            with a 64-bit atomicMin on key = range_bits << 32 | source pixel into key plane 0 (all points) and, when it is a
//            pair with normals, into key plane 1;
//   resolve  every output pixel decodes its two winners and RECOMPUTES q, R n and d = q - m from the winner's source pixel: the
//            same operations on the same operands give the same bits, the range is the key's upper half.  No staging records: the
//            winner's operands are twelve planes that the step has just streamed (they sit in the L2 / infinity cache), and a
//            16-byte record per source pixel would cost more to write than the gathers cost to read.
// Order-independent integer atomics only; the launches are fill -> vote -> resolve on one stream.
#include "common.h"

__device__ __forceinline__ bool reproject_block(int S, int G, int& s, int& chunk) {   // project.hip's scan-to-XCD mapping for S >= 8
  const int b = blockIdx.x;
  if (S >= 8) {
    const int q = b >> 3;
    s = (q / G) * 8 + (b & 7);
    chunk = q % G;
  } else {
    s = b / G;
    chunk = b % G;
  }
  return s < S;
}
static inline int reproject_grid(int S, int G) { return S >= 8 ? 8 * G * ((S + 7) / 8) : S * G; }

// q = R p + t: the operations of the loss kernel (loss.hip accumulate_pair2), per row fma(m2, z, fma(m1, y, m0 * x)) + m3
__device__ __forceinline__ void reproject_point(const float (&m)[12], float x, float y, float z, float& qx, float& qy, float& qz) {
  qx = (fmaf(m[2], z, fmaf(m[1], y, (m[0] * x))) + m[3]);
  qy = (fmaf(m[6], z, fmaf(m[5], y, (m[4] * x))) + m[7]);
  qz = (fmaf(m[10], z, fmaf(m[9], y, (m[8] * x))) + m[11]);
}
__device__ __forceinline__ void reproject_normal(const float (&m)[12], float x, float y, float z, float& rx, float& ry, float& rz) {
  rx = fmaf(m[2], z, fmaf(m[1], y, (m[0] * x)));
  ry = fmaf(m[6], z, fmaf(m[5], y, (m[4] * x)));
  rz = fmaf(m[10], z, fmaf(m[9], y, (m[8] * x)));
}

__global__ __launch_bounds__(DL_BLOCK) void k_reproject_vote(
    const float* __restrict__ src, int64_t src_ss, const float* __restrict__ srcn, int64_t srcn_ss, const float* __restrict__ match,
    int64_t match_ss, const int32_t* __restrict__ nn_pix, const float* __restrict__ T, int B, int G, SensorK sen,
    unsigned long long* __restrict__ keys) {
  int b, chunk;
  if (!reproject_block(B, G, b, chunk)) return;
  const int HW = sen.HW;
  const int px = chunk * DL_BLOCK + threadIdx.x;
  if (px >= HW) return;
  const float* sp = src + (size_t)b * src_ss + px;
  const float x = sp[0], y = sp[HW], z = sp[2 * HW];
  if (x == 0.f && y == 0.f && z == 0.f) return;          // the occupancy rule of the correspondence search (nn.hip k_nn_window)
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = T[b * 16 + i];
  float qx, qy, qz;
  reproject_point(m, x, y, z, qx, qy, qz);
  const float r = norm3f(qx, qy, qz);
  float u = coord_u_fast(qx, qy, sen);
  float v = coord_v_fast(qx, qy, qz, sen);
  if (near_rounding_boundary(u, sen.tol_u) || near_rounding_boundary(v, sen.tol_v)) {     // NaN takes this path and stays NaN
    u = coord_u(qx, qy, sen);
    v = coord_v(qx, qy, qz, sen);
  }
  const float ru = rintf(u), rv = rintf(v);
  if (!(ru <= sen.wm1f && ru >= 0.0f && rv <= sen.hm1f && rv >= 0.0f)) return;             // a NaN coordinate is outside
  const int out = (int)rv * sen.W + (int)ru;
  const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | (unsigned int)px;
  unsigned long long* kp = keys + (size_t)b * 2 * HW;
  atomicMin(&kp[out], key);
  if (!nn_pix) return;
  // a pair with normals (icp_losses.py:48-52,110-121): matched, and a normal on both sides
  if (nn_pix[(size_t)b * HW + px] < 0) return;
  const float* np_ = srcn + (size_t)b * srcn_ss + px;
  if (!((np_[0] != 0.f) || (np_[HW] != 0.f) || (np_[2 * HW] != 0.f))) return;
  const float* mp = match + (size_t)b * match_ss + px;
  if (!((mp[3 * HW] != 0.f) || (mp[4 * HW] != 0.f) || (mp[5 * HW] != 0.f))) return;
  atomicMin(&kp[HW + out], key);
}

__global__ __launch_bounds__(DL_BLOCK) void k_reproject_resolve(
    const float* __restrict__ src, int64_t src_ss, const float* __restrict__ srcn, int64_t srcn_ss, const float* __restrict__ match,
    int64_t match_ss, const float* __restrict__ T, int B, int G, SensorK sen, const unsigned long long* __restrict__ keys,
    float* __restrict__ moved4, float* __restrict__ paired9, int32_t* __restrict__ src_pix) {
  int b, chunk;
  if (!reproject_block(B, G, b, chunk)) return;
  const int HW = sen.HW;
  const int px = chunk * DL_BLOCK + threadIdx.x;
  if (px >= HW) return;
  float m[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) m[i] = T[b * 16 + i];
  const unsigned long long* kp = keys + (size_t)b * 2 * HW;
  const unsigned long long k0 = kp[px];
  const unsigned long long k1 = paired9 ? kp[HW + px] : ~0ull;
  float* mv = moved4 + (size_t)b * 4 * HW + px;
  int w0 = -1, w1 = -1;
  if (k0 != ~0ull) {
    w0 = (int)(unsigned int)(k0 & 0xffffffffu);
    const float* sp = src + (size_t)b * src_ss + w0;
    float qx, qy, qz;
    reproject_point(m, sp[0], sp[HW], sp[2 * HW], qx, qy, qz);
    mv[0] = qx; mv[HW] = qy; mv[2 * HW] = qz; mv[3 * HW] = __uint_as_float((unsigned int)(k0 >> 32));   // the range the vote computed
  } else {
    mv[0] = 0.f; mv[HW] = 0.f; mv[2 * HW] = 0.f; mv[3 * HW] = 0.f;
  }
  if (paired9) {
    float* pp = paired9 + (size_t)b * 9 * HW + px;
    float o[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (k1 != ~0ull) {
      w1 = (int)(unsigned int)(k1 & 0xffffffffu);
      const float* sp = src + (size_t)b * src_ss + w1;
      const float* np_ = srcn + (size_t)b * srcn_ss + w1;
      const float* mp = match + (size_t)b * match_ss + w1;
      reproject_point(m, sp[0], sp[HW], sp[2 * HW], o[0], o[1], o[2]);
      reproject_normal(m, np_[0], np_[HW], np_[2 * HW], o[3], o[4], o[5]);
      o[6] = o[0] - mp[0]; o[7] = o[1] - mp[HW]; o[8] = o[2] - mp[2 * HW];
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) pp[c * HW] = o[c];
  }
  if (src_pix) {
    src_pix[(size_t)b * 2 * HW + px] = w0;
    src_pix[(size_t)b * 2 * HW + HW + px] = w1;
  }
}

extern "C" size_t dl_reproject_workspace_bytes(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (((size_t)B * 2 * H * W * sizeof(uint64_t)) + 15) & ~(size_t)15;
}

extern "C" int dl_reproject(const float* src_image4, int64_t src_ss, const float* src_normals, int64_t srcn_ss, const float* match,
                            int64_t match_ss, const int32_t* nn_pix, const float* T, int32_t B, const dl_sensor* sensor,
                            float* moved4, float* paired9, int32_t* src_pix, void* workspace, dl_stream stream) {
  if (!src_image4 || !T || !sensor || !moved4 || !workspace)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: null pointer argument");
  if (B <= 0 || sensor->H < 2 || sensor->W < 2)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: bad sizes B=%d H=%d W=%d", B, sensor->H, sensor->W);
  const int64_t HW = (int64_t)sensor->H * sensor->W;
  if (HW * 2 * B > 0x7fffffffLL)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: B=%d images of H=%d W=%d exceed 2^31 key words", B, sensor->H, sensor->W);
  const int pairs = (src_normals ? 1 : 0) + (match ? 1 : 0) + (nn_pix ? 1 : 0);
  if (pairs != 0 && pairs != 3)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: src_normals, match and nn_pix may be NULL only together");
  if (paired9 && !pairs) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: paired9 needs src_normals, match and nn_pix");
  if (src_ss < 3 * HW || (pairs && (srcn_ss < 3 * HW || match_ss < 6 * HW)))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: scan strides src_ss=%lld srcn_ss=%lld match_ss=%lld below the dense sizes of H*W=%lld",
                   (long long)src_ss, (long long)srcn_ss, (long long)match_ss, (long long)HW);
  if ((uintptr_t)workspace & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_reproject: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const SensorK sen = make_sensor(sensor);
  unsigned long long* keys = (unsigned long long*)workspace;                 // [B][2][H*W]
  dl_fill_words(keys, 0xffffffffu, (size_t)B * 2 * sen.HW * 2, st);          // a kernel node, not a memset node, under capture
  const int G = (sen.HW + DL_BLOCK - 1) / DL_BLOCK;
  const bool vote_pairs = pairs && paired9;                                  // without paired9 plane 1 stays empty: src_pix plane 1 is -1
  hipLaunchKernelGGL(k_reproject_vote, dim3(reproject_grid(B, G)), dim3(DL_BLOCK), 0, st, src_image4, src_ss, src_normals, srcn_ss, match,
                     match_ss, vote_pairs ? nn_pix : (const int32_t*)nullptr, T, B, G, sen, keys);
  hipLaunchKernelGGL(k_reproject_resolve, dim3(reproject_grid(B, G)), dim3(DL_BLOCK), 0, st, src_image4, src_ss, src_normals, srcn_ss, match,
                     match_ss, T, B, G, sen, (const unsigned long long*)keys, moved4, paired9, src_pix);
  return dl_check_launch("dl_reproject");
}
