// The stem of the pose CNN in half precision (config key amp_stem under amp_dtype): the transposing copy of the planar fp32 input to
// channels-last F16 / BF16, conv1 (3x3, stride (1,2), 8 -> 64 channels, wrap-around width) + activation on
// v_mfma_f32_32x32x16_{f16,bf16}, the 3x3 / stride-(1,2) max-pooling on the half map with its int8 window plane, and conv1's weight
// gradient fused with the pooling backward and the activation derivative.  The fp32 stem (csrc/stem.hip, conv.hip) is untouched.
//
//   x8h [N][H][W][8]      = h(x [N][8][H][W])                      h = ch_f2h: round to nearest even, torch's .to(dtype)
//   a   [N][H][W/2][64]   = h(act(sum_{r,s,c} h(w1[k][r][s][c]) x8h[y + r - 1][(2 wc + s - 1) mod W][c]))      fp32 accumulation
//   y   [N][H][W/4][64], win int8                                  the window rule of k_pool_nhwc_fwd (csrc/stem.hip) on the half values
//   dw  [64][8][3][3]     = sum_pixels gc x8h,  gc = h(act'(a) * sum of g over the windows that selected the element), never in memory
//
// Operand map of the 32x32x16 MFMA (lane l, li = l & 31, half = l >> 5): A[row li][k = 8 half + j], B[k = 8 half + j][col li], j = 0..7
// in one 16-byte register quad; D[row (r & 3) + 8 (r >> 2) + 4 half][col li] in accumulator register r.
#include "common.h"
#include "convh_common.h"

typedef float f32x4h __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// x [N][8][H][W] fp32 -> x8h [N][H][W][8]: one thread = one pixel, eight plane reads (each coalesced over the wave), one 16-byte store.
template <bool F16>
__global__ __launch_bounds__(DL_BLOCK) void k_stemh_input(const float* __restrict__ x, uint32_t HW, uint32_t total, u16* __restrict__ x8h) {
  const uint32_t i = blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i >= total) return;
  const uint32_t n = i / HW, p = i - n * HW;
  const float* src = x + (size_t)n * 8 * HW + p;
  u16x8 o;
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = ch_f2h<F16>(src[(size_t)c * HW]);
  reinterpret_cast<u16x8*>(x8h)[i] = o;
}

// ---------------------------------------------------------------------------------------------------------------------
// conv1 + activation.  The conv1-output pixels of the whole batch are one flat list (n, y, wc); a wave takes 32 consecutive ones per
// tile (a tile may cross a row's or an image's end: every lane derives its own row and column).  M = 64 output channels (A: the
// weights, two 32-row subtiles), N = 32 pixels (B), reduction k = (tap, c): a lane's B fragment of step t is its pixel's 16-byte x8h
// record at tap 2 t + half -- nine taps are five steps, the upper half of the fifth is zero.  The 40 registers of A are built once
// per wave from the raw fp32 parameter [64][3][3][8] (18 KB: no prepared buffer).  The accumulators hold 4 consecutive channels per
// register quad; they leave through a wave-private 32 x 64 LDS tile (pitch 72: the quads of a pixel row spread over the banks) as
// 16-byte pieces of the tile's contiguous 4 KB.
#define SH_TILE 32
#define SH_PITCH 72
#define SH_MAX_GRID 1024          // four workgroups per CU; beyond 4096 tiles a wave takes every (4 grid)-th tile
template <bool F16>
__global__ __launch_bounds__(DL_BLOCK) void k_stemh_conv1(const u16* __restrict__ x8h, const float* __restrict__ w1, int H, int W,
                                                          uint32_t total, int tiles, int iters, int act, u16* __restrict__ a) {
  __shared__ __attribute__((aligned(16))) u16 tile[4][SH_TILE * SH_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, half = lane >> 5;
  const uint32_t Wc = (uint32_t)W >> 1;
  s16x8 wa[5][2];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int ms = 0; ms < 2; ++ms) {
      const int tap = 2 * t + half;
      s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (tap < 9) {
        const float* p = w1 + ((ms * 32 + li) * 9 + tap) * 8;
        const f32x4h lo = *reinterpret_cast<const f32x4h*>(p), hi = *reinterpret_cast<const f32x4h*>(p + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          v[j] = (short)ch_f2h<F16>(lo[j]);
          v[4 + j] = (short)ch_f2h<F16>(hi[j]);
        }
      }
      wa[t][ms] = v;
    }
  u16* my = tile[wave];
  const int nwaves = gridDim.x * 4, gw = blockIdx.x * 4 + wave;
  for (int it = 0; it < iters; ++it) {                                         // the same trip count for every wave: barriers inside
    const int tl = it * nwaves + gw;
    const bool live = tl < tiles;
    const uint32_t pix = (uint32_t)(live ? tl : 0) * SH_TILE + li;
    f32x16 acc[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = acc[1][r] = 0.f;
    if (live) {
      const bool in = pix < total;
      const uint32_t nr = (in ? pix : 0) / Wc;                                 // n * H + y
      const int wc = (int)((in ? pix : 0) - nr * Wc), y = (int)(nr % (uint32_t)H);
      s16x8 xb[5];
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const int tap = 2 * t + half, r = tap / 3, s = tap - 3 * r;
        const int yy = y + r - 1;
        int col = 2 * wc + s - 1;
        col = col < 0 ? col + W : col;                                         // 2 wc + 1 <= W - 1: only the left neighbour wraps
        s16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (in && tap < 9 && yy >= 0 && yy < H) v = *reinterpret_cast<const s16x8*>(x8h + (((size_t)nr + r - 1) * W + col) * 8);
        xb[t] = v;
      }
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        acc[0] = ch_mfma<F16>(wa[t][0], xb[t], acc[0]);
        acc[1] = ch_mfma<F16>(wa[t][1], xb[t], acc[1]);
      }
    }
    __syncthreads();                                                           // the previous tile's pieces have been read
    if (live) {
#pragma unroll
      for (int ms = 0; ms < 2; ++ms)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          s16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = (short)ch_f2h<F16>(ch_act(acc[ms][4 * q + j], act));
          *reinterpret_cast<s16x4*>(my + li * SH_PITCH + ms * 32 + 8 * q + 4 * half) = o;
        }
    }
    __syncthreads();
    if (live) {
      const size_t base = (size_t)tl * SH_TILE;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int piece = u * 64 + lane, pl = piece >> 3, part = piece & 7;
        if (base + pl < total)
          *reinterpret_cast<s16x8*>(a + (base + pl) * 64 + part * 8) = *reinterpret_cast<const s16x8*>(my + pl * SH_PITCH + part * 8);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The pooling on the half map: one thread = one pooled pixel x 8 channels (16-byte loads; a 64-channel pixel is read whole by 8
// neighbouring lanes).  The comparison runs on the exactly converted fp32 values with the rule of k_pool_nhwc_fwd, so y and win are
// those of the fp32 pooling of float(a), and y converts back without rounding.
template <bool F16>
__global__ __launch_bounds__(DL_BLOCK) void k_stemh_pool(const u16* __restrict__ a, int H, int Wc, int C8, uint32_t total, u16* __restrict__ y,
                                                         int8_t* __restrict__ win) {
  const uint32_t i = blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int Wp = Wc >> 1;
  const uint32_t pix = i / (uint32_t)C8;
  const int c8 = (int)(i - pix * (uint32_t)C8);
  const uint32_t nr = pix / (uint32_t)Wp;
  const int q = (int)(pix - nr * (uint32_t)Wp);
  const int r = (int)(nr % (uint32_t)H);
  const int first = r > 0 ? 0 : 3;
  float best[8];
  u16x8 bits;
  uint32_t k[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    best[e] = -INFINITY;
    bits[e] = ch_f2h<F16>(-INFINITY);
    k[e] = (uint32_t)first;
  }
#pragma unroll
  for (int dh = -1; dh <= 1; ++dh) {
    if (r + dh < 0 || r + dh >= H) continue;
    const u16* row = a + ((size_t)(nr + dh) * Wc) * (size_t)(8 * C8) + 8 * c8;
#pragma unroll
    for (int dw = -1; dw <= 1; ++dw) {
      int j = 2 * q + dw;
      j = j < 0 ? j + Wc : j;
      const u16x8 v = *reinterpret_cast<const u16x8*>(row + (size_t)j * (8 * C8));
      const uint32_t kk = (uint32_t)((dh + 1) * 3 + dw + 1);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = ch_h2f<F16>(v[e]);
        if (f > best[e] || f != f) { best[e] = f; bits[e] = v[e]; k[e] = kk; }
      }
    }
  }
  reinterpret_cast<u16x8*>(y)[i] = bits;
  uint2 w;
  w.x = k[0] | (k[1] << 8) | (k[2] << 16) | (k[3] << 24);
  w.y = k[4] | (k[5] << 8) | (k[6] << 16) | (k[7] << 24);
  reinterpret_cast<uint2*>(win)[i] = w;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of conv1 fused with the pooling backward and the activation derivative, on half operands.  The launch plan is that
// of k_stem_wgrad (csrc/stem.hip): 64-pixel chunks of the conv1-output rows (the last chunk of a row may hang over its end), a
// workgroup walks a slab of consecutive chunks, at most 512 slabs, partials [slab][64][72] in the workspace, summed in a fixed order
// by k_stemh_wgrad_reduce.  M = 64 k (two subtiles), N = 72 (tap, c) columns in three 32-column subtiles, reduction = pixels, 16 per
// MFMA: both operands are wanted with eight consecutive PIXELS per lane, so the 256 threads write both tiles transposed --
//   gct [k][pixel]            gc = h(act'(a) * (sum of the six candidate gradients in the order of pool_bwd_value, fp32))
//   xt  [(tap, c)][pixel]     x8h[y + r - 1][(2 (wc0 + pixel) + s - 1) mod W][c]: a record of the 3 x 130 patch goes to the plane of
//                             every tap that reads it (even patch columns: s = 0 and s = 2 of the pixel before; odd ones: s = 1)
// -- and wave w multiplies the pixels 16 w .. 16 w + 15 of every chunk (6 MFMAs).  The four waves' accumulators are added in the order
// ((0 + 1) + 2) + 3.  No float atomics; the same bits from run to run.
#define SGH_PX 64
#define SGH_PITCH 72                 // halves per row of both transposed tiles: 144 bytes, every 8-pixel fragment 16-byte aligned
#define SGH_XCOLS (2 * SGH_PX + 2)

template <bool F16>
__device__ __forceinline__ void stemh_gc8(const u16* __restrict__ g, const u16* __restrict__ a, const int8_t* __restrict__ win, int H, int Wc,
                                          int act, uint32_t nr, int r, int j, int c8, u16* out) {
  const int Wp = Wc >> 1;
  const int q0 = j >> 1, col0 = 1 + (j & 1);
  const int q1 = (q0 + 1 == Wp) ? 0 : q0 + 1;
  const bool two = (j & 1) != 0;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
  for (int d = -1; d <= 1; ++d) {                        // pooled row r + d sees this element at window row 1 - d
    const bool row_ok = r + d >= 0 && r + d < H;
    const size_t rowbase = (size_t)(nr + (row_ok ? d : 0)) * Wp;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const size_t e0 = ((rowbase + ((t && two) ? q1 : q0)) * 8 + c8) * 8;      // 64 channels: 8 groups of 8
      const uint2 w = *reinterpret_cast<const uint2*>(win + e0);
      const u16x8 gv = *reinterpret_cast<const u16x8*>(g + e0);
      const uint32_t code = (row_ok && (t == 0 || two)) ? (uint32_t)((1 - d) * 3 + (t ? 0 : col0)) : 0xffu;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t we = ((e < 4 ? w.x : w.y) >> (8 * (e & 3))) & 0xffu;
        acc[e] += we == code ? ch_h2f<F16>(gv[e]) : 0.f;
      }
    }
  }
  const u16x8 av = *reinterpret_cast<const u16x8*>(a + (((size_t)nr * Wc + j) * 8 + c8) * 8);
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float y = ch_h2f<F16>(av[e]);
    float v = acc[e];
    if (act == 1) v = acc[e] * (1.f - y * y);
    else if (act == 2) v = y <= 0.f ? 0.f : acc[e];
    out[e] = ch_f2h<F16>(v);
  }
}

template <bool F16>
__global__ __launch_bounds__(DL_BLOCK, 2) void k_stemh_wgrad(const u16* __restrict__ g, const u16* __restrict__ a, const int8_t* __restrict__ win,
                                                             const u16* __restrict__ x8h, int N, int H, int Wc, int act, int chunks_per_slab,
                                                             float* __restrict__ part) {
  constexpr int K = 64;
  __shared__ __attribute__((aligned(16))) u16 gct[K * SGH_PITCH];              // [k][pixel]
  __shared__ __attribute__((aligned(16))) u16 xt[72 * SGH_PITCH];              // [(tap, c)][pixel]
  __shared__ float red[3 * 1024];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, half = lane >> 5;
  const int W = 2 * Wc;
  const int cpr = (Wc + SGH_PX - 1) / SGH_PX;
  const int total = N * H * cpr;
  const int ch_begin = blockIdx.x * chunks_per_slab, ch_end = min(ch_begin + chunks_per_slab, total);
  f32x16 acc[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  int b_row[3];                                                                // columns 72..95 read a valid row, unused
#pragma unroll
  for (int ns = 0; ns < 3; ++ns) b_row[ns] = min(li + 32 * ns, 71);
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const int cb = ch % cpr;
    const uint32_t nr = (uint32_t)(ch / cpr);                                  // n * H + h
    const int h = (int)(nr % (uint32_t)H), wc0 = cb * SGH_PX;
    __syncthreads();                                                           // the previous chunk's fragments have been read
#pragma unroll
    for (int it = 0; it < SGH_PX * 8 / DL_BLOCK; ++it) {
      const int q = tid + it * DL_BLOCK, pl = q >> 3, c8 = q & 7;
      u16 v[8];
      if (wc0 + pl < Wc) stemh_gc8<F16>(g, a, win, H, Wc, act, nr, h, wc0 + pl, c8, v);
      else
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0;                                  // pixels beyond the row's end contribute nothing
#pragma unroll
      for (int e = 0; e < 8; ++e) gct[(c8 * 8 + e) * SGH_PITCH + pl] = v[e];
    }
    for (int q = tid; q < 3 * SGH_XCOLS; q += DL_BLOCK) {                      // one 16-byte record: (row, patch column m)
      const int m = q % SGH_XCOLS, row = q / SGH_XCOLS;
      const int hh = h + row - 1;
      int w = (2 * wc0 - 1 + m) % W;
      w = w < 0 ? w + W : w;
      u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (hh >= 0 && hh < H) v = *reinterpret_cast<const u16x8*>(x8h + (((size_t)nr + row - 1) * W + w) * 8);
      // patch column m = 2 pl + s
      if (m & 1) {
        const int pl = m >> 1;                                                 // s = 1; m <= 127 here (m = 129 is odd: pl = 64, no pixel)
        if (pl < SGH_PX)
#pragma unroll
          for (int c = 0; c < 8; ++c) xt[((row * 3 + 1) * 8 + c) * SGH_PITCH + pl] = v[c];
      } else {
        const int pl = m >> 1;                                                 // s = 0 of pixel pl, s = 2 of pixel pl - 1
        if (pl < SGH_PX)
#pragma unroll
          for (int c = 0; c < 8; ++c) xt[((row * 3 + 0) * 8 + c) * SGH_PITCH + pl] = v[c];
        if (pl >= 1)
#pragma unroll
          for (int c = 0; c < 8; ++c) xt[((row * 3 + 2) * 8 + c) * SGH_PITCH + pl - 1] = v[c];
      }
    }
    __syncthreads();
    const int p0 = wave * 16 + 8 * half;                                       // this lane's eight pixels of the wave's sixteen
    const s16x8 a0 = *reinterpret_cast<const s16x8*>(gct + li * SGH_PITCH + p0);
    const s16x8 a1 = *reinterpret_cast<const s16x8*>(gct + (32 + li) * SGH_PITCH + p0);
#pragma unroll
    for (int ns = 0; ns < 3; ++ns) {
      const s16x8 b = *reinterpret_cast<const s16x8*>(xt + b_row[ns] * SGH_PITCH + p0);
      acc[0][ns] = ch_mfma<F16>(a0, b, acc[0][ns]);
      acc[1][ns] = ch_mfma<F16>(a1, b, acc[1][ns]);
    }
  }
  // ((wave 0 + wave 1) + wave 2) + wave 3 through LDS, one accumulator at a time, then the slab's partial [64][72]
#pragma unroll
  for (int ms = 0; ms < 2; ++ms)
#pragma unroll
    for (int ns = 0; ns < 3; ++ns) {
      __syncthreads();
      if (wave > 0)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[(wave - 1) * 1024 + r * 64 + lane] = acc[ms][ns][r];
      __syncthreads();
      if (wave == 0) {
        const int j = ns * 32 + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float t = ((acc[ms][ns][r] + red[r * 64 + lane]) + red[1024 + r * 64 + lane]) + red[2048 + r * 64 + lane];
          const int k = ms * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
          if (j < 72) part[((size_t)blockIdx.x * K + k) * 72 + j] = t;
        }
      }
    }
}

// dw [64][8][3][3] = sum over slabs of part[slab][k][(r * 3 + s) * 8 + c]: wave w of a workgroup adds the slabs w, w + 4, ... in
// order, the four sums are added in wave order (the walk of k_stem_wgrad_reduce, csrc/stem.hip).
__global__ __launch_bounds__(DL_BLOCK) void k_stemh_wgrad_reduce(const float* __restrict__ part, int nslabs, float* __restrict__ dw) {
  __shared__ float red[4][64];
  const int i = blockIdx.x * 64 + (threadIdx.x & 63), w = threadIdx.x >> 6;      // (k, j) with j = tap * 8 + c
  float s = 0.f;
  int sl = w;
  for (; sl + 28 < nslabs; sl += 32) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(sl + 4 * u) * 64 * 72 + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; sl < nslabs; sl += 4) s += part[(size_t)sl * 64 * 72 + i];
  red[w][threadIdx.x & 63] = s;
  __syncthreads();
  if (w == 0) {
    const float t = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
    const int k = i / 72, j = i % 72, tap = j >> 3, c = j & 7;
    dw[(k * 8 + c) * 9 + tap] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static bool sh_misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

static int sh_dtype(const char* what, int dtype) {
  if (dtype != DL_DTYPE_F16 && dtype != DL_DTYPE_BF16)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: dtype=%d not supported (1 DL_DTYPE_F16, 2 DL_DTYPE_BF16)", what, dtype);
  return DL_OK;
}

#define SH_LIMIT ((size_t)1 << 31)

/* see include/delora_hip.h */
extern "C" int dl_stem_input_nhwc_h(const float* x_nchw, int32_t N, int32_t H, int32_t W, int32_t dtype, void* x8h, dl_stream stream) {
  const char* what = "dl_stem_input_nhwc_h";
  if (!x_nchw) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x_nchw is NULL", what);
  if (!x8h) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x8h is NULL", what);
  if (N <= 0 || H <= 0 || W <= 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: N=%d H=%d W=%d must be positive", what, N, H, W);
  if (sh_misaligned(x_nchw, 4)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x_nchw is not 4-byte aligned", what);
  if (sh_misaligned(x8h, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x8h is not 16-byte aligned", what);
  if (int rc = sh_dtype(what, dtype)) return rc;
  if (W % 4) return dl_fail(DL_ERR_UNSUPPORTED, "%s: W=%d must be a multiple of 4", what, W);
  if ((size_t)N * H * W * 8 >= SH_LIMIT) return dl_fail(DL_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d: the image has 2^31 elements or more", what, N, H, W);
  const uint32_t total = (uint32_t)N * H * W;
  const dim3 grid((total + DL_BLOCK - 1) / DL_BLOCK);
  const DlProfTag tag{"k_stemh_input", "fwd", N, H, W, 8, 8, 1, 1, 1, 0.0, (double)total * 8 * 6};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DL_DTYPE_F16) DL_LAUNCH(tag, k_stemh_input<true>, grid, dim3(DL_BLOCK), st, x_nchw, (uint32_t)(H * W), total, (u16*)x8h);
  else DL_LAUNCH(tag, k_stemh_input<false>, grid, dim3(DL_BLOCK), st, x_nchw, (uint32_t)(H * W), total, (u16*)x8h);
  return dl_check_launch(what);
}

/* see include/delora_hip.h */
extern "C" int dl_stem_conv1_h(const void* x8h, const float* w1, int32_t N, int32_t H, int32_t W, int32_t act, int32_t dtype, void* a,
                               dl_stream stream) {
  const char* what = "dl_stem_conv1_h";
  if (!x8h) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x8h is NULL", what);
  if (!w1) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: w1 is NULL", what);
  if (!a) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: a is NULL", what);
  if (N <= 0 || H <= 0 || W <= 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: N=%d H=%d W=%d must be positive", what, N, H, W);
  if (act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: act=%d is not 0 (none), 1 (tanh) or 2 (relu)", what, act);
  if (sh_misaligned(x8h, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: x8h is not 16-byte aligned", what);
  if (sh_misaligned(w1, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: w1 is not 16-byte aligned", what);
  if (sh_misaligned(a, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: a is not 16-byte aligned", what);
  if (int rc = sh_dtype(what, dtype)) return rc;
  if (W % 4) return dl_fail(DL_ERR_UNSUPPORTED, "%s: W=%d must be a multiple of 4", what, W);
  if ((size_t)N * H * W * 32 >= SH_LIMIT)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d: the output a has 2^31 elements or more", what, N, H, W);
  const uint32_t total = (uint32_t)N * H * (W / 2);
  const int tiles = (int)((total + SH_TILE - 1) / SH_TILE);
  const int grid = min((tiles + 3) / 4, SH_MAX_GRID), iters = (tiles + grid * 4 - 1) / (grid * 4);
  const DlProfTag tag{"k_stemh_conv1", "fwd", N, H, W, 8, 64, 3, 1, 2, 2.0 * total * 64.0 * 72.0, (double)total * (2 * 16 + 128)};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DL_DTYPE_F16)
    DL_LAUNCH(tag, k_stemh_conv1<true>, dim3(grid), dim3(DL_BLOCK), st, (const u16*)x8h, w1, H, W, total, tiles, iters, act, (u16*)a);
  else
    DL_LAUNCH(tag, k_stemh_conv1<false>, dim3(grid), dim3(DL_BLOCK), st, (const u16*)x8h, w1, H, W, total, tiles, iters, act, (u16*)a);
  return dl_check_launch(what);
}

/* see include/delora_hip.h */
extern "C" int dl_stem_pool_fwd_h(const void* a, int32_t N, int32_t H, int32_t Wc, int32_t C, int32_t dtype, void* y, int8_t* win,
                                  dl_stream stream) {
  const char* what = "dl_stem_pool_fwd_h";
  if (!a) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: a is NULL", what);
  if (!y) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: y is NULL", what);
  if (!win) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: win is NULL", what);
  if (N <= 0 || H <= 0 || Wc <= 0 || C <= 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: N=%d H=%d Wc=%d C=%d must be positive", what, N, H, Wc, C);
  if (sh_misaligned(a, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: a is not 16-byte aligned", what);
  if (sh_misaligned(y, 16)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: y is not 16-byte aligned", what);
  if (sh_misaligned(win, 8)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: win is not 8-byte aligned", what);
  if (int rc = sh_dtype(what, dtype)) return rc;
  if (Wc & 1) return dl_fail(DL_ERR_UNSUPPORTED, "%s: Wc=%d must be even", what, Wc);
  if (C & 7) return dl_fail(DL_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of 8", what, C);
  if ((size_t)N * H * Wc * C >= SH_LIMIT)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: N=%d H=%d Wc=%d C=%d: the map a has 2^31 elements or more", what, N, H, Wc, C);
  const uint32_t total = (uint32_t)((size_t)N * H * (Wc / 2) * (C / 8));
  const dim3 grid((total + DL_BLOCK - 1) / DL_BLOCK);
  const DlProfTag tag{"k_stemh_pool", "fwd", N, H, Wc, C, C, 3, 1, 2, 0.0, (double)total * 8 * (4 + 2 + 1)};
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DL_DTYPE_F16) DL_LAUNCH(tag, k_stemh_pool<true>, grid, dim3(DL_BLOCK), st, (const u16*)a, H, Wc, C / 8, total, (u16*)y, win);
  else DL_LAUNCH(tag, k_stemh_pool<false>, grid, dim3(DL_BLOCK), st, (const u16*)a, H, Wc, C / 8, total, (u16*)y, win);
  return dl_check_launch(what);
}

static int stemh_wgrad_slabs(int total_chunks) { return total_chunks < 512 ? total_chunks : 512; }

/* see include/delora_hip.h */
extern "C" size_t dl_stem_wgrad_h_workspace_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0 || W % 4 || (size_t)N * H * W * 32 >= SH_LIMIT) return 0;
  return (size_t)stemh_wgrad_slabs(N * H * ((W / 2 + SGH_PX - 1) / SGH_PX)) * 64 * 72 * sizeof(float);
}

/* see include/delora_hip.h */
extern "C" int dl_stem_wgrad_h(const void* g_pooled, const void* a, const int8_t* win, const void* x8h, int32_t N, int32_t H, int32_t W,
                               int32_t act, int32_t dtype, void* workspace, float* dw, dl_stream stream) {
  const char* what = "dl_stem_wgrad_h";
  const struct { const void* p; const char* name; size_t align; } ptrs[] = {
      {g_pooled, "g_pooled", 16}, {a, "a", 16}, {win, "win", 8}, {x8h, "x8h", 16}, {workspace, "workspace", 16}, {dw, "dw", 4}};
  for (const auto& q : ptrs)
    if (!q.p) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: %s is NULL", what, q.name);
  if (N <= 0 || H <= 0 || W <= 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: N=%d H=%d W=%d must be positive", what, N, H, W);
  if (act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: act=%d is not 0 (none), 1 (tanh) or 2 (relu)", what, act);
  for (const auto& q : ptrs)
    if (sh_misaligned(q.p, q.align)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: %s is not %d-byte aligned", what, q.name, (int)q.align);
  if (int rc = sh_dtype(what, dtype)) return rc;
  if (W % 4) return dl_fail(DL_ERR_UNSUPPORTED, "%s: W=%d must be a multiple of 4", what, W);
  if ((size_t)N * H * W * 32 >= SH_LIMIT)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: N=%d H=%d W=%d: conv1's output a has 2^31 elements or more", what, N, H, W);
  const int Wc = W / 2, total = N * H * ((Wc + SGH_PX - 1) / SGH_PX), nslabs = stemh_wgrad_slabs(total);
  const int cps = (total + nslabs - 1) / nslabs, grid = (total + cps - 1) / cps;
  hipStream_t st = (hipStream_t)stream;
  const DlProfTag tag{"k_stemh_wgrad", "wgrad", N, H, W, 8, 64, 3, 1, 2, 2.0 * N * H * Wc * 64.0 * 72.0,
                      2.0 * ((double)N * H * Wc * 64 * 1.5 + (double)N * H * W * 8) + (double)N * H * (Wc / 2) * 64};
  if (dtype == DL_DTYPE_F16)
    DL_LAUNCH(tag, k_stemh_wgrad<true>, dim3(grid), dim3(DL_BLOCK), st, (const u16*)g_pooled, (const u16*)a, win, (const u16*)x8h, N, H, Wc, act,
              cps, (float*)workspace);
  else
    DL_LAUNCH(tag, k_stemh_wgrad<false>, dim3(grid), dim3(DL_BLOCK), st, (const u16*)g_pooled, (const u16*)a, win, (const u16*)x8h, N, H, Wc, act,
              cps, (float*)workspace);
  DL_LAUNCH_PLAIN(k_stemh_wgrad_reduce, dim3(64 * 72 / 64), dim3(DL_BLOCK), st, (const float*)workspace, grid, dw);
  return dl_check_launch(what);
}
