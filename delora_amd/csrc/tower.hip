// The "narrow" fp32 family: 3x3, stride-1 ring convolutions with FEW channels (4 .. 64) on channels-last tensors, for the per-image
// feature tower in front of the pose CNN (reference src/models/model.py:30-54: five CircularPad + Conv2d(4->8->16->24->32->40) +
// activation layers at full image resolution, torch Conv2d = a library convolution there) and its autograd.
//
// The direct family (conv.hip) tiles 64 output channels and 8 / 64 input channels; a 4 -> 8 or 32 -> 40 layer would spend most of
// a 32x32x2 MFMA on padding.  Here the arithmetic is v_mfma_f32_16x16x4_f32 (exact fp32, one rounding per product): output
// channels in tiles of 16, input channels in steps of 4, so that a layer pays for ceil(K / 16) * 16 x C.
//
//   forward / input gradient (k_tower_conv)   GEMM: M = pixels, N = output channels, reduction = (tap, input channel).  A workgroup
//     (4 waves) owns 4 rows x 64 columns of one image; wave r owns row r as four 16-pixel M tiles times NT = ceil(K / 16) N tiles.
//     Per chunk of 16 input channels the 6 x 66 halo tile and the [tap][channel][K] weight slab are staged in LDS once (wrap-around
//     columns and zero rows are addressing in the loader: no padded tensor exists); the fragments are ds_read_b32 with the
//     four reduction channels of an MFMA on the lane quarters (pixel stride 20 floats, weight row stride 16 * odd: conflict free).
//     The tail (activation, or multiplication by act' of a saved activation) runs on the accumulators.
//   weight gradient (k_tower_wgrad)           GEMM: M = output channels, N = input channels, reduction = pixels.  No LDS staging: a
//     lane's A operand is g[pixel][k], its B operand x[pixel + tap][c], both read straight from memory (16 lanes = 64 consecutive
//     bytes; the three taps of a row re-read the same lines from L1).  A wave walks a 256-column segment of one image row, a
//     workgroup a run of such segments for ONE tap row (grid.y = 3); its four waves are added in a fixed order through LDS and the
//     workgroup writes its partial dW to the workspace, which k_tower_wgrad_reduce sums in slab order.  No float atomics.
//
// Every tensor is addressed through a view (pitch, offset, group): pixel p of image n, channel c lies at
//     ((n / group) * H * W + p) * pitch + offset + (n % group) * CH + c        (CH = the tensor's own channel count)
// so that the fifth layer of the two images of a sample writes channels 0..39 and 40..79 of one wide stem input and the backward
// reads its slices from there: the reference's torch.cat (model.py:52) is never a copy.
#include "common.h"

typedef float tw_f32x4 __attribute__((ext_vector_type(4)));

#define TW_THREADS 256
#define TW_TH 4                    // tile rows = waves
#define TW_TW 64                   // tile columns
#define TW_RH (TW_TH + 2)
#define TW_RW (TW_TW + 2)
#define TW_CK 16                   // input channels staged per chunk
#define TW_S (TW_CK + 4)           // floats per staged pixel: 4 * odd
#define TW_EPI_ACT 2u
#define TW_EPI_DACT 4u
#define TW_SEG 256                 // columns per weight-gradient work unit
#define TW_MAX_SLABS 512

struct TwView {
  int pitch, off, group;
};

struct TwConvArgs {
  const float* x;      // view xv, C channels
  const float* w;      // BT = 0: [K][9][C]   BT = 1: [C][9][K] read with flipped taps
  float* y;            // view yv, K channels
  const float* dsrc;   // view dv, K channels, or null
  TwView xv, yv, dv;
  int N, H, W, C, K;
  int act;
  unsigned epi;
};

__device__ __forceinline__ float tw_act(float v, int act) {
  if (act == 1) return dl_tanh(v);
  if (act == 2) return v < 0.f ? 0.f : v;
  return v;
}
__device__ __forceinline__ float tw_dact(float y, int act) {
  if (act == 1) return 1.f - y * y;
  if (act == 2) return y <= 0.f ? 0.f : 1.f;
  return 1.f;
}
// element offset of pixel 0, channel 0 of image n in a view of a tensor with `ch` channels of its own (32-bit: the entry points
// keep every tensor below 2^31 elements)
__device__ __forceinline__ int tw_base(const TwView& v, int n, int hw, int ch) {
  return (n / v.group) * hw * v.pitch + v.off + (n % v.group) * ch;
}

template <int NT, bool BT>
__global__ __launch_bounds__(TW_THREADS, 2) void k_tower_conv(TwConvArgs a) {
  constexpr int KP = NT * 16;
  constexpr int KS = (KP % 32 == 0) ? KP + 16 : KP;          // weight row stride: 16 * odd floats
  constexpr int NI = TW_RH * TW_RW * (TW_CK / 4);              // float4 items of the halo tile
  constexpr int NI_IT = (NI + TW_THREADS - 1) / TW_THREADS;
  constexpr int NWE = 9 * TW_CK * KP;                          // weight elements of a chunk
  __shared__ __attribute__((aligned(16))) float in_lds[TW_RH * TW_RW * TW_S];
  __shared__ float w_lds[9 * TW_CK * KS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const int tiles_w = (a.W + TW_TW - 1) / TW_TW, tiles_h = (a.H + TW_TH - 1) / TW_TH;
  int t = blockIdx.x;
  const int tw_i = t % tiles_w; t /= tiles_w;
  const int th_i = t % tiles_h;
  const int n = t / tiles_h;
  const int h0 = th_i * TW_TH, w0 = tw_i * TW_TW;
  const int hw = a.H * a.W;
  const float* xn = a.x + tw_base(a.xv, n, hw, a.C);

  // chunk-invariant staging items: the lane's float4 (four channels c4*4 .. c4*4+3 of one halo pixel); -1: reads zeros / no item
  const int c4 = tid & 3;                  // (TW_THREADS % 4 == 0: the same for every item of a thread)
  int in_g[NI_IT], in_l[NI_IT];
#pragma unroll
  for (int it = 0; it < NI_IT; ++it) {
    const int q = tid + it * TW_THREADS;
    const int pc = q >> 2;
    const int col = pc % TW_RW, row = pc / TW_RW;
    const int h = h0 - 1 + row;
    int w = (w0 - 1 + col) % a.W;          // overhanging tiles of narrow images reach several widths out: a true modulo
    w = w < 0 ? w + a.W : w;
    in_l[it] = q < NI ? pc * TW_S + c4 * 4 : -1;
    in_g[it] = (q < NI && h >= 0 && h < a.H) ? (h * a.W + w) * a.xv.pitch + c4 * 4 : -1;
  }

  tw_f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  const int a_base = (wave * TW_RW + li) * TW_S + kg;
  const int b_base = kg * KS + li;

  for (int c0 = 0; c0 < a.C; c0 += TW_CK) {
    const int cs = min(TW_CK, a.C - c0);               // channels of this chunk: a multiple of 4
    if (c0) __syncthreads();                           // every wave is done with the previous chunk
    if (c4 * 4 < cs) {
#pragma unroll
      for (int it = 0; it < NI_IT; ++it) {
        if (in_l[it] < 0) continue;
        tw_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (in_g[it] >= 0) v = *reinterpret_cast<const tw_f32x4*>(xn + in_g[it] + c0);
        *reinterpret_cast<tw_f32x4*>(in_lds + in_l[it]) = v;
      }
    }
    for (int idx = tid; idx < NWE; idx += TW_THREADS) {
      int c, k, tap;
      if (BT) { k = idx % KP; c = (idx / KP) % TW_CK; tap = idx / (KP * TW_CK); }
      else { c = idx % TW_CK; k = (idx / TW_CK) % KP; tap = idx / (KP * TW_CK); }
      if (c >= cs) continue;
      float v = 0.f;                                   // output channels K .. KP-1 are padding: zero weights
      if (k < a.K) v = BT ? a.w[((c0 + c) * 9 + (8 - tap)) * a.K + k] : a.w[(k * 9 + tap) * a.C + c0 + c];
      w_lds[(tap * TW_CK + c) * KS + k] = v;
    }
    __syncthreads();
    const int nsteps = cs >> 2;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dh = tap / 3, dw = tap % 3;
      for (int s = 0; s < nsteps; ++s) {
        float av[4], bv[NT];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) av[mi] = in_lds[a_base + (dh * TW_RW + dw + mi * 16) * TW_S + s * 4];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) bv[ni] = w_lds[b_base + (tap * TW_CK + s * 4) * KS + ni * 16];
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
    }
  }

  // Epilogue: accumulator (mi, ni), register r of lane (li, kg) = pixel mi*16 + 4*kg + r of the wave's row, channel ni*16 + li
  const int h = h0 + wave;
  if (h >= a.H) return;
  const bool f_act = a.epi & TW_EPI_ACT, f_dact = a.epi & TW_EPI_DACT;
  float* yn = a.y + tw_base(a.yv, n, hw, a.K);
  const float* dn = f_dact ? a.dsrc + tw_base(a.dv, n, hw, a.K) : nullptr;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = w0 + mi * 16 + kg * 4 + r;
      if (w >= a.W) continue;
      const int p = h * a.W + w;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int k = ni * 16 + li;
        if (k >= a.K) continue;
        float v = acc[mi][ni][r];
        if (f_act) v = tw_act(v, a.act);
        if (f_dact) v *= tw_dact(dn[p * a.dv.pitch + k], a.act);
        yn[p * a.yv.pitch + k] = v;
      }
    }
}

struct TwWgArgs {
  const float* x;    // view xv, C channels
  const float* g;    // view gv, K channels
  float* part;       // [nslabs][K][9][C]
  TwView xv, gv;
  int N, H, W, C, K;
  int nseg, units, units_per_slab;
};

template <int MT, int NT>
__global__ __launch_bounds__(TW_THREADS) void k_tower_wgrad(TwWgArgs a) {
  __shared__ float red[MT * NT * 3 * 4 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const int dh = blockIdx.y;
  const int hw = a.H * a.W;
  tw_f32x4 acc[MT][NT][3];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][d][r] = 0.f;

  const int u0 = blockIdx.x * a.units_per_slab, u1 = min(u0 + a.units_per_slab, a.units);
  for (int u = u0 + wave; u < u1; u += 4) {                 // (wave-uniform)
    const int row = u / a.nseg, seg = u % a.nseg;
    const int n = row / a.H, h = row % a.H;
    const int hx = h + dh - 1;
    if (hx < 0 || hx >= a.H) continue;                      // the zero row above / below the image
    const int wbeg = seg * TW_SEG, wend = min(a.W, wbeg + TW_SEG);
    const float* grow = a.g + tw_base(a.gv, n, hw, a.K) + h * a.W * a.gv.pitch;
    const float* xrow = a.x + tw_base(a.xv, n, hw, a.C) + hx * a.W * a.xv.pitch;
    for (int wq = wbeg; wq < wend; wq += 4) {
      const int w = wq + kg;                                // the lane's pixel of this reduction step
      const bool ok = w < wend;
      const int wm = w == 0 ? a.W - 1 : w - 1, wp = w + 1 >= a.W ? w + 1 - a.W : w + 1;
      float av[MT], bv[NT][3];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int k = mt * 16 + li;
        av[mt] = (ok && k < a.K) ? grow[w * a.gv.pitch + k] : 0.f;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int c = nt * 16 + li;
        const bool okc = ok && c < a.C;                     // (a pixel beyond the row must not feed a NaN into 0 * x)
        bv[nt][0] = okc ? xrow[wm * a.xv.pitch + c] : 0.f;
        bv[nt][1] = okc ? xrow[w * a.xv.pitch + c] : 0.f;
        bv[nt][2] = okc ? xrow[wp * a.xv.pitch + c] : 0.f;
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int d = 0; d < 3; ++d) acc[mt][nt][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt][d], acc[mt][nt][d], 0, 0, 0);
    }
  }

  // the four waves in a fixed order: ((w0 + w1) + w2) + w3, every lane on its own LDS slots
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int d = 0; d < 3; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = ((((mt * NT + nt) * 3 + d) * 4) + r) * 64 + lane;
              red[i] = wv ? red[i] + acc[mt][nt][d][r] : acc[mt][nt][d][r];
            }
    }
    __syncthreads();
  }
  // slot (mt, nt, d, r, lane) = dW[k = mt*16 + 4*(lane >> 4) + r][tap = dh*3 + d][c = nt*16 + (lane & 15)]
  float* part = a.part + (size_t)blockIdx.x * a.K * 9 * a.C;
  for (int i = tid; i < MT * NT * 3 * 4 * 64; i += TW_THREADS) {
    const int l = i & 63, r = (i >> 6) & 3;
    int q = i >> 8;
    const int d = q % 3; q /= 3;
    const int nt = q % NT, mt = q / NT;
    const int k = mt * 16 + 4 * (l >> 4) + r, c = nt * 16 + (l & 15);
    if (k < a.K && c < a.C) part[(k * 9 + dh * 3 + d) * a.C + c] = red[i];
  }
}

__global__ __launch_bounds__(TW_THREADS) void k_tower_wgrad_reduce(const float* __restrict__ part, int nslabs, int count, float* __restrict__ dw) {
  const int i = blockIdx.x * TW_THREADS + threadIdx.x;
  if (i >= count) return;
  float s = part[i];
  for (int j = 1; j < nslabs; ++j) s += part[(size_t)j * count + i];
  dw[i] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {
// (a view is usable when its slices are 16-byte granular and lie inside a pixel's pitch)
bool tw_view_ok(const TwView& v, int ch, int N) {
  return v.group >= 1 && N % v.group == 0 && v.pitch > 0 && v.off >= 0 && v.pitch % 4 == 0 && v.off % 4 == 0 &&
         (long long)v.off + (long long)v.group * ch <= v.pitch;
}
bool tw_view_small(const TwView& v, int N, int H, int W) {
  return (size_t)(N / v.group) * H * W * (size_t)v.pitch < ((size_t)1 << 31);
}
bool tw_channels_ok(int C, int K) { return C >= 4 && K >= 8 && C <= 64 && K <= 64 && C % 4 == 0 && K % 8 == 0; }

struct TwPlan {
  int nseg, units, units_per_slab, nslabs;
};
TwPlan tw_wgrad_plan(int N, int H, int W) {
  TwPlan p;
  p.nseg = (W + TW_SEG - 1) / TW_SEG;
  p.units = N * H * p.nseg;
  int per = (p.units + TW_MAX_SLABS - 1) / TW_MAX_SLABS;
  per = (per + 3) / 4 * 4;                              // every wave of a workgroup gets the same number of units
  p.units_per_slab = per;
  p.nslabs = (p.units + per - 1) / per;
  return p;
}

template <int NT>
void tw_launch_conv(const TwConvArgs& a, bool bt, const DlProfTag& tag, hipStream_t st) {
  const int tiles = a.N * ((a.H + TW_TH - 1) / TW_TH) * ((a.W + TW_TW - 1) / TW_TW);
  if (bt) DL_LAUNCH(tag, (k_tower_conv<NT, true>), dim3(tiles), dim3(TW_THREADS), st, a);
  else DL_LAUNCH(tag, (k_tower_conv<NT, false>), dim3(tiles), dim3(TW_THREADS), st, a);
}
template <int MT>
void tw_launch_wgrad(const TwWgArgs& a, int nt, dim3 grid, const DlProfTag& tag, hipStream_t st) {
  switch (nt) {
    case 1: DL_LAUNCH(tag, (k_tower_wgrad<MT, 1>), grid, dim3(TW_THREADS), st, a); break;
    case 2: DL_LAUNCH(tag, (k_tower_wgrad<MT, 2>), grid, dim3(TW_THREADS), st, a); break;
    case 3: DL_LAUNCH(tag, (k_tower_wgrad<MT, 3>), grid, dim3(TW_THREADS), st, a); break;
    default: DL_LAUNCH(tag, (k_tower_wgrad<MT, 4>), grid, dim3(TW_THREADS), st, a); break;
  }
}
}  // namespace

/* see include/delora_hip.h */
extern "C" int dl_tower_conv3x3_nhwc_f32(const float* x, const float* w, float* y, const float* dsrc, int32_t N, int32_t H, int32_t W,
                                         int32_t C, int32_t K, const int32_t* x_view, const int32_t* y_view, const int32_t* dsrc_view,
                                         int32_t transposed, int32_t act, uint32_t epilogue, dl_stream stream) {
  if (!x || !w || !y || !x_view || !y_view || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_conv3x3_nhwc_f32: bad argument (null pointer or empty shape)");
  if (act < 0 || act > 2 || (epilogue & ~(TW_EPI_ACT | TW_EPI_DACT)) || ((epilogue & TW_EPI_DACT) && (!dsrc || !dsrc_view)))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_conv3x3_nhwc_f32: epilogue operand missing / bad activation or flag");
  if (!tw_channels_ok(C, K))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_tower_conv3x3_nhwc_f32: C=%d K=%d is outside the narrow family (C %% 4 == 0, K %% 8 == 0, both <= 64)", C, K);
  const bool f_dact = epilogue & TW_EPI_DACT;
  TwView xv{x_view[0], x_view[1], x_view[2]}, yv{y_view[0], y_view[1], y_view[2]}, dv{K, 0, 1};
  if (f_dact) dv = TwView{dsrc_view[0], dsrc_view[1], dsrc_view[2]};
  if (!tw_view_ok(xv, C, N) || !tw_view_ok(yv, K, N) || !tw_view_ok(dv, K, N))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_conv3x3_nhwc_f32: a view (pitch, offset, group) does not hold its channels in 16-byte steps");
  if (!tw_view_small(xv, N, H, W) || !tw_view_small(yv, N, H, W) || !tw_view_small(dv, N, H, W))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_tower_conv3x3_nhwc_f32: tensors beyond 2^31 elements are not supported (split the batch)");
  TwConvArgs a{x, w, y, f_dact ? dsrc : nullptr, xv, yv, dv, N, H, W, C, K, act, epilogue};
  const DlProfTag tag{"k_tower_conv", transposed ? "dgrad" : "fwd", N, H, W, C, K, 3, 1, 1, 2.0 * N * H * W * (double)K * C * 9,
                      4.0 * ((double)N * H * W * (C + K) + 9.0 * K * C)};
  hipStream_t st = (hipStream_t)stream;
  switch ((K + 15) / 16) {
    case 1: tw_launch_conv<1>(a, transposed != 0, tag, st); break;
    case 2: tw_launch_conv<2>(a, transposed != 0, tag, st); break;
    case 3: tw_launch_conv<3>(a, transposed != 0, tag, st); break;
    default: tw_launch_conv<4>(a, transposed != 0, tag, st); break;
  }
  return dl_check_launch("dl_tower_conv3x3_nhwc_f32");
}

/* see include/delora_hip.h */
extern "C" size_t dl_tower_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K) {
  if (N <= 0 || H <= 0 || W <= 0 || !tw_channels_ok(C, K) || (size_t)N * H * W * 64 >= ((size_t)1 << 31)) return 0;
  return (size_t)tw_wgrad_plan(N, H, W).nslabs * K * 9 * C * sizeof(float);
}

/* see include/delora_hip.h */
extern "C" int dl_tower_wgrad3x3_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W,
                                          int32_t C, int32_t K, const int32_t* x_view, const int32_t* g_view, dl_stream stream) {
  if (!x || !g || !dw || !workspace || !x_view || !g_view || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_wgrad3x3_nhwc_f32: bad argument (null pointer or empty shape)");
  if (!tw_channels_ok(C, K))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_tower_wgrad3x3_nhwc_f32: C=%d K=%d is outside the narrow family (C %% 4 == 0, K %% 8 == 0, both <= 64)", C, K);
  TwView xv{x_view[0], x_view[1], x_view[2]}, gv{g_view[0], g_view[1], g_view[2]};
  if (!tw_view_ok(xv, C, N) || !tw_view_ok(gv, K, N))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_tower_wgrad3x3_nhwc_f32: a view (pitch, offset, group) does not hold its channels in 16-byte steps");
  if (!tw_view_small(xv, N, H, W) || !tw_view_small(gv, N, H, W) || (size_t)N * H * W * 64 >= ((size_t)1 << 31))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_tower_wgrad3x3_nhwc_f32: tensors beyond 2^31 elements are not supported (split the batch)");
  const TwPlan p = tw_wgrad_plan(N, H, W);
  TwWgArgs a{x, g, (float*)workspace, xv, gv, N, H, W, C, K, p.nseg, p.units, p.units_per_slab};
  const DlProfTag tag{"k_tower_wgrad", "wgrad", N, H, W, C, K, 3, 1, 1, 2.0 * N * H * W * (double)K * C * 9,
                      4.0 * ((double)N * H * W * (C + K) + 9.0 * K * C)};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(p.nslabs, 3);
  const int nt = (C + 15) / 16;
  switch ((K + 15) / 16) {
    case 1: tw_launch_wgrad<1>(a, nt, grid, tag, st); break;
    case 2: tw_launch_wgrad<2>(a, nt, grid, tag, st); break;
    case 3: tw_launch_wgrad<3>(a, nt, grid, tag, st); break;
    default: tw_launch_wgrad<4>(a, nt, grid, tag, st); break;
  }
  DL_PLAN_NOTE("slabs=%d", p.nslabs);
  const int count = K * 9 * C;
  DL_LAUNCH_PLAIN(k_tower_wgrad_reduce, dim3((count + TW_THREADS - 1) / TW_THREADS), dim3(TW_THREADS), st, (const float*)workspace, p.nslabs,
                  count, dw);
  return dl_check_launch("dl_tower_wgrad3x3_nhwc_f32");
}
