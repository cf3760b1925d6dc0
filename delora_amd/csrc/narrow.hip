// The narrow fp32 family for the layers of a NARROW pose network (factor_fewer_resnet_channels 2 and 4: widths 32/64/128/256 and
// 16/32/64/128, reference src/models/resnet_modified.py:28-31): what csrc/tower.hip does for the feature tower -- channels-last,
// v_mfma_f32_16x16x4_f32 (exact fp32), wrap-around columns and zero rows as addressing, tiles that hang over the edges, fixed summation
// orders, no float atomics -- extended by what a residual network needs on top: stride (1,2), 1x1 filters, a residual-add epilogue and
// the strided layers' input gradient.  Dense tensors only (the tower's views are not needed here).
//
//   k_narrow_conv<NT, BT, SW, UP>   GEMM: M = output pixels, N = output channels, reduction = (tap, input channel), as k_tower_conv: a
//     workgroup of 4 waves owns 4 rows x (64 / SW) output columns, wave r owns row r as 4 / SW 16-pixel M tiles times NT N tiles.  Per
//     chunk of 16 input channels a 6 x 66 halo tile and the weight slab are staged in LDS.
//       SW = 2 (stride (1,2)): the TILE WIDTH IS HALVED to 32 output columns, so that the halo stays 66 input columns (65 used) and
//         the LDS budget stays that of the stride-1 kernel: 31.7 KB halo + 46.1 KB weights (NT = 4) = 77.8 KB, two workgroups per CU
//         of 160 KB.  The loader de-interleaves the halo -- even columns first, odd columns from slot 33 on -- so that the 16 pixels
//         of an A fragment stay 20 floats apart (tap 0: even slot m, tap 1: odd slot m, tap 2: even slot m + 1) and the fragment
//         reads are as conflict free as at stride 1.
//       UP (input gradient of a stride-(1,2) layer): the output gradient g [N][H][ceil(W/2)][K] is read as if zeros stood between
//         its columns -- halo column v of the W-wide ring reads g[v / 2] for even v and zero for odd v -- and the stride-1 transposed
//         convolution runs on that virtual image.  Zero insertion is exact on any width, odd ones included (column W - 1 of an odd
//         ring is even and holds the last gradient column; its right neighbour is column 0), and never exists in memory.  It issues
//         twice the MFMA work the phase-split form would: the two strided 3x3 layers of a narrow network are a small part of a step.
//       ks = 1 runs the centre tap alone.
//     Tail on the accumulators, in the order of dl_conv2d_nhwc_f32: ADD, ADD_GRID (even columns), ACT, DACT.
//   k_narrow_wgrad<MT, NT, ND>      k_tower_wgrad with a column stride between the gradient's and the input's pixels: GEMM M = output
//     channels, N = input channels, reduction = gradient pixels, operands read straight from memory, one tap row per grid.y (ND = 3
//     taps each; ND = 1: the 1x1 filter), the four waves added in a fixed order through LDS, one partial dW per workgroup, summed in
//     a fixed order (16 strands of every 16th slab, then the strands) by k_narrow_wgrad_reduce.
#include "common.h"

typedef float nr_f32x4 __attribute__((ext_vector_type(4)));

#define NR_THREADS 256
#define NR_TH 4                    // tile rows = waves
#define NR_RH (NR_TH + 2)
#define NR_RW 66                   // staged input columns: 64 + 2 at stride 1, 2 * 31 + 3 = 65 used at stride 2
#define NR_ODD 33                  // stride 2: first slot of the odd halo columns
#define NR_CK 16                   // input channels staged per chunk
#define NR_S (NR_CK + 4)           // floats per staged pixel: 4 * odd
#define NR_EPI_ADD 1u
#define NR_EPI_ACT 2u
#define NR_EPI_DACT 4u
#define NR_EPI_ADD_GRID 8u
#define NR_SEG 256                 // gradient columns per weight-gradient work unit
#define NR_MAX_SLABS 512

struct NrConvArgs {
  const float* x;      // [N][H][Wx][C]
  const float* w;      // BT = 0: [K][ks][ks][C]   BT = 1: [C][ks][ks][K] read with flipped taps
  float* y;            // [N][H][Wo][K]
  const float* add;    // ADD: [N][H][Wo][K]; ADD_GRID: [N][H][ceil(Wo / 2)][K]; or null
  const float* dsrc;   // [N][H][Wo][K], or null
  int N, H, W;         // W: the ring the columns wrap around (the input image, or the virtual zero-inserted one)
  int Wx, Wo;          // stored input columns, output columns
  int C, K, ks;
  int act;
  unsigned epi;
};

__device__ __forceinline__ float nr_act(float v, int act) {
  if (act == 1) return dl_tanh(v);
  if (act == 2) return v < 0.f ? 0.f : v;
  return v;
}
__device__ __forceinline__ float nr_dact(float y, int act) {
  if (act == 1) return 1.f - y * y;
  if (act == 2) return y <= 0.f ? 0.f : 1.f;
  return 1.f;
}

template <int NT, bool BT, int SW, bool UP>
__global__ __launch_bounds__(NR_THREADS, 2) void k_narrow_conv(NrConvArgs a) {
  constexpr int KP = NT * 16;
  constexpr int KS = (KP % 32 == 0) ? KP + 16 : KP;          // weight row stride: 16 * odd floats
  constexpr int MI = 4 / SW;                                   // 16-pixel M tiles of a wave's row
  constexpr int TWO = MI * 16;                                 // output columns of a tile
  constexpr int NI = NR_RH * NR_RW * (NR_CK / 4);              // float4 items of the halo tile
  constexpr int NI_IT = (NI + NR_THREADS - 1) / NR_THREADS;
  constexpr int NWE = 9 * NR_CK * KP;                          // weight elements of a chunk
  __shared__ __attribute__((aligned(16))) float in_lds[NR_RH * NR_RW * NR_S];
  __shared__ float w_lds[9 * NR_CK * KS];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const int tiles_w = (a.Wo + TWO - 1) / TWO, tiles_h = (a.H + NR_TH - 1) / NR_TH;
  int t = blockIdx.x;
  const int tw_i = t % tiles_w; t /= tiles_w;
  const int th_i = t % tiles_h;
  const int n = t / tiles_h;
  const int h0 = th_i * NR_TH, w0 = tw_i * TWO;
  const bool ks1 = a.ks == 1;
  const float* xn = a.x + (size_t)n * a.H * a.Wx * a.C;

  // chunk-invariant staging items: the lane's float4 (four channels c4*4 .. c4*4+3 of one halo pixel); -1: reads zeros / no item
  const int c4 = tid & 3;                  // (NR_THREADS % 4 == 0: the same for every item of a thread)
  int in_g[NI_IT], in_l[NI_IT];
#pragma unroll
  for (int it = 0; it < NI_IT; ++it) {
    const int q = tid + it * NR_THREADS;
    const int pc = q >> 2;
    const int col = pc % NR_RW, row = pc / NR_RW;
    const int h = h0 - 1 + row;
    int v = (w0 * SW - 1 + col) % a.W;     // overhanging tiles of narrow images reach several widths out: a true modulo
    v = v < 0 ? v + a.W : v;
    const bool live = !UP || !(v & 1);     // UP: the odd columns of the ring are the inserted zeros
    const int wx = UP ? v >> 1 : v;
    const int slot = SW == 2 ? (col & 1) * NR_ODD + (col >> 1) : col;
    in_l[it] = q < NI ? (row * NR_RW + slot) * NR_S + c4 * 4 : -1;
    in_g[it] = (q < NI && live && h >= 0 && h < a.H) ? (h * a.Wx + wx) * a.C + c4 * 4 : -1;
  }

  nr_f32x4 acc[MI][NT];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  const int a_base = (wave * NR_RW + li) * NR_S + kg;
  const int b_base = kg * KS + li;
  const int ntaps = a.ks * a.ks;

  for (int c0 = 0; c0 < a.C; c0 += NR_CK) {
    const int cs = min(NR_CK, a.C - c0);               // channels of this chunk: a multiple of 4
    if (c0) __syncthreads();                           // every wave is done with the previous chunk
    if (c4 * 4 < cs) {
#pragma unroll
      for (int it = 0; it < NI_IT; ++it) {
        if (in_l[it] < 0) continue;
        nr_f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (in_g[it] >= 0) v = *reinterpret_cast<const nr_f32x4*>(xn + in_g[it] + c0);
        *reinterpret_cast<nr_f32x4*>(in_lds + in_l[it]) = v;
      }
    }
    for (int idx = tid; idx < NWE; idx += NR_THREADS) {
      int c, k, tap;
      if (BT) { k = idx % KP; c = (idx / KP) % NR_CK; tap = idx / (KP * NR_CK); }
      else { c = idx % NR_CK; k = (idx / NR_CK) % KP; tap = idx / (KP * NR_CK); }
      if (c >= cs || (ks1 && tap != 4)) continue;
      const int tg = ks1 ? 0 : tap;                    // the tap's index in the stored filter
      float v = 0.f;                                   // output channels K .. KP-1 are padding: zero weights
      if (k < a.K) v = BT ? a.w[((c0 + c) * ntaps + (ntaps - 1 - tg)) * a.K + k] : a.w[(k * ntaps + tg) * a.C + c0 + c];
      w_lds[(tap * NR_CK + c) * KS + k] = v;
    }
    __syncthreads();
    const int nsteps = cs >> 2;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      if (ks1 && tap != 4) continue;                   // (uniform)
      const int dh = tap / 3, dw = tap % 3;
      const int dslot = SW == 2 ? (dw == 1 ? NR_ODD : dw >> 1) : dw;     // slot of the tap's column for pixel 0 of the row
      for (int s = 0; s < nsteps; ++s) {
        float av[MI], bv[NT];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) av[mi] = in_lds[a_base + (dh * NR_RW + dslot + mi * 16) * NR_S + s * 4];
#pragma unroll
        for (int ni = 0; ni < NT; ++ni) bv[ni] = w_lds[b_base + (tap * NR_CK + s * 4) * KS + ni * 16];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
          for (int ni = 0; ni < NT; ++ni) acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
      }
    }
  }

  // Epilogue: accumulator (mi, ni), register r of lane (li, kg) = pixel mi*16 + 4*kg + r of the wave's row, channel ni*16 + li
  const int h = h0 + wave;
  if (h >= a.H) return;
  const bool f_add = a.epi & NR_EPI_ADD, f_grid = a.epi & NR_EPI_ADD_GRID, f_act = a.epi & NR_EPI_ACT, f_dact = a.epi & NR_EPI_DACT;
  const int Wg = (a.Wo + 1) >> 1;
  const size_t img = (size_t)n * a.H * a.Wo * a.K;
  float* yn = a.y + img;
  const float* an = f_add ? a.add + img : f_grid ? a.add + (size_t)n * a.H * Wg * a.K : nullptr;
  const float* dn = f_dact ? a.dsrc + img : nullptr;
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int w = w0 + mi * 16 + kg * 4 + r;
      if (w >= a.Wo) continue;
      const int p = h * a.Wo + w;
#pragma unroll
      for (int ni = 0; ni < NT; ++ni) {
        const int k = ni * 16 + li;
        if (k >= a.K) continue;
        float v = acc[mi][ni][r];
        if (f_add) v += an[p * a.K + k];
        if (f_grid && !(w & 1)) v += an[(h * Wg + (w >> 1)) * a.K + k];
        if (f_act) v = nr_act(v, a.act);
        if (f_dact) v *= nr_dact(dn[p * a.K + k], a.act);
        yn[p * a.K + k] = v;
      }
    }
}

struct NrWgArgs {
  const float* x;    // [N][H][W][C]
  const float* g;    // [N][H][Wo][K]
  float* part;       // [nslabs][K][ks*ks][C]
  int N, H, W, Wo, C, K, sw;
  int nseg, units, units_per_slab;
};

template <int MT, int NT, int ND>
__global__ __launch_bounds__(NR_THREADS) void k_narrow_wgrad(NrWgArgs a) {
  __shared__ float red[MT * NT * ND * 4 * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, kg = lane >> 4;
  const int dh = ND == 3 ? (int)blockIdx.y : 1;               // (the 1x1 filter is the centre tap)
  nr_f32x4 acc[MT][NT][ND];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int d = 0; d < ND; ++d)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][d][r] = 0.f;

  const int u0 = blockIdx.x * a.units_per_slab, u1 = min(u0 + a.units_per_slab, a.units);
  for (int u = u0 + wave; u < u1; u += 4) {                 // (wave-uniform)
    const int row = u / a.nseg, seg = u % a.nseg;
    const int n = row / a.H, h = row % a.H;
    const int hx = h + dh - 1;
    if (hx < 0 || hx >= a.H) continue;                      // the zero row above / below the image
    const int wbeg = seg * NR_SEG, wend = min(a.Wo, wbeg + NR_SEG);
    const float* grow = a.g + ((size_t)n * a.H + h) * a.Wo * a.K;
    const float* xrow = a.x + ((size_t)n * a.H + hx) * a.W * a.C;
    for (int wq = wbeg; wq < wend; wq += 4) {
      const int w = wq + kg;                                // the lane's gradient pixel of this reduction step
      const bool ok = w < wend;
      const int xc = w * a.sw;                              // its centre column of the input (ok: below W)
      const int wm = xc == 0 ? a.W - 1 : xc - 1, wp = xc + 1 >= a.W ? xc + 1 - a.W : xc + 1;
      float av[MT], bv[NT][ND];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int k = mt * 16 + li;
        av[mt] = (ok && k < a.K) ? grow[w * a.K + k] : 0.f;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int c = nt * 16 + li;
        const bool okc = ok && c < a.C;                     // (a pixel beyond the row must not feed a NaN into 0 * x)
        if (ND == 3) {
          bv[nt][0] = okc ? xrow[wm * a.C + c] : 0.f;
          bv[nt][ND / 2] = okc ? xrow[xc * a.C + c] : 0.f;
          bv[nt][ND - 1] = okc ? xrow[wp * a.C + c] : 0.f;
        } else {
          bv[nt][0] = okc ? xrow[xc * a.C + c] : 0.f;
        }
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int d = 0; d < ND; ++d) acc[mt][nt][d] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt], bv[nt][d], acc[mt][nt][d], 0, 0, 0);
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
          for (int d = 0; d < ND; ++d)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = ((((mt * NT + nt) * ND + d) * 4) + r) * 64 + lane;
              red[i] = wv ? red[i] + acc[mt][nt][d][r] : acc[mt][nt][d][r];
            }
    }
    __syncthreads();
  }
  // slot (mt, nt, d, r, lane) = dW[k = mt*16 + 4*(lane >> 4) + r][tap = dh*3 + d (1x1: 0)][c = nt*16 + (lane & 15)]
  constexpr int TAPS = ND * ND;
  float* part = a.part + (size_t)blockIdx.x * a.K * TAPS * a.C;
  for (int i = tid; i < MT * NT * ND * 4 * 64; i += NR_THREADS) {
    const int l = i & 63, r = (i >> 6) & 3;
    int q = i >> 8;
    const int d = q % ND; q /= ND;
    const int nt = q % NT, mt = q / NT;
    const int k = mt * 16 + 4 * (l >> 4) + r, c = nt * 16 + (l & 15);
    const int tap = ND == 3 ? dh * 3 + d : 0;
    if (k < a.K && c < a.C) part[(k * TAPS + tap) * a.C + c] = red[i];
  }
}

// The slab sum in a fixed order that does not depend on the launch: a workgroup owns 16 consecutive elements of dW; thread (q, e) adds
// the slabs q, q + 16, q + 32, .. of element e in increasing order, then the 16 strands of an element are added in order of q.  (One
// thread per element walking all of up to 512 slabs is a chain of dependent loads: 47 us per layer at 64x2048, B = 8.)
#define NR_RED_Q 16
__global__ __launch_bounds__(NR_THREADS) void k_narrow_wgrad_reduce(const float* __restrict__ part, int nslabs, int count, float* __restrict__ dw) {
  __shared__ float strand[NR_RED_Q][NR_THREADS / NR_RED_Q];
  const int e = threadIdx.x % (NR_THREADS / NR_RED_Q), q = threadIdx.x / (NR_THREADS / NR_RED_Q);
  const int i = blockIdx.x * (NR_THREADS / NR_RED_Q) + e;
  float s = 0.f;
  if (i < count)
    for (int j = q; j < nslabs; j += NR_RED_Q) s += part[(size_t)j * count + i];
  strand[q][e] = s;
  __syncthreads();
  if (q == 0 && i < count) {
    float t = strand[0][e];
    for (int k = 1; k < NR_RED_Q; ++k) t += strand[k][e];
    dw[i] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {
bool nr_channels_ok(int C, int K) { return C >= 4 && K >= 8 && C <= 64 && K <= 64 && C % 4 == 0 && K % 8 == 0; }
// (32-bit pixel offsets inside an image, at most 64 channels per pixel)
bool nr_small(int N, int H, int W) { return (size_t)N * H * W * 64 < ((size_t)1 << 31); }

// the checks every entry point shares; C, K: the LAYER's input / output channels.  0, or the status dl_fail returned
int nr_check_layer(const char* who, int N, int H, int W, int C, int K, int ksize, int stride_h, int stride_w) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: empty shape (N=%d H=%d W=%d C=%d K=%d)", who, N, H, W, C, K);
  if (ksize != 3 && ksize != 1) return dl_fail(DL_ERR_UNSUPPORTED, "%s: ksize=%d (the narrow family has 3x3 and 1x1 filters)", who, ksize);
  if (stride_h != 1 || (stride_w != 1 && stride_w != 2))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: stride (%d,%d) (the narrow family has stride (1,1) and (1,2))", who, stride_h, stride_w);
  if (!nr_channels_ok(C, K))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: C=%d K=%d is outside the narrow family (C %% 4 == 0, K %% 8 == 0, both <= 64)", who, C, K);
  if (!nr_small(N, H, W)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: tensors beyond 2^31 elements are not supported (split the batch)", who);
  return 0;
}

struct NrPlan {
  int nseg, units, units_per_slab, nslabs;
};
NrPlan nr_wgrad_plan(int N, int H, int Wo) {
  NrPlan p;
  p.nseg = (Wo + NR_SEG - 1) / NR_SEG;
  p.units = N * H * p.nseg;
  int per = (p.units + NR_MAX_SLABS - 1) / NR_MAX_SLABS;
  per = (per + 3) / 4 * 4;                              // every wave of a workgroup gets the same number of units
  p.units_per_slab = per;
  p.nslabs = (p.units + per - 1) / per;
  return p;
}

// mode 0: forward at stride 1; 1: forward at stride (1,2); 2: transposed; 3: transposed on the zero-inserted gradient
template <int NT>
void nr_launch_conv(const NrConvArgs& a, int mode, const DlProfTag& tag, hipStream_t st) {
  const int two = mode == 1 ? 32 : 64;
  const dim3 grid(a.N * ((a.H + NR_TH - 1) / NR_TH) * ((a.Wo + two - 1) / two)), block(NR_THREADS);
  switch (mode) {
    case 0: DL_LAUNCH(tag, (k_narrow_conv<NT, false, 1, false>), grid, block, st, a); break;
    case 1: DL_LAUNCH(tag, (k_narrow_conv<NT, false, 2, false>), grid, block, st, a); break;
    case 2: DL_LAUNCH(tag, (k_narrow_conv<NT, true, 1, false>), grid, block, st, a); break;
    default: DL_LAUNCH(tag, (k_narrow_conv<NT, true, 1, true>), grid, block, st, a); break;
  }
}
void nr_conv(const NrConvArgs& a, int mode, const DlProfTag& tag, hipStream_t st) {
  switch ((a.K + 15) / 16) {
    case 1: nr_launch_conv<1>(a, mode, tag, st); break;
    case 2: nr_launch_conv<2>(a, mode, tag, st); break;
    case 3: nr_launch_conv<3>(a, mode, tag, st); break;
    default: nr_launch_conv<4>(a, mode, tag, st); break;
  }
}
template <int MT, int ND>
void nr_launch_wgrad(const NrWgArgs& a, int nt, dim3 grid, const DlProfTag& tag, hipStream_t st) {
  switch (nt) {
    case 1: DL_LAUNCH(tag, (k_narrow_wgrad<MT, 1, ND>), grid, dim3(NR_THREADS), st, a); break;
    case 2: DL_LAUNCH(tag, (k_narrow_wgrad<MT, 2, ND>), grid, dim3(NR_THREADS), st, a); break;
    case 3: DL_LAUNCH(tag, (k_narrow_wgrad<MT, 3, ND>), grid, dim3(NR_THREADS), st, a); break;
    default: DL_LAUNCH(tag, (k_narrow_wgrad<MT, 4, ND>), grid, dim3(NR_THREADS), st, a); break;
  }
}
template <int ND>
void nr_wgrad(const NrWgArgs& a, dim3 grid, const DlProfTag& tag, hipStream_t st) {
  const int nt = (a.C + 15) / 16;
  switch ((a.K + 15) / 16) {
    case 1: nr_launch_wgrad<1, ND>(a, nt, grid, tag, st); break;
    case 2: nr_launch_wgrad<2, ND>(a, nt, grid, tag, st); break;
    case 3: nr_launch_wgrad<3, ND>(a, nt, grid, tag, st); break;
    default: nr_launch_wgrad<4, ND>(a, nt, grid, tag, st); break;
  }
}
}  // namespace

/* see include/delora_hip.h */
extern "C" int dl_narrow_conv2d_nhwc_f32(const float* x, const float* w, float* y, const float* add, const float* dsrc, int32_t N, int32_t H,
                                         int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, int32_t transposed,
                                         int32_t act, uint32_t epilogue, dl_stream stream) {
  const char* who = "dl_narrow_conv2d_nhwc_f32";
  if (!x || !w || !y) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer (x, w or y)", who);
  if (epilogue & ~(NR_EPI_ADD | NR_EPI_ACT | NR_EPI_DACT)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: unknown epilogue flag in %u", who, epilogue);
  if (act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: act=%d outside 0..2", who, act);
  if ((epilogue & NR_EPI_ADD) && !add) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: DL_CONV_ADD without add", who);
  if ((epilogue & NR_EPI_DACT) && !dsrc) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: DL_CONV_DACT without dsrc", who);
  // transposed: x is the output gradient (C = the layer's output channels), y the input gradient
  if (int rc = nr_check_layer(who, N, H, W, transposed ? K : C, transposed ? C : K, ksize, stride_h, stride_w)) return rc;
  if (transposed && stride_w != 1)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: transposed with stride (%d,%d): the strided input gradient is dl_narrow_dgrad_strided_nhwc_f32", who,
                   stride_h, stride_w);
  const int Wo = (W + stride_w - 1) / stride_w;
  NrConvArgs a{x, w, y, (epilogue & NR_EPI_ADD) ? add : nullptr, (epilogue & NR_EPI_DACT) ? dsrc : nullptr, N, H, W, W, Wo, C, K, ksize, act, epilogue};
  const DlProfTag tag{"k_narrow_conv", transposed ? "dgrad" : "fwd", N, H, W, C, K, ksize, stride_h, stride_w,
                      2.0 * N * H * Wo * (double)K * C * ksize * ksize, 4.0 * ((double)N * H * ((double)W * C + (double)Wo * K) + (double)ksize * ksize * K * C)};
  nr_conv(a, transposed ? 2 : stride_w == 2 ? 1 : 0, tag, (hipStream_t)stream);
  return dl_check_launch(who);
}

/* see include/delora_hip.h */
extern "C" int dl_narrow_dgrad_strided_nhwc_f32(const float* g, const float* w, float* dx, const float* add_grid, const float* dsrc, int32_t N,
                                                int32_t H, int32_t W, int32_t K, int32_t C, int32_t ksize, int32_t stride_h, int32_t stride_w,
                                                int32_t dense, int32_t act, uint32_t epilogue, dl_stream stream) {
  const char* who = "dl_narrow_dgrad_strided_nhwc_f32";
  if (!g || !w || !dx) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer (g, w or dx)", who);
  if (epilogue & ~(NR_EPI_ADD_GRID | NR_EPI_DACT)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: unknown epilogue flag in %u", who, epilogue);
  if (act < 0 || act > 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: act=%d outside 0..2", who, act);
  if ((epilogue & NR_EPI_ADD_GRID) && !add_grid) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: DL_CONV_ADD_GRID without add_grid", who);
  if ((epilogue & NR_EPI_DACT) && !dsrc) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: DL_CONV_DACT without dsrc", who);
  if (int rc = nr_check_layer(who, N, H, W, C, K, ksize, stride_h, stride_w)) return rc;
  if (stride_w != 2) return dl_fail(DL_ERR_UNSUPPORTED, "%s: stride (%d,%d): a stride-1 layer's input gradient is the transposed dl_narrow_conv2d_nhwc_f32", who,
                                    stride_h, stride_w);
  if (dense && (ksize != 1 || epilogue))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: dense is the 1x1 layers' gradient on the grid, without an epilogue (ksize=%d, epilogue=%u)", who, ksize, epilogue);
  const int Wg = (W + 1) / 2;
  // as a convolution: input g with the layer's K channels, output dx with its C channels
  NrConvArgs a{g, w, dx, (epilogue & NR_EPI_ADD_GRID) ? add_grid : nullptr, (epilogue & NR_EPI_DACT) ? dsrc : nullptr, N, H, dense ? Wg : W, Wg,
               dense ? Wg : W, K, C, ksize, act, epilogue};
  const DlProfTag tag{"k_narrow_conv", "dgrad_strided", N, H, W, C, K, ksize, stride_h, stride_w, 2.0 * N * H * a.Wo * (double)K * C * ksize * ksize,
                      4.0 * ((double)N * H * ((double)a.Wo * C + (double)Wg * K) + (double)ksize * ksize * K * C)};
  nr_conv(a, dense ? 2 : 3, tag, (hipStream_t)stream);
  return dl_check_launch(who);
}

/* see include/delora_hip.h */
extern "C" size_t dl_narrow_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t ksize, int32_t stride_h,
                                                  int32_t stride_w) {
  if (N <= 0 || H <= 0 || W <= 0 || (ksize != 1 && ksize != 3) || stride_h != 1 || (stride_w != 1 && stride_w != 2) || !nr_channels_ok(C, K) ||
      !nr_small(N, H, W))
    return 0;
  return (size_t)nr_wgrad_plan(N, H, (W + stride_w - 1) / stride_w).nslabs * K * ksize * ksize * C * sizeof(float);
}

/* see include/delora_hip.h */
extern "C" int dl_narrow_wgrad_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H, int32_t W, int32_t C,
                                        int32_t K, int32_t ksize, int32_t stride_h, int32_t stride_w, dl_stream stream) {
  const char* who = "dl_narrow_wgrad_nhwc_f32";
  if (!x || !g || !dw || !workspace) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer (x, g, dw or workspace)", who);
  if (int rc = nr_check_layer(who, N, H, W, C, K, ksize, stride_h, stride_w)) return rc;
  const int Wo = (W + stride_w - 1) / stride_w;
  const NrPlan p = nr_wgrad_plan(N, H, Wo);
  NrWgArgs a{x, g, (float*)workspace, N, H, W, Wo, C, K, stride_w, p.nseg, p.units, p.units_per_slab};
  const DlProfTag tag{"k_narrow_wgrad", "wgrad", N, H, W, C, K, ksize, stride_h, stride_w, 2.0 * N * H * Wo * (double)K * C * ksize * ksize,
                      4.0 * ((double)N * H * ((double)W * C + (double)Wo * K) + (double)ksize * ksize * K * C)};
  hipStream_t st = (hipStream_t)stream;
  if (ksize == 3) nr_wgrad<3>(a, dim3(p.nslabs, 3), tag, st);
  else nr_wgrad<1>(a, dim3(p.nslabs, 1), tag, st);
  DL_PLAN_NOTE("slabs=%d", p.nslabs);
  const int count = K * ksize * ksize * C;
  constexpr int per = NR_THREADS / NR_RED_Q;            // elements of dW per workgroup
  DL_LAUNCH_PLAIN(k_narrow_wgrad_reduce, dim3((count + per - 1) / per), dim3(NR_THREADS), st, (const float*)workspace, p.nslabs, count, dw);
  return dl_check_launch(who);
}
