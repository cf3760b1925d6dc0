// Stride-1 3x3 convolutions of the pose CNN as fused Winograd F(2x2, 3x3) on the fp32 matrix cores of gfx950.
//
// The 13 stride-1 3x3 layers (reference src/models/resnet_modified.py:159-177, 85 % of the network's multiplications) run
// forward and backward-data through this kernel: 2.25x fewer multiplications than the direct form, the same algorithm
// class the library's fp32 path (MIOpen's Winograd f2x3 assembly) uses, here on the matrix cores and with the layer's
// elementwise tail fused.  Everything happens in ONE launch per layer -- input transform, 16 batched GEMMs, output
// transform, epilogue -- so the transformed tensors (4x the activation's size) never touch HBM:
//
//   per workgroup (8 waves): 64 Winograd tiles (2x2 output pixels each) x 64 output channels
//   per chunk of 8 input channels:
//     raw   (2TR+2) x (2TC+2) x 8 input patch, wrap-around columns / zero rows by addressing      global -> regs -> LDS
//     V     = B^T d B  per (tile, channel):  16 planes [xi][tile][8]                              LDS -> regs -> LDS
//     U     transformed weights [xi][k][8] of this chunk (k_wino_weights, once per step)         global -> regs -> LDS
//     M[xi] += V[xi] (tiles x 8) * U[xi]^T (8 x k)        v_mfma_f32_32x32x2_f32, 16 independent GEMMs
//   wave (mb, nb, xh) owns tiles mb*32.., channels nb*32.., and the 8 planes xi = 8*xh..8*xh+7 (rows a = 2xh, 2xh+1 of the
//   4x4 Winograd domain): 8 accumulators = 128 VGPRs.  Output transform Y = A^T M A: the column pass is lane-local, the
//   row pass needs both halves -- the two waves of a block exchange 2x16 registers through LDS, after which wave xh holds
//   output row xh of every tile.  Epilogue (shortcut add, activation, activation derivative) as in conv.hip.
//
// Fragments use the same reduction-index permutation as conv.hip (one ds_read_b128 = four MFMAs); the [tile][8] rows are
// XOR-swizzled in 16-byte granules (bit 3 of the row index) so that those reads are bank-conflict free without padding.
//
// Numerics: fp32 throughout; Winograd F(2x2,3x3) adds/subtracts before and after the products, error ~1e-6 relative to the
// layer's output scale (tests/test_gpu_conv.py bounds it against torch's direct convolution at 1e-4).
#include "common.h"
#include "wgrad_batch.h"
#include <cstdlib>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

#define WN_THREADS 512
#define WN_CK 8
#define WN_KB 64
#define WN_TILES 64
#define WN_PLANE (WN_TILES * WN_CK + 16)      // floats per xi plane (+16: the four b-planes a lane group writes hit different banks)
#define WN_EPI_ADD 1u
#define WN_EPI_ACT 2u
#define WN_EPI_DACT 4u

struct WinoArgs {
  const float* x;      // [N][H][W][C]
  const float* u;      // [C/8][16][K][8] transformed weights (k_wino_weights)
  float* y;            // [N][H][W][K]
  const float* add;
  const float* dsrc;
  int N, H, W, C, K;
  int act;
  unsigned epi;
  int splits;          // k_wino_conv<.., .., true> only: the input channels are cut into this many ranges, one workgroup each; y then is
                       // the partial-sum workspace [splits][N][H][W][K] and k_wino_split_sum adds the ranges up and runs the epilogue
};

__device__ __forceinline__ float wn_act(float v, int act) {
  if (act == 1) return dl_tanh(v);
  if (act == 2) return v < 0.f ? 0.f : v;
  return v;
}
__device__ __forceinline__ float wn_dact(float y, int act) {
  if (act == 1) return 1.f - y * y;
  if (act == 2) return y <= 0.f ? 0.f : 1.f;
  return 1.f;
}

__device__ __forceinline__ int wn_xcd_swizzle(int id, int n) {
  const int q = n / 8, r = n % 8, xcd = id % 8, k = id / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// U = G g G^T for one (k, c): g 3x3 -> 4x4.  G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]].
__device__ __forceinline__ void wn_weight_transform(const float (&g)[3][3], float (&u)[4][4]) {
  float t[4][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    t[0][j] = g[0][j];
    t[1][j] = 0.5f * (g[0][j] + g[1][j] + g[2][j]);
    t[2][j] = 0.5f * (g[0][j] - g[1][j] + g[2][j]);
    t[3][j] = g[2][j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i][0] = t[i][0];
    u[i][1] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
    u[i][2] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
    u[i][3] = t[i][2];
  }
}

// Layout of the Winograd-domain weights (round 6): the reduction channels in chunks of 8, the output rows (k of u_fwd, c of u_bwd) in
// blocks of 64, and inside a (chunk, block) the 16 planes as the bytes k_wino_conv wants to find in LDS: [16][64 rows][8] with the
// 16-byte halves of a row swapped where bit 3 of the row index is set (the XOR swizzle of the fragment reads).  The DMA of a chunk is
// then a LINEAR copy of 32 KiB -- one per-lane offset (16 lane) for every piece, pieces addressed by immediate offsets from one M0 --
// instead of a gather with the swizzle in per-lane source offsets and an M0 write per piece.  Row counts that do not divide into blocks
// of 64 (never consumed by k_wino_conv) keep the plain [chunk][16][rows][8] order.
__device__ __host__ __forceinline__ size_t wn_u_row(int rows, int chunk, int xi, int r) {           // first float of row r's eight
  if (rows % 64) return (((size_t)chunk * 16 + xi) * rows + r) * 8;
  return ((((size_t)chunk * (rows / 64) + (r >> 6)) * 16 + xi) * 64 + (r & 63)) * 8;
}
__device__ __host__ __forceinline__ size_t wn_u_index(int rows, int chunk, int xi, int r, int e) {
  return wn_u_row(rows, chunk, xi, r) + ((rows % 64) ? e : ((((e >> 2) ^ ((r >> 3) & 1)) << 2) | (e & 3)));
}

// w [K][3][3][C] -> u_fwd (reduction over c, rows k) and u_bwd (the transposed convolution of the input gradient: taps flipped, channel
// roles swapped, reduction over k, rows c).  One thread per (k, c).
__global__ __launch_bounds__(256) void k_wino_weights(const float* __restrict__ w, float* __restrict__ u_fwd,
                                                      float* __restrict__ u_bwd, int K, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K * C) return;
  const int c = i % C, k = i / C;
  float g[3][3], gf[3][3], u[4][4];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      g[r][s] = w[((size_t)(k * 3 + r) * 3 + s) * C + c];
      gf[2 - r][2 - s] = g[r][s];
    }
  if (u_fwd) {
    wn_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u_fwd[wn_u_index(K, c / 8, xi, k, c % 8)] = u[xi / 4][xi % 4];
  }
  if (u_bwd) {
    wn_weight_transform(gf, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u_bwd[wn_u_index(C, k / 8, xi, c, k % 8)] = u[xi / 4][xi % 4];
  }
}

// x - y and -x - y of sixteen accumulator registers as eight packed instructions each (the compiler emits scalar v_sub_f32 for vector
// subtractions; outside the chunk loop the vector ALU is what the workgroup waits for)
#define WN_PK16(MODS)                                                                                                     \
  f32x2 r0, r1, r2, r3, r4, r5, r6, r7;                                                                                   \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r0) : "v"(__builtin_shufflevector(x, x, 0, 1)), "v"(__builtin_shufflevector(y, y, 0, 1)));     \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r1) : "v"(__builtin_shufflevector(x, x, 2, 3)), "v"(__builtin_shufflevector(y, y, 2, 3)));     \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r2) : "v"(__builtin_shufflevector(x, x, 4, 5)), "v"(__builtin_shufflevector(y, y, 4, 5)));     \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r3) : "v"(__builtin_shufflevector(x, x, 6, 7)), "v"(__builtin_shufflevector(y, y, 6, 7)));     \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r4) : "v"(__builtin_shufflevector(x, x, 8, 9)), "v"(__builtin_shufflevector(y, y, 8, 9)));     \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r5) : "v"(__builtin_shufflevector(x, x, 10, 11)), "v"(__builtin_shufflevector(y, y, 10, 11))); \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r6) : "v"(__builtin_shufflevector(x, x, 12, 13)), "v"(__builtin_shufflevector(y, y, 12, 13))); \
  asm volatile("v_pk_add_f32 %0, %1, %2 " MODS : "=v"(r7) : "v"(__builtin_shufflevector(x, x, 14, 15)), "v"(__builtin_shufflevector(y, y, 14, 15))); \
  const f32x4 a0 = __builtin_shufflevector(r0, r1, 0, 1, 2, 3), a1 = __builtin_shufflevector(r2, r3, 0, 1, 2, 3);         \
  const f32x4 a2 = __builtin_shufflevector(r4, r5, 0, 1, 2, 3), a3 = __builtin_shufflevector(r6, r7, 0, 1, 2, 3);         \
  typedef float f32x8_ __attribute__((ext_vector_type(8)));                                                               \
  const f32x8_ b0 = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7), b1 = __builtin_shufflevector(a2, a3, 0, 1, 2, 3, 4, 5, 6, 7); \
  return __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15);
__device__ __forceinline__ f32x16 wn_sub16(f32x16 x, f32x16 y) { WN_PK16("neg_lo:[0,1] neg_hi:[0,1]") }
__device__ __forceinline__ f32x16 wn_nsub16(f32x16 x, f32x16 y) { WN_PK16("neg_lo:[1,1] neg_hi:[1,1]") }
#undef WN_PK16

// The stores of a tile group for the flag combinations the network uses (tanh or no activation): compile-time flags, so the eight items of
// a lane are read, computed and stored in three straight batches instead of eight branchy read -> compute -> store chains.
template <bool ADD, bool ACT, bool DACT, bool RAG>
__device__ __forceinline__ void wn_store_items(const float* ep_lane, const f32x4 (&opv)[8], const unsigned (&ooff)[8], const unsigned (&aoff)[8], float* ysp,
                                               const float* add) {
  f32x4 v[8];
#pragma unroll
  for (int it = 0; it < 8; ++it) v[it] = *reinterpret_cast<const f32x4*>(ep_lane + it * 8 * 32);
  if (ADD && DACT) {
    f32x4 sc[8];
#pragma unroll
    for (int it = 0; it < 8; ++it) sc[it] = *reinterpret_cast<const f32x4*>(add + ((!RAG || ooff[it] != 0xffffffffu) ? aoff[it] : 0u));
#pragma unroll
    for (int it = 0; it < 8; ++it) v[it] += sc[it];
  } else if (ADD) {
#pragma unroll
    for (int it = 0; it < 8; ++it) v[it] += opv[it];
  }
  if (ACT) {
#pragma unroll
    for (int it = 0; it < 8; ++it) { v[it][0] = dl_tanh(v[it][0]); v[it][1] = dl_tanh(v[it][1]); v[it][2] = dl_tanh(v[it][2]); v[it][3] = dl_tanh(v[it][3]); }
  }
  if (DACT) {
#pragma unroll
    for (int it = 0; it < 8; ++it) v[it] *= 1.f - opv[it] * opv[it];
  }
#pragma unroll
  for (int it = 0; it < 8; ++it)
    if (!RAG || ooff[it] != 0xffffffffu) *reinterpret_cast<f32x4*>(ysp + ooff[it]) = v[it];
}

// TC tile columns x TR tile rows = 64 tiles per workgroup.
//
// Pipeline (one barrier per chunk).  LDS holds two (V, U) buffers and two raw-patch buffers.  While the waves multiply
// chunk c out of (V, U)[c & 1]:
//   * the LDS DMA (global_load_lds, no registers) brings U of chunk c+1 into (V, U)[(c+1) & 1] and the raw input patch of
//     chunk c+2 -- (2TR+2) x (2TC+2) pixels x 8 channels, wrap-around columns by addressing -- into raw[c & 1]; both have
//     the whole chunk to land;
//   * every thread turns the raw patch of chunk c+1 (raw[(c+1) & 1], landed during chunk c-1) into its column b of
//     V = B^T d B for its (tile, channel quad): 8 x 16-byte LDS reads, a few adds, 4 x 16-byte LDS writes.
// All of that is sliced into small pieces placed behind individual MFMAs: in-order issue means a wave's next MFMA on the
// same accumulator cannot issue for 64 cycles anyway, and a piece runs in that shadow.  The fences keep hipcc from
// sinking every piece to its first use.  (Fetching the raw pieces straight into registers -- 8 scattered 16-byte loads
// per thread and chunk, each 32-byte pixel slice requested by ~4 threads -- measured 15 % slower: the vector-memory
// path, not the matrix pipe, became the limit.)
// Ablation switches of the tuning builds (tools/wino_lab.hip; results are WRONG with any of them set, only the time is of interest):
// WN_ABL bit 0: no U DMA in the chunk loop, 1: no raw DMA, 2: no input transform, 3: no chunk barrier, 4: no fragment reads
#ifndef WN_ABL
#define WN_ABL 0
#endif

#if WN_ABL & 1
#define WN_IF_U(...)
#else
#define WN_IF_U(...) __VA_ARGS__
#endif
#if WN_ABL & 2
#define WN_IF_RAW(...)
#else
#define WN_IF_RAW(...) __VA_ARGS__
#endif
#if WN_ABL & 4
#define WN_IF_T(...)
#else
#define WN_IF_T(...) __VA_ARGS__
#endif
#if WN_ABL & 8
#define WN_IF_BAR(...)
#else
#define WN_IF_BAR(...) __VA_ARGS__
#endif
#if WN_ABL & 16
#define WN_IF_FR(...)
#else
#define WN_IF_FR(...) __VA_ARGS__
#endif
#ifdef CV_TUNE
__device__ unsigned long long g_wn_t[8 * 8192];       // phase time stamps per group (tools/conv_harness wino-phases)
#define WN_T(I) { if (tid == 0 && grp < 8192) g_wn_t[grp * 8 + (I)] = clock64(); }
#else
#define WN_T(I)
#endif
// RAG: the image does not divide into groups of TR x TC tiles (or has an odd width / height): the last group of a row / column
// hangs over the edge.  Its surplus tiles transform wrapped (valid) addresses and multiply like the others; only the epilogue
// differs -- surplus output pixels are neither fetched from the epilogue operands nor stored.
// SPLIT: split-K for SMALL problems.  A workgroup walks ALL input channels of its 64 tiles x 64 output channels: 8 ... 64 chunks of
// ~5400 cycles each, whatever the batch size -- at the reference's default batch size 1 (64x720: 24 ... 48 tile groups for 256 CUs) a
// layer4 launch was 170 us of ONE workgroup's serial chain with 90 % of the chip idle.  With SPLIT the group index also selects one of
// `splits` channel ranges; the workgroup accumulates that range only and stores its raw partial sums (no epilogue) to
// y + split * N*H*W*K; k_wino_split_sum adds the ranges in a fixed order and applies the epilogue.  SPLIT = false compiles to the
// code of round 4 (the split index and the chunk base are compile-time zeros).
// STR: a stride-(1,2) 3x3 layer as a stride-1 layer on the pixel-pair view [N][H][W/2][2C] of the same memory (the
// launch's a.W is W/2, its channel count 2C).  The rearranged kernel has no tap in its third column, so the four planes with xi-column
// 3 of U = G g G^T are zero (forward, STR = 1); for the transposed kernel of the input gradient it is xi-column 0 (STR = 2).  Those planes
// are left out at compile time: 6 of a wave's 8 planes multiply, their U pieces are not fetched, and the output transform drops their
// terms.  STR = 2 also adds the down-sampling branch's gradient `add` from its compact grid [N][H][W/2][K/2], on the even-pixel half of
// the output channels only.  STR = 0 is the stride-1 kernel, textually what it was.
template <int TC, bool RAG, bool SPLIT = false>
__global__ __launch_bounds__(WN_THREADS) void k_wino_conv(WinoArgs a) {
  constexpr int STR = 0;
#include "wino_conv_body.h"
}
// the pixel-pair form of a stride-(1,2) layer: STR = 1 forward, 2 input gradient (images that divide into tile groups, one channel range).
// The body is included, not called: as an inlined device function it compiles to different code than as the kernel's own text.
template <int TC, int STR>
__global__ __launch_bounds__(WN_THREADS) void k_wino_conv_strided(WinoArgs a) {
  constexpr bool RAG = false, SPLIT = false;
#include "wino_conv_body.h"
}

// The same transform for up to DL_WINO_BATCH layers in ONE launch (the 13 stride-1 layers of the trunk took 13 launches of
// 4-24 us, most of it launch latency and the ramp of a small grid): the layer table travels in the kernel arguments.
struct WinoBatchArgs {
  const float* w[DL_WINO_BATCH];
  float* u_fwd[DL_WINO_BATCH];
  float* u_bwd[DL_WINO_BATCH];
  int K[DL_WINO_BATCH], C[DL_WINO_BATCH];
  int first_block[DL_WINO_BATCH + 1];          // prefix sums of the layers' block counts
  int n;
};
// A workgroup transforms 8 output channels x 32 input channels (K, C multiples of 64).  One thread per (k, c) as in k_wino_weights, but
// the results go through LDS so that the stores are contiguous runs: u_bwd [K/8][16][C][8] receives, per plane, the 32 c x 8 k of the
// block as ONE 1 KiB run (a thread per (k, c) writes it as 4-byte elements 32 bytes apart: 0.118 ms per step for 216 MB), u_fwd
// [C/8][16][K][8] four runs of 256 bytes.  (Round 5: the transform runs once per optimiser step whatever the batch size -- 5 % of the
// reference's default batch-1 step.)
__global__ __launch_bounds__(256) void k_wino_weights_batch(WinoBatchArgs a) {
  __shared__ float stage[16 * 256];
  const int l = dl_table_slot<DL_WINO_BATCH>(a.first_block, a.n, (int)blockIdx.x);
  const int K = a.K[l], C = a.C[l];
  const int blk = (int)blockIdx.x - a.first_block[l];
  const int cblocks = C / 32;
  const int k0 = (blk / cblocks) * 8, c0 = (blk % cblocks) * 32;
  if (k0 >= K) return;                                       // (uniform per block)
  const float* __restrict__ w = a.w[l];
  float* __restrict__ u_fwd = a.u_fwd[l];
  float* __restrict__ u_bwd = a.u_bwd[l];
  const int t = threadIdx.x, kk = t >> 5, cc = t & 31;
  const int k = k0 + kk, c = c0 + cc;
  float g[3][3], gf[3][3], u[4][4];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int s2 = 0; s2 < 3; ++s2) {
      g[r][s2] = w[((size_t)(k * 3 + r) * 3 + s2) * C + c];
      gf[2 - r][2 - s2] = g[r][s2];
    }
  if (u_fwd) {
    wn_weight_transform(g, u);
    // stage[xi][c / 8][k][c % 8] = the block's share of plane xi in u_fwd's own order: 4 runs (c / 8) of 64 floats -- 8 consecutive rows
    // of one block of 64 (k0 is a multiple of 8: the rows share bit 3, i.e. the swap of their 16-byte halves)
    const int ef = (((cc >> 2) & 1) ^ ((k0 >> 3) & 1)) * 4 + (cc & 3);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) stage[xi * 256 + ((cc >> 3) * 8 + kk) * 8 + ef] = u[xi / 4][xi % 4];
    __syncthreads();
    const int cg = t >> 6, rest = t & 63;
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
      u_fwd[wn_u_row(K, c0 / 8 + cg, xi, k0) + rest] = stage[xi * 256 + t];
    __syncthreads();
  }
  if (u_bwd) {
    wn_weight_transform(gf, u);
    // stage[xi][c][k % 8]: one run of 256 floats per plane (32 consecutive rows of one block of 64)
    const int eb = (((kk >> 2) & 1) ^ (((c0 + cc) >> 3) & 1)) * 4 + (kk & 3);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) stage[xi * 256 + cc * 8 + eb] = u[xi / 4][xi % 4];
    __syncthreads();
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
      u_bwd[wn_u_row(C, k0 / 8, xi, c0) + t] = stage[xi * 256 + t];
  }
}

/* see include/delora_hip.h */
extern "C" int dl_wino_weights_batch_f32(const dl_wino_layer* layers, int32_t n, dl_stream stream) {
  if (!layers || n <= 0 || n > DL_WINO_BATCH) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_weights_batch_f32: 1..%d layers per call", DL_WINO_BATCH);
  WinoBatchArgs a{};
  a.n = n;
  int blocks = 0;
  bool tiles = true;                                   // every layer divides into the batched kernel's 8 k x 32 c blocks
  for (int i = 0; i < n; ++i) {
    const dl_wino_layer& L = layers[i];
    if (!L.w || (!L.u_fwd && !L.u_bwd) || L.K <= 0 || L.C <= 0 || L.K % 8 || L.C % 8)
      return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_weights_batch_f32: bad layer %d (K, C multiples of 8)", i);
    a.w[i] = L.w; a.u_fwd[i] = L.u_fwd; a.u_bwd[i] = L.u_bwd; a.K[i] = L.K; a.C[i] = L.C;
    a.first_block[i] = blocks;
    blocks += (L.K / 8) * ((L.C + 31) / 32);
    tiles = tiles && L.C % 64 == 0 && L.K % 64 == 0;
  }
  a.first_block[n] = blocks;
  if (tiles) hipLaunchKernelGGL(k_wino_weights_batch, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  else                                                 // (no layer of the trunk: channel counts that are not multiples of 64 -- one plain launch per layer)
    for (int i = 0; i < n; ++i)
      hipLaunchKernelGGL(k_wino_weights, dim3((layers[i].K * layers[i].C + 255) / 256), dim3(256), 0, (hipStream_t)stream, layers[i].w,
                         layers[i].u_fwd, layers[i].u_bwd, layers[i].K, layers[i].C);
  return dl_check_launch("dl_wino_weights_batch_f32");
}

extern "C" size_t dl_wino_weights_floats(int32_t K, int32_t C) { return (size_t)16 * K * C; }

extern "C" int dl_wino_weights_f32(const float* w, float* u_fwd, float* u_bwd, int32_t K, int32_t C, dl_stream stream) {
  if (!w || (!u_fwd && !u_bwd) || K <= 0 || C <= 0 || K % 8 || C % 8)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_weights_f32: bad argument (K, C multiples of 8)");
  hipLaunchKernelGGL(k_wino_weights, dim3((K * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, u_fwd, u_bwd, K, C);
  return dl_check_launch("dl_wino_weights_f32");
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradient of a stride-1 3x3 layer in the Winograd domain:
//   dw_tile = G^T [ (A g A^T) .* (B^T d B) ] G        g: 2x2 tile of the output gradient, d: the 4x4 input patch around it
//   dU[xi][k][c] += Gh[xi][tile][k] * Dh[xi][tile][c]   (16 products per tile and (k,c) pair instead of 36)
// Workgroup = 512 threads, output block 64 k x 64 c x 16 planes (the accumulator layout of k_wino_conv), reduction index =
// tiles, 8 consecutive tiles of one tile row per chunk; a workgroup walks a slab of chunks and writes one partial
// [16][K][C] block; k_wino_wgrad_sum adds the slabs in a fixed order (deterministic), k_wino_wgrad_out applies G^T . G.
// Per chunk every thread produces, for ONE channel and FOUR tiles, one column of B^T d B (from the raw patch that the LDS
// DMA brought in) and one column of A g A^T (16 scalar loads of g, coalesced over the 64 channels of a wave), written as
// 16-byte rows [xi][channel][4 tiles]: lane (i, half) reads tiles 4 half .. 4 half+3 of its row, MFMA j reduces over tiles
// {j, 4 + j}.  Addressing validated by tools/exp/wino_wgrad_emulate.py; tools/exp/wino_wgrad.hip is the stand-alone check.
// Measured (B=8, slab sum and G^T . G kernels included): layer2 259 us (direct kernel 335), layer3 463 (607), layer4 464 (608); 64-channel layers stay direct.
#define WW_THREADS 512
// ablation switches of the tuning builds (see WN_ABL): bit 0 no DMA in the chunk loop, 1 no transforms, 2 no barriers, 3 no fragment reads
#ifndef WW_ABL
#define WW_ABL 0
#endif
#if WW_ABL & 1
#define WW_IF_DMA(...)
#else
#define WW_IF_DMA(...) __VA_ARGS__
#endif
#if WW_ABL & 2
#define WW_IF_T(...)
#else
#define WW_IF_T(...) __VA_ARGS__
#endif
#if WW_ABL & 4
#define WW_IF_BAR(...)
#else
#define WW_IF_BAR(...) __VA_ARGS__
#endif
#if WW_ABL & 8
#define WW_IF_FR(...)
#else
#define WW_IF_FR(...) __VA_ARGS__
#endif
#define WW_PLANE 528                     // floats per plane: 64 rows x 8 tiles + 16 of padding
#define WW_BUF (2 * 16 * WW_PLANE)       // one (Gh, Dh) pair
#define WW_RAWPIX 72                     // raw input patch of a chunk: 4 rows x 18 columns (8 tiles), 64 channels each
#define WW_RAW (WW_RAWPIX * 64)          // floats
#define WW_GRAW (2 * 16 * 64)            // floats: the 2 x 16 output-gradient pixels of a chunk, 64 channels each

struct WWArgs {
  const float* x;    // [N][H][W][C]
  const float* g;    // [N][H][W][K]
  float* ws;         // [nslabs][16][K][C]
  int N, H, W, C, K, chunks_per_slab, nslabs;
};

// Pipeline (round 3; the first version ran the transforms in a phase of their own between two barriers while the matrix pipe
// idled: 557 us on layer3, this one 463): the transforms of chunk ch+1 are sliced into small pieces placed behind the individual
// MFMAs of chunk ch (as k_wino_conv does), branch-free, with the LDS reads of a piece issued one slot ahead of their use.
// Per iteration:
//   planes 0..2   || the raw input patch and the output-gradient patch of chunk ch+1 (both landed by DMA during the previous
//                    iteration) are read and turned into the thread's columns of Dh(ch+1) = B^T d B and Gh(ch+1) = A g A^T
//   barrier M     every thread has read the raw patches
//   planes 3..6   || DMA of the patches of chunk ch+2; Dh(ch+1), Gh(ch+1) -> buf[nxt]
//   wait + barrier E, then plane 7 || first fragments of chunk ch+1
// Chunk indices beyond the slab are clamped (a harmless repeat of the last chunk: no branch in the loop body).
// RAG: odd image sizes / tile rows that do not divide into chunks of 8 tiles -- the last chunk of a tile row hangs over the edge: the
// output-gradient values of pixels outside the image are zeroed in the transform (their tiles then contribute nothing, whatever the
// wrapped input patch holds), and an odd height masks the input row below the image as well.
template <bool RAG>
__device__ __forceinline__ void wino_wgrad_body(const WWArgs& a, const int blk) {
  static_assert((2 * WW_BUF + WW_RAW + WW_GRAW) * 4 <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) float lds[2 * WW_BUF + WW_RAW + WW_GRAW];
  float* raw = lds + 2 * WW_BUF;
  float* graw = raw + WW_RAW;                    // output-gradient patch of a chunk: [2 rows][16 pixels][64 k]
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, half = lane >> 5;
  const int mb = wave & 1, nb = (wave >> 1) & 1, xh = wave >> 2;
  const int CT = a.C / 64;
  int t = blk;
  const int slab = t % a.nslabs; t /= a.nslabs;
  const int ct = t % CT;
  const int kt = t / CT;
  const int k0 = kt * 64, c0 = ct * 64;
  const int th = RAG ? (a.H + 1) / 2 : a.H / 2, tw8 = RAG ? ((a.W + 1) / 2 + 7) / 8 : (a.W / 2) / 8;
  const int total_chunks = a.N * th * tw8;
  const int ch_begin = slab * a.chunks_per_slab;
  const int ch_end = min(ch_begin + a.chunks_per_slab, total_chunks);
  if (ch_begin >= ch_end) return;                                                   // (never: every slab holds a chunk)

  // transform role: channel r of the block (c for Dh, k for Gh), tile quad tq, column bcol of the 4x4 domain (wave-uniform tq, bcol)
  const int r = lane, tq = wave & 1, bcol = wave >> 1;
  const int j0 = bcol == 0 ? 0 : 1, j1 = bcol == 3 ? 3 : 2;                       // (d B)[.][bcol] = sg0 d[.][j0] + sg1 d[.][j1]
  const float sg0 = bcol == 2 ? -1.f : 1.f, sg1 = (bcol == 0 || bcol == 3) ? -1.f : 1.f;
  const int w_off = r * 8 + ((tq ^ ((r >> 3) & 1)) * 4);                           // 16-byte slot of (row r, tiles 4tq..4tq+3)

  auto chunk_pos = [&](int ch, int& n, int& ta, int& b8) {
    int u = ch;
    b8 = u % tw8; u /= tw8;
    ta = u % th;
    n = u / th;
  };
  // chunk-invariant lane roles of the three DMA pieces of this wave (pixel (pi, pj) of the 4 x 18 patch, 16-byte channel quad)
  int dma_pi[3], dma_pj[3], dma_l[3];
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const int piece = min(wave + 8 * it, WW_RAWPIX / 4 - 1);
    const int pix = piece * 4 + (lane >> 4);
    dma_pi[it] = pix / 18; dma_pj[it] = pix % 18;
    dma_l[it] = piece * 256;
  }
  const int x_lane = c0 + (lane & 15) * 4;
  // (LDS DMA from inline assembly, as in k_wino_conv: wave-uniform 64-bit base of the sample + per-lane 32-bit byte offset; the waits
  // that hand the patches over are the explicit s_waitcnt vmcnt(0) in front of barrier E and in the prologue)
  const unsigned ww_lds_base = (unsigned)(__SIZE_TYPE__)((__attribute__((address_space(3))) char*)lds);
#define WW2_GLDS(BASE, OFFB, LOFF_FLOATS)                                                                                 \
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"                                           \
               :: "v"(OFFB), "s"(BASE), "s"(__builtin_amdgcn_readfirstlane((int)(ww_lds_base + 4u * (unsigned)(LOFF_FLOATS)))) : "memory");
#define WW2_DMA(CH)                                                                                                       \
  {                                                                                                                       \
    int n_, ta_, b8_;                                                                                                     \
    chunk_pos((CH), n_, ta_, b8_);                                                                                        \
    const float* xn_ = a.x + ((size_t)n_ * a.H * a.W) * a.C;                                                              \
    _Pragma("unroll") for (int it = 0; it < 3; ++it) {                                                                    \
      int row = 2 * ta_ - 1 + dma_pi[it];                                                                                 \
      row = row < 0 ? 0 : (row >= a.H ? a.H - 1 : row);                                                                   \
      int col = 16 * b8_ - 1 + dma_pj[it];                                                                                \
      if (RAG) { col %= a.W; col = col < 0 ? col + a.W : col; }                                                           \
      else col = col < 0 ? col + a.W : (col >= a.W ? col - a.W : col);                                                    \
      WW2_GLDS(xn_, 4u * (unsigned)((row * a.W + col) * a.C + x_lane), (int)(raw - lds) + dma_l[it])                      \
    }                                                                                                                     \
    /* the output-gradient patch: wave w brings pixels 4w .. 4w+3 of the 2 x 16 (one 1 KiB piece; lane = pixel, channel quad) */ \
    /* (pixels outside the image: a clamped, valid address -- the transform zeroes them) */                              \
    const int grow_ = RAG ? min(2 * ta_ + g_p, a.H - 1) : 2 * ta_ + g_p, gcol_ = RAG ? min(16 * b8_ + g_px, a.W - 1) : 16 * b8_ + g_px; \
    const float* gn_ = a.g + ((size_t)n_ * a.H * a.W) * a.K;                                                              \
    WW2_GLDS(gn_, 4u * (unsigned)((grow_ * a.W + gcol_) * a.K + k0 + (lane & 15) * 4), (int)(graw - lds) + wave * 256)    \
  }
  // the four gradient values of tile E of this thread's four: g[p][2 (4 tq + E) + q][k = r], two LDS reads of two rows each
  const int g_p = (wave * 4 + (lane >> 4)) >> 4, g_px = (wave * 4 + (lane >> 4)) & 15;     // DMA role: pixel of the 2 x 16 patch
  const float* gb = graw + (8 * tq) * 64 + r;
#define WW2_TGL(E)                                                                                                        \
  {                                                                                                                       \
    _Pragma("unroll") for (int q = 0; q < 2; ++q)                                                                         \
      _Pragma("unroll") for (int p = 0; p < 2; ++p) gq[E][p][q] = gb[(p * 16 + 2 * (E) + q) * 64];                        \
  }
  // Dh = B^T d B, column bcol, tile E of this thread's four: 8 LDS reads of the raw patch (issued one slot ahead of their use),
  // rows outside the image masked
  const float* rb0 = raw + (2 * 4 * tq + j0) * 64 + r;
  const float* rb1 = raw + (2 * 4 * tq + j1) * 64 + r;
#define WW2_TDL(E)                                                                                                        \
  {                                                                                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                       \
      dd[E][2 * i] = rb0[(i * 18 + 2 * (E)) * 64];                                                                        \
      dd[E][2 * i + 1] = rb1[(i * 18 + 2 * (E)) * 64];                                                                    \
    }                                                                                                                     \
  }
#define WW2_TD(E)                                                                                                         \
  {                                                                                                                       \
    float tt_[4];                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                       \
      const unsigned m_ = i == 0 ? mask_top : (i == 3 ? mask_bot : (i == 2 ? mask_r2 : 0xffffffffu));                     \
      const float d0 = __uint_as_float(__float_as_uint(dd[E][2 * i]) & m_);                                               \
      const float d1 = __uint_as_float(__float_as_uint(dd[E][2 * i + 1]) & m_);                                           \
      tt_[i] = sg0 * d0 + sg1 * d1;                                                                                       \
    }                                                                                                                     \
    vv[0][E] = tt_[0] - tt_[2]; vv[1][E] = tt_[1] + tt_[2]; vv[2][E] = tt_[2] - tt_[1]; vv[3][E] = tt_[1] - tt_[3];       \
  }
#define WW2_WRITE(BASE, V) { _Pragma("unroll") for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4*>((BASE) + (i * 4 + bcol) * WW_PLANE) = V[i]; }
  // Gh = A g A^T, column bcol, tile E:  (g A^T)[p][bcol] = ca g[p][0] + cb g[p][1]  (branch-free: wave-uniform coefficients), then A .
  const float ca = bcol == 3 ? 0.f : 1.f, cb = bcol == 0 ? 0.f : (bcol == 1 ? 1.f : -1.f);
#define WW2_TG(E)                                                                                                         \
  {                                                                                                                       \
    if (RAG) {                                   /* zero the gradient of pixels outside the image (wave-uniform conditions) */ \
      const bool c0_ = (gmask >> (2 * (E))) & 1u, c1_ = (gmask >> (2 * (E) + 1)) & 1u, r1_ = mask_r2 != 0u;               \
      gq[E][0][0] = c0_ ? gq[E][0][0] : 0.f; gq[E][0][1] = c1_ ? gq[E][0][1] : 0.f;                                       \
      gq[E][1][0] = (c0_ && r1_) ? gq[E][1][0] : 0.f; gq[E][1][1] = (c1_ && r1_) ? gq[E][1][1] : 0.f;                     \
    }                                                                                                                     \
    const float h0_ = ca * gq[E][0][0] + cb * gq[E][0][1], h1_ = ca * gq[E][1][0] + cb * gq[E][1][1];                     \
    vg[0][E] = h0_; vg[1][E] = h0_ + h1_; vg[2][E] = h0_ - h1_; vg[3][E] = -h1_;                                          \
  }

  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
  const int arow = mb * 32 + li, brow = nb * 32 + li;
  const int a_off = arow * 8 + ((half ^ ((arow >> 3) & 1)) * 4);
  const int b_off = 16 * WW_PLANE + brow * 8 + ((half ^ ((brow >> 3) & 1)) * 4);
  f32x4 vv[4], vg[4];
  float dd[4][8], gq[4][2][2];
  unsigned mask_top, mask_bot, mask_r2 = 0xffffffffu, gmask = 0xffu;
  // rows 2ta-1 .. 2ta+2 of the input patch: the first may lie above the image, the last (and, for an odd height, the third) below it;
  // gmask bit 2E+q: column 16 b8 + 2 (4 tq + E) + q of the output gradient lies inside the image
#define WW2_MASKS(CH)                                                                                                     \
  {                                                                                                                       \
    int n_, ta_, b8_;                                                                                                     \
    chunk_pos((CH), n_, ta_, b8_);                                                                                        \
    mask_top = ta_ > 0 ? 0xffffffffu : 0u;                                                                                \
    mask_bot = 2 * ta_ + 2 < a.H ? 0xffffffffu : 0u;                                                                      \
    if (RAG) {                                                                                                            \
      mask_r2 = 2 * ta_ + 1 < a.H ? 0xffffffffu : 0u;                                                                     \
      gmask = 0u;                                                                                                         \
      _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) gmask |= (16 * b8_ + 8 * tq + e_ < a.W) ? (1u << e_) : 0u;         \
    }                                                                                                                     \
  }

  // prologue: operands of the first chunk, then the raw patch / gradient values of the second
  WW2_DMA(ch_begin)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  WW2_MASKS(ch_begin)
  WW2_TDL(0) WW2_TD(0) WW2_TDL(1) WW2_TD(1) WW2_TDL(2) WW2_TD(2) WW2_TDL(3) WW2_TD(3)
  WW2_WRITE(lds + 16 * WW_PLANE + w_off, vv)
  WW2_TGL(0) WW2_TG(0) WW2_TGL(1) WW2_TG(1) WW2_TGL(2) WW2_TG(2) WW2_TGL(3) WW2_TG(3)
  WW2_WRITE(lds + w_off, vg)
  __syncthreads();
  {
    const int c1 = min(ch_begin + 1, ch_end - 1);
    WW2_DMA(c1)
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

#define WW2_FR_FROM(XL, BP)                                                                                               \
  {                                                                                                                       \
    av[(XL) & 1] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WW_PLANE + a_off);                            \
    bv[(XL) & 1] = *reinterpret_cast<const f32x4*>((BP) + (xh * 8 + (XL)) * WW_PLANE + b_off);                            \
  }
#define WW2_FR(XL) WW2_FR_FROM(XL, cur)
#define WW2_M(XL, J, ...)                                                                                                 \
  {                                                                                                                       \
    acc[XL] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[(XL) & 1][J], bv[(XL) & 1][J], acc[XL], 0, 0, 0);                   \
    asm volatile("" : "+v"(acc[XL]) :: "memory");          /* pins the MFMA in front of its slice ... */                     \
    __builtin_amdgcn_sched_barrier(0);                     /* ... and the slice's arithmetic behind it */                    \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }
  f32x4 av[2], bv[2];
  {
    const float* cur = lds;
    WW2_FR(0)
  }
  // Barrier M sits right behind the last read of the raw patch (the gradient registers are private and need no barrier), so the DMA
  // of chunk ch+2 has two thirds of the iteration to land; barrier E sits in front of the LAST plane, whose fragments every wave
  // already holds: its four MFMAs run behind the barrier and cover the fetch of the next chunk's first fragments.
  for (int ch = ch_begin; ch < ch_end; ++ch) {
    const float* cur = lds + ((ch - ch_begin) & 1) * WW_BUF;
    float* nxt = lds + ((ch - ch_begin + 1) & 1) * WW_BUF;
    const int c1 = min(ch + 1, ch_end - 1), c2 = min(ch + 2, ch_end - 1);
    WW2_MASKS(c1)
    // LDS reads in the first two slices of a plane, arithmetic two slices later: the compiler guards the first use of an LDS result
    // with a wait for ALL outstanding LDS operations, and with this layout everything it waits for is at least two slices old
    WW2_M(0, 0, WW_IF_FR(WW2_FR(1)) WW_IF_T(WW2_TDL(0) WW2_TDL(1))) WW2_M(0, 1, WW_IF_T(WW2_TGL(0) WW2_TGL(1))) WW2_M(0, 2, ) WW2_M(0, 3, WW_IF_T(WW2_TD(0) WW2_TG(0)))
    WW2_M(1, 0, WW_IF_FR(WW2_FR(2)) WW_IF_T(WW2_TDL(2) WW2_TDL(3))) WW2_M(1, 1, WW_IF_T(WW2_TGL(2) WW2_TGL(3))) WW2_M(1, 2, WW_IF_T(WW2_TD(1) WW2_TG(1))) WW2_M(1, 3, WW_IF_T(WW2_TD(2) WW2_TG(2)))
    WW2_M(2, 0, WW_IF_FR(WW2_FR(3))) WW2_M(2, 1, ) WW2_M(2, 2, WW_IF_T(WW2_TD(3) WW2_TG(3))) WW2_M(2, 3, )
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    WW_IF_BAR(__builtin_amdgcn_s_barrier();)                                         // M: the raw patches have been read by everybody
    __builtin_amdgcn_sched_barrier(0);
    WW2_M(3, 0, WW_IF_FR(WW2_FR(4)) WW_IF_DMA(WW2_DMA(c2))) WW2_M(3, 1, WW_IF_T(WW2_WRITE(nxt + 16 * WW_PLANE + w_off, vv))) WW2_M(3, 2, WW_IF_T(WW2_WRITE(nxt + w_off, vg))) WW2_M(3, 3, )
    WW2_M(4, 0, WW_IF_FR(WW2_FR(5))) WW2_M(4, 1, ) WW2_M(4, 2, ) WW2_M(4, 3, )
    WW2_M(5, 0, WW_IF_FR(WW2_FR(6))) WW2_M(5, 1, ) WW2_M(5, 2, ) WW2_M(5, 3, )
    WW2_M(6, 0, WW_IF_FR(WW2_FR(7))) WW2_M(6, 1, ) WW2_M(6, 2, ) WW2_M(6, 3, )
#if WW_ABL & 16
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
#endif
    WW_IF_BAR(__builtin_amdgcn_s_barrier();)                                         // E: operands of chunk ch+1 visible, raw patch landed
    __builtin_amdgcn_sched_barrier(0);
    WW2_M(7, 0, WW_IF_FR(WW2_FR_FROM(0, nxt))) WW2_M(7, 1, ) WW2_M(7, 2, ) WW2_M(7, 3, )
  }
#undef WW2_DMA
#undef WW2_GLDS
#undef WW2_TGL
#undef WW2_TD
#undef WW2_TDL
#undef WW2_TG
#undef WW2_WRITE
#undef WW2_MASKS
#undef WW2_FR
#undef WW2_FR_FROM
#undef WW2_M
  // partial of this slab: ws[slab][xi][k0 + m][c0 + n]; accumulator register q of lane (li, half) is
  // row m = mb*32 + 8*(q/4) + 4*half + q%4, column n = nb*32 + li
  float* wp = a.ws + ((size_t)slab * 16) * a.K * a.C;
#pragma unroll
  for (int xl = 0; xl < 8; ++xl) {
    const int xi = xh * 8 + xl;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = mb * 32 + 8 * (q / 4) + 4 * half + (q % 4);
      wp[((size_t)xi * a.K + k0 + m) * a.C + c0 + nb * 32 + li] = acc[xl][q];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 6: the chunk loop for images that divide into chunks (RAG = false: every BASELINE shape).  What changed and why
// (tools/exp/mfma_overlap.hip, profiles/r06_mfma_shadow.txt): v_mfma_f32_32x32x2_f32 runs at the fp32 VECTOR rate because it shares the
// SIMD's vector issue -- a VALU instruction next to it is not hidden in its shadow, it costs the SIMD 3.3 cycles of matrix time with two
// waves per SIMD (packed fp32: 5.3, v_readfirstlane: 6, an LDS read: 1.1-1.4, a scalar instruction: ~0.5).  The round-3 body spent 171
// VALU instructions per wave and chunk on the two transforms (22 % of the kernel by ablation): every thread formed ONE column of
// B^T d B / A g A^T for four tiles from scalar LDS reads, with multiplications by +-1 / 0 to stay branch-free.  Here:
//   * thread = (channel, tile pair) and forms ALL sixteen Winograd-domain values of its two tiles: waves 0-3 the input patches (24 LDS
//     reads, 32 packed adds), waves 4-7 the output-gradient tiles (8 reads, 20 packed operations) -- a SIMD hosts one wave of each kind.
//     Both row stages run on (row, row + 1) register pairs; the half selectors and sign modifiers of the packed instructions do what
//     the multiplications did (inline assembly; tools/exp/pk_probe.hip checks the modifier semantics on the hardware);
//   * operand layout [plane pair (a >> 1, b)][row][tile][a & 1]: a thread's results are 16-byte rows (two tiles x two planes), and one
//     16-byte fragment read still feeds four MFMAs -- two for each plane of the pair, both owned by the reading wave;
//   * rows above / below the image are zeroed under a chunk-uniform branch instead of masking every value of every chunk;
//   * the chunk's position in the image advances incrementally in scalar registers (no division); every DMA piece is 4 pixels x 64
//     channels of ONE image row with a chunk-invariant per-lane offset and a scalar base, and the pieces of a wave share one M0 write:
//     the instruction's immediate offset moves the LDS address and the global address together (pk_probe.hip), the base compensates.
#define W3_PLANE 1024                    // floats of one plane pair: 64 rows x (8 tiles x 2 planes)
#define W3_OPER (8 * W3_PLANE)           // one operand: 8 plane pairs
#define W3_BUF (2 * W3_OPER)             // (Gh, Dh)
#define W3_RAWROW (20 * 64)              // floats of one input-patch row: 5 DMA pieces of 4 pixels x 64 channels (18 pixels used)
#define W3_RAW (4 * W3_RAWROW)
#define W3_GRAW (2 * 16 * 64)

// (x.lo - y.lo, x.hi + y.lo) and (y.lo - x.hi, x.hi - y.hi): the second row stage of B^T . on the row pairs x = (T0, T1), y = (T2, T3)
__device__ __forceinline__ f32x2 w3_v01(f32x2 x, f32x2 y) {
  f32x2 r;
  asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,0]" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
__device__ __forceinline__ f32x2 w3_v23(f32x2 x, f32x2 y) {
  f32x2 r;
  asm volatile("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[1,0] neg_hi:[0,1]" : "=v"(r) : "v"(x), "v"(y));
  return r;
}
// A . on the row pair h = (h0, h1): (h0, h0 + h1) and (h0 - h1, -h1); NEG: the same for -h.  c01 = (0, 1), c10 = (1, 0): a product
// with 1 is exact and the sum is rounded once, so the results are those of the plain additions.
template <bool NEG> __device__ __forceinline__ f32x2 w3_g01(f32x2 h, f32x2 c01) {
  f32x2 r;
  if (NEG) asm volatile("v_pk_fma_f32 %0, %1, %2, %1 op_sel:[1,0,0] op_sel_hi:[1,1,0] neg_lo:[1,0,1] neg_hi:[1,0,1]" : "=v"(r) : "v"(h), "s"(c01));
  else asm volatile("v_pk_fma_f32 %0, %1, %2, %1 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(r) : "v"(h), "s"(c01));
  return r;
}
template <bool NEG> __device__ __forceinline__ f32x2 w3_g23(f32x2 h, f32x2 c10) {
  f32x2 r;
  if (NEG) asm volatile("v_pk_fma_f32 %0, %1, %2, %1 op_sel:[0,0,1] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]" : "=v"(r) : "v"(h), "s"(c10));
  else asm volatile("v_pk_fma_f32 %0, %1, %2, %1 op_sel:[0,0,1] op_sel_hi:[0,1,1] neg_lo:[0,0,1] neg_hi:[0,0,1]" : "=v"(r) : "v"(h), "s"(c10));
  return r;
}

struct W3Pos { int n, ta, b8; };

// LIVE: the xi-columns b of the 4x4 domain that are computed (bit b).  0xF is the stride-1 layer.  The pixel-pair view of a stride-(1,2)
// layer (x read as [N][H][W/2][2C]) has no tap in its third column, and its even-pixel channels have a tap in the
// middle column only: dW = G^T dU G with the last row of G = (0, 0, 1) needs b in {0,1,2} (0x7) for the odd-pixel channel blocks and
// b in {1,2} (0x6) for the even-pixel ones.  A dead column has no half planes (8 MFMAs per wave and chunk), no accumulators, no transform
// pieces on either operand side and no store; the side work and the two barriers are re-placed over the half planes that remain.
// a.C is then the pair view's 2C; the block's planes go to ws[slab][a][live b][K][C] of the block's own kind (a.ws, see k_wino_swgrad_batch).
static_assert((2 * W3_BUF + W3_RAW + W3_GRAW) * 4 <= 163840, "LDS budget");
__shared__ __attribute__((aligned(16))) float w3_lds[2 * W3_BUF + W3_RAW + W3_GRAW];      // one array for every column set a kernel instantiates
template <int LIVE, bool UPPER = LIVE == 0x7>
__device__ __forceinline__ void wino_wgrad_body3_live(const WWArgs& a, const int blk) {
  static_assert(LIVE == 0xF || LIVE == 0x7 || LIVE == 0x6, "column sets with a schedule");
  float* const lds = w3_lds;
  float* raw = lds + 2 * W3_BUF;
  float* graw = raw + W3_RAW;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, half = lane >> 5;
  const int mb = wave & 1, nb = (wave >> 1) & 1, xh = wave >> 2;
  const int CT = LIVE == 0xF ? a.C / 64 : a.C / 128;                                 // the 64-channel blocks of the launch / of one pixel phase
  int t = blk;
  const int slab = t % a.nslabs; t /= a.nslabs;
  const int ct = t % CT;
  const int kt = t / CT;
  const int k0 = kt * 64, c0 = ct * 64 + (UPPER ? a.C / 2 : 0);                      // (the odd pixels' channels are the pair's upper half)
  const int th = a.H / 2, tw8 = (a.W / 2) / 8;
  const int total_chunks = a.N * th * tw8;
  const int ch_begin = slab * a.chunks_per_slab;
  const int ch_end = min(ch_begin + a.chunks_per_slab, total_chunks);
  if (ch_begin >= ch_end) return;                                                   // (never: every slab holds a chunk)

  // ---- transform role: waves 0-3 form Dh = B^T d B (rows = input channels), waves 4-7 Gh = A g A^T (rows = output channels); lane = row
  // of the block, tp = tile pair (tiles 2 tp, 2 tp + 1 of the chunk's eight)
  const unsigned lds_base = (unsigned)(__SIZE_TYPE__)((__attribute__((address_space(3))) char*)lds);
  const int tp = wave & 3;
  // 16-byte slot of (row, tile pair) inside the row's 64 bytes, XOR-swizzled: f(row) = (bit 2, bit 1 ^ bit 3) makes the 16-byte fragment reads
  // (16-lane groups of rows {0-3, 12-15, 20-27}, 64 banks) AND these 16-byte stores (8 consecutive rows, 32 banks) conflict-free
#define W3_SWZ(R) ((((R) >> 2) & 1) | (((((R) >> 1) ^ ((R) >> 3)) & 1) << 1))
  const int w_off = lane * 16 + ((tp ^ W3_SWZ(lane)) * 4);
  const float* rsrc = (xh == 0 ? raw : graw) + (4 * tp) * 64 + lane;
  // ---- DMA role: wave w brings pieces of patch row w >> 1 (even waves: pixels 0-11, odd waves: 12-19) and pixels 4 (w & 3) .. of row w >> 2
  // of the output-gradient patch.  Per-lane byte offsets (pixel lane >> 4 of the piece, 16-byte channel quad lane & 15):
  const unsigned voff_x = (unsigned)((lane >> 4) * a.C * 4 + (lane & 15) * 16);
  const unsigned voff_g = (unsigned)((lane >> 4) * a.K * 4 + (lane & 15) * 16);
  // first piece of the first chunk of an image row: pixel 0 is column W - 1 (wrap-around), pixels 1-3 columns 0-2, relative to the row's start;
  // last piece of the last chunk: pixel 0 is column W - 1, pixel 1 column 0 (pixels 2, 3 are not used: column 0 again)
  const unsigned voff_l = (unsigned)(((lane >> 4) == 0 ? a.W - 1 : (lane >> 4) - 1) * a.C * 4 + (lane & 15) * 16);
  const unsigned voff_r = (unsigned)(((lane >> 4) == 0 ? a.W - 1 : 0) * a.C * 4 + (lane & 15) * 16);
  const int d_row = wave >> 1, d_odd = wave & 1;
  const int m0_raw = __builtin_amdgcn_readfirstlane((int)(lds_base + 4u * (unsigned)((int)(raw - lds) + d_row * W3_RAWROW + d_odd * 3 * 256)));
  const int m0_g = __builtin_amdgcn_readfirstlane((int)(lds_base + 4u * (unsigned)((int)(graw - lds) + wave * 256)));
  // (LDS DMA from inline assembly, as in k_wino_conv; one M0 write per group of pieces, the pieces 1 KiB apart in LDS by the immediate
  // offset -- which moves the global address as well: piece s takes its base minus s KiB)
  auto dma = [&](const W3Pos& p) {
    int row = 2 * p.ta - 1 + d_row;
    row = row < 0 ? 0 : (row >= a.H ? a.H - 1 : row);                                       // (rows outside the image: zeroed by the transform)
    const float* xrow = a.x + ((size_t)(p.n * a.H + row) * a.W) * a.C + c0;                  // column 0 of the image row
    const float* xcol = xrow + (ptrdiff_t)(16 * p.b8 - 1 + 12 * d_odd) * a.C;                // first pixel of this wave's first piece
    const float* x1 = xcol + 4 * a.C - 256;
    if (!d_odd) {
      const float* x2 = xcol + 8 * a.C - 512;
      if (p.b8 == 0)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %3, %4 offset:1024\n\tglobal_load_lds_dwordx4 %3, %5 offset:2048"
                     :: "s"(m0_raw), "v"(voff_l), "s"(xrow), "v"(voff_x), "s"(x1), "s"(x2) : "memory");
      else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %3 offset:1024\n\tglobal_load_lds_dwordx4 %1, %4 offset:2048"
                     :: "s"(m0_raw), "v"(voff_x), "s"(xcol), "s"(x1), "s"(x2) : "memory");
    } else {
      if (p.b8 == tw8 - 1)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %3, %4 offset:1024"
                     :: "s"(m0_raw), "v"(voff_x), "s"(xcol), "v"(voff_r), "s"(xrow - 256) : "memory");
      else
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\tglobal_load_lds_dwordx4 %1, %3 offset:1024"
                     :: "s"(m0_raw), "v"(voff_x), "s"(xcol), "s"(x1) : "memory");
    }
    const float* gp = a.g + ((size_t)(p.n * a.H + 2 * p.ta + (wave >> 2)) * a.W + 16 * p.b8 + 4 * (wave & 3)) * a.K + k0;
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" :: "s"(m0_g), "v"(voff_g), "s"(gp) : "memory");
  };
  auto advance = [&](W3Pos& p) {                                                      // the next chunk in (n, tile row, block of 8 tiles) order
    if (++p.b8 == tw8) { p.b8 = 0; if (++p.ta == th) { p.ta = 0; ++p.n; } }
  };

  f32x16 acc[8];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
  // fragment reads: lane (li, half) of a plane pair reads the 16-byte slots `half` and `2 + half` of its row (tiles {2 half, 2 half + 1} and
  // {4 + 2 half, ..} x both planes): element e of a read is plane e & 1, tile (e >> 1) of the slot's two
  const int arow = mb * 32 + li, brow = nb * 32 + li;
  const int a_off0 = xh * 4 * W3_PLANE + arow * 16 + ((half ^ W3_SWZ(arow)) * 4);
  const int a_off1 = xh * 4 * W3_PLANE + arow * 16 + (((2 + half) ^ W3_SWZ(arow)) * 4);
  const int b_off0 = W3_OPER + xh * 4 * W3_PLANE + brow * 16 + ((half ^ W3_SWZ(brow)) * 4);
  const int b_off1 = W3_OPER + xh * 4 * W3_PLANE + brow * 16 + (((2 + half) ^ W3_SWZ(brow)) * 4);

  // ---- the two transforms, in pieces (placed behind individual MFMAs below)
  f32x2 P[2][6];                       // Dh: input patch, rows (2 rp, 2 rp + 1) x columns 4 tp .. 4 tp + 5;  Gh: P[0][0..3] = (g[0][px], g[1][px])
  f32x2 T[2][4], V01[2][4], V23[2][4];
  const f32x2 c01 = {0.f, 1.f}, c10 = {1.f, 0.f};
  // (row, row + 1) pairs straight from LDS: ds_read2st64_b32 takes two offsets in units of 64 floats = one pixel.  Issued from inline assembly
  // (the compiler merges plain scalar reads into NEIGHBOURING-pixel pairs and then needs a v_mov per value to re-pair them); it does not
  // count these reads, so every use is behind an explicit s_waitcnt lgkmcnt(0) (barrier M / the prologue's) -- its own counted waits only
  // become more conservative
  const unsigned rsrc_a = lds_base + 4u * (unsigned)(rsrc - lds);
#define W3_RD2(DST, O0, O1) asm volatile("ds_read2st64_b32 %0, %1 offset0:" #O0 " offset1:" #O1 : "=v"(DST) : "v"(rsrc_a) : "memory");
#define W3_DLD_0A() W3_RD2(P[0][0], 0, 20) W3_RD2(P[0][1], 1, 21) W3_RD2(P[0][2], 2, 22)
#define W3_DLD_0B() W3_RD2(P[0][3], 3, 23) W3_RD2(P[0][4], 4, 24) W3_RD2(P[0][5], 5, 25)
#define W3_DLD_1A() W3_RD2(P[1][0], 40, 60) W3_RD2(P[1][1], 41, 61) W3_RD2(P[1][2], 42, 62)
#define W3_DLD_1B() W3_RD2(P[1][3], 43, 63) W3_RD2(P[1][4], 44, 64) W3_RD2(P[1][5], 45, 65)
#define W3_DMASK()          { if (top) { _Pragma("unroll") for (int j = 0; j < 6; ++j) P[0][j][0] = 0.f; }                        \
                              if (bot) { _Pragma("unroll") for (int j = 0; j < 6; ++j) P[1][j][1] = 0.f; } }
#define W3_DT(E, RP, B)     { constexpr int o_ = 2 * (E);                                                                           \
                              T[RP][B] = (B) == 0 ? P[RP][o_] - P[RP][o_ + 2] : (B) == 1 ? P[RP][o_ + 1] + P[RP][o_ + 2]               \
                                       : (B) == 2 ? P[RP][o_ + 2] - P[RP][o_ + 1] : P[RP][o_ + 1] - P[RP][o_ + 3]; }
#define W3_DV(E, B)         { V01[E][B] = w3_v01(T[0][B], T[1][B]); V23[E][B] = w3_v23(T[0][B], T[1][B]); }
#define W3_WR(OPER, B)      { f32x4 lo_ = {V01[0][B][0], V01[0][B][1], V01[1][B][0], V01[1][B][1]};                                  \
                              f32x4 hi_ = {V23[0][B][0], V23[0][B][1], V23[1][B][0], V23[1][B][1]};                                  \
                              *reinterpret_cast<f32x4*>(nxt + (OPER) + (B) * W3_PLANE + w_off) = lo_;                                \
                              *reinterpret_cast<f32x4*>(nxt + (OPER) + (4 + (B)) * W3_PLANE + w_off) = hi_; }
#define W3_GLD()            W3_RD2(P[0][0], 0, 16) W3_RD2(P[0][1], 1, 17) W3_RD2(P[0][2], 2, 18) W3_RD2(P[0][3], 3, 19)
  // tile E of the pair: columns 2 E, 2 E + 1 of the thread's four.  h_b: b = 0: g0, 1: g0 + g1, 2: g0 - g1, 3: -g1 (as modifiers)
#define W3_GH(E)            { T[E][1] = P[0][2 * (E)] + P[0][2 * (E) + 1]; T[E][2] = P[0][2 * (E)] - P[0][2 * (E) + 1]; }
#define W3_GV(E, B)         { if ((B) == 0) { V01[E][0] = w3_g01<false>(P[0][2 * (E)], c01); V23[E][0] = w3_g23<false>(P[0][2 * (E)], c10); }              \
                              else if ((B) == 3) { V01[E][3] = w3_g01<true>(P[0][2 * (E) + 1], c01); V23[E][3] = w3_g23<true>(P[0][2 * (E) + 1], c10); } \
                              else { V01[E][B] = w3_g01<false>(T[E][B], c01); V23[E][B] = w3_g23<false>(T[E][B], c10); } }
#define W3_B(B, ...)        { if constexpr ((LIVE >> (B)) & 1) { __VA_ARGS__ } }                            // a piece of column B, if it is live
  // the patch columns the live xi-columns read: 0x7 columns 0-4, 0x6 columns 1-4 of the thread's six
#define W3_DLD7_0A() W3_RD2(P[0][0], 0, 20) W3_RD2(P[0][1], 1, 21) W3_RD2(P[0][2], 2, 22)
#define W3_DLD7_1A() W3_RD2(P[1][0], 40, 60) W3_RD2(P[1][1], 41, 61) W3_RD2(P[1][2], 42, 62)
#define W3_DLD6_0A() W3_RD2(P[0][1], 1, 21) W3_RD2(P[0][2], 2, 22)
#define W3_DLD6_1A() W3_RD2(P[1][1], 41, 61) W3_RD2(P[1][2], 42, 62)
#define W3_DLDL_0B() W3_RD2(P[0][3], 3, 23) W3_RD2(P[0][4], 4, 24)
#define W3_DLDL_1B() W3_RD2(P[1][3], 43, 63) W3_RD2(P[1][4], 44, 64)

#define W3_FR_FROM(HP, BP)                                                                                                \
  {                                                                                                                       \
    av[(HP) & 1] = *reinterpret_cast<const f32x4*>((BP) + ((HP) >> 1) * W3_PLANE + (((HP) & 1) ? a_off1 : a_off0));       \
    bv[(HP) & 1] = *reinterpret_cast<const f32x4*>((BP) + ((HP) >> 1) * W3_PLANE + (((HP) & 1) ? b_off1 : b_off0));       \
  }
#define W3_FR(HP) W3_FR_FROM(HP, cur)
  // MFMA J of half plane HP = (plane pair HP >> 1, slots HP & 1): plane J & 1 of the pair, accumulator (J & 1) * 4 + (HP >> 1)
#define W3_M(HP, J, ...)                                                                                                  \
  {                                                                                                                       \
    acc[((J) & 1) * 4 + ((HP) >> 1)] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[(HP) & 1][J], bv[(HP) & 1][J], acc[((J) & 1) * 4 + ((HP) >> 1)], 0, 0, 0); \
    asm volatile("" : "+v"(acc[((J) & 1) * 4 + ((HP) >> 1)]) :: "memory");                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    __VA_ARGS__                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
  }

  // prologue: patches of the first chunk, its operands, patches of the second chunk
  W3Pos p1;
  {
    int u = ch_begin;
    p1.b8 = u % tw8; u /= tw8;
    p1.ta = u % th;
    p1.n = u / th;
  }
  dma(p1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  {
    float* nxt = lds;
    const bool top = p1.ta == 0, bot = p1.ta == th - 1;
    if (xh == 0) {
      W3_DLD_0A() W3_DLD_0B() W3_DLD_1A() W3_DLD_1B()
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      W3_DMASK()
      W3_B(0, W3_DT(0, 0, 0)) W3_B(1, W3_DT(0, 0, 1)) W3_B(2, W3_DT(0, 0, 2)) W3_B(3, W3_DT(0, 0, 3))
      W3_B(0, W3_DT(0, 1, 0)) W3_B(1, W3_DT(0, 1, 1)) W3_B(2, W3_DT(0, 1, 2)) W3_B(3, W3_DT(0, 1, 3))
      W3_B(0, W3_DV(0, 0)) W3_B(1, W3_DV(0, 1)) W3_B(2, W3_DV(0, 2)) W3_B(3, W3_DV(0, 3))
      W3_B(0, W3_DT(1, 0, 0)) W3_B(1, W3_DT(1, 0, 1)) W3_B(2, W3_DT(1, 0, 2)) W3_B(3, W3_DT(1, 0, 3))
      W3_B(0, W3_DT(1, 1, 0)) W3_B(1, W3_DT(1, 1, 1)) W3_B(2, W3_DT(1, 1, 2)) W3_B(3, W3_DT(1, 1, 3))
      W3_B(0, W3_DV(1, 0)) W3_B(1, W3_DV(1, 1)) W3_B(2, W3_DV(1, 2)) W3_B(3, W3_DV(1, 3))
      W3_B(0, W3_WR(W3_OPER, 0)) W3_B(1, W3_WR(W3_OPER, 1)) W3_B(2, W3_WR(W3_OPER, 2)) W3_B(3, W3_WR(W3_OPER, 3))
    } else {
      W3_GLD()
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      W3_GH(0) W3_GH(1)
      W3_B(0, W3_GV(0, 0)) W3_B(1, W3_GV(0, 1)) W3_B(2, W3_GV(0, 2)) W3_B(3, W3_GV(0, 3))
      W3_B(0, W3_GV(1, 0)) W3_B(1, W3_GV(1, 1)) W3_B(2, W3_GV(1, 2)) W3_B(3, W3_GV(1, 3))
      W3_B(0, W3_WR(0, 0)) W3_B(1, W3_WR(0, 1)) W3_B(2, W3_WR(0, 2)) W3_B(3, W3_WR(0, 3))
    }
  }
  __syncthreads();
  if (ch_begin + 1 < ch_end) advance(p1);
  dma(p1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  constexpr int HP0 = LIVE & 1 ? 0 : 2;                   // the first live half plane
  f32x4 av[2], bv[2];
  {
    const float* cur = lds;
    W3_FR(HP0)
  }
  // Per iteration: half planes 0-1 multiply while every thread reads the patches of chunk ch + 1 (landed during the previous iteration);
  // barrier M (patches read); the DMA of chunk ch + 2 goes out and the transforms run, two packed instructions per MFMA, results to the
  // other buffer; barrier E in front of the LAST half plane, whose fragments every wave holds already.
#define W3_TAIL()                                                                                                         \
    W3_M(6, 0, W3_FR(7)) W3_M(6, 1, ) W3_M(6, 2, ) W3_M(6, 3, )                                                           \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                           \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    W3_M(7, 0, W3_FR_FROM(0, nxt)) W3_M(7, 1, ) W3_M(7, 2, ) W3_M(7, 3, )
#define W3_BAR_M()                                                                                                        \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                    \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);
#define W3_BAR_E()                                                                                                        \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                                           \
    __builtin_amdgcn_s_barrier();                                                                                         \
    __builtin_amdgcn_sched_barrier(0);
  // Fewer half planes: the iteration is rotated so that the DMA keeps the longest window the shorter chunk has.  The patch reads of chunk
  // ch + 1 go behind the first MFMAs of the LAST half plane (after barrier E, its other MFMAs cover their latency), barrier M opens the
  // next iteration, the DMA of chunk ch + 2 goes out behind its first MFMA and the transforms follow, at most two packed pieces per MFMA.
  if constexpr (LIVE != 0xF) {                            // the reads of the first iteration
    if (xh == 0) { if constexpr (LIVE == 0x7) { W3_DLD7_0A() W3_DLD7_1A() } else { W3_DLD6_0A() W3_DLD6_1A() } W3_DLDL_0B() W3_DLDL_1B() }
    else { W3_GLD() }
  }
  if constexpr (LIVE == 0x7) {
    // 6 half planes (24 MFMAs): barrier M, 0-4 || DMA + transforms of columns 0-2, barrier E, 5 || patch reads
    if (xh == 0) {
      for (int ch = ch_begin; ch < ch_end; ++ch) {
        const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
        float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
        const bool top = p1.ta == 0, bot = p1.ta == th - 1;
        W3Pos p2 = p1;
        if (ch + 2 < ch_end) advance(p2);
        W3_BAR_M()
        W3_M(0, 0, W3_FR(1) dma(p2);) W3_M(0, 1, W3_DMASK() W3_DT(0, 0, 0) W3_DT(0, 0, 1)) W3_M(0, 2, W3_DT(0, 0, 2) W3_DT(0, 1, 0)) W3_M(0, 3, W3_DT(0, 1, 1) W3_DT(0, 1, 2))
        W3_M(1, 0, W3_FR(2) W3_DV(0, 0)) W3_M(1, 1, W3_DV(0, 1)) W3_M(1, 2, W3_DV(0, 2)) W3_M(1, 3, W3_DT(1, 0, 0) W3_DT(1, 0, 1))
        W3_M(2, 0, W3_FR(3) W3_DT(1, 0, 2)) W3_M(2, 1, W3_DT(1, 1, 0) W3_DT(1, 1, 1)) W3_M(2, 2, W3_DT(1, 1, 2)) W3_M(2, 3, W3_DV(1, 0))
        W3_M(3, 0, W3_FR(4) W3_WR(W3_OPER, 0)) W3_M(3, 1, W3_DV(1, 1)) W3_M(3, 2, W3_WR(W3_OPER, 1)) W3_M(3, 3, W3_DV(1, 2))
        W3_M(4, 0, W3_FR(5) W3_WR(W3_OPER, 2)) W3_M(4, 1, ) W3_M(4, 2, ) W3_M(4, 3, )
        W3_BAR_E()
        W3_M(5, 0, W3_FR_FROM(0, nxt) W3_DLD7_0A() W3_DLDL_0B()) W3_M(5, 1, W3_DLD7_1A() W3_DLDL_1B()) W3_M(5, 2, ) W3_M(5, 3, )
        p1 = p2;
      }
    } else {
      for (int ch = ch_begin; ch < ch_end; ++ch) {
        const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
        float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
        W3Pos p2 = p1;
        if (ch + 2 < ch_end) advance(p2);
        W3_BAR_M()
        W3_M(0, 0, W3_FR(1) dma(p2);) W3_M(0, 1, W3_GH(0)) W3_M(0, 2, W3_GV(0, 0)) W3_M(0, 3, W3_GV(0, 1))
        W3_M(1, 0, W3_FR(2)) W3_M(1, 1, W3_GV(0, 2)) W3_M(1, 2, W3_GH(1)) W3_M(1, 3, W3_GV(1, 0))
        W3_M(2, 0, W3_FR(3) W3_WR(0, 0)) W3_M(2, 1, W3_GV(1, 1)) W3_M(2, 2, W3_WR(0, 1)) W3_M(2, 3, W3_GV(1, 2))
        W3_M(3, 0, W3_FR(4) W3_WR(0, 2)) W3_M(3, 1, ) W3_M(3, 2, ) W3_M(3, 3, )
        W3_M(4, 0, W3_FR(5)) W3_M(4, 1, ) W3_M(4, 2, ) W3_M(4, 3, )
        W3_BAR_E()
        W3_M(5, 0, W3_FR_FROM(0, nxt) W3_GLD()) W3_M(5, 1, ) W3_M(5, 2, ) W3_M(5, 3, )
        p1 = p2;
      }
    }
  } else if constexpr (LIVE == 0x6) {
    // 4 half planes (16 MFMAs): barrier M, 2-4 || DMA + transforms of columns 1-2, barrier E, 5 || patch reads
    if (xh == 0) {
      for (int ch = ch_begin; ch < ch_end; ++ch) {
        const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
        float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
        const bool top = p1.ta == 0, bot = p1.ta == th - 1;
        W3Pos p2 = p1;
        if (ch + 2 < ch_end) advance(p2);
        W3_BAR_M()
        W3_M(2, 0, W3_FR(3) dma(p2);) W3_M(2, 1, W3_DMASK() W3_DT(0, 0, 1) W3_DT(0, 0, 2)) W3_M(2, 2, W3_DT(0, 1, 1) W3_DT(0, 1, 2)) W3_M(2, 3, W3_DV(0, 1))
        W3_M(3, 0, W3_FR(4) W3_DV(0, 2)) W3_M(3, 1, W3_DT(1, 0, 1) W3_DT(1, 0, 2)) W3_M(3, 2, W3_DT(1, 1, 1) W3_DT(1, 1, 2)) W3_M(3, 3, W3_DV(1, 1))
        W3_M(4, 0, W3_FR(5) W3_WR(W3_OPER, 1)) W3_M(4, 1, W3_DV(1, 2)) W3_M(4, 2, W3_WR(W3_OPER, 2)) W3_M(4, 3, )
        W3_BAR_E()
        W3_M(5, 0, W3_FR_FROM(2, nxt) W3_DLD6_0A() W3_DLDL_0B()) W3_M(5, 1, W3_DLD6_1A() W3_DLDL_1B()) W3_M(5, 2, ) W3_M(5, 3, )
        p1 = p2;
      }
    } else {
      for (int ch = ch_begin; ch < ch_end; ++ch) {
        const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
        float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
        W3Pos p2 = p1;
        if (ch + 2 < ch_end) advance(p2);
        W3_BAR_M()
        W3_M(2, 0, W3_FR(3) dma(p2);) W3_M(2, 1, W3_GH(0)) W3_M(2, 2, W3_GV(0, 1)) W3_M(2, 3, W3_GV(0, 2))
        W3_M(3, 0, W3_FR(4)) W3_M(3, 1, W3_GH(1)) W3_M(3, 2, W3_GV(1, 1)) W3_M(3, 3, W3_GV(1, 2))
        W3_M(4, 0, W3_FR(5) W3_WR(0, 1)) W3_M(4, 1, W3_WR(0, 2)) W3_M(4, 2, ) W3_M(4, 3, )
        W3_BAR_E()
        W3_M(5, 0, W3_FR_FROM(2, nxt) W3_GLD()) W3_M(5, 1, ) W3_M(5, 2, ) W3_M(5, 3, )
        p1 = p2;
      }
    }
  } else if (xh == 0) {
    for (int ch = ch_begin; ch < ch_end; ++ch) {
      const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
      float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
      const bool top = p1.ta == 0, bot = p1.ta == th - 1;                           // of chunk ch + 1, whose patches are in LDS
      W3Pos p2 = p1;
      if (ch + 2 < ch_end) advance(p2);
      W3_M(0, 0, WW_IF_FR(W3_FR(1)) WW_IF_T(W3_DLD_0A())) W3_M(0, 1, WW_IF_T(W3_DLD_0B())) W3_M(0, 2, WW_IF_T(W3_DLD_1A())) W3_M(0, 3, WW_IF_T(W3_DLD_1B()))
      W3_M(1, 0, WW_IF_FR(W3_FR(2))) W3_M(1, 1, ) W3_M(1, 2, ) W3_M(1, 3, )
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      WW_IF_BAR(__builtin_amdgcn_s_barrier();)
      __builtin_amdgcn_sched_barrier(0);
      W3_M(2, 0, WW_IF_FR(W3_FR(3)) WW_IF_DMA(dma(p2);)) W3_M(2, 1, WW_IF_T(W3_DMASK()) WW_IF_T(W3_DT(0, 0, 0)) WW_IF_T(W3_DT(0, 0, 1))) W3_M(2, 2, WW_IF_T(W3_DT(0, 0, 2)) WW_IF_T(W3_DT(0, 0, 3))) W3_M(2, 3, WW_IF_T(W3_DT(0, 1, 0)) WW_IF_T(W3_DT(0, 1, 1)))
      W3_M(3, 0, WW_IF_FR(W3_FR(4)) WW_IF_T(W3_DT(0, 1, 2)) WW_IF_T(W3_DT(0, 1, 3))) W3_M(3, 1, WW_IF_T(W3_DV(0, 0))) W3_M(3, 2, WW_IF_T(W3_DV(0, 1))) W3_M(3, 3, WW_IF_T(W3_DV(0, 2)))
      W3_M(4, 0, WW_IF_FR(W3_FR(5)) WW_IF_T(W3_DV(0, 3))) W3_M(4, 1, WW_IF_T(W3_DT(1, 0, 0)) WW_IF_T(W3_DT(1, 0, 1))) W3_M(4, 2, WW_IF_T(W3_DT(1, 0, 2)) WW_IF_T(W3_DT(1, 0, 3))) W3_M(4, 3, WW_IF_T(W3_DT(1, 1, 0)) WW_IF_T(W3_DT(1, 1, 1)))
      W3_M(5, 0, WW_IF_FR(W3_FR(6)) WW_IF_T(W3_DT(1, 1, 2)) WW_IF_T(W3_DT(1, 1, 3))) W3_M(5, 1, WW_IF_T(W3_DV(1, 0)) WW_IF_T(W3_WR(W3_OPER, 0))) W3_M(5, 2, WW_IF_T(W3_DV(1, 1)) WW_IF_T(W3_WR(W3_OPER, 1))) W3_M(5, 3, WW_IF_T(W3_DV(1, 2)) WW_IF_T(W3_WR(W3_OPER, 2)))
      W3_M(6, 0, WW_IF_FR(W3_FR(7)) WW_IF_T(W3_DV(1, 3)) WW_IF_T(W3_WR(W3_OPER, 3))) W3_M(6, 1, ) W3_M(6, 2, ) W3_M(6, 3, )
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      WW_IF_BAR(__builtin_amdgcn_s_barrier();)
      __builtin_amdgcn_sched_barrier(0);
      W3_M(7, 0, WW_IF_FR(W3_FR_FROM(0, nxt))) W3_M(7, 1, ) W3_M(7, 2, ) W3_M(7, 3, )
      p1 = p2;
    }
  } else {
    for (int ch = ch_begin; ch < ch_end; ++ch) {
      const float* cur = lds + ((ch - ch_begin) & 1) * W3_BUF;
      float* nxt = lds + ((ch - ch_begin + 1) & 1) * W3_BUF;
      W3Pos p2 = p1;
      if (ch + 2 < ch_end) advance(p2);
      W3_M(0, 0, WW_IF_FR(W3_FR(1)) WW_IF_T(W3_GLD())) W3_M(0, 1, ) W3_M(0, 2, ) W3_M(0, 3, )
      W3_M(1, 0, WW_IF_FR(W3_FR(2))) W3_M(1, 1, ) W3_M(1, 2, ) W3_M(1, 3, )
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      WW_IF_BAR(__builtin_amdgcn_s_barrier();)
      __builtin_amdgcn_sched_barrier(0);
      W3_M(2, 0, WW_IF_FR(W3_FR(3)) WW_IF_DMA(dma(p2);)) W3_M(2, 1, WW_IF_T(W3_GH(0))) W3_M(2, 2, WW_IF_T(W3_GV(0, 0))) W3_M(2, 3, WW_IF_T(W3_GV(0, 1)))
      W3_M(3, 0, WW_IF_FR(W3_FR(4))) W3_M(3, 1, WW_IF_T(W3_GV(0, 2))) W3_M(3, 2, WW_IF_T(W3_GV(0, 3))) W3_M(3, 3, WW_IF_T(W3_GH(1)))
      W3_M(4, 0, WW_IF_FR(W3_FR(5))) W3_M(4, 1, WW_IF_T(W3_GV(1, 0)) WW_IF_T(W3_WR(0, 0))) W3_M(4, 2, WW_IF_T(W3_GV(1, 1)) WW_IF_T(W3_WR(0, 1))) W3_M(4, 3, WW_IF_T(W3_GV(1, 2)) WW_IF_T(W3_WR(0, 2)))
      W3_M(5, 0, WW_IF_FR(W3_FR(6))) W3_M(5, 1, WW_IF_T(W3_GV(1, 3)) WW_IF_T(W3_WR(0, 3))) W3_M(5, 2, ) W3_M(5, 3, )
      W3_M(6, 0, WW_IF_FR(W3_FR(7))) W3_M(6, 1, ) W3_M(6, 2, ) W3_M(6, 3, )
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      WW_IF_BAR(__builtin_amdgcn_s_barrier();)
      __builtin_amdgcn_sched_barrier(0);
      W3_M(7, 0, WW_IF_FR(W3_FR_FROM(0, nxt))) W3_M(7, 1, ) W3_M(7, 2, ) W3_M(7, 3, )
      p1 = p2;
    }
  }
#undef W3_SWZ
#undef W3_TAIL
#undef W3_BAR_M
#undef W3_RD2
#undef W3_DLD_0A
#undef W3_DLD_0B
#undef W3_DLD_1A
#undef W3_DLD_1B
#undef W3_DMASK
#undef W3_DT
#undef W3_DV
#undef W3_WR
#undef W3_GLD
#undef W3_GH
#undef W3_GV
#undef W3_FR
#undef W3_FR_FROM
#undef W3_M
#undef W3_B
#undef W3_BAR_E
#undef W3_DLD7_0A
#undef W3_DLD7_1A
#undef W3_DLD6_0A
#undef W3_DLD6_1A
#undef W3_DLDL_0B
#undef W3_DLDL_1B
  // partial of this slab: ws[slab][xi][k0 + m][c0 + n]; accumulator register q of lane (li, half) is
  // row m = mb*32 + 8*(q/4) + 4*half + q%4, column n = nb*32 + li; accumulator xl = (a & 1) * 4 + b is plane xi = xh * 8 + xl
  if constexpr (LIVE == 0xF) {
    float* wp = a.ws + ((size_t)slab * 16) * a.K * a.C;
#pragma unroll
    for (int xl = 0; xl < 8; ++xl) {
      const int xi = xh * 8 + xl;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = mb * 32 + 8 * (q / 4) + 4 * half + (q % 4);
        wp[((size_t)xi * a.K + k0 + m) * a.C + c0 + nb * 32 + li] = acc[xl][q];
      }
    }
  } else {
    // live planes only, of the block's own pixel phase: ws[slab][a][live b][K][C]  (C = a.C / 2 channels of the layer)
    constexpr int NB = (LIVE & 1) + ((LIVE >> 1) & 1) + ((LIVE >> 2) & 1) + ((LIVE >> 3) & 1);
    const int CL = a.C / 2, cl0 = c0 >= CL ? c0 - CL : c0;
    float* wp = a.ws + ((size_t)slab * 4 * NB) * a.K * CL;
#pragma unroll
    for (int xl = 0; xl < 8; ++xl) {
      const int b = xl & 3;
      if (!((LIVE >> b) & 1)) continue;
      int bi = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) bi += (j < b && ((LIVE >> j) & 1)) ? 1 : 0;
      const int plane = (xh * 2 + (xl >> 2)) * NB + bi;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int m = mb * 32 + 8 * (q / 4) + 4 * half + (q % 4);
        wp[((size_t)plane * a.K + k0 + m) * CL + cl0 + nb * 32 + li] = acc[xl][q];
      }
    }
  }
}

__device__ __forceinline__ void wino_wgrad_body3(const WWArgs& a, const int blk) { wino_wgrad_body3_live<0xF>(a, blk); }

template <bool RAG>
__global__ __launch_bounds__(WW_THREADS) void k_wino_wgrad(WWArgs a) {
#ifndef WW_OLD
  if constexpr (!RAG) wino_wgrad_body3(a, blockIdx.x);
  else
#endif
  wino_wgrad_body<RAG>(a, blockIdx.x);
}

// Several layers in one launch (dl_wino_wgrad3x3_batch_nhwc_f32, see include/delora_hip.h): the layer table travels in the kernel
// arguments, layers ordered by decreasing work per workgroup
struct WWBatchArgs {
  WWArgs layer[DL_WGRAD_BATCH];
  int first_wg[DL_WGRAD_BATCH + 1];
  int n;
};
template <bool RAG>
__global__ __launch_bounds__(WW_THREADS) void k_wino_wgrad_batch(WWBatchArgs b) {
  const int l = dl_table_slot<DL_WGRAD_BATCH>(b.first_wg, b.n, (int)blockIdx.x);
  const WWArgs a = b.layer[l];
#ifndef WW_OLD
  if constexpr (!RAG) wino_wgrad_body3(a, (int)blockIdx.x - b.first_wg[l]);
  else
#endif
  wino_wgrad_body<RAG>(a, (int)blockIdx.x - b.first_wg[l]);
}

// Weight gradients of stride-(1,2) 3x3 layers on the pixel-pair view (dl_wino_strided_wgrad3x3_batch_nhwc_f32).  A layer is TWO items of
// the table: its odd-pixel channel blocks (pair channels >= C: 12 live planes) and its even-pixel ones (8 live planes).  The two kinds
// cost different time per chunk, so each has its own slab plan and its own partials; which body runs is workgroup-uniform.  One launch
// with both bodies: each stays below the stride-1 body's registers, and a second launch would leave the chip idle at the tail of the first.
#define SW_ITEMS (2 * DL_WGRAD_BATCH)
struct SWBatchArgs {
  WWArgs layer[SW_ITEMS];                // an item each; the pair view: W = W/2 pixels of C = 2C channels; ws = the item's own partials
  int first_wg[SW_ITEMS + 1];
  int odd[SW_ITEMS];
  int n;
};
// ALL12 (DL_SWGRAD_ALL12=1, a measurement switch of tools/conv_harness): the even-pixel blocks run the 12-plane body as well
template <bool ALL12>
__global__ __launch_bounds__(WW_THREADS) void k_wino_wgrad_strided_batch(SWBatchArgs b) {
  const int l = dl_table_slot<SW_ITEMS>(b.first_wg, b.n, (int)blockIdx.x);
  const WWArgs a = b.layer[l];
  if (b.odd[l]) wino_wgrad_body3_live<0x7>(a, (int)blockIdx.x - b.first_wg[l]);
  else if constexpr (ALL12) wino_wgrad_body3_live<0x7, false>(a, (int)blockIdx.x - b.first_wg[l]);
  else wino_wgrad_body3_live<0x6>(a, (int)blockIdx.x - b.first_wg[l]);
}

// U[xi][k][c] = sum over slabs of ws[slab][xi][k][c] in a fixed order (deterministic), four channels per thread
__device__ __forceinline__ void wino_wgrad_sum_body(const float* __restrict__ ws, int nslabs, size_t count4, float* __restrict__ u, size_t i) {
  if (i >= count4) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (int sl = 0; sl < nslabs; ++sl) s += reinterpret_cast<const f32x4*>(ws)[(size_t)sl * count4 + i];
  reinterpret_cast<f32x4*>(u)[i] = s;
}
__global__ __launch_bounds__(256) void k_wino_wgrad_sum(const float* __restrict__ ws, int nslabs, size_t count4, float* __restrict__ u) {
  wino_wgrad_sum_body(ws, nslabs, count4, u, (size_t)blockIdx.x * 256 + threadIdx.x);
}

__device__ __forceinline__ void wino_wgrad_out_body(const float* __restrict__ uu, int K, int C, float* __restrict__ dw, size_t i);
__global__ __launch_bounds__(256) void k_wino_wgrad_out(const float* __restrict__ uu, int K, int C, float* __restrict__ dw) {
  wino_wgrad_out_body(uu, K, C, dw, (size_t)blockIdx.x * 256 + threadIdx.x);
}

// the two small passes for a table of layers in one launch each
struct WWPostArgs {
  const float* src[DL_WGRAD_BATCH];      // sum: slab partials; out: the summed Winograd-domain gradient
  float* dst[DL_WGRAD_BATCH];            // sum: the summed gradient; out: dw
  int K[DL_WGRAD_BATCH], C[DL_WGRAD_BATCH], nslabs[DL_WGRAD_BATCH];
  int first_block[DL_WGRAD_BATCH + 1];
  int n;
};
__global__ __launch_bounds__(256) void k_wino_wgrad_sum_batch(WWPostArgs b) {
  const int l = dl_table_slot<DL_WGRAD_BATCH>(b.first_block, b.n, (int)blockIdx.x);
  wino_wgrad_sum_body(b.src[l], b.nslabs[l], (size_t)16 * b.K[l] * b.C[l] / 4, b.dst[l], (size_t)((int)blockIdx.x - b.first_block[l]) * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void k_wino_wgrad_out_batch(WWPostArgs b) {
  const int l = dl_table_slot<DL_WGRAD_BATCH>(b.first_block, b.n, (int)blockIdx.x);
  wino_wgrad_out_body(b.src[l], b.K[l], b.C[l], b.dst[l], (size_t)((int)blockIdx.x - b.first_block[l]) * 256 + threadIdx.x);
}

// dw[k][r][s][c] = (G^T U G)[r][s]
__device__ __forceinline__ void wino_wgrad_out_body(const float* __restrict__ uu, int K, int C, float* __restrict__ dw, size_t i) {
  if (i >= (size_t)K * C) return;
  const int k = (int)(i / C), c = (int)(i % C);
  float u[4][4];
#pragma unroll
  for (int xi = 0; xi < 16; ++xi) u[xi / 4][xi % 4] = uu[((size_t)xi * K + k) * C + c];
  // G^T = [[1, 1/2, 1/2, 0], [0, 1/2, -1/2, 0], [0, 1/2, 1/2, 1]]
  float p[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    p[0][j] = u[0][j] + 0.5f * (u[1][j] + u[2][j]);
    p[1][j] = 0.5f * (u[1][j] - u[2][j]);
    p[2][j] = 0.5f * (u[1][j] + u[2][j]) + u[3][j];
  }
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {
    dw[(((size_t)k * 3 + rr) * 3 + 0) * C + c] = p[rr][0] + 0.5f * (p[rr][1] + p[rr][2]);
    dw[(((size_t)k * 3 + rr) * 3 + 1) * C + c] = 0.5f * (p[rr][1] - p[rr][2]);
    dw[(((size_t)k * 3 + rr) * 3 + 2) * C + c] = 0.5f * (p[rr][1] + p[rr][2]) + p[rr][3];
  }
}

// CU count of the current device (the persistent grid's size), cached per device id
#include <atomic>
static int wn_cu_count() {
  if (g_dl_plan && g_dl_plan->cu_count > 0) return g_dl_plan->cu_count;      // dl_conv_plan_describe: the caller's CU count
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  int cus = cache[dev].load(std::memory_order_relaxed);
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

static int ww_slabs(int total_chunks, int tiles) { return dl_single_slabs(total_chunks, tiles, 256).nslabs; }      // one 512-thread workgroup per CU

static bool ww_supported(int N, int H, int W, int C, int K) {
  return N > 0 && H > 0 && W >= 2 && C % 64 == 0 && K % 64 == 0 && (size_t)N * H * W * (C > K ? C : K) < ((size_t)1 << 31) &&
         (size_t)H * W * (C > K ? C : K) < ((size_t)1 << 30);      // (per-sample byte offsets are 32-bit)
}
static bool ww_exact(int H, int W) { return !(H & 1) && !(W & 1) && ((W / 2) % 8) == 0; }
static int ww_chunks(int N, int H, int W) { return N * ((H + 1) / 2) * (((W + 1) / 2 + 7) / 8); }

/* see include/delora_hip.h */
extern "C" size_t dl_wino_wgrad_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K) {
  if (!ww_supported(N, H, W, C, K)) return 0;
  const int tiles = (K / 64) * (C / 64);
  return ((size_t)ww_slabs(ww_chunks(N, H, W), tiles) + 1) * 16 * K * C * sizeof(float);     // slab partials + their sum
}

extern "C" int dl_wino_wgrad3x3_nhwc_f32(const float* x, const float* g, float* dw, void* workspace, int32_t N, int32_t H,
                                         int32_t W, int32_t C, int32_t K, dl_stream stream) {
  if (!x || !g || !dw || !workspace) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_wgrad3x3_nhwc_f32: null pointer argument");
  if (!ww_supported(N, H, W, C, K))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_wino_wgrad3x3_nhwc_f32: shape N=%d H=%d W=%d C=%d K=%d not supported (C, K %% 64, < 2^31 elements)",
                   N, H, W, C, K);
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int tiles = (K / 64) * (C / 64);
  const int total_chunks = ww_chunks(N, H, W);
  const int nslabs = ww_slabs(total_chunks, tiles);
  WWArgs a{x, g, ws, N, H, W, C, K, (total_chunks + nslabs - 1) / nslabs, nslabs};
  const DlProfTag tag{"k_wino_wgrad", "wgrad", N, H, W, C, K, 3, 1, 1, 2.0 * 16.0 * (double)N * ((H + 1) / 2) * ((W + 1) / 2) * (double)C * K,
                      4.0 * ((double)N * H * W * (C + K) + 9.0 * C * K)};
  if (ww_exact(H, W)) DL_LAUNCH(tag, k_wino_wgrad<false>, dim3(tiles * nslabs), dim3(WW_THREADS), st, a);
  else DL_LAUNCH(tag, k_wino_wgrad<true>, dim3(tiles * nslabs), dim3(WW_THREADS), st, a);
  DL_PLAN_NOTE("slabs=%d", nslabs);
  const size_t count4 = (size_t)16 * K * C / 4;
  float* usum = ws + (size_t)nslabs * 16 * K * C;
  DL_LAUNCH_PLAIN(k_wino_wgrad_sum, dim3((unsigned)((count4 + 255) / 256)), dim3(256), st, (const float*)ws, nslabs, count4, usum);
  DL_LAUNCH_PLAIN(k_wino_wgrad_out, dim3((unsigned)(((size_t)K * C + 255) / 256)), dim3(256), st, (const float*)usum, K, C, dw);
  return dl_check_launch("dl_wino_wgrad3x3_nhwc_f32");
}

// ---- several layers in one call (the host side shared with the other families: wgrad_batch.h)
namespace {
struct WWItem : DlBatchItem {          // key: 1 for an image that does not divide into chunks of 8 tiles (RAG)
  WWArgs a;
  float* dw;
  WWArgs args() const { WWArgs r = a; r.ws = part; r.chunks_per_slab = p.chunks_per_slab; r.nslabs = p.nslabs; return r; }
};
const std::vector<int> kWWKeys{0, 1};
int ww_batch_plan(const dl_wgrad_layer* L, int n, std::vector<WWItem>& items) {
  if (!L || n <= 0 || n > DL_WGRAD_BATCH) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_wgrad3x3_batch_nhwc_f32: 1..%d layers per call", DL_WGRAD_BATCH);
  items.resize(n);
  for (int i = 0; i < n; ++i) {
    const dl_wgrad_layer& l = L[i];
    if (l.ksize != 3 || l.stride_h != 1 || l.stride_w != 1 || !ww_supported(l.N, l.H, l.W, l.C, l.K))
      return dl_fail(DL_ERR_UNSUPPORTED, "dl_wino_wgrad3x3_batch_nhwc_f32: layer %d: N=%d H=%d W=%d C=%d K=%d kernel %d stride (%d,%d) not supported "
                     "(3x3 stride 1, C, K %% 64, < 2^31 elements)", i, l.N, l.H, l.W, l.C, l.K, l.ksize, l.stride_h, l.stride_w);
    WWItem& it = items[i];
    it.a = WWArgs{(const float*)l.x, (const float*)l.g, nullptr, l.N, l.H, l.W, l.C, l.K, 0, 0};
    it.dw = l.dw;
    it.plane = (size_t)16 * l.K * l.C;
    it.p = DlSlabPlan{(l.K / 64) * (l.C / 64), ww_chunks(l.N, l.H, l.W), ww_chunks(l.N, l.H, l.W), 0, 0};
    it.key = ww_exact(l.H, l.W) ? 0 : 1;
    it.flop = 2.0 * 16.0 * (double)l.N * ((l.H + 1) / 2) * ((l.W + 1) / 2) * (double)l.C * l.K;
    it.bytes = 4.0 * ((double)l.N * l.H * l.W * (l.C + l.K) + 9.0 * l.C * l.K);
  }
  dl_plan_slabs(items, kWWKeys, 256, 10);                 // one 512-thread workgroup per CU
  return DL_OK;
}
}  // namespace

/* see include/delora_hip.h */
extern "C" size_t dl_wino_wgrad3x3_batch_workspace_bytes(const dl_wgrad_layer* layers, int32_t n) {
  std::vector<WWItem> items;
  if (ww_batch_plan(layers, n, items)) return 0;
  return dl_carve_workspace(items, nullptr, true, 0) * sizeof(float);
}

extern "C" int dl_wino_wgrad3x3_batch_nhwc_f32(const dl_wgrad_layer* layers, int32_t n, void* workspace, dl_stream stream) {
  if (!workspace) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_wgrad3x3_batch_nhwc_f32: null workspace");
  std::vector<WWItem> items;
  const int rc0 = ww_batch_plan(layers, n, items);
  if (rc0) return rc0;
  for (int i = 0; i < n; ++i)
    if (!layers[i].x || !layers[i].g || !layers[i].dw) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_wgrad3x3_batch_nhwc_f32: layer %d: null pointer", i);
  hipStream_t st = (hipStream_t)stream;
  dl_carve_workspace(items, (float*)workspace, true, 0);  // [slab partials (only when split)] [their sum]: a single slab IS the sum
  std::vector<const WWItem*> grp;
  for (int rag : kWWKeys) {
    WWBatchArgs b{};
    const DlGroupWork w = dl_fill_group(items, rag, [](const WWItem& it) { return it.p.chunks_per_slab; }, b, grp);
    if (!b.n) continue;
    const WWArgs& f = grp[0]->a;
    const DlProfTag tag{"k_wino_wgrad", b.n > 1 ? "wgrad-batch" : "wgrad", f.N, f.H, f.W, f.C, f.K, 3, 1, 1, w.flop, w.bytes};
    if (rag) DL_LAUNCH(tag, k_wino_wgrad_batch<true>, dim3(w.wgs), dim3(WW_THREADS), st, b);
    else DL_LAUNCH(tag, k_wino_wgrad_batch<false>, dim3(w.wgs), dim3(WW_THREADS), st, b);
    for (int i = 0; i < b.n; ++i) DL_PLAN_NOTE("slabs=%d", b.layer[i].nslabs);
  }
  WWPostArgs sum{}, out{};
  const int sum_blocks = dl_fill_post(items, true, 256, sum, [](WWPostArgs& t, int j, const WWItem& it) {
    t.src[j] = it.part; t.dst[j] = it.sum; t.K[j] = it.a.K; t.C[j] = it.a.C; t.nslabs[j] = it.p.nslabs;
    return it.plane / 4;
  });
  const int out_blocks = dl_fill_post(items, false, 256, out, [](WWPostArgs& t, int j, const WWItem& it) {
    t.src[j] = it.sum; t.dst[j] = it.dw; t.K[j] = it.a.K; t.C[j] = it.a.C;
    return (size_t)it.a.K * it.a.C;
  });
  if (sum.n) DL_LAUNCH_PLAIN(k_wino_wgrad_sum_batch, dim3(sum_blocks), dim3(256), st, sum);
  DL_LAUNCH_PLAIN(k_wino_wgrad_out_batch, dim3(out_blocks), dim3(256), st, out);
  return dl_check_launch("dl_wino_wgrad3x3_batch_nhwc_f32");
}

// ---- stride-(1,2) layers: the pixel-pair view's live planes (k_wino_wgrad_strided_batch)
struct SWSumArgs {
  const float* src[SW_ITEMS];
  float* dst[SW_ITEMS];
  int count4[SW_ITEMS], nslabs[SW_ITEMS];
  int first_block[SW_ITEMS + 1];
  int n;
};
__global__ __launch_bounds__(256) void k_wino_wgrad_strided_sum_batch(SWSumArgs b) {
  const int l = dl_table_slot<SW_ITEMS>(b.first_block, b.n, (int)blockIdx.x);
  wino_wgrad_sum_body(b.src[l], b.nslabs[l], (size_t)b.count4[l], b.dst[l], (size_t)((int)blockIdx.x - b.first_block[l]) * 256 + threadIdx.x);
}
// dw [K][3][3][C] of the layer from the summed live planes: uo [4][3][K][C] (odd pixels: b = 0, 1, 2), ue [4][2][K][C] (even pixels: b = 1, 2).
// The pair kernel's tap columns (dW G of the live columns; its third column does not exist):
//   dw[k][r][0][c] = column 0 of pair channel C + c,  dw[k][r][1][c] = column 1 of pair channel c,  dw[k][r][2][c] = column 1 of pair channel C + c
struct SWOutArgs {
  const float* uo[DL_WGRAD_BATCH];
  const float* ue[DL_WGRAD_BATCH];
  float* dw[DL_WGRAD_BATCH];
  int K[DL_WGRAD_BATCH], C[DL_WGRAD_BATCH];
  int first_block[DL_WGRAD_BATCH + 1];
  int n, eb;                            // eb: live columns the even-pixel planes hold (2; 3 under DL_SWGRAD_ALL12, the first unused)
};
__device__ __forceinline__ float sw_gt(int rr, float u0, float u1, float u2, float u3) {     // row rr of G^T = [[1, 1/2, 1/2, 0], [0, 1/2, -1/2, 0], [0, 1/2, 1/2, 1]]
  return rr == 0 ? u0 + 0.5f * (u1 + u2) : rr == 1 ? 0.5f * (u1 - u2) : 0.5f * (u1 + u2) + u3;
}
__global__ __launch_bounds__(256) void k_wino_wgrad_strided_out_batch(SWOutArgs b) {
  const int l = dl_table_slot<DL_WGRAD_BATCH>(b.first_block, b.n, (int)blockIdx.x);
  const int K = b.K[l], C = b.C[l];
  const size_t i = (size_t)((int)blockIdx.x - b.first_block[l]) * 256 + threadIdx.x;
  if (i >= (size_t)K * C) return;
  const int k = (int)(i / C), c = (int)(i % C);
  const float* __restrict__ uo = b.uo[l];
  const float* __restrict__ ue = b.ue[l];
  float* __restrict__ dw = b.dw[l];
  float o[4][3], e[4][2];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[a][j] = uo[((size_t)(a * 3 + j) * K + k) * C + c];
#pragma unroll
    for (int j = 0; j < 2; ++j) e[a][j] = ue[((size_t)(a * b.eb + b.eb - 2 + j) * K + k) * C + c];
  }
#pragma unroll
  for (int rr = 0; rr < 3; ++rr) {
    const float p0 = sw_gt(rr, o[0][0], o[1][0], o[2][0], o[3][0]);
    const float p1 = sw_gt(rr, o[0][1], o[1][1], o[2][1], o[3][1]);
    const float p2 = sw_gt(rr, o[0][2], o[1][2], o[2][2], o[3][2]);
    const float q1 = sw_gt(rr, e[0][0], e[1][0], e[2][0], e[3][0]);
    const float q2 = sw_gt(rr, e[0][1], e[1][1], e[2][1], e[3][1]);
    dw[(((size_t)k * 3 + rr) * 3 + 0) * C + c] = p0 + 0.5f * (p1 + p2);
    dw[(((size_t)k * 3 + rr) * 3 + 1) * C + c] = 0.5f * (q1 - q2);
    dw[(((size_t)k * 3 + rr) * 3 + 2) * C + c] = 0.5f * (p1 - p2);
  }
}

static bool sw_takes(int N, int H, int W, int C, int K, int sh, int sw) {
  return sh == 1 && sw == 2 && N > 0 && H > 0 && W > 0 && C > 0 && K > 0 && !(H & 1) && W % 32 == 0 && C % 64 == 0 && K % 64 == 0 &&
         ww_supported(N, H, W / 2, 2 * C, K);
}
/* see include/delora_hip.h */
extern "C" int dl_wino_strided_wgrad_takes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride_h, int32_t stride_w) {
  return sw_takes(N, H, W, C, K, stride_h, stride_w) ? 1 : 0;
}

namespace {
// An even-pixel block runs 16 of the odd-pixel block's 24 MFMAs per chunk, with the same DMA, barriers and per-column side work: the plan
// weighs its chunks 3/4 (between the 2/3 of the matrix work alone and the 0.84-0.89 that dropping a quarter of k_wino_conv's planes left
// of its time, profiles/strided_wino_harness.txt).
struct SWItem : DlBatchItem {
  WWArgs a;              // pair view
  int odd, layer, planes;
  WWArgs args() const { WWArgs r = a; r.ws = part; r.chunks_per_slab = p.chunks_per_slab; r.nslabs = p.nslabs; return r; }
};
bool sw_all12() {
  static const bool on = [] { const char* e = getenv("DL_SWGRAD_ALL12"); return e && e[0] == '1'; }();
  return on;
}
int sw_batch_plan(const dl_wgrad_layer* L, int n, std::vector<SWItem>& items) {
  const char* me = "dl_wino_strided_wgrad3x3_batch_nhwc_f32";
  if (!L || n <= 0 || n > DL_WGRAD_BATCH) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: 1..%d layers per call", me, DL_WGRAD_BATCH);
  for (int i = 0; i < n; ++i) {
    const dl_wgrad_layer& l = L[i];
    if (l.ksize != 3) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: ksize %d (must be 3)", me, i, l.ksize);
    if (l.stride_h != 1 || l.stride_w != 2) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: stride_h, stride_w (%d,%d) (must be (1,2))", me, i, l.stride_h, l.stride_w);
    if (l.H <= 0 || (l.H & 1)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: H %d (must be even)", me, i, l.H);
    if (l.W <= 0 || l.W % 32) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: W %d (must be a multiple of 32)", me, i, l.W);
    if (l.C <= 0 || l.C % 64) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: C %d (must be a multiple of 64)", me, i, l.C);
    if (l.K <= 0 || l.K % 64) return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: K %d (must be a multiple of 64)", me, i, l.K);
    if (!sw_takes(l.N, l.H, l.W, l.C, l.K, 1, 2))
      return dl_fail(DL_ERR_UNSUPPORTED, "%s: layer %d: N %d with H=%d W=%d C=%d K=%d (positive, below 2^31 elements and 2^30 per sample)", me, i, l.N, l.H, l.W, l.C, l.K);
  }
  items.resize(2 * n);
  for (int i = 0; i < n; ++i) {
    const dl_wgrad_layer& l = L[i];
    const int chunks = l.N * (l.H / 2) * (l.W / 32);
    for (int odd = 1; odd >= 0; --odd) {
      SWItem& it = items[2 * i + (1 - odd)];
      it.a = WWArgs{(const float*)l.x, (const float*)l.g, nullptr, l.N, l.H, l.W / 2, 2 * l.C, l.K, 0, 0};
      it.odd = odd; it.layer = i; it.key = 0;              // one launch with both bodies
      it.planes = odd || sw_all12() ? 12 : 8;
      it.plane = (size_t)it.planes * l.K * l.C;
      it.p = DlSlabPlan{(l.K / 64) * (l.C / 64), chunks, it.planes == 12 ? chunks : (3 * chunks + 3) / 4, 0, 0};
      // the live planes' multiply-adds: 2 . {12 | 8} . tiles . 64 . 64 per block; the layer's bytes counted once, with its odd item
      it.flop = 2.0 * it.planes * (double)l.N * (l.H / 2) * (l.W / 4) * 64.0 * 64.0 * it.p.tiles;
      it.bytes = odd ? 4.0 * ((double)l.N * l.H * (l.W / 2) * (2 * l.C + l.K) + 9.0 * l.C * l.K) : 0.0;
    }
  }
  dl_plan_slabs(items, {0}, 256, 10);                      // one 512-thread workgroup per CU
  return DL_OK;
}
}  // namespace

/* see include/delora_hip.h */
extern "C" size_t dl_wino_strided_wgrad3x3_batch_workspace_bytes(const dl_wgrad_layer* layers, int32_t n) {
  std::vector<SWItem> items;
  if (sw_batch_plan(layers, n, items)) return 0;
  return dl_carve_workspace(items, nullptr, true, 0) * sizeof(float);
}

extern "C" int dl_wino_strided_wgrad3x3_batch_nhwc_f32(const dl_wgrad_layer* layers, int32_t n, void* workspace, dl_stream stream) {
  if (!workspace) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_strided_wgrad3x3_batch_nhwc_f32: null workspace");
  std::vector<SWItem> items;
  const int rc0 = sw_batch_plan(layers, n, items);
  if (rc0) return rc0;
  for (int i = 0; i < n; ++i)
    if (!layers[i].x || !layers[i].g || !layers[i].dw) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_strided_wgrad3x3_batch_nhwc_f32: layer %d: null pointer", i);
  hipStream_t st = (hipStream_t)stream;
  dl_carve_workspace(items, (float*)workspace, true, 0);  // [slab partials (only when split)] [their sum]: a single slab IS the sum
  std::vector<const SWItem*> grp;
  SWBatchArgs b{};
  // by decreasing time per workgroup (chunks x MFMAs per chunk)
  const DlGroupWork w = dl_fill_group(items, 0, [](const SWItem& it) { return it.p.chunks_per_slab * (it.planes / 4 + 1); }, b, grp);
  for (int i = 0; i < b.n; ++i) b.odd[i] = grp[i]->odd;
  const dl_wgrad_layer& f = layers[grp[0]->layer];
  const DlProfTag tag{"k_wino_wgrad_strided", n > 1 ? "wgrad-batch" : "wgrad", f.N, f.H, f.W, f.C, f.K, 3, 1, 2, w.flop, w.bytes};
  if (sw_all12()) DL_LAUNCH(tag, k_wino_wgrad_strided_batch<true>, dim3(w.wgs), dim3(WW_THREADS), st, b);
  else DL_LAUNCH(tag, k_wino_wgrad_strided_batch<false>, dim3(w.wgs), dim3(WW_THREADS), st, b);
  for (int i = 0; i < b.n; ++i) DL_PLAN_NOTE("%s slabs=%d", b.odd[i] ? "odd" : "even", b.layer[i].nslabs);
  SWSumArgs sum{};
  const int sum_blocks = dl_fill_post(items, true, 256, sum, [](SWSumArgs& t, int j, const SWItem& it) {
    t.src[j] = it.part; t.dst[j] = it.sum; t.count4[j] = (int)(it.plane / 4); t.nslabs[j] = it.p.nslabs;
    return it.plane / 4;
  });
  SWOutArgs out{};                                         // one entry per LAYER, from the sums of its two items
  int out_blocks = 0;
  for (const auto& it : items) (it.odd ? out.uo : out.ue)[it.layer] = it.sum;
  for (int i = 0; i < n; ++i) {
    out.dw[i] = layers[i].dw; out.K[i] = layers[i].K; out.C[i] = layers[i].C;
    out.first_block[i] = out_blocks;
    out_blocks += (int)(((size_t)layers[i].K * layers[i].C + 255) / 256);
  }
  out.n = n; out.eb = sw_all12() ? 3 : 2;
  out.first_block[n] = out_blocks;
  if (sum.n) DL_LAUNCH_PLAIN(k_wino_wgrad_strided_sum_batch, dim3(sum_blocks), dim3(256), st, sum);
  DL_LAUNCH_PLAIN(k_wino_wgrad_strided_out_batch, dim3(out_blocks), dim3(256), st, out);
  return dl_check_launch("dl_wino_strided_wgrad3x3_batch_nhwc_f32");
}

// Sum of the channel ranges of a split launch + the layer's epilogue (as in k_wino_conv: shortcut add, activation, activation
// derivative of the saved forward activation), four channels per thread, ranges added in index order (deterministic).
__global__ __launch_bounds__(256) void k_wino_split_sum(const float* __restrict__ part, int splits, size_t count4, float* __restrict__ y,
                                                         const float* __restrict__ add, const float* __restrict__ dsrc, int act, unsigned epi) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= count4) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(part) + i;
  f32x4 v = p[0];
  for (int s = 1; s < splits; ++s) v += p[(size_t)s * count4];
  if (epi & WN_EPI_ADD) v += reinterpret_cast<const f32x4*>(add)[i];
  if (epi & WN_EPI_ACT) {
    if (act == 1) { v[0] = dl_tanh(v[0]); v[1] = dl_tanh(v[1]); v[2] = dl_tanh(v[2]); v[3] = dl_tanh(v[3]); }
    else { v[0] = wn_act(v[0], act); v[1] = wn_act(v[1], act); v[2] = wn_act(v[2], act); v[3] = wn_act(v[3], act); }
  }
  if (epi & WN_EPI_DACT) {
    const f32x4 sv = reinterpret_cast<const f32x4*>(dsrc)[i];
    if (act == 1) v *= 1.f - sv * sv;
    else { v[0] *= wn_dact(sv[0], act); v[1] *= wn_dact(sv[1], act); v[2] *= wn_dact(sv[2], act); v[3] *= wn_dact(sv[3], act); }
  }
  reinterpret_cast<f32x4*>(y)[i] = v;
}

// (tile-group shape, number of groups) of a launch: images that divide take 2 x 32 or 4 x 16 tiles per group (the two shapes the
// network's BASELINE images need); every other image -- the reference's shipped 64x720 (feature maps 180 / 90 / 45 / 23 wide) and
// 64x512 (layer4: 32x16) -- takes the shape that wastes the fewest tiles, with overhanging groups at the right / lower edge.
struct WinoPlan { int tc; bool rag; int groups; int splits; };
static WinoPlan wino_plan(int N, int H, int W, int C, int K, int cap) {
  const int tw = (W + 1) / 2, th = (H + 1) / 2;                     // 2x2 output tiles (the last one of an odd row / column is partial)
  const bool even = !(H & 1) && !(W & 1);
  WinoPlan p{32, false, 0, 1};
  if (even && tw % 32 == 0 && th % 2 == 0) { p.tc = 32; p.groups = N * (th / 2) * (tw / 32) * (K / WN_KB); }
  else if (even && tw % 16 == 0 && th % 4 == 0) { p.tc = 16; p.groups = N * (th / 4) * (tw / 16) * (K / WN_KB); }
  else {
    int best_tc = 0;
    long best_tiles = 0;
    for (int tc = 32; tc >= 4; tc >>= 1) {
      const int tr = WN_TILES / tc;
      const long tiles = (long)((tw + tc - 1) / tc) * tc * (long)((th + tr - 1) / tr) * tr;
      if (!best_tc || tiles < best_tiles) { best_tc = tc; best_tiles = tiles; }
    }
    const int tr = WN_TILES / best_tc;
    p.tc = best_tc; p.rag = true;
    p.groups = N * ((th + tr - 1) / tr) * ((tw + best_tc - 1) / best_tc) * (K / WN_KB);
  }
  // Split-K when the launch leaves most of the chip idle: double the number of channel ranges while all workgroups still fit one
  // round of the CUs and a range keeps at least 4 chunks (32 channels: below that the fixed cost of a group -- prologue, output
  // transform, stores, ~2 chunks' worth -- and the partial-sum traffic eat the gain).  Layers with fewer than 128 input channels are
  // left alone: their chain is 8 chunks, a split saves ~10 us of GPU time and costs a second launch (~18 us of host time in a step
  // that is host-bound at batch 1).  DL_WINO_SPLIT=0 turns it off (A/B).
  static const bool allow = [] { const char* e = getenv("DL_WINO_SPLIT"); return !(e && e[0] == '0'); }();
  const int nchunks = C / WN_CK;
  if (allow && cap > 0 && nchunks >= 16)
    while (p.groups * p.splits * 2 <= cap && nchunks % (p.splits * 2) == 0 && nchunks / (p.splits * 2) >= 4) p.splits *= 2;
  return p;
}

extern "C" size_t dl_wino_conv3x3_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || C % WN_CK || K % WN_KB) return 0;
  const WinoPlan p = wino_plan(N, H, W, C, K, wn_cu_count());
  return p.splits > 1 ? (size_t)p.splits * N * H * W * K * sizeof(float) : 0;
}

extern "C" int dl_wino_conv3x3_nhwc_f32(const float* x, const float* u, float* y, const float* add, const float* dsrc,
                                        int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t act,
                                        uint32_t epilogue, void* workspace, dl_stream stream) {
  if (!x || !u || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_conv3x3_nhwc_f32: bad argument");
  if (((epilogue & WN_EPI_ADD) && !add) || ((epilogue & WN_EPI_DACT) && !dsrc) || act < 0 || act > 2)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_conv3x3_nhwc_f32: epilogue operand missing / bad activation");
  if (C % WN_CK || K % WN_KB || (size_t)N * H * W * (C > K ? C : K) >= ((size_t)1 << 31) || (size_t)H * W * C >= ((size_t)1 << 30))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_wino_conv3x3_nhwc_f32: shape N=%d H=%d W=%d C=%d K=%d not supported (C %% 8, K %% 64, < 2^31 elements)", N, H, W, C, K);
  WinoArgs a{x, u, y, add, dsrc, N, H, W, C, K, act, epilogue, 1};
  hipStream_t st = (hipStream_t)stream;
  const int tw = (W + 1) / 2, th = (H + 1) / 2;                     // 2x2 output tiles (the last one of an odd row / column is partial)
  // what the algorithm asks of the matrix cores: 16 multiply-adds per 2x2 output tile and (c, k) pair (a direct convolution: 36)
  const DlProfTag tag{"k_wino_conv", "conv", N, H, W, C, K, 3, 1, 1, 2.0 * 16.0 * (double)N * th * tw * (double)C * K,
                      4.0 * ((double)N * H * W * (C + K) + 16.0 * C * K)};
  // persistent workgroups: one per CU (a 512-thread workgroup with 162 KB of LDS fills a CU); the CU count is read once per device
  int cap = wn_cu_count();
#ifdef CV_TUNE
  if (const char* e = getenv("DL_WN_GRID")) cap = atoi(e);
#endif
  WinoPlan p = wino_plan(N, H, W, C, K, cap);
  if (p.splits > 1 && (!workspace || (size_t)p.splits * N * H * W * K >= ((size_t)1 << 31))) p.splits = 1;   // no scratch given: one range
  if (p.splits > 1) {
    // the channel ranges of a SMALL launch on otherwise idle CUs; partial sums + epilogue in a second, elementwise launch
    a.y = (float*)workspace; a.add = nullptr; a.dsrc = nullptr; a.act = 0; a.epi = 0; a.splits = p.splits;
    const dim3 grid(p.groups * p.splits);             // <= cap by construction
    if (!p.rag && p.tc == 32) DL_LAUNCH(tag, (k_wino_conv<32, false, true>), grid, dim3(WN_THREADS), st, a);
    else if (!p.rag) DL_LAUNCH(tag, (k_wino_conv<16, false, true>), grid, dim3(WN_THREADS), st, a);
    else switch (p.tc) {
      case 32: DL_LAUNCH(tag, (k_wino_conv<32, true, true>), grid, dim3(WN_THREADS), st, a); break;
      case 16: DL_LAUNCH(tag, (k_wino_conv<16, true, true>), grid, dim3(WN_THREADS), st, a); break;
      case 8: DL_LAUNCH(tag, (k_wino_conv<8, true, true>), grid, dim3(WN_THREADS), st, a); break;
      default: DL_LAUNCH(tag, (k_wino_conv<4, true, true>), grid, dim3(WN_THREADS), st, a); break;
    }
    DL_PLAN_NOTE("splits=%d", p.splits);
    const size_t count4 = (size_t)N * H * W * K / 4;
    const DlProfTag tag2{"k_wino_split_sum", "conv", N, H, W, C, K, 3, 1, 1, 0.0, 4.0 * (double)N * H * W * K * (p.splits + 1)};
    DL_LAUNCH(tag2, k_wino_split_sum, dim3((unsigned)((count4 + 255) / 256)), dim3(256), st, (const float*)workspace, p.splits, count4, y, add,
              dsrc, act, epilogue);
    return dl_check_launch("dl_wino_conv3x3_nhwc_f32");
  }
  const dim3 grid(cap > 0 && p.groups > cap ? cap : p.groups);
  if (!p.rag && p.tc == 32) DL_LAUNCH(tag, (k_wino_conv<32, false>), grid, dim3(WN_THREADS), st, a);
  else if (!p.rag) DL_LAUNCH(tag, (k_wino_conv<16, false>), grid, dim3(WN_THREADS), st, a);
  else switch (p.tc) {
    case 32: DL_LAUNCH(tag, (k_wino_conv<32, true>), grid, dim3(WN_THREADS), st, a); break;
    case 16: DL_LAUNCH(tag, (k_wino_conv<16, true>), grid, dim3(WN_THREADS), st, a); break;
    case 8: DL_LAUNCH(tag, (k_wino_conv<8, true>), grid, dim3(WN_THREADS), st, a); break;
    default: DL_LAUNCH(tag, (k_wino_conv<4, true>), grid, dim3(WN_THREADS), st, a); break;
  }
  return dl_check_launch("dl_wino_conv3x3_nhwc_f32");
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-(1,2) 3x3 layers on the fused Winograd kernel.  With wrap-around columns and an even width the layer is a
// stride-1 3x3 convolution of the SAME memory read as [N][H][W/2][2C] -- a pixel pair is one pixel with 2C channels, the even pixel's
// first -- with the kernel
//   tap column 0: odd-pixel channels  <- w[:, :, 0]        tap column 1: even-pixel channels <- w[:, :, 1], odd-pixel channels <- w[:, :, 2]
//   tap column 2: zero
// and its input gradient is the stride-1 convolution of g [N][H][W/2][K] with the flipped, transposed kernel into 2C channels, which IS
// dx [N][H][W][C].  k_wino_weights_strided writes U = G g G^T of the rearranged kernel in the wn_u_index layout (u_fwd: rows K,
// reduction 2C; u_bwd: rows 2C, reduction K), all 16 planes -- the planes of xi-column 3 (forward) / 0 (input gradient) are exact zeros
// and k_wino_conv_strided never reads them.  One thread per (k, pair channel).
__global__ __launch_bounds__(256) void k_wino_weights_strided(const float* __restrict__ w, float* __restrict__ u_fwd,
                                                              float* __restrict__ u_bwd, int K, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int C2 = 2 * C;
  if (i >= K * C2) return;
  const int c2 = i % C2, k = i / C2;
  const bool odd = c2 >= C;
  const int c = odd ? c2 - C : c2;
  float g[3][3], gf[3][3], u[4][4];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float* wr = w + ((size_t)(k * 3 + r) * 3) * C + c;
    g[r][0] = odd ? wr[0] : 0.f;
    g[r][1] = odd ? wr[2 * (size_t)C] : wr[C];
    g[r][2] = 0.f;
#pragma unroll
    for (int s = 0; s < 3; ++s) gf[2 - r][2 - s] = g[r][s];
  }
  if (u_fwd) {
    wn_weight_transform(g, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u_fwd[wn_u_index(K, c2 / 8, xi, k, c2 % 8)] = u[xi / 4][xi % 4];
  }
  if (u_bwd) {
    wn_weight_transform(gf, u);
#pragma unroll
    for (int xi = 0; xi < 16; ++xi) u_bwd[wn_u_index(C2, k / 8, xi, c2, k % 8)] = u[xi / 4][xi % 4];
  }
}

// Whether the pixel-pair view of a stride-(sh, sw) layer on an H x W image divides into whole tile groups (the only launches
// k_wino_conv_strided has), and the group shape.  Stride (2,2) stays on the direct kernel.
static bool wn_strided_tiles(int N, int H, int W, int C, int K, int sh, int sw, int* tc) {
  if (sh != 1 || sw != 2 || N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || (H & 1) || (W & 3) || C % 64 || K % 64) return false;
  const int wide = 2 * C > K ? 2 * C : K;
  if ((size_t)N * H * (W / 2) * wide >= ((size_t)1 << 31) || (size_t)H * (W / 2) * wide >= ((size_t)1 << 30)) return false;
  const int tw = W / 4, th = H / 2;
  if (tw % 32 == 0 && th % 2 == 0) { *tc = 32; return true; }
  if (tw % 16 == 0 && th % 4 == 0) { *tc = 16; return true; }
  return false;
}

/* see include/delora_hip.h */
extern "C" int dl_wino_strided_takes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride_h, int32_t stride_w,
                                     int32_t cu_count) {
  int tc;
  if (!wn_strided_tiles(N, H, W, C, K, stride_h, stride_w, &tc)) return 0;
  const int cap = cu_count > 0 ? cu_count : wn_cu_count();
  // a launch that the stride-1 dispatch would cut into channel ranges leaves most of the chip idle as one range: it stays direct
  return wino_plan(N, H, W / 2, 2 * C, K, cap).splits == 1 && wino_plan(N, H, W / 2, K, 2 * C, cap).splits == 1;
}

extern "C" size_t dl_wino_strided_weights_floats(int32_t K, int32_t C, int32_t stride_h, int32_t stride_w) {
  return stride_h == 1 && stride_w == 2 && K > 0 && C > 0 ? (size_t)16 * K * 2 * C : 0;
}

extern "C" int dl_wino_strided_weights_f32(const float* w, float* u_fwd, float* u_bwd, int32_t K, int32_t C, int32_t stride_h,
                                           int32_t stride_w, dl_stream stream) {
  if (!w || (!u_fwd && !u_bwd) || K <= 0 || C <= 0 || K % 8 || C % 8 || stride_h != 1 || stride_w != 2)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_strided_weights_f32: bad argument (K, C multiples of 8, stride (1,2))");
  hipLaunchKernelGGL(k_wino_weights_strided, dim3((K * 2 * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, u_fwd, u_bwd, K, C);
  return dl_check_launch("dl_wino_strided_weights_f32");
}

// one launch of the pixel-pair form: a is the reinterpreted stride-1 problem, (H, W, C, K, sh, sw) the layer as the profile names it
static int wn_strided_launch(const char* what, WinoArgs a, int str, int tc, int H, int W, int C, int K, int sh, int sw, hipStream_t st) {
  const int tw = a.W / 2, th = a.H / 2;
  // 12 of the 16 planes multiply: the multiply-adds the matrix cores are actually given
  const DlProfTag tag{"k_wino_conv", "conv", a.N, H, W, C, K, 3, sh, sw, 2.0 * 12.0 * (double)a.N * th * tw * (double)a.C * a.K,
                      4.0 * ((double)a.N * a.H * a.W * (a.C + a.K) + 12.0 * a.C * a.K)};
  const int groups = a.N * (th / (WN_TILES / tc)) * (tw / tc) * (a.K / WN_KB);
  const int cap = wn_cu_count();
  const dim3 grid(cap > 0 && groups > cap ? cap : groups);
  if (str == 1) {
    if (tc == 32) DL_LAUNCH(tag, (k_wino_conv_strided<32, 1>), grid, dim3(WN_THREADS), st, a);
    else DL_LAUNCH(tag, (k_wino_conv_strided<16, 1>), grid, dim3(WN_THREADS), st, a);
  } else {
    if (tc == 32) DL_LAUNCH(tag, (k_wino_conv_strided<32, 2>), grid, dim3(WN_THREADS), st, a);
    else DL_LAUNCH(tag, (k_wino_conv_strided<16, 2>), grid, dim3(WN_THREADS), st, a);
  }
  return dl_check_launch(what);
}

extern "C" int dl_wino_strided_conv3x3_nhwc_f32(const float* x, const float* u_fwd, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                                                int32_t K, int32_t stride_h, int32_t stride_w, int32_t act, uint32_t epilogue,
                                                dl_stream stream) {
  if (!x || !u_fwd || !y || act < 0 || act > 2 || (epilogue & ~WN_EPI_ACT))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_strided_conv3x3_nhwc_f32: bad argument (epilogue: the activation bit or none)");
  int tc;
  if (!wn_strided_tiles(N, H, W, C, K, stride_h, stride_w, &tc))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_wino_strided_conv3x3_nhwc_f32: N=%d H=%d W=%d C=%d K=%d stride (%d,%d) does not tile", N, H, W, C, K, stride_h, stride_w);
  WinoArgs a{x, u_fwd, y, nullptr, nullptr, N, H, W / 2, 2 * C, K, act, epilogue, 1};
  return wn_strided_launch("dl_wino_strided_conv3x3_nhwc_f32", a, 1, tc, H, W, C, K, stride_h, stride_w, (hipStream_t)stream);
}

extern "C" int dl_wino_strided_dgrad3x3_nhwc_f32(const float* g, const float* u_bwd, float* dx, const float* add_grid, const float* dsrc,
                                                 int32_t N, int32_t H, int32_t W, int32_t K, int32_t C, int32_t stride_h, int32_t stride_w,
                                                 int32_t act, uint32_t epilogue, dl_stream stream) {
  const uint32_t EPI_GRID = 8u;                       // the add-on-the-grid bit of dl_conv2d_dgrad_strided_nhwc_f32
  if (!g || !u_bwd || !dx || act < 0 || act > 2 || (epilogue & ~(EPI_GRID | WN_EPI_DACT)) || ((epilogue & EPI_GRID) && !add_grid) ||
      ((epilogue & WN_EPI_DACT) && !dsrc))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_wino_strided_dgrad3x3_nhwc_f32: bad argument (epilogue bits 8 / 4 and their operands)");
  int tc;
  if (!wn_strided_tiles(N, H, W, C, K, stride_h, stride_w, &tc))
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_wino_strided_dgrad3x3_nhwc_f32: N=%d H=%d W=%d C=%d K=%d stride (%d,%d) does not tile", N, H, W, C, K, stride_h, stride_w);
  const unsigned epi = ((epilogue & EPI_GRID) ? WN_EPI_ADD : 0u) | (epilogue & WN_EPI_DACT);
  WinoArgs a{g, u_bwd, dx, add_grid, dsrc, N, H, W / 2, K, 2 * C, act, epi, 1};
  return wn_strided_launch("dl_wino_strided_dgrad3x3_nhwc_f32", a, 2, tc, H, W, C, K, stride_h, stride_w, (hipStream_t)stream);
}
