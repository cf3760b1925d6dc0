// What the two streaming passes over matched pairs share (loss.hip: the ICP loss and its gradient moments; info.hip: the
// point-to-plane normal equations): the grid, the thirteen 16-byte load streams of one 256-pixel chunk, packed fp32 arithmetic and
// the workgroup reduction that leaves one partial row per workgroup.
#pragma once
#include "common.h"

#define LOSS_PX 4            // consecutive pixels per lane (16-byte loads of every streamed plane)

#ifndef LOSS_WG_PER_SAMPLE
#define LOSS_WG_PER_SAMPLE 128  // workgroups (4 waves each) per sample: 512 waves, 1 chunk per wave at 64x2048
#endif
static inline int loss_blocks(int HW) {
  const int chunks = (HW + DL_WAVE * LOSS_PX - 1) / (DL_WAVE * LOSS_PX);
  int wg = (chunks + 3) / 4;
  return wg < LOSS_WG_PER_SAMPLE ? wg : LOSS_WG_PER_SAMPLE;
}

// Packed fp32: the kernels are bound by VALU issue once their operands sit in the infinity cache (which they do right after
// the correspondence search), so two pixels travel through every arithmetic instruction (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32 on the register pairs the 16-byte loads deliver) and the accumulators hold even/odd-pixel partial sums.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ f2 pk_fma(float a, f2 b, f2 c) { return __builtin_elementwise_fma((f2){a, a}, b, c); }
__device__ __forceinline__ f2 pk_mul(float a, f2 b) { return (f2){a, a} * b; }

// A value of another lane of the same 16-lane DPP row (CTRL: quad_perm 0x00-0xFF, row_ror:n 0x120+n, ...): a VALU
// operand modifier -- no LDS traffic, unlike the ds_bpermute behind __shfl_xor.
template <int CTRL>
__device__ __forceinline__ float dpp_get(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

// Streamed operands of one 256-pixel chunk as a wave loads them: lane l holds pixels 4l..4l+3 of every plane.
struct StreamRegs {
  int4 j;                       // correspondence (validity)
  float4 x, y, z, a, b, c;      // source point and normal
  float4 tx, ty, tz, ta, tb, tc; // matched target point and normal
};

__device__ __forceinline__ StreamRegs load_stream(const int32_t* __restrict__ nn, const float* __restrict__ sp,
                                                  const float* __restrict__ sn, const float* __restrict__ mt, int q4,
                                                  int g4) {
  StreamRegs r;
  // Non-temporal hint on the thirteen streams (round 6): every byte is read once per launch, and with it a launch behind clean caches
  // takes 13.2 us instead of 13.9 (0.50-0.51 of 8 TB/s instead of 0.48; with the operands in the infinity cache nothing changes).
  typedef float nt_f4 __attribute__((ext_vector_type(4)));
  typedef int nt_i4 __attribute__((ext_vector_type(4)));
  auto ld4 = [](const float* p, int i) { const nt_f4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_f4*>(p) + i); return make_float4(v.x, v.y, v.z, v.w); };
#define LD4(P, I) ld4(P, I)
  { const nt_i4 v = __builtin_nontemporal_load(reinterpret_cast<const nt_i4*>(nn) + g4); r.j = make_int4(v.x, v.y, v.z, v.w); }
  r.x = LD4(sp, g4);
  r.y = LD4(sp, q4 + g4);
  r.z = LD4(sp, 2 * q4 + g4);
  r.a = LD4(sn, g4);
  r.b = LD4(sn, q4 + g4);
  r.c = LD4(sn, 2 * q4 + g4);
  r.tx = LD4(mt, g4);
  r.ty = LD4(mt, q4 + g4);
  r.tz = LD4(mt, 2 * q4 + g4);
  r.ta = LD4(mt, 3 * q4 + g4);
  r.tb = LD4(mt, 4 * q4 + g4);
  r.tc = LD4(mt, 5 * q4 + g4);
#undef LD4
  return r;
}

// Reduction of NA packed accumulators over the workgroup into ONE partial row of PITCH floats (columns NA..PITCH-1 zero).
// Even/odd pixels first; then the four lanes of every quad TRANSPOSE-reduce the NA values (each butterfly step halves the number
// of values a lane carries: lane l of a quad ends up with the quad sums of accumulators 4k + l), two row rotations add the four
// quads of a 16-lane DPP row, and the 16 row sums of the workgroup meet in LDS where they are added in a fixed order.  ~70 VALU
// instructions for 24 values instead of the 144 adds + 144 ds_bpermute of a shuffle tree per value, and no LDS traffic in the wave
// part.  `red`: LDS, (DL_BLOCK / 16) * PITCH floats.  Every thread of the workgroup calls it.
template <int NA, int PITCH>
__device__ __forceinline__ void wg_reduce_row(const f2 (&acc)[NA], float* __restrict__ red, float* __restrict__ partial_row) {
  constexpr int ROWS = DL_BLOCK / 16;
  constexpr int NP = (NA + 3) / 4 * 4;
  static_assert(NP <= PITCH, "a partial row holds every accumulator");
  const int lane = threadIdx.x & (DL_WAVE - 1);
  float v[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) v[i] = i < NA ? acc[i].x + acc[i].y : 0.f;
  const bool b0 = lane & 1, b1 = lane & 2;
  float u[NP / 2];
#pragma unroll
  for (int k = 0; k < NP / 2; ++k) {
    const float keep = b0 ? v[2 * k + 1] : v[2 * k], send = b0 ? v[2 * k] : v[2 * k + 1];
    u[k] = keep + dpp_get<0xB1>(send);                  // quad_perm [1,0,3,2]: lane ^ 1
  }
  float q[NP / 4];
#pragma unroll
  for (int k = 0; k < NP / 4; ++k) {
    const float keep = b1 ? u[2 * k + 1] : u[2 * k], send = b1 ? u[2 * k] : u[2 * k + 1];
    q[k] = keep + dpp_get<0x4E>(send);                  // quad_perm [2,3,0,1]: lane ^ 2
    q[k] += dpp_get<0x124>(q[k]);                       // row_ror:4
    q[k] += dpp_get<0x128>(q[k]);                       // row_ror:8
  }
  if ((lane & 12) == 0) {                               // the first quad of every row holds the row's NA sums
    float* dst = red + (threadIdx.x >> 4) * PITCH + (lane & 3);
#pragma unroll
    for (int k = 0; k < NP / 4; ++k) dst[4 * k] = q[k];
  }
  __syncthreads();
  if (threadIdx.x < PITCH) {
    const int t = threadIdx.x;
    float s = 0.f;
    if (t < NA) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) s += red[r * PITCH + t];
    }
    partial_row[t] = s;
  }
}
