// Exact nearest neighbour between two free-form point lists by tree search (dl_nn_list_build / dl_nn_list_query): what the
// reference does with scipy's cKDTree (src/losses/icp_losses.py:24-34), for callers that hold lists and no range image.
//
//   build   bounding box of the finite targets (256 partial boxes, re-reduced by whoever needs the box) -> 63-bit Morton key per
//           point -> stable LSD radix sort of (key, index), 8 passes of 8 bits -> packed records (x, y, z, index bits) in curve
//           order, 64 per leaf, with the leaf's exact axis-aligned box -> levels of 64 children per node up to <= 64 top nodes.
//   query   the same key (clamped to the target box) and sort for the queries, so that a wave holds 64 neighbouring queries;
//           every lane finds its rank among the target keys (binary search), the wave tests the leaves at those ranks (the seed),
//           then walks the levels top-down as one packet: 64 children of a node are screened lane-parallel against the packet's box,
//           the survivors are opened when some lane's own lower bound reaches them, an opened leaf goes through the wave's 1 KB of
//           LDS and every lane tests its 64 points.
//
// Exactness: every deciding comparison is nl_dist2 (the expression of k_nn_bruteforce, fp64 on the fp32 coordinates) with the
// lower original index winning ties; lower bounds are the same fp64 arithmetic on exact box corners (rounding is monotone, so a
// bound never exceeds the distance of a point inside the box) and a subtree is skipped only when its bound is strictly greater than
// the best so far.  The keys order the data and decide nothing: any key assignment gives the same indices.
// No atomics anywhere; no host synchronisation; workspace sizes depend on the counts alone.
#include <math.h>

#include <utility>

#include "common.h"

#define NL_LEAF 64                   // points per leaf = lanes per wave
#define NL_FAN 64                    // children per node
#define NL_LEVELS 4                  // leaves + 3 levels of nodes: 64^4 leaves at most, top level <= 64 nodes
#define NL_MAX_POINTS (1 << 30)      // 32-bit indices everywhere: larger lists are rejected
#define NL_TILE 2048                 // elements per workgroup of the sort (4 waves x 8 rows of 64)
#define NL_ROWS (NL_TILE / DL_BLOCK)
#define NL_PARTS 256                 // partial bounding boxes (= DL_BLOCK: one per thread when they are re-reduced)
#define NL_PARTS_BYTES (NL_PARTS * 8 * sizeof(float))
#define NL_KEY_BITS 21               // per axis
#define NL_NO_INDEX 0x7fffffff

namespace {

struct NLTree {
  float* parts;                      // [NL_PARTS][8]: lo x y z -, hi x y z -
  float4* recs;                      // [P]: x, y, z, original index as bits; P = Mt rounded up to whole leaves, padding is NaN / -1
  uint64_t *key_a, *key_b;           // [P] each; the sorted keys end in key_a
  uint32_t *val_a, *val_b;           // [P] each
  float4* box[NL_LEVELS];            // [n[l]][2]: lo, hi
  int n[NL_LEVELS];
  int levels;                        // levels in use (0 for an empty list); n[levels - 1] <= NL_FAN
  uint32_t* hist;                    // [256][sort workgroups]
  int P;
  size_t bytes;
};

struct NLSort {
  uint64_t *key_a, *key_b;
  uint32_t *val_a, *val_b;
  uint32_t* hist;
  size_t bytes;
};

inline int nl_round_leaf(int n) { return (int)(((int64_t)n + NL_LEAF - 1) / NL_LEAF * NL_LEAF); }
inline int nl_sort_groups(int n) { return n > 0 ? (n + NL_TILE - 1) / NL_TILE : 0; }

NLTree nl_carve_tree(void* base, int Mt) {
  NLTree t = {};
  char* p = (char*)base;
  const size_t P = (size_t)nl_round_leaf(Mt);
  t.P = (int)P;
  t.parts = (float*)p; p += NL_PARTS_BYTES;
  t.recs = (float4*)p; p += P * 16;
  t.key_a = (uint64_t*)p; p += P * 8;
  t.key_b = (uint64_t*)p; p += P * 8;
  t.val_a = (uint32_t*)p; p += P * 4;
  t.val_b = (uint32_t*)p; p += P * 4;
  int n = (int)(P / NL_LEAF);
  while (n > 0 && t.levels < NL_LEVELS) {
    t.n[t.levels] = n;
    t.box[t.levels] = (float4*)p; p += (size_t)n * 32;
    ++t.levels;
    if (n <= NL_FAN) break;
    n = (n + NL_FAN - 1) / NL_FAN;
  }
  t.hist = (uint32_t*)p; p += (size_t)nl_sort_groups(Mt) * 256 * 4;
  t.bytes = (size_t)(p - (char*)base);
  return t;
}

NLSort nl_carve_sort(void* base, int Ms) {
  NLSort s = {};
  char* p = (char*)base;
  const size_t P = (size_t)nl_round_leaf(Ms);
  s.key_a = (uint64_t*)p; p += P * 8;
  s.key_b = (uint64_t*)p; p += P * 8;
  s.val_a = (uint32_t*)p; p += P * 4;
  s.val_b = (uint32_t*)p; p += P * 4;
  s.hist = (uint32_t*)p; p += (size_t)nl_sort_groups(Ms) * 256 * 4;
  s.bytes = (size_t)(p - (char*)base);
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// The one distance every decision uses: the expression of k_nn_bruteforce, operand for operand.
__device__ __forceinline__ double nl_dist2(double qx, double qy, double qz, float px, float py, float pz) {
  const double dx = qx - (double)px, dy = qy - (double)py, dz = qz - (double)pz;
  return dx * dx + dy * dy + dz * dz;
}

// Lower bound of nl_dist2 over the points of a box: the same operations on the nearest corner coordinate per axis.  fp64
// subtraction, multiplication and addition round monotonically, so this is <= nl_dist2 of every point inside, bit for bit.
__device__ __forceinline__ double nl_box_lower(double qx, double qy, double qz, float lx, float ly, float lz, float hx, float hy,
                                               float hz) {
  const double dx = fmax(fmax((double)lx - qx, qx - (double)hx), 0.0), dy = fmax(fmax((double)ly - qy, qy - (double)hy), 0.0),
               dz = fmax(fmax((double)lz - qz, qz - (double)hz), 0.0);
  return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ bool nl_finite3(float x, float y, float z) {
  return fabsf(x) <= 3.4028235e38f && fabsf(y) <= 3.4028235e38f && fabsf(z) <= 3.4028235e38f;   // false for NaN and inf
}

__device__ __forceinline__ float nl_readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

__device__ __forceinline__ float nl_wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, DL_WAVE));
  return v;
}
__device__ __forceinline__ float nl_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, DL_WAVE));
  return v;
}
__device__ __forceinline__ double nl_wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, DL_WAVE));
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Bounding box of the finite points: NL_PARTS workgroups, one partial box each (an empty one is +inf / -inf).
__global__ __launch_bounds__(DL_BLOCK) void k_nl_bbox(const float* __restrict__ pts, int64_t cs, int n, float* __restrict__ parts) {
  __shared__ float red[DL_BLOCK / DL_WAVE][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * DL_BLOCK + threadIdx.x; i < n; i += (int64_t)NL_PARTS * DL_BLOCK) {
    const float x = pts[i], y = pts[cs + i], z = pts[2 * cs + i];
    if (nl_finite3(x, y, z)) {
      lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
    }
  }
  const int w = threadIdx.x / DL_WAVE, lane = threadIdx.x % DL_WAVE;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = nl_wave_min(lo[a]); hi[a] = nl_wave_max(hi[a]);
    if (lane == 0) { red[w][a] = lo[a]; red[w][3 + a] = hi[a]; }
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int a = threadIdx.x;
    float v = 0.f;
    if (a < 3) v = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
    else if (a >= 4 && a < 7) v = fmaxf(fmaxf(red[0][a - 1], red[1][a - 1]), fmaxf(red[2][a - 1], red[3][a - 1]));
    parts[blockIdx.x * 8 + a] = v;
  }
}

__device__ __forceinline__ uint64_t nl_spread3(uint32_t v) {        // 21 bits -> every third bit of 61
  uint64_t x = v & 0x1fffffu;
  x = (x | x << 32) & 0x001f00000000ffffull;
  x = (x | x << 16) & 0x001f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

// Morton key of every point relative to the box of `parts` (clamped to it; a point with a non-finite coordinate gets the largest
// key and sorts behind all others), and the identity permutation next to it.
__global__ __launch_bounds__(DL_BLOCK) void k_nl_keys(const float* __restrict__ pts, int64_t cs, int n, const float* __restrict__ parts,
                                                      uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  __shared__ float red[DL_BLOCK / DL_WAVE][6];
  const int w = threadIdx.x / DL_WAVE, lane = threadIdx.x % DL_WAVE;
  {
    const float4 l = reinterpret_cast<const float4*>(parts)[2 * threadIdx.x], h = reinterpret_cast<const float4*>(parts)[2 * threadIdx.x + 1];
    const float v[6] = {nl_wave_min(l.x), nl_wave_min(l.y), nl_wave_min(l.z), nl_wave_max(h.x), nl_wave_max(h.y), nl_wave_max(h.z)};
    if (lane == 0)
      for (int a = 0; a < 6; ++a) red[w][a] = v[a];
  }
  __syncthreads();
  double lo[3], inv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float l = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
    const float h = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
    const double ext = (double)h - (double)l;
    const bool ok = ext > 0.0 && ext < 1e39;                        // false for an empty box and for a flat axis
    lo[a] = ok ? (double)l : 0.0;
    inv[a] = ok ? (double)((1 << NL_KEY_BITS) - 1) / ext : 0.0;
  }
  const int i = blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float x = pts[i], y = pts[cs + i], z = pts[2 * cs + i];
  uint64_t key = ~0ull;
  if (nl_finite3(x, y, z)) {
    const double top = (double)((1 << NL_KEY_BITS) - 1);
    const uint32_t cx = (uint32_t)fmin(fmax(((double)x - lo[0]) * inv[0], 0.0), top), cy = (uint32_t)fmin(fmax(((double)y - lo[1]) * inv[1], 0.0), top),
                   cz = (uint32_t)fmin(fmax(((double)z - lo[2]) * inv[2], 0.0), top);
    key = (nl_spread3(cx) << 2) | (nl_spread3(cy) << 1) | nl_spread3(cz);
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// ---------------------------------------------------------------------------------------------------------------------
// Stable LSD radix sort, 8 bits per pass.  A workgroup owns NL_TILE consecutive elements, wave w of it rows w*NL_ROWS .. of 64.
// Ranks come from ballots (the lanes of a row that share a digit find each other with eight of them; the lowest such lane keeps the
// wave's running count of the digit in LDS), so the order of equal digits is lane order, row order, wave order, workgroup order:
// stable by construction, no atomics.
__device__ __forceinline__ unsigned long long nl_match8(unsigned d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(valid && bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

// counts of the wave's digits into cnt[256] (the wave's own LDS row, zeroed by the caller)
__device__ __forceinline__ void nl_count_wave(const uint64_t* __restrict__ keys, int n, int shift, int base, volatile uint32_t* cnt) {
  const int lane = threadIdx.x % DL_WAVE;
  for (int r = 0; r < NL_ROWS; ++r) {
    const int i = base + r * DL_WAVE + lane;
    const bool valid = i < n;
    const unsigned d = valid ? (unsigned)(keys[i] >> shift) & 255u : 0u;
    const unsigned long long m = nl_match8(d, valid);
    if (valid && lane == __builtin_ctzll(m)) cnt[d] = cnt[d] + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ __launch_bounds__(DL_BLOCK) void k_nl_sort_hist(const uint64_t* __restrict__ keys, int n, int shift, uint32_t* __restrict__ hist,
                                                           int groups) {
  __shared__ uint32_t cnt[DL_BLOCK / DL_WAVE][256];
  for (int k = threadIdx.x; k < (DL_BLOCK / DL_WAVE) * 256; k += DL_BLOCK) (&cnt[0][0])[k] = 0u;
  __syncthreads();
  const int w = threadIdx.x / DL_WAVE;
  nl_count_wave(keys, n, shift, blockIdx.x * NL_TILE + w * (NL_ROWS * DL_WAVE), cnt[w]);
  __syncthreads();
  hist[(size_t)threadIdx.x * groups + blockIdx.x] = cnt[0][threadIdx.x] + cnt[1][threadIdx.x] + cnt[2][threadIdx.x] + cnt[3][threadIdx.x];
}

// exclusive prefix sum of hist[0 .. m) in place, one workgroup of 1024 threads (m = 256 x workgroups of the sort: 32 k entries for
// 262 144 elements)
__global__ __launch_bounds__(1024) void k_nl_sort_scan(uint32_t* __restrict__ hist, int64_t m) {
  __shared__ uint32_t wsum[16];
  const int64_t per = (m + 1023) / 1024, a = threadIdx.x * per, b = a + per < m ? a + per : m;
  uint32_t s = 0;
  for (int64_t k = a; k < b; ++k) s += hist[k];
  const int lane = threadIdx.x % DL_WAVE, w = threadIdx.x / DL_WAVE;
  uint32_t inc = s;
#pragma unroll
  for (int o = 1; o < DL_WAVE; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, DL_WAVE);
    if (lane >= o) inc += t;
  }
  if (lane == DL_WAVE - 1) wsum[w] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  for (int k = 0; k < w; ++k) run += wsum[k];
  for (int64_t k = a; k < b; ++k) {
    const uint32_t v = hist[k];
    hist[k] = run;
    run += v;
  }
}

__global__ __launch_bounds__(DL_BLOCK) void k_nl_sort_scatter(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int n, int shift,
                                                              const uint32_t* __restrict__ hist, int groups, uint64_t* __restrict__ keys_out,
                                                              uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t cnt[DL_BLOCK / DL_WAVE][256];
  for (int k = threadIdx.x; k < (DL_BLOCK / DL_WAVE) * 256; k += DL_BLOCK) (&cnt[0][0])[k] = 0u;
  __syncthreads();
  const int w = threadIdx.x / DL_WAVE, lane = threadIdx.x % DL_WAVE;
  const int base = blockIdx.x * NL_TILE + w * (NL_ROWS * DL_WAVE);
  nl_count_wave(keys, n, shift, base, cnt[w]);
  __syncthreads();
  {                                                                 // counts -> first output slot of (wave, digit)
    uint32_t run = hist[(size_t)threadIdx.x * groups + blockIdx.x];
#pragma unroll
    for (int k = 0; k < DL_BLOCK / DL_WAVE; ++k) {
      const uint32_t c = cnt[k][threadIdx.x];
      cnt[k][threadIdx.x] = run;
      run += c;
    }
  }
  __syncthreads();
  volatile uint32_t* mine = cnt[w];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int r = 0; r < NL_ROWS; ++r) {
    const int i = base + r * DL_WAVE + lane;
    const bool valid = i < n;
    const uint64_t key = valid ? keys[i] : 0ull;
    const unsigned d = (unsigned)(key >> shift) & 255u;
    const unsigned long long m = nl_match8(d, valid);
    const uint32_t first = valid ? mine[d] : 0u;
    __builtin_amdgcn_wave_barrier();
    if (valid && lane == __builtin_ctzll(m)) mine[d] = first + (uint32_t)__popcll(m);
    __builtin_amdgcn_wave_barrier();
    const uint32_t pos = first + (uint32_t)__popcll(m & below);
    if (valid && pos < (uint32_t)n) {                               // pos < n by construction; the test keeps a damaged histogram in bounds
      keys_out[pos] = key;
      vals_out[pos] = vals[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Leaves: the records in curve order and the exact box of each leaf's finite points (one wave per leaf).
__global__ __launch_bounds__(DL_BLOCK) void k_nl_leaves(const float* __restrict__ tgt, int64_t cs, int n, int P, const uint32_t* __restrict__ order,
                                                        float4* __restrict__ recs, float4* __restrict__ box) {
  const int i = blockIdx.x * DL_BLOCK + threadIdx.x;
  if (i >= P) return;                                               // P is a multiple of 64: whole waves leave
  float x = NAN, y = NAN, z = NAN;
  int idx = -1;
  if (i < n) {
    const uint32_t o = order[i];
    if (o < (uint32_t)n) { idx = (int)o; x = tgt[o]; y = tgt[cs + o]; z = tgt[2 * cs + o]; }
  }
  recs[i] = make_float4(x, y, z, __int_as_float(idx));
  const bool fin = nl_finite3(x, y, z);
  const float lx = nl_wave_min(fin ? x : INFINITY), ly = nl_wave_min(fin ? y : INFINITY), lz = nl_wave_min(fin ? z : INFINITY);
  const float hx = nl_wave_max(fin ? x : -INFINITY), hy = nl_wave_max(fin ? y : -INFINITY), hz = nl_wave_max(fin ? z : -INFINITY);
  if (threadIdx.x % DL_WAVE == 0) {
    box[2 * (i / NL_LEAF)] = make_float4(lx, ly, lz, 0.f);
    box[2 * (i / NL_LEAF) + 1] = make_float4(hx, hy, hz, 0.f);
  }
}

// One level up: the box of up to 64 child boxes (one wave per node).
__global__ __launch_bounds__(DL_BLOCK) void k_nl_nodes(const float4* __restrict__ child, int n_child, float4* __restrict__ box, int n_nodes) {
  const int node = blockIdx.x * (DL_BLOCK / DL_WAVE) + threadIdx.x / DL_WAVE, lane = threadIdx.x % DL_WAVE;
  if (node >= n_nodes) return;
  const int c = node * NL_FAN + lane;
  float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
  if (c < n_child) { lo = child[2 * c]; hi = child[2 * c + 1]; }
  const float lx = nl_wave_min(lo.x), ly = nl_wave_min(lo.y), lz = nl_wave_min(lo.z);
  const float hx = nl_wave_max(hi.x), hy = nl_wave_max(hi.y), hz = nl_wave_max(hi.z);
  if (lane == 0) {
    box[2 * node] = make_float4(lx, ly, lz, 0.f);
    box[2 * node + 1] = make_float4(hx, hy, hz, 0.f);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The walk.  One wave = one packet of 64 queries that are neighbours on the curve; everything below is wave-uniform control flow.
struct NLPacket {
  double qx, qy, qz;                 // NaN in lanes that hold no finite query: they never win a comparison and never vote
  double best;
  int bidx;
  float thr;                         // fp32 screen: a candidate whose fp32 distance exceeds it cannot beat or tie `best`
  bool alive;
  float fx, fy, fz;
  float plo[3], phi[3];              // the packet's box
  int seeded0, seeded1;              // leaves every lane has already tested
  float4* lds;                       // the wave's 64 records
};

__device__ __forceinline__ void nl_test_leaf(const float4* __restrict__ recs, int leaf, NLPacket& q) {
  const int lane = threadIdx.x % DL_WAVE;
  const float4 mine = recs[(size_t)leaf * NL_LEAF + lane];
  __builtin_amdgcn_wave_barrier();
  q.lds[lane] = mine;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 2
  for (int k0 = 0; k0 < NL_LEAF; k0 += 4) {
    float4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = q.lds[k0 + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // fp32 screen (4 ulp of slack are covered by the 1e-5 in thr); NaN coordinates and NaN queries fail it
      const float dx = q.fx - v[u].x, dy = q.fy - v[u].y, dz = q.fz - v[u].z;
      if (dx * dx + dy * dy + dz * dz <= q.thr) {
        const double d2 = nl_dist2(q.qx, q.qy, q.qz, v[u].x, v[u].y, v[u].z);
        const int pi = __float_as_int(v[u].w);
        if (d2 < q.best || (d2 == q.best && pi < q.bidx)) {
          q.best = d2; q.bidx = pi;
          q.thr = fmaf((float)d2, 1.0f + 1e-5f, 1e-37f);            // rounded up, also where fp32 is subnormal
        }
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
}

template <int L>
__device__ __forceinline__ void nl_walk(const NLTree& t, int parent, NLPacket& q) {
  const int lane = threadIdx.x % DL_WAVE;
  const int c0 = parent * NL_FAN;
  const int cnt = t.n[L] - c0 < NL_FAN ? t.n[L] - c0 : NL_FAN;
  // screen of the children, one per lane, against the packet's box and the packet's largest bound
  const double pmax = nl_wave_max_d(q.alive ? q.best : -1.0);
  float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
  if (lane < cnt) { lo = t.box[L][2 * (c0 + lane)]; hi = t.box[L][2 * (c0 + lane) + 1]; }
  const double gx = fmax(fmax((double)lo.x - (double)q.phi[0], (double)q.plo[0] - (double)hi.x), 0.0),
               gy = fmax(fmax((double)lo.y - (double)q.phi[1], (double)q.plo[1] - (double)hi.y), 0.0),
               gz = fmax(fmax((double)lo.z - (double)q.phi[2], (double)q.plo[2] - (double)hi.z), 0.0);
  unsigned long long mask = __ballot(lane < cnt && !(gx * gx + gy * gy + gz * gz > pmax));
  while (mask) {
    const int c = __builtin_ctzll(mask);
    mask &= mask - 1ull;
    if (L == 0 && (c0 + c == q.seeded0 || c0 + c == q.seeded1)) continue;
    const double lb = nl_box_lower(q.qx, q.qy, q.qz, nl_readlane_f(lo.x, c), nl_readlane_f(lo.y, c), nl_readlane_f(lo.z, c),
                                   nl_readlane_f(hi.x, c), nl_readlane_f(hi.y, c), nl_readlane_f(hi.z, c));
    if (!__ballot(q.alive && !(lb > q.best))) continue;             // skipped only when strictly farther than every lane's best
    if constexpr (L == 0) nl_test_leaf(t.recs, c0 + c, q);
    else nl_walk<L - 1>(t, c0 + c, q);
  }
}

__global__ __launch_bounds__(DL_BLOCK) void k_nl_walk(const float* __restrict__ src, int64_t cs, int Ms, const uint64_t* __restrict__ qkeys,
                                                      const uint32_t* __restrict__ qorder, NLTree t, int Mt, int32_t* __restrict__ nn) {
  __shared__ float4 lds[DL_BLOCK / DL_WAVE][NL_LEAF];
  const int i = blockIdx.x * DL_BLOCK + threadIdx.x;
  int qi = -1;
  if (i < Ms) {
    const uint32_t o = qorder[i];
    if (o < (uint32_t)Ms) qi = (int)o;
  }
  NLPacket q;
  q.fx = q.fy = q.fz = NAN;
  if (qi >= 0) { q.fx = src[qi]; q.fy = src[cs + qi]; q.fz = src[2 * cs + qi]; }
  q.alive = nl_finite3(q.fx, q.fy, q.fz);
  if (!q.alive) q.fx = q.fy = q.fz = NAN;
  q.qx = (double)q.fx; q.qy = (double)q.fy; q.qz = (double)q.fz;
  q.best = 1e300;                                                   // as the exhaustive kernel: nothing at or beyond it is accepted
  q.bidx = NL_NO_INDEX;
  q.thr = INFINITY;
  q.seeded0 = q.seeded1 = -1;
  q.lds = lds[threadIdx.x / DL_WAVE];
  unsigned long long todo = __ballot(q.alive);
  if (todo && t.levels > 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = a == 0 ? q.fx : a == 1 ? q.fy : q.fz;
      q.plo[a] = nl_wave_min(q.alive ? v : INFINITY);
      q.phi[a] = nl_wave_max(q.alive ? v : -INFINITY);
    }
    // seed: the leaf at the lane's own rank in the target order; the wave tests each distinct one for all lanes
    int leaf = 0;
    if (q.alive) {
      const uint64_t key = qkeys[i];
      int a = 0, b = Mt;                                            // first target key >= key
      while (a < b) {
        const int m = a + (b - a) / 2;
        if (t.key_a[m] < key) a = m + 1; else b = m;
      }
      leaf = (a < Mt ? a : Mt - 1) / NL_LEAF;
    }
    while (todo) {
      const int l = __builtin_amdgcn_readlane(leaf, __builtin_ctzll(todo));
      nl_test_leaf(t.recs, l, q);
      if (q.seeded0 < 0) q.seeded0 = l; else if (q.seeded1 < 0) q.seeded1 = l;
      todo &= ~__ballot(leaf == l);
    }
    switch (t.levels) {
      case 1: nl_walk<0>(t, 0, q); break;
      case 2: nl_walk<1>(t, 0, q); break;
      case 3: nl_walk<2>(t, 0, q); break;
      default: nl_walk<3>(t, 0, q); break;
    }
  }
  if (qi >= 0) nn[qi] = q.bidx == NL_NO_INDEX ? -1 : q.bidx;
}

// (keys, values) of `n` elements in key_a / val_a -> sorted, again in key_a / val_a (8 passes: an even number of swaps)
void nl_sort(uint64_t* key_a, uint64_t* key_b, uint32_t* val_a, uint32_t* val_b, uint32_t* hist, int n, hipStream_t st) {
  const int groups = nl_sort_groups(n);
  for (int pass = 0; pass < 8; ++pass) {
    hipLaunchKernelGGL(k_nl_sort_hist, dim3(groups), dim3(DL_BLOCK), 0, st, (const uint64_t*)key_a, n, 8 * pass, hist, groups);
    hipLaunchKernelGGL(k_nl_sort_scan, dim3(1), dim3(1024), 0, st, hist, (int64_t)256 * groups);
    hipLaunchKernelGGL(k_nl_sort_scatter, dim3(groups), dim3(DL_BLOCK), 0, st, (const uint64_t*)key_a, (const uint32_t*)val_a, n, 8 * pass,
                       (const uint32_t*)hist, groups, key_b, val_b);
    std::swap(key_a, key_b);
    std::swap(val_a, val_b);
  }
}

}  // namespace

/* see include/delora_hip.h */
extern "C" size_t dl_nn_list_tree_bytes(int32_t Mt) {
  if (Mt < 0 || Mt > NL_MAX_POINTS) return 0;
  return nl_carve_tree(nullptr, Mt).bytes;
}

extern "C" size_t dl_nn_list_query_workspace_bytes(int32_t Ms) {
  if (Ms < 0 || Ms > NL_MAX_POINTS) return 0;
  return nl_carve_sort(nullptr, Ms).bytes;
}

extern "C" int dl_nn_list_build(const float* tgt, int64_t mt_cs, int32_t Mt, void* tree, dl_stream stream) {
  if (Mt < 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_build: negative size");
  if (Mt > NL_MAX_POINTS) return dl_fail(DL_ERR_UNSUPPORTED, "dl_nn_list_build: at most %d points (got %d)", NL_MAX_POINTS, Mt);
  if (!tree || (Mt > 0 && !tgt)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_build: null pointer argument");
  if ((uintptr_t)tree & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_build: the tree buffer must be 16-byte aligned");
  if (Mt > 0 && mt_cs < Mt) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_build: column stride %lld below the count %d", (long long)mt_cs, Mt);
  hipStream_t st = (hipStream_t)stream;
  const NLTree t = nl_carve_tree(tree, Mt);
  hipLaunchKernelGGL(k_nl_bbox, dim3(NL_PARTS), dim3(DL_BLOCK), 0, st, tgt, mt_cs, Mt, t.parts);    // also for Mt == 0: queries read the box
  if (Mt == 0) return dl_check_launch("dl_nn_list_build");
  hipLaunchKernelGGL(k_nl_keys, dim3((Mt + DL_BLOCK - 1) / DL_BLOCK), dim3(DL_BLOCK), 0, st, tgt, mt_cs, Mt, (const float*)t.parts, t.key_a,
                     t.val_a);
  nl_sort(t.key_a, t.key_b, t.val_a, t.val_b, t.hist, Mt, st);
  hipLaunchKernelGGL(k_nl_leaves, dim3(t.P / DL_BLOCK + 1), dim3(DL_BLOCK), 0, st, tgt, mt_cs, Mt, t.P, (const uint32_t*)t.val_a, t.recs,
                     t.box[0]);
  for (int l = 1; l < t.levels; ++l)
    hipLaunchKernelGGL(k_nl_nodes, dim3((t.n[l] + DL_BLOCK / DL_WAVE - 1) / (DL_BLOCK / DL_WAVE)), dim3(DL_BLOCK), 0, st,
                       (const float4*)t.box[l - 1], t.n[l - 1], t.box[l], t.n[l]);
  return dl_check_launch("dl_nn_list_build");
}

extern "C" int dl_nn_list_query(const float* src, int64_t ms_cs, int32_t Ms, const float* tgt, int64_t mt_cs, int32_t Mt, const void* tree,
                                int32_t* nn, void* workspace, dl_stream stream) {
  (void)tgt; (void)mt_cs;                                           // the tree holds its own copy of the coordinates
  if (Ms < 0 || Mt < 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_query: negative size");
  if (Ms > NL_MAX_POINTS || Mt > NL_MAX_POINTS)
    return dl_fail(DL_ERR_UNSUPPORTED, "dl_nn_list_query: at most %d points per list (got %d, %d)", NL_MAX_POINTS, Ms, Mt);
  if (Ms == 0) return DL_OK;
  if (!src || !nn || !tree || !workspace) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_query: null pointer argument");
  if (((uintptr_t)tree & 15) || ((uintptr_t)workspace & 15))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_query: tree and workspace must be 16-byte aligned");
  if (ms_cs < Ms) return dl_fail(DL_ERR_INVALID_ARGUMENT, "dl_nn_list_query: column stride %lld below the count %d", (long long)ms_cs, Ms);
  hipStream_t st = (hipStream_t)stream;
  const NLTree t = nl_carve_tree(const_cast<void*>(tree), Mt);
  const NLSort s = nl_carve_sort(workspace, Ms);
  hipLaunchKernelGGL(k_nl_keys, dim3((Ms + DL_BLOCK - 1) / DL_BLOCK), dim3(DL_BLOCK), 0, st, src, ms_cs, Ms, (const float*)t.parts, s.key_a,
                     s.val_a);
  nl_sort(s.key_a, s.key_b, s.val_a, s.val_b, s.hist, Ms, st);
  hipLaunchKernelGGL(k_nl_walk, dim3((Ms + DL_BLOCK - 1) / DL_BLOCK), dim3(DL_BLOCK), 0, st, src, ms_cs, Ms, (const uint64_t*)s.key_a,
                     (const uint32_t*)s.val_a, t, Mt, nn);
  return dl_check_launch("dl_nn_list_query");
}
