// Inference without Python (include/delora_hip.h): the eval-mode layer walk of the pose CNN -- what models/ring_conv.py
// (RingStem, RingSegment.forward) and model_parts.FusedHeads do per forward pass -- as a plan-and-forward family on the library's own
// entry points, and the streaming scan -> pose call on top of it.  Nothing here computes: apart from the input interleave below every
// launch is one of the existing entry points', called with the operands the Python path gives it, so the results are the same bits.
#include <initializer_list>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "common.h"

// ---------------------------------------------------------------------------------------------------------------------
// Input interleave: two planar images [B][4][H][W] (independent scan strides) -> [B][H][W][8], channels 0..3 = the first image.
// One lane per pixel: eight 4-byte plane reads, each coalesced over the wave (consecutive lanes = consecutive pixels of a plane),
// and two 16-byte stores.  A bit copy: the values travel as integers.
typedef uint32_t u32x4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(DL_BLOCK) void k_interleave_pair(const uint32_t* __restrict__ prev, size_t prev_ss, const uint32_t* __restrict__ cur,
                                                              size_t cur_ss, uint32_t HW, uint32_t total, u32x4i* __restrict__ x8) {
  const uint32_t i = blockIdx.x * DL_BLOCK + threadIdx.x;            // pixel of the batch: b * HW + p
  if (i >= total) return;
  const uint32_t b = i / HW, p = i - b * HW;
  const uint32_t* a = prev + (size_t)b * prev_ss + p;
  const uint32_t* c = cur + (size_t)b * cur_ss + p;
  const u32x4i lo = {a[0], a[HW], a[2 * (size_t)HW], a[3 * (size_t)HW]};
  const u32x4i hi = {c[0], c[HW], c[2 * (size_t)HW], c[3 * (size_t)HW]};
  x8[2 * (size_t)i] = lo;
  x8[2 * (size_t)i + 1] = hi;
}

// the CSR offsets {0, n} of a single scan, written on the stream (no host copy: the call stays asynchronous and capturable)
__global__ void k_single_scan_offsets(int32_t* __restrict__ offs, int32_t n) {
  if (threadIdx.x < 2) offs[threadIdx.x] = threadIdx.x ? n : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kAlign = 256;
inline size_t align_up(size_t n) { return (n + kAlign - 1) / kAlign * kAlign; }
inline int ceil_div(int n, int s) { return (n + s - 1) / s; }

// Refusals.  Scope = ring_conv.supported / stem_supported of the Python path restricted to the 8-channel, two-MLP network.
int pose_check(const char* who, const dl_pose_net* net, int B, int H, int W) {
  if (!net) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null net", who);
  if (net->act != DL_POSE_ACT_TANH && net->act != DL_POSE_ACT_RELU)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: act=%d is not served (1 tanh, 2 relu)", who, net->act);
  if (net->n_blocks < 1 || net->n_blocks > DL_POSE_NET_MAX_BLOCKS)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: n_blocks=%d is not served (1..%d)", who, net->n_blocks, DL_POSE_NET_MAX_BLOCKS);
  if (B < 1 || H < 1 || W < 1) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
  if (B > 16) return dl_fail(DL_ERR_UNSUPPORTED, "%s: B=%d is not served (1 <= B <= 16, the bound of dl_heads_fwd)", who, B);
  if (W % 4) return dl_fail(DL_ERR_UNSUPPORTED, "%s: W=%d is not served (the stem halves the width twice: a multiple of 4)", who, W);
  if (!net->conv1_w) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: conv1_w is null", who);
  if ((uintptr_t)net->conv1_w & 15) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: conv1_w is not 16-byte aligned", who);
  if ((size_t)B * H * (W / 2) * 64 >= ((size_t)1 << 31))
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: B=%d H=%d W=%d: conv1's output reaches 2^31 elements", who, B, H, W);
  int h = H, w = W / 4, c = 64;                                       // the pooled stem output [B][H][W/4][64]
  for (int i = 0; i < net->n_blocks; ++i) {
    const dl_pose_block& b = net->blocks[i];
    if (b.cin <= 0 || b.cin % 64) return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d].cin=%d is not served (full-width networks: multiples of 64)", who, i, b.cin);
    if (b.cout <= 0 || b.cout % 64) return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d].cout=%d is not served (full-width networks: multiples of 64)", who, i, b.cout);
    if (b.cin != c) return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d].cin=%d does not continue the %d channels in front of it", who, i, b.cin, c);
    const bool s11 = b.stride_h == 1 && b.stride_w == 1;
    if (!s11 && !(b.stride_h == 1 && b.stride_w == 2) && !(b.stride_h == 2 && b.stride_w == 2))
      return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d].stride=(%d,%d) is not served ((1,1), (1,2), (2,2))", who, i, b.stride_h, b.stride_w);
    if ((b.has_downsample != 0) == s11 || (!b.has_downsample && b.cin != b.cout))
      return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d].has_downsample=%d with stride (%d,%d), %d -> %d channels is not served (the 1x1 shortcut "
                     "belongs to the strided blocks; the others keep their channels)", who, i, b.has_downsample, b.stride_h, b.stride_w, b.cin, b.cout);
    const struct { const float* p; const char* name; bool need; } ptrs[3] = {{b.w1, "w1", true}, {b.w2, "w2", true}, {b.wd, "wd", b.has_downsample != 0}};
    for (const auto& q : ptrs) {
      if (q.need && !q.p) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: blocks[%d].%s is null", who, i, q.name);
      if (q.need && ((uintptr_t)q.p & 15)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: blocks[%d].%s is not 16-byte aligned", who, i, q.name);
    }
    const size_t wide = (size_t)(b.cin > b.cout ? b.cin : b.cout);
    if ((size_t)B * h * w * wide >= ((size_t)1 << 31) || (size_t)h * w * wide >= ((size_t)1 << 30))
      return dl_fail(DL_ERR_UNSUPPORTED, "%s: blocks[%d]: B=%d on a %dx%d map with %zu channels reaches the 32-bit offsets of the convolutions", who, i, B, h, w, wide);
    h = ceil_div(h, b.stride_h); w = ceil_div(w, b.stride_w); c = b.cout;
  }
  if (net->F != c) return dl_fail(DL_ERR_UNSUPPORTED, "%s: F=%d is not the last block's %d channels", who, net->F, c);
  if (net->R < 1 || net->R > (1 << 20)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: R=%d is not served", who, net->R);
  if (net->Hd < 1 || net->Hd > (1 << 20)) return dl_fail(DL_ERR_UNSUPPORTED, "%s: Hd=%d is not served", who, net->Hd);
  const dl_heads_params& hp = net->heads;
  const struct { const float* p; const char* name; } heads[10] = {{hp.fc_w, "fc_w"}, {hp.fc_b, "fc_b"}, {hp.r1_w, "r1_w"}, {hp.r1_b, "r1_b"}, {hp.r3_w, "r3_w"},
                                                                 {hp.r3_b, "r3_b"}, {hp.t1_w, "t1_w"}, {hp.t1_b, "t1_b"}, {hp.t3_w, "t3_w"}, {hp.t3_b, "t3_b"}};
  for (const auto& q : heads)
    if (!q.p) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: heads.%s is null", who, q.name);
  return DL_OK;
}
// One trunk convolution.  The table of these records is the single statement of the layer walk: the plan sizes the workspace from it,
// prepare fills the records' ranges of `prepared`, forward runs them in order.
enum LayerKind { kWino, kDirect, kHalf };           // dl_wino_conv3x3_nhwc_f32, dl_conv2d_nhwc_f32, dl_conv2d_nhwc_h
constexpr size_t kNone = ~(size_t)0;

struct Layer {
  LayerKind kind;
  int block;                                        // error texts say blocks[block].name
  const char* name;                                 // "w1", "wd", "w2"
  const float* weight;                              // the fp32 parameter [cout][taps][cin]
  int taps, cin, cout;
  int h, w, sh, sw;                                 // input map and stride
  int in, out, add;                                 // activation slots; add < 0: no addend
  int act;
  uint32_t epilogue;
  size_t prepared;                                  // byte offset of the layer's weights in `prepared`; kNone: it reads the parameter
};

// Where everything lives.  Four rotating activation slots: the stem puts the interleaved input, conv1's output and the pooled map
// into slots 0, 1, 2; a block whose input sits in slot s writes y1 to s+1, the shortcut to s+2 and y2 to s+3 (mod 4), and y2 is the
// next block's input -- at no time more than those four tensors are alive.  A slot is as large as the largest tensor it ever holds.
struct PosePlan {
  Layer layers[3 * DL_POSE_NET_MAX_BLOCKS];         // in execution order: w1, wd, w2 per block
  int n_layers;
  int last_slot, last_hw;                           // the last block's output: its slot and its pixels per image
  size_t slot_bytes[4], slot_off[4];
  size_t win_off, split_off, feat_off, a1_off, a2_off, rot_off, norm_off, total;
  size_t split_bytes, prepared_bytes;
};

// A 3x3 layer runs as Winograd iff its stride is (1,1): inside pose_check's scope (channel counts multiples of 64) the shape rule of
// the Python plan (ring_conv.wino_ok: C % 8 == 0, K % 64 == 0) holds for every such layer, and the launch itself refuses what it cannot run.
inline bool runs_wino(int sh, int sw) { return sh == 1 && sw == 1; }

// The table and the sizes for a network pose_check has accepted.  dtype DL_DTYPE_F32: Winograd / direct layers, fp32 throughout, the
// pooling's int8 window plane and the largest split-K scratch.  Half precision (ResNetModified.pooled_features_drop inside
// torch.autocast): interleave and conv1 stay fp32 (slots 0 and 1), the pooled map and everything behind it has 2-byte elements, every
// layer is dl_conv2d_nhwc_h (one kernel family: nothing to route), no window plane, no split-K scratch.
// `prepared` offsets follow the header's layout, not the execution order: per block w1, w2, wd, those that have prepared weights --
// fp32: the Winograd layers, dl_wino_weights_floats floats each, packed; half: every layer's w_fwd [taps][K][C], each rounded up to 256 bytes.
PosePlan pose_plan(const dl_pose_net* net, int dtype, int B, int H, int W) {
  PosePlan p{};
  const bool half = dtype != DL_DTYPE_F32;
  const size_t es = half ? 2 : 4;
  auto hold = [&](int slot, size_t bytes) { if (bytes > p.slot_bytes[slot]) p.slot_bytes[slot] = bytes; };
  auto layer = [&](int block, const char* name, const float* weight, int taps, int cin, int cout, int h, int w, int sh, int sw, int in, int out, int add,
                   int act, uint32_t epilogue) {
    const LayerKind kind = half ? kHalf : taps == 9 && runs_wino(sh, sw) ? kWino : kDirect;      // the one routing decision
    Layer* l = &p.layers[p.n_layers++];
    *l = Layer{kind, block, name, weight, taps, cin, cout, h, w, sh, sw, in, out, add, act, epilogue, kNone};
    hold(out, (size_t)B * ceil_div(h, sh) * ceil_div(w, sw) * cout * es);
    if (kind == kWino) {
      const size_t n = dl_wino_conv3x3_workspace_bytes(B, h, w, cin, cout);
      if (n > p.split_bytes) p.split_bytes = n;
    }
    return l;
  };
  hold(0, (size_t)B * H * W * 8 * 4);
  hold(1, (size_t)B * H * (W / 2) * 64 * 4);
  hold(2, (size_t)B * H * (W / 4) * 64 * es);
  const size_t win_bytes = half ? 0 : (size_t)B * H * (W / 4) * 64;
  int s = 2, h = H, w = W / 4;
  for (int i = 0; i < net->n_blocks; ++i) {
    const dl_pose_block& b = net->blocks[i];
    const int y1 = (s + 1) & 3, sc = (s + 2) & 3, y2 = (s + 3) & 3;
    const int ho = ceil_div(h, b.stride_h), wo = ceil_div(w, b.stride_w);
    Layer* const l1 = layer(i, "w1", b.w1, 9, b.cin, b.cout, h, w, b.stride_h, b.stride_w, s, y1, -1, net->act, DL_CONV_ACT);
    Layer* const ld = b.has_downsample ? layer(i, "wd", b.wd, 1, b.cin, b.cout, h, w, b.stride_h, b.stride_w, s, sc, -1, 0, 0) : nullptr;
    Layer* const l2 = layer(i, "w2", b.w2, 9, b.cout, b.cout, ho, wo, 1, 1, y1, y2, ld ? sc : s, net->act, DL_CONV_ADD | DL_CONV_ACT);
    for (Layer* l : {l1, l2, ld}) {
      if (!l || l->kind == kDirect) continue;
      l->prepared = p.prepared_bytes;
      p.prepared_bytes += half ? align_up((size_t)l->taps * l->cout * l->cin * 2) : dl_wino_weights_floats(l->cout, l->cin) * sizeof(float);
    }
    s = y2; h = ho; w = wo;
  }
  p.last_slot = s; p.last_hw = h * w;
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t at = off; off += align_up(bytes); return at; };
  for (int i = 0; i < 4; ++i) p.slot_off[i] = carve(p.slot_bytes[i]);
  p.win_off = carve(win_bytes);
  p.split_off = carve(p.split_bytes);
  p.feat_off = carve((size_t)B * net->F * 4);
  p.a1_off = carve((size_t)B * net->R * 4);
  p.a2_off = carve((size_t)B * 2 * net->Hd * 4);
  p.rot_off = carve((size_t)B * 4 * 4);
  p.norm_off = carve(4);
  p.total = off;
  return p;
}

// a failing entry point keeps its own text; the caller's name and the layer go in front of it
int at_layer(const char* who, const char* what, int block, int rc) {
  if (!rc) return DL_OK;
  char inner[160];
  snprintf(inner, sizeof(inner), "%s", g_dl_err);
  if (block >= 0) return dl_fail(rc, "%s: blocks[%d].%s: %s", who, block, what, inner);
  return dl_fail(rc, "%s: %s: %s", who, what, inner);
}

int dtype_check(const char* who, int dtype) {
  if (dtype != DL_DTYPE_F16 && dtype != DL_DTYPE_BF16)
    return dl_fail(DL_ERR_UNSUPPORTED, "%s: dtype=%d is not served (1 DL_DTYPE_F16, 2 DL_DTYPE_BF16; fp32 is the family without _h)", who, dtype);
  return DL_OK;
}

// dl_pose_net_prepared_bytes / _workspace_bytes (dtype DL_DTYPE_F32) and their _h forms: 0 when the network is refused
size_t pose_sizes(const char* who, const dl_pose_net* net, int dtype, int B, int H, int W, bool workspace) {
  if (pose_check(who, net, B, H, W)) return 0;
  const PosePlan p = pose_plan(net, dtype, B, H, W);
  return workspace ? p.total : p.prepared_bytes;
}

// dl_pose_net_prepare (dtype DL_DTYPE_F32: dl_wino_weights_batch_f32, forward set only, DL_WINO_BATCH layers per launch) and
// dl_pose_net_prepare_h (dl_conv_weights_batch_h, forward layout only, DL_CONVH_BATCH per launch): every record that has a range of
// `prepared` gets it filled from its parameter
int pose_prepare(const char* who, const dl_pose_net* net, int dtype, int B, int H, int W, void* prepared, dl_stream stream) {
  if (int rc = pose_check(who, net, B, H, W)) return rc;
  if (!prepared || ((uintptr_t)prepared & (kAlign - 1))) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: prepared must be a 256-byte aligned buffer", who);
  const PosePlan p = pose_plan(net, dtype, B, H, W);
  const bool half = dtype != DL_DTYPE_F32;
  dl_wino_layer wino[DL_WINO_BATCH];
  dl_convh_layer convh[DL_CONVH_BATCH];
  int n = 0;
  auto flush = [&]() {
    const int m = n;
    n = 0;
    if (!m) return (int)DL_OK;
    if (half) return at_layer(who, "half-precision weights", -1, dl_conv_weights_batch_h(convh, m, dtype, stream));
    return at_layer(who, "Winograd weights", -1, dl_wino_weights_batch_f32(wino, m, stream));
  };
  for (int i = 0; i < p.n_layers; ++i) {
    const Layer& l = p.layers[i];
    if (l.prepared == kNone) continue;
    char* const u = (char*)prepared + l.prepared;
    if (half) convh[n++] = dl_convh_layer{l.weight, u, nullptr, l.cout, l.taps, l.cin};
    else wino[n++] = dl_wino_layer{l.weight, (float*)u, nullptr, l.cout, l.cin};
    if (n == (half ? DL_CONVH_BATCH : DL_WINO_BATCH))
      if (int rc = flush()) return rc;
  }
  return flush();
}

// The walk: in half precision what the fp32 one does with the trunk on dl_conv2d_nhwc_h and the pooling writing the storage type (the
// Python path pools in fp32 and casts: the same bits); conv1, the pooled feature, the heads and T are fp32 in both.
int pose_forward(const char* who, const dl_pose_net* net, int dtype, const PosePlan& p, const void* prepared, const float* image_prev, int64_t prev_ss,
                 const float* image_cur, int64_t cur_ss, int B, int H, int W, void* workspace, float* translation, float* quaternion, float* T,
                 dl_stream stream) {
  char* const ws = (char*)workspace;
  void* slot[4];
  for (int i = 0; i < 4; ++i) slot[i] = ws + p.slot_off[i];
  void* const split_ws = p.split_bytes ? (void*)(ws + p.split_off) : nullptr;
  const bool half = dtype != DL_DTYPE_F32;
  const int act = net->act;
  hipStream_t st = (hipStream_t)stream;
  // 1. the transposing gather (x.permute(0, 2, 3, 1).contiguous() of the stacked pair)
  const uint32_t total = (uint32_t)B * H * W;
  hipLaunchKernelGGL(k_interleave_pair, dim3((total + DL_BLOCK - 1) / DL_BLOCK), dim3(DL_BLOCK), 0, st, (const uint32_t*)image_prev, (size_t)prev_ss,
                     (const uint32_t*)image_cur, (size_t)cur_ss, (uint32_t)(H * W), total, (u32x4i*)slot[0]);
  if (int rc = dl_check_launch(who)) return rc;
  // 2. conv1 (3x3, stride (1,2)) + activation in fp32, 3. the pooling: fp32 with its window plane, or fp32 -> half
  if (int rc = at_layer(who, "conv1", -1, dl_conv2d_nhwc_f32((const float*)slot[0], net->conv1_w, (float*)slot[1], nullptr, nullptr, B, H, W, 8, 64, 3, 1, 2,
                                                            0, act, DL_CONV_ACT, stream)))
    return rc;
  if (int rc = at_layer(who, "pooling", -1, half ? dl_pool3x3s12_nhwc_fwd_h((const float*)slot[1], B, H, W / 2, 64, dtype, slot[2], stream)
                                                 : dl_pool3x3s12_nhwc_fwd((const float*)slot[1], B, H, W / 2, 64, (float*)slot[2], (int8_t*)(ws + p.win_off), stream)))
    return rc;
  // 4. the residual blocks
  for (int i = 0; i < p.n_layers; ++i) {
    const Layer& l = p.layers[i];
    const void* x = slot[l.in];
    void* y = slot[l.out];
    const void* add = l.add >= 0 ? slot[l.add] : nullptr;
    const void* u = l.prepared == kNone ? nullptr : (const char*)prepared + l.prepared;
    const int ks = l.taps == 9 ? 3 : 1;
    int rc = DL_OK;
    switch (l.kind) {
      case kWino:
        rc = dl_wino_conv3x3_nhwc_f32((const float*)x, (const float*)u, (float*)y, (const float*)add, nullptr, B, l.h, l.w, l.cin, l.cout, l.act, l.epilogue, split_ws, stream);
        break;
      case kDirect:
        rc = dl_conv2d_nhwc_f32((const float*)x, l.weight, (float*)y, (const float*)add, nullptr, B, l.h, l.w, l.cin, l.cout, ks, l.sh, l.sw, 0, l.act, l.epilogue, stream);
        break;
      case kHalf:
        rc = dl_conv2d_nhwc_h(x, u, y, add, nullptr, B, l.h, l.w, l.cin, l.cout, ks, l.sh, l.sw, 0, dtype, l.act, l.epilogue, stream);
        break;
    }
    if ((rc = at_layer(who, l.name, l.block, rc))) return rc;
  }
  // 5. global average pooling to the fp32 feature, 6. fc + heads + the whole-batch quaternion norm, 7. quaternion -> T
  float* feat = (float*)(ws + p.feat_off);
  if (int rc = at_layer(who, "pooled feature", -1, half ? dl_mean_hw_nhwc_h(slot[p.last_slot], B, p.last_hw, net->F, dtype, feat, stream)
                                                        : dl_mean_hw_nhwc_f32((const float*)slot[p.last_slot], B, p.last_hw, net->F, feat, stream)))
    return rc;
  if (int rc = at_layer(who, "heads", -1, dl_heads_fwd(feat, &net->heads, B, net->F, net->R, net->Hd, act, (float*)(ws + p.a1_off), (float*)(ws + p.a2_off),
                                                        (float*)(ws + p.rot_off), translation, quaternion, (float*)(ws + p.norm_off), stream)))
    return rc;
  return at_layer(who, "T", -1, dl_quat_to_T_fwd(translation, quaternion, B, 1e-12f, T, stream));
}

int forward_args(const char* who, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur, int64_t cur_ss, int H, int W,
                 const void* workspace, const float* translation, const float* quaternion, const float* T) {
  if (!prepared || !image_prev || !image_cur || !workspace || !translation || !quaternion || !T)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument (prepared, images, workspace, translation, quaternion, T)", who);
  if (((uintptr_t)workspace & (kAlign - 1))) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 256-byte aligned", who);
  if (((uintptr_t)prepared & (kAlign - 1))) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: prepared must be 256-byte aligned", who);
  if (((uintptr_t)image_prev & 3) || ((uintptr_t)image_cur & 3)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: an image is not 4-byte aligned", who);
  if (prev_ss < (int64_t)4 * H * W || cur_ss < (int64_t)4 * H * W)
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: scan strides prev_ss=%lld cur_ss=%lld are below the dense 4*H*W=%lld", who, (long long)prev_ss,
                   (long long)cur_ss, (long long)4 * H * W);
  return DL_OK;
}

// dl_pose_net_forward (dtype DL_DTYPE_F32) and dl_pose_net_forward_h
int pose_net_forward(const char* who, const dl_pose_net* net, int dtype, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur,
                     int64_t cur_ss, int B, int H, int W, void* workspace, float* translation, float* quaternion, float* T, dl_stream stream) {
  if (int rc = pose_check(who, net, B, H, W)) return rc;
  if (int rc = forward_args(who, prepared, image_prev, prev_ss, image_cur, cur_ss, H, W, workspace, translation, quaternion, T)) return rc;
  return pose_forward(who, net, dtype, pose_plan(net, dtype, B, H, W), prepared, image_prev, prev_ss, image_cur, cur_ss, B, H, W, workspace, translation,
                      quaternion, T, stream);
}

// workspace of the streaming calls: the forward's workspace (B = 1) | pix2pt [H*W] int32 | the projection's scratch (grows with the scan)
int odometry_check(const char* who, const dl_pose_net* net, const dl_sensor* sensor) {
  if (!sensor) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null sensor", who);
  if (sensor->H < 2 || sensor->W < 2) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sensor H=%d W=%d", who, sensor->H, sensor->W);
  return pose_check(who, net, 1, sensor->H, sensor->W);
}

// dl_odometry_workspace_bytes (dtype DL_DTYPE_F32) and dl_odometry_workspace_bytes_h
size_t odometry_workspace(const char* who, const dl_pose_net* net, int dtype, const dl_sensor* sensor, int32_t max_points, int32_t H, int32_t W) {
  if (odometry_check(who, net, sensor)) return 0;
  if (H != sensor->H || W != sensor->W || max_points < 0) {
    dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: H=%d W=%d must be the sensor's %dx%d, max_points=%d not negative", who, H, W, sensor->H, sensor->W, max_points);
    return 0;
  }
  return pose_plan(net, dtype, 1, H, W).total + align_up((size_t)H * W * 4) + align_up(dl_project_workspace_bytes(1, H, W, max_points, 3));
}

int push_alignment(const char* who, const void* workspace, const float* image_cur, const int32_t* offs) {
  if (((uintptr_t)workspace & (kAlign - 1))) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: workspace must be 256-byte aligned", who);
  if (((uintptr_t)image_cur & 3) || ((uintptr_t)offs & 3)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: image_cur / offs are not 4-byte aligned", who);
  return DL_OK;
}

// The body of the four push calls behind odometry_check and the scan's own argument checks: the CSR offsets {0, n} of the single scan,
// project(pix2pt, scratch) -- the new scan alone into image_cur -- and, from the second scan on, the forward on (image_prev, image_cur).
template <class Project>
int odometry_push_body(const char* who, int dtype, const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, int32_t n, int32_t* offs,
                       const float* image_prev, float* image_cur, void* workspace, float* translation, float* quaternion, float* T, dl_stream stream,
                       Project project) {
  const int H = sensor->H, W = sensor->W;
  const int64_t ss = (int64_t)4 * H * W;
  if (image_prev)
    if (int rc = forward_args(who, prepared, image_prev, ss, image_cur, ss, H, W, workspace, translation, quaternion, T)) return rc;
  const PosePlan p = pose_plan(net, dtype, 1, H, W);
  char* const ws = (char*)workspace;
  int32_t* pix2pt = (int32_t*)(ws + p.total);
  void* project_ws = ws + p.total + align_up((size_t)H * W * 4);
  hipLaunchKernelGGL(k_single_scan_offsets, dim3(1), dim3(64), 0, (hipStream_t)stream, offs, n);
  if (int rc = dl_check_launch(who)) return rc;
  if (int rc = at_layer(who, "projection", -1, project(pix2pt, project_ws))) return rc;
  if (!image_prev) return DL_OK;
  return pose_forward(who, net, dtype, p, prepared, image_prev, ss, image_cur, ss, 1, H, W, workspace, translation, quaternion, T, stream);
}

// dl_odometry_push (dtype DL_DTYPE_F32) and dl_odometry_push_h
int odometry_push(const char* who, int dtype, const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const float* pts, int64_t pts_cs,
                  int32_t n_points, int32_t* offs, const float* image_prev, float* image_cur, void* workspace, float* translation, float* quaternion,
                  float* T, dl_stream stream) {
  if (int rc = odometry_check(who, net, sensor)) return rc;
  if (!offs || !image_cur || !workspace || (!pts && n_points > 0)) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument (pts, offs, image_cur, workspace)", who);
  if (n_points < 0 || pts_cs < n_points) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes n_points=%d pts_cs=%lld", who, n_points, (long long)pts_cs);
  if (int rc = push_alignment(who, workspace, image_cur, offs)) return rc;
  return odometry_push_body(who, dtype, net, prepared, sensor, n_points, offs, image_prev, image_cur, workspace, translation, quaternion, T, stream,
                            [&](int32_t* pix2pt, void* project_ws) {
                              return dl_project(pts, pts_cs, n_points, offs, 1, 3, n_points, sensor, image_cur, nullptr, nullptr, nullptr, pix2pt, project_ws,
                                                nullptr, nullptr, stream);
                            });
}

// dl_odometry_push_records (dtype DL_DTYPE_F32) and dl_odometry_push_records_h; the projection's scratch is the key plane alone:
// dl_odometry_workspace_bytes with max_points = 0
int odometry_push_records(const char* who, int dtype, const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const void* records,
                          int32_t n_records, const dl_record_layout* layout, int32_t* offs, const float* image_prev, float* image_cur, void* workspace,
                          float* translation, float* quaternion, float* T, dl_stream stream) {
  if (int rc = odometry_check(who, net, sensor)) return rc;
  if (!offs || !image_cur || !workspace || !layout || (!records && n_records > 0))
    return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: null pointer argument (records, layout, offs, image_cur, workspace)", who);
  if (n_records < 0) return dl_fail(DL_ERR_INVALID_ARGUMENT, "%s: bad sizes n_records=%d", who, n_records);
  if (int rc = push_alignment(who, workspace, image_cur, offs)) return rc;
  if (int rc = dl_record_layout_check(who, records, layout)) return rc;
  return odometry_push_body(who, dtype, net, prepared, sensor, n_records, offs, image_prev, image_cur, workspace, translation, quaternion, T, stream,
                            [&](int32_t* pix2pt, void* project_ws) {
                              return dl_project_records(records, n_records, layout, offs, 1, n_records, sensor, image_cur, nullptr, pix2pt, project_ws, nullptr,
                                                        nullptr, stream);
                            });
}

}  // namespace

/* The entry points (see include/delora_hip.h): the fp32 family passes DL_DTYPE_F32 to the shared bodies, the _h family checks its dtype first. */
extern "C" size_t dl_pose_net_prepared_bytes(const dl_pose_net* net, int32_t B, int32_t H, int32_t W) {
  return pose_sizes("dl_pose_net_prepared_bytes", net, DL_DTYPE_F32, B, H, W, false);
}

extern "C" size_t dl_pose_net_prepared_bytes_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype) {
  const char* who = "dl_pose_net_prepared_bytes_h";
  return dtype_check(who, dtype) ? 0 : pose_sizes(who, net, dtype, B, H, W, false);
}

extern "C" size_t dl_pose_net_workspace_bytes(const dl_pose_net* net, int32_t B, int32_t H, int32_t W) {
  return pose_sizes("dl_pose_net_workspace_bytes", net, DL_DTYPE_F32, B, H, W, true);
}

extern "C" size_t dl_pose_net_workspace_bytes_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype) {
  const char* who = "dl_pose_net_workspace_bytes_h";
  return dtype_check(who, dtype) ? 0 : pose_sizes(who, net, dtype, B, H, W, true);
}

extern "C" int dl_pose_net_prepare(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, void* prepared, dl_stream stream) {
  return pose_prepare("dl_pose_net_prepare", net, DL_DTYPE_F32, B, H, W, prepared, stream);
}

extern "C" int dl_pose_net_prepare_h(const dl_pose_net* net, int32_t B, int32_t H, int32_t W, int32_t dtype, void* prepared, dl_stream stream) {
  const char* who = "dl_pose_net_prepare_h";
  if (int rc = dtype_check(who, dtype)) return rc;
  return pose_prepare(who, net, dtype, B, H, W, prepared, stream);
}

extern "C" int dl_pose_net_forward(const dl_pose_net* net, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur,
                                   int64_t cur_ss, int32_t B, int32_t H, int32_t W, void* workspace, float* translation, float* quaternion, float* T,
                                   dl_stream stream) {
  return pose_net_forward("dl_pose_net_forward", net, DL_DTYPE_F32, prepared, image_prev, prev_ss, image_cur, cur_ss, B, H, W, workspace, translation,
                          quaternion, T, stream);
}

extern "C" int dl_pose_net_forward_h(const dl_pose_net* net, const void* prepared, const float* image_prev, int64_t prev_ss, const float* image_cur,
                                     int64_t cur_ss, int32_t B, int32_t H, int32_t W, int32_t dtype, void* workspace, float* translation,
                                     float* quaternion, float* T, dl_stream stream) {
  const char* who = "dl_pose_net_forward_h";
  if (int rc = dtype_check(who, dtype)) return rc;
  return pose_net_forward(who, net, dtype, prepared, image_prev, prev_ss, image_cur, cur_ss, B, H, W, workspace, translation, quaternion, T, stream);
}

extern "C" size_t dl_odometry_workspace_bytes(const dl_pose_net* net, const dl_sensor* sensor, int32_t max_points, int32_t H, int32_t W) {
  return odometry_workspace("dl_odometry_workspace_bytes", net, DL_DTYPE_F32, sensor, max_points, H, W);
}

extern "C" size_t dl_odometry_workspace_bytes_h(const dl_pose_net* net, const dl_sensor* sensor, int32_t max_points, int32_t H, int32_t W, int32_t dtype) {
  const char* who = "dl_odometry_workspace_bytes_h";
  return dtype_check(who, dtype) ? 0 : odometry_workspace(who, net, dtype, sensor, max_points, H, W);
}

extern "C" int dl_odometry_push(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const float* pts, int64_t pts_cs, int32_t n_points,
                                int32_t* offs, const float* image_prev, float* image_cur, void* workspace, float* translation, float* quaternion,
                                float* T, dl_stream stream) {
  return odometry_push("dl_odometry_push", DL_DTYPE_F32, net, prepared, sensor, pts, pts_cs, n_points, offs, image_prev, image_cur, workspace, translation,
                       quaternion, T, stream);
}

extern "C" int dl_odometry_push_h(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const float* pts, int64_t pts_cs, int32_t n_points,
                                  int32_t* offs, const float* image_prev, float* image_cur, int32_t dtype, void* workspace, float* translation,
                                  float* quaternion, float* T, dl_stream stream) {
  const char* who = "dl_odometry_push_h";
  if (int rc = dtype_check(who, dtype)) return rc;
  return odometry_push(who, dtype, net, prepared, sensor, pts, pts_cs, n_points, offs, image_prev, image_cur, workspace, translation, quaternion, T, stream);
}

extern "C" int dl_odometry_push_records(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const void* records, int32_t n_records,
                                        const dl_record_layout* layout, int32_t* offs, const float* image_prev, float* image_cur, void* workspace,
                                        float* translation, float* quaternion, float* T, dl_stream stream) {
  return odometry_push_records("dl_odometry_push_records", DL_DTYPE_F32, net, prepared, sensor, records, n_records, layout, offs, image_prev, image_cur,
                               workspace, translation, quaternion, T, stream);
}

extern "C" int dl_odometry_push_records_h(const dl_pose_net* net, const void* prepared, const dl_sensor* sensor, const void* records, int32_t n_records,
                                          const dl_record_layout* layout, int32_t* offs, const float* image_prev, float* image_cur, int32_t dtype,
                                          void* workspace, float* translation, float* quaternion, float* T, dl_stream stream) {
  const char* who = "dl_odometry_push_records_h";
  if (int rc = dtype_check(who, dtype)) return rc;
  return odometry_push_records(who, dtype, net, prepared, sensor, records, n_records, layout, offs, image_prev, image_cur, workspace, translation,
                               quaternion, T, stream);
}
