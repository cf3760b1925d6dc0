// Merged weight-gradient launches: what every family of them shares.  A family -- direct fp32 (conv.hip), half precision
// (wgradh.hip), Winograd and pixel-pair Winograd (wino.hip) -- supplies its kernel argument struct, the validation of a layer with its
// error text, the tiles / chunks arithmetic, a key per item (its kernel instantiation), the sort weight, the kernel dispatch and the names
// in the profile tag.  Grouping by key, the slab plan per group, the workspace carving, the launch order inside a group and the tables
// of the launches are here, once.
#ifndef DELORA_WGRAD_BATCH_H
#define DELORA_WGRAD_BATCH_H
#include <algorithm>
#include <vector>

#include "common.h"

// --------------------------------------------------------------------------------------------------------------------- device
// Which table entry a workgroup belongs to: first[] holds the prefix sums of the entries' block counts (first[n] = the grid).  The loop is
// unrolled over the table's capacity, so the table is read at constant offsets of the kernel arguments.
template <int CAP>
__device__ __forceinline__ int dl_table_slot(const int (&first)[CAP + 1], int n, int block) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < CAP; ++i)
    if (i < n && block >= first[i]) l = i;
  return l;
}

// dw = sum of the slab partials in a fixed order (slab 0, 1, 2, ... per element: deterministic), four elements from index i.  Eight
// slabs are loaded per trip so that eight independent 16-byte loads are in flight per lane -- the one-load-per-trip form ran at 1.7 TB/s.
__device__ __forceinline__ void dl_slab_sum_body(const float* __restrict__ part, int nslabs, size_t count, float* __restrict__ dw, size_t i) {
  typedef float f32x4 __attribute__((ext_vector_type(4)));
  if (i >= count) return;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= nslabs; k += 8) {
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(part + (size_t)(k + u) * count + i));
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < nslabs; ++k) s += __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(part + (size_t)k * count + i));
  *reinterpret_cast<f32x4*>(dw + i) = s;
}

// ----------------------------------------------------------------------------------------------------------------------- host
// Slab plan of one item of a table: every one of its `tiles` output tiles is reduced by nslabs workgroups of chunks_per_slab pixel chunks.
struct DlSlabPlan {
  int tiles;
  int total_chunks;       // chunks of one tile
  int plan_chunks;        // what the planner is told: total_chunks, or fewer for an item whose chunks are cheaper than the table's others
  int chunks_per_slab, nslabs;
};

// What the helpers read and write of an item; a family's item derives from it and adds its kernel arguments.
struct DlBatchItem {
  DlSlabPlan p;
  int key;                // items with one key share a launch
  size_t plane;           // floats of one slab partial (= of the summed result)
  float* part;            // carved: nslabs partials -- the result itself when there is one slab
  float* sum;             // the result: given by the family (in place) or carved behind the partials (a plane of its own)
  double flop, bytes;     // for the profile tag of the item's launch
};

// The rule of the single-layer entry points: enough slabs for `slots` workgroups, as equal as whole chunks allow.
static inline DlSlabPlan dl_single_slabs(int total_chunks, int tiles, int slots) {
  int want = (slots + tiles - 1) / tiles;
  if (want > total_chunks) want = total_chunks;
  if (want < 1) want = 1;
  const int per = (total_chunks + want - 1) / want;
  return DlSlabPlan{tiles, total_chunks, total_chunks, per, (total_chunks + per - 1) / per};
}

// Slab plans of a table: the items of each key (in key_order; keys without items are passed over) are planned together by dl_plan_batch.
// The planner never returns more slabs than the chunks it was told of; an item with plan_chunks < total_chunks keeps that bound too.
template <class Item>
void dl_plan_slabs(std::vector<Item>& items, const std::vector<int>& key_order, int slots, int partial_cost) {
  for (int key : key_order) {
    std::vector<int> tl, ch, idx;
    for (size_t i = 0; i < items.size(); ++i)
      if (items[i].key == key) { tl.push_back(items[i].p.tiles); ch.push_back(items[i].p.plan_chunks); idx.push_back((int)i); }
    if (idx.empty()) continue;
    std::vector<int> ns(idx.size());
    dl_plan_batch(tl.data(), ch.data(), (int)idx.size(), slots, partial_cost, ns.data());
    for (size_t j = 0; j < idx.size(); ++j) {
      DlSlabPlan& p = items[idx[j]].p;
      const int want = ns[j] < p.total_chunks ? ns[j] : p.total_chunks;
      p.chunks_per_slab = (p.total_chunks + want - 1) / want;
      p.nslabs = (p.total_chunks + p.chunks_per_slab - 1) / p.chunks_per_slab;
    }
  }
}

template <class Item>
std::vector<int> dl_keys_as_they_appear(const std::vector<Item>& items) {
  std::vector<int> keys;
  for (const auto& it : items) if (std::find(keys.begin(), keys.end(), it.key) == keys.end()) keys.push_back(it.key);
  return keys;
}

// Workspace of a table, in item order: partials only for the items that were split; with sum_plane a plane for the result behind them
// (the Winograd families: a further pass reads it), without one the family's own `sum` (a single slab then writes the result in place).
// Returns the floats used, base included; ws == nullptr only counts (the *_workspace_bytes queries).
template <class Item>
size_t dl_carve_workspace(std::vector<Item>& items, float* ws, bool sum_plane, size_t base_floats) {
  size_t off = 0;
  for (auto& it : items) {
    const bool split = it.p.nslabs > 1;
    if (split) { it.part = ws ? ws + off : nullptr; off += (size_t)it.p.nslabs * it.plane; }
    if (sum_plane) { it.sum = ws ? ws + off : nullptr; off += it.plane; }
    if (!split) it.part = it.sum;
  }
  return base_floats + off;
}

// One launch = the items of one key, ordered (stably) by decreasing weight -- the family's measure of time per workgroup -- so that the
// long workgroups start first.  Fills b.layer[], b.first_wg[], b.n from Item::args() and returns the grid with the summed work.
struct DlGroupWork {
  int wgs;
  double flop, bytes;
};
template <class Item, class Args, class Weight>
DlGroupWork dl_fill_group(const std::vector<Item>& items, int key, Weight weight, Args& b, std::vector<const Item*>& grp) {
  grp.clear();
  for (const auto& it : items) if (it.key == key) grp.push_back(&it);
  std::stable_sort(grp.begin(), grp.end(), [&](const Item* x, const Item* y) { return weight(*x) > weight(*y); });
  DlGroupWork w{0, 0.0, 0.0};
  b.n = (int)grp.size();
  for (int i = 0; i < b.n; ++i) {
    b.layer[i] = grp[i]->args();
    b.first_wg[i] = w.wgs;
    w.wgs += grp[i]->p.tiles * grp[i]->p.nslabs;
    w.flop += grp[i]->flop; w.bytes += grp[i]->bytes;
  }
  b.first_wg[b.n] = w.wgs;
  return w;
}

// Table of a pass behind the main launch (slab sum: the items that were split; output transform: all): entry(t, slot, item) fills the
// slot's fields and returns its thread count.  Fills t.first_block[], t.n; returns the grid in blocks of `threads`.
template <class Item, class Args, class Entry>
int dl_fill_post(const std::vector<Item>& items, bool split_only, int threads, Args& t, Entry entry) {
  int blocks = 0;
  t.n = 0;
  for (const auto& it : items) {
    if (split_only && it.p.nslabs <= 1) continue;
    t.first_block[t.n] = blocks;
    blocks += (int)((entry(t, t.n, it) + threads - 1) / threads);
    ++t.n;
  }
  t.first_block[t.n] = blocks;
  return blocks;
}
#endif
