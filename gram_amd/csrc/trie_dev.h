// trie_dev.h -- device helpers on the flat Trie and the per-user item filters that the search step (beam.hip) and the sampling step
// (sample.hip) share: one definition of "child of a node", of the order-preserving integer image of a float and of "alive for a user".
#pragma once

#include <type_traits>

#include "common.h"

namespace {

__device__ __forceinline__ uint32_t f2ord(float f) {
  uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) {
  uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __uint_as_float(u);
}

// index of tok among node's children, or -1
__device__ int find_child(const gram_trie_t& tr, int node, int tok) {
  if (node < 0) return -1;
  int lo = tr.child_off[node], hi = tr.child_off[node + 1];
  while (lo < hi) {
    int mid = (lo + hi) >> 1;
    int v = tr.child_tok[mid];
    if (v == tok) return mid;
    if (v < tok) lo = mid + 1; else hi = mid;
  }
  return -1;
}

// ---- per-user item filters (gram_user_items_t).  FILT is a compile-time property of the step kernels: the unfiltered instantiations
// carry none of this.  node_alive below is the ONE definition of "alive" that the search step's key builders, its ranked walk and
// filler loop, the greedy step and the sampling step all share.
// A step kernel's filter is in its trailing parameter pack UI: nothing (unfiltered: the parameter list and the code of a kernel
// without the pack) or one gram_user_items_t (FILT).  (The search step's pack can end with one more operand, step_dev.h's StepBias.)
struct StepBias;  // (defined in step_dev.h)
template <typename... UI>
struct StepPack : std::false_type {};  // the packs a step kernel may carry, exactly:
template <> struct StepPack<> : std::true_type {};
template <> struct StepPack<gram_user_items_t> : std::true_type {};
template <> struct StepPack<StepBias> : std::true_type {};
template <> struct StepPack<gram_user_items_t, StepBias> : std::true_type {};
template <typename... UI>
constexpr bool filtered() {
  static_assert(StepPack<UI...>::value, "a step kernel's trailing pack is empty, one gram_user_items_t, one StepBias, or the two in that order");
  return (false || ... || std::is_same_v<UI, gram_user_items_t>);
}
__device__ __forceinline__ const gram_user_items_t* items_ptr() { return nullptr; }
__device__ __forceinline__ const gram_user_items_t* items_ptr(const gram_user_items_t& u) { return &u; }

// first index in r[0, n) whose value is >= v
__device__ __forceinline__ int rank_lower_bound(const int32_t* __restrict__ r, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (r[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// does user b keep an item below `node`?  c = the user's ranks inside the node's leaf range [lo, hi): allow mode keeps the node
// iff c > 0, exclude mode iff some leaf of the range is not listed (the ranks are distinct: c <= hi - lo)
__device__ __forceinline__ bool node_alive(const gram_user_items_t& ui, int b, int node) {
  const int lo = ui.leaf_lo[node], hi = ui.leaf_hi[node];
  const int32_t* __restrict__ r = ui.ranks + (size_t)b * ui.stride;
  int n = ui.count[b];
  n = n < 0 ? 0 : (n > ui.stride ? ui.stride : n);  // (a wrong count must not reach past the user's row)
  const int c = rank_lower_bound(r, n, hi) - rank_lower_bound(r, n, lo);
  return ui.mode == GRAM_ITEMS_ALLOW ? c > 0 : c < hi - lo;
}

// the per-user lists of the *_items entry points (gram_user_items_t): every array present, stride and mode in range
inline int check_items(const gram_user_items_t* it) {
  if (!it || !it->leaf_lo || !it->leaf_hi || !it->ranks || !it->count || it->stride < 1 || it->stride > GRAM_MAX_USER_ITEMS ||
      (it->mode != GRAM_ITEMS_EXCLUDE && it->mode != GRAM_ITEMS_ALLOW))
    return GRAM_E_ARG;
  return 0;
}

}  // namespace
