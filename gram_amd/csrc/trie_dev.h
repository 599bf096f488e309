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
template <> struct StepPack<gram_user_mask_t> : std::true_type {};  // (the search and greedy steps only: per-user item masks, below)
template <typename... UI>
constexpr bool filtered() {
  static_assert(StepPack<UI...>::value, "a step kernel's trailing pack is empty, one gram_user_items_t, one StepBias, the two in that order, or one gram_user_mask_t");
  return (false || ... || std::is_same_v<UI, gram_user_items_t>);
}
// which alive test a step kernel carries: none, the lists' (two binary searches) or the mask's (two record loads)
enum : int { kFilterNone = 0, kFilterLists = 1, kFilterMask = 2 };
template <typename... UI>
constexpr int filter_kind() {
  return filtered<UI...>() ? kFilterLists : (false || ... || std::is_same_v<UI, gram_user_mask_t>) ? kFilterMask : kFilterNone;
}
__device__ __forceinline__ const gram_user_items_t* items_ptr() { return nullptr; }
__device__ __forceinline__ const gram_user_items_t* items_ptr(const gram_user_items_t& u) { return &u; }
__device__ __forceinline__ const gram_user_items_t* items_ptr(const gram_user_mask_t&) { return nullptr; }
template <typename... UI>
__device__ __forceinline__ const gram_user_mask_t* mask_ptr(const UI&...) { return nullptr; }
__device__ __forceinline__ const gram_user_mask_t* mask_ptr(const gram_user_mask_t& u) { return &u; }

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

// ---- per-user item masks (gram_user_mask_t): a user's set as a bitset over the leaf ranks, every 32-bit word with the
// number of kept leaves in front of it beside it.  count(x) = the user's kept leaves below rank x: one 8-byte load.
__device__ __forceinline__ int mask_count(const uint2* __restrict__ row, int x) {
  const uint2 r = row[x >> 5];  // {bits, before}
  return (int)r.y + __popc(r.x & ((1u << (x & 31)) - 1u));
}
// does user b keep an item below `node`?  The kept leaves inside the node's leaf range [lo, hi): two record loads, whatever the set's size
__device__ __forceinline__ bool node_alive(const gram_user_mask_t& um, int b, int node) {
  int lo = um.leaf_lo[node], hi = um.leaf_hi[node];
  lo = lo < 0 ? 0 : (lo > um.n_leaves ? um.n_leaves : lo);  // (wrong tables must not reach past the user's row: its last record
  hi = hi < 0 ? 0 : (hi > um.n_leaves ? um.n_leaves : hi);  //  is n_leaves / 32)
  const uint2* __restrict__ row = reinterpret_cast<const uint2*>(um.words) + (size_t)b * um.stride;
  return mask_count(row, hi) - mask_count(row, lo) > 0;
}

// the per-user masks of the *_mask entry points (gram_user_mask_t): every array present, at least one leaf, a row that holds its records
inline int check_mask(const gram_user_mask_t* um) {
  if (!um || !um->leaf_lo || !um->leaf_hi || !um->words || um->n_leaves < 1 || um->stride < (int64_t)um->n_leaves / 32 + 1 ||
      (reinterpret_cast<uintptr_t>(um->words) & 7))
    return GRAM_E_ARG;
  return 0;
}

// the per-user lists of the *_items entry points (gram_user_items_t): every array present, stride and mode in range
inline int check_items(const gram_user_items_t* it) {
  if (!it || !it->leaf_lo || !it->leaf_hi || !it->ranks || !it->count || it->stride < 1 || it->stride > GRAM_MAX_USER_ITEMS ||
      (it->mode != GRAM_ITEMS_EXCLUDE && it->mode != GRAM_ITEMS_ALLOW))
    return GRAM_E_ARG;
  return 0;
}

}  // namespace
