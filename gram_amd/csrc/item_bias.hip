// item_bias.hip -- the potentials of a biased beam search (gram_item_bias_table).
//
// generate(item_bias=T) adds, on every Trie edge a beam takes, the DIFFERENCE of two potentials; along a root-to-leaf path the
// differences telescope to T[item].  The potential of a leaf is its item's bias; the potential of an internal node is the largest
// bias below it (lookahead) or 0; the root and the start node are 0.  The leaves below node n are the contiguous leaf ranks
// [leaf_lo[n], leaf_hi[n]) (FlatTrie.leaf_ranges), so a node's potential is a max over a contiguous slice of the bias row, gathered
// through the leaf-rank -> candidate table.  The max runs over the ordered integer image of the floats (f2ord: a total order, -0 below
// +0), so every evaluation order returns the same bits.
//
// One launch: one lane per (row, node).  A lane walks a range of up to kLaneMax ranks itself; the longer ranges of a wave's 64
// nodes are then taken one after the other by the whole wave (64 ranks per trip, cross-lane max).  Total reads per row: the sum of
// the range lengths = the sum of the leaves' depths.  No atomics: every phi entry has one writer.
#include "common.h"
#include "trie_dev.h"

namespace {

constexpr int kLaneMax = 16;  // ranges up to this long stay on their lane (a chain-like tail: most nodes of a real Trie)

__device__ __forceinline__ uint32_t leaf_value(const float* __restrict__ row, const int32_t* __restrict__ leaf_item, int n_items, int rank) {
  const int it = leaf_item[rank];
  return f2ord(it >= 0 && it < n_items ? row[it] : 0.f);  // (a leaf that no candidate names carries no bias)
}

__global__ __launch_bounds__(256) void item_bias_table_kernel(const float* __restrict__ bias, long long bias_stride, int n_items,
                                                              const int32_t* __restrict__ leaf_item, int n_leaves,
                                                              const int32_t* __restrict__ leaf_lo, const int32_t* __restrict__ leaf_hi,
                                                              gram_trie_t tr, int start_token, int lookahead, float* __restrict__ phi) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 256 + threadIdx.x;
  const float* __restrict__ row = bias + (size_t)r * bias_stride;
  __shared__ int s_start;  // the start node, looked up once per workgroup
  if (threadIdx.x == 0) {
    const int e0 = find_child(tr, 0, start_token);
    s_start = e0 < 0 ? -1 : tr.child_node[e0];
  }
  gram_sync();
  const int start_node = s_start;
  int lo = 0, hi = 0;
  if (n > 0 && n < tr.n_nodes && n != start_node) {
    const bool leaf = tr.child_off[n + 1] == tr.child_off[n];
    if (leaf || lookahead) {
      lo = leaf_lo[n];
      hi = leaf_hi[n];
      lo = lo < 0 ? 0 : lo;  // (a wrong table must not reach past the leaf table)
      hi = hi > n_leaves ? n_leaves : hi;
    }
  }
  const int len = hi > lo ? hi - lo : 0;
  uint32_t best = 0u;  // below every float's image
  if (len <= kLaneMax)
    for (int i = lo; i < lo + len; ++i) {
      const uint32_t v = leaf_value(row, leaf_item, n_items, i);
      best = v > best ? v : best;
    }
  // the wave's long ranges, one after the other (the ballot is uniform over the wave: every lane takes every trip)
  unsigned long long todo = __ballot(len > kLaneMax);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int slo = __shfl(lo, src, 64), shi = __shfl(hi, src, 64);
    uint32_t m = 0u;
    for (int i = slo + lane; i < shi; i += 64) {
      const uint32_t v = leaf_value(row, leaf_item, n_items, i);
      m = v > m ? v : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t x = (uint32_t)__shfl_xor((int)m, o, 64);
      m = x > m ? x : m;
    }
    if (lane == src) best = m;
  }
  if (n < tr.n_nodes) phi[(size_t)r * tr.n_nodes + n] = len > 0 ? ord2f(best) : 0.f;
}

}  // namespace

extern "C" int gram_item_bias_table(const float* bias, int64_t bias_stride, int rows, int n_items, const int32_t* leaf_item, int n_leaves,
                                    const int32_t* leaf_lo, const int32_t* leaf_hi, const gram_trie_t* tr, int start_token,
                                    int lookahead, float* phi, void* stream) {
  if (!bias || !leaf_item || !leaf_lo || !leaf_hi || !tr || !tr->child_off || !tr->child_tok || !tr->child_node || !phi) return GRAM_E_ARG;
  if (rows < 1 || rows > 65535 || n_items < 1 || n_leaves < 1 || tr->n_nodes < 1) return GRAM_E_ARG;
  if (bias_stride < 0 || (rows > 1 && bias_stride < n_items)) return GRAM_E_ARG;
  hipLaunchKernelGGL(item_bias_table_kernel, dim3((tr->n_nodes + 255) / 256, rows), dim3(256), 0, (hipStream_t)stream, bias,
                     (long long)bias_stride, n_items, leaf_item, n_leaves, leaf_lo, leaf_hi, *tr, start_token, lookahead != 0 ? 1 : 0, phi);
  GRAM_CHECK_LAUNCH();
  return 0;
}
