// self_attn_row.h -- the causal decoder self-attention of one query row, written once for its three kernels: dec_self_attn_kernel
// (dec_attn.hip: one cached decode step), dec_self_attn_tf_kernel (tf_attn.hip: whole label sequences) and dec_self_attn_tree_kernel
// (tree_attn.hip: one row per Trie node).  16 lanes per query, 4 dims of the head per lane.  All three share the arithmetic: Q, K and V
// as the fp32 sum of their pieces, smallest first (sa_sum, sa_load); one position of the online softmax over positions 0..t in order
// (sa_step); 1 / l and the piece split of the output (sa_store).  The kernels keep what is their own: where a position's K and V come
// from (the cache through the ancestor table, LDS, the ancestors' q|k|v rows) and which rows a workgroup serves.
// hipcc decides per call site, and per unrolled copy of a call site, whether a * b + c becomes one fused operation: the same source came
// out fused for two of the four accumulators in one kernel and for all four in another.  So contraction is off in these functions and
// every fused operation is an fmaf: a prefix gives the same bits whichever kernel computes it, however that kernel's loop is scheduled,
// because the arithmetic is this one text.
#pragma once
#include "common.h"

namespace {

// x as an fp32 value in a register: what is computed into it is rounded to fp32 before anything converts it further (the compiler
// otherwise folds a product and its conversion to 16 bits into one mixed-precision instruction, which rounds once)
__device__ __forceinline__ float in_f32(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

// four values as the fp32 sum of their pieces, smallest first (exact for two pieces)
template <int S>
__device__ __forceinline__ void sa_sum(const p16x4 (&x)[S], float (&v)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = 0.f;
#pragma unroll
  for (int pc = S - 1; pc >= 0; --pc)
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)x[pc][e];
}
// the same of the pieces at p, ps elements apart
template <int S>
__device__ __forceinline__ void sa_load(const p16* __restrict__ p, long ps, float (&v)[4]) {
  p16x4 x[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) x[pc] = *reinterpret_cast<const p16x4*>(p + pc * ps);
  sa_sum<S>(x, v);
}

// One position of the online softmax: the score of (qf, kj) summed over the query's 16 lanes plus the bias of the distance; (m, l, acc)
// take the position in.  Every lane of the 16 must be here.
__device__ __forceinline__ void sa_step(const float (&qf)[4], const float (&kj)[4], const float (&vj)[4], float bias_d, float& m, float& l,
                                        float (&acc)[4]) {
#pragma clang fp contract(off)
  float s = qf[0] * kj[0] + qf[1] * kj[1] + qf[2] * kj[2] + qf[3] * kj[3];  // four products, three additions: nothing fused
  s += __shfl_xor(s, 1, 64);
  s += __shfl_xor(s, 2, 64);
  s += __shfl_xor(s, 4, 64);
  s += __shfl_xor(s, 8, 64);
  s += bias_d;
  const float mn = fmaxf(m, s);
  const float alpha = __expf(m - mn);
  const float p = __expf(s - mn);
  m = mn;
  l = fmaf(l, alpha, p);
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = fmaf(acc[e], alpha, p * vj[e]);
}

// acc / l as S pieces -> columns n..n + 3 of the output row orow (S == 2: an interleaved row [2 * inner], the O GEMM's A operand).
// acc * inv is rounded to fp32 and then to 16 bits; the second piece is what the first left of it, the product unrounded.
template <int S>
__device__ __forceinline__ void sa_store(p16* __restrict__ orow, int n, float l, const float (&acc)[4]) {
#pragma clang fp contract(off)
  const float inv = 1.f / l;
  p16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (p16)in_f32(acc[e] * inv);
  *reinterpret_cast<p16x4*>(orow + (S == 2 ? inter_off(n, 0) : n)) = o;
  if constexpr (S == 2) {
    p16x4 o1;
#pragma unroll
    for (int e = 0; e < 4; ++e) o1[e] = (p16)in_f32(fmaf(acc[e], inv, -(float)o[e]));
    *reinterpret_cast<p16x4*>(orow + inter_off(n, 1)) = o1;
  }
}

}  // namespace
