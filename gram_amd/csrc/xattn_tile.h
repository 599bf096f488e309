// xattn_tile.h -- what the cross-attention kernels of dec_attn.hip (<= 4096 fused keys) and xattn_long.hip (<= 16 384) share: the
// LDS-DMA of a 32-key step's K / V^T tiles, the tiles' bank-conflict swizzles, the row lookup and the piece store.
#pragma once
#include "common.h"

namespace {

// LDS-DMA through inline asm (see gemm.hip: the builtin makes hipcc wait lgkmcnt(0) in front of every DMA)
__device__ __forceinline__ void dma16(uint32_t lds_addr /*wave-uniform*/, uint32_t voff, const char* base /*uniform*/) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory");
}
// the same with the streaming (nontemporal) hint: the bank is read once per step and never again before the next step's sweep
__device__ __forceinline__ void dma16_nt(uint32_t lds_addr /*wave-uniform*/, uint32_t voff, const char* base /*uniform*/) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %1, %2 nt" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// K tile [32 keys][128 B]: 16-B chunk ch of key row r sits at position ch ^ ksw(r).  A fragment read touches the 16 rows
// 8a + b (+ 4t), a, b = 0..3: (b >> 1, a) gives 8 distinct swizzles, b & 1 the other half of the banks -> conflict-free.
__device__ __forceinline__ int ksw(int row) { return ((row >> 1) & 1) | (((row >> 3) & 3) << 1); }
// V^T tile [64 d][64 B]: chunk ch of row d at position ch ^ F[(d >> 2) & 3], F = {0, 2, 3, 1} (16 consecutive rows, one chunk)
__device__ __forceinline__ int vsw(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }

constexpr int XA_TILE = 4096;  // one K tile or one V^T tile of a 32-key step, per piece

// The running sum of the online softmax, whose rounding depends on an fma-contraction decision, spelled out once for every kernel
// (every instantiation must return the same bits for the same (user, head) -- a user's result does not depend on the batch
// it is scored in -- and hipcc decides contraction per call site).
__device__ __forceinline__ float xa_l_update(float l, float alpha, float ps) { return __builtin_fmaf(l, alpha, ps); }

// row of q / out that holds `beam` of user b: -1 = no such beam, or (live-row step) the beam is not live
template <bool LIVE>
__device__ __forceinline__ int xa_row(int b, int K, int beam, const int32_t* __restrict__ rowpos) {
  int row = beam < K ? b * K + beam : -1;
  if constexpr (LIVE) {
    if (row >= 0) row = rowpos[row];
  }
  return row;
}
// four output columns from n of row `orow`, as S pieces (the plain running remainder: batch invariance depends on these bits)
template <int S>
__device__ __forceinline__ void xa_store(p16* __restrict__ out, int orow, int inner, int n, f32x4 v) {
#pragma unroll
  for (int pc = 0; pc < S; ++pc) {
    p16x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = (p16)v[e];
      v[e] -= (float)r[e];
    }
    // (S == 2: interleaved rows [2 * inner], the O GEMM's A operand)
    *reinterpret_cast<p16x4*>(out + (size_t)orow * inner * S + (S == 2 ? inter_off(n, pc) : n)) = r;
  }
}

}  // namespace
