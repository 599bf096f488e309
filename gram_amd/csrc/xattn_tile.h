// xattn_tile.h -- the 32-key step of the cross-attention, written once for its four kernels: cross_attn_kernel and
// cross_attn_runs_kernel (dec_attn.hip, <= 4096 fused keys), cross_attn_long_kernel (xattn_long.hip, <= 16 384) and
// cross_attn_probs_kernel (xattn_probs.hip, no V).  All four share the arithmetic: S^T = K Q^T (xa_scores), the online softmax with the
// piece split of exp(S^T) (xa_row_max, xa_l_update, xa_step_qk), O^T += V^T P^T (xa_step_pv); the LDS-DMA instruction, the tiles'
// bank-conflict swizzles, the row lookup and the piece store.  The two kernels of dec_attn.hip also share the key-step setup
// (xa_key_steps), the DMA issue (xa_issue_k / xa_issue_v) and the fragment reads (xa_read_k / xa_read_v).  The kernels keep what is
// their own: the loop over the steps and how these are dealt to the waves, the waits and barriers, the merges and the stores.
// Everything is a forceinline function over references to the caller's register arrays; a row's bits are the same in every kernel
// because the arithmetic is this one text.  Where a kernel spells a piece out that others share, a comment there says why.
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

// 4 * S DMA instructions each: the step's K tiles (streaming hint: measured) / V^T tiles of every piece -> the stage
// at LDS address dst, whose pieces are PSTR bytes apart (K tile first, V^T tile XA_TILE behind it); kb / vt: the (user, head)'s bank slices
template <int S, int PSTR>
__device__ __forceinline__ void xa_issue_k(uint32_t dst, const char* kb, long bank_pstride, int step, const uint32_t (&koff)[4]) {
#pragma unroll
  for (int pc = 0; pc < S; ++pc) {
    const char* kbase = kb + (size_t)pc * bank_pstride * 2 + (size_t)step * (32 * 128);
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16_nt(dst + pc * PSTR + i * 1024, koff[i], kbase);
  }
}
template <int S, int PSTR>
__device__ __forceinline__ void xa_issue_v(uint32_t dst, const char* vt, long bank_pstride, int step, const uint32_t (&voff)[4]) {
#pragma unroll
  for (int pc = 0; pc < S; ++pc) {
    const char* vbase = vt + (size_t)pc * bank_pstride * 2 + (size_t)step * 4096;
#pragma unroll
    for (int i = 0; i < 4; ++i) dma16(dst + pc * PSTR + XA_TILE + i * 1024, voff[i], vbase);
  }
}

// The step's K / V^T fragments, pulled out of the stage at stg (pieces PSTR apart) into registers: the arithmetic works on registers only,
// so a half of the stage is re-filled as soon as its reads have returned.  Lane (c, g) = (lane & 15, lane >> 4).
template <int S, int PSTR>
__device__ __forceinline__ void xa_read_k(const char* stg, int c, int g, p16x8 (&kf)[S][2][2]) {
  const int krow = 8 * (c >> 2) + (c & 3);  // + 4t: key row of S^T tile t this lane feeds
#pragma unroll
  for (int pc = 0; pc < S; ++pc)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) {
        const int r = krow + 4 * t;
        kf[pc][t][kd] = *reinterpret_cast<const p16x8*>(stg + pc * PSTR + r * 128 + (((g + 4 * kd) ^ ksw(r)) << 4));
      }
}
template <int S, int PSTR>
__device__ __forceinline__ void xa_read_v(const char* stg, int c, int g, p16x8 (&vf)[S][4]) {
#pragma unroll
  for (int pc = 0; pc < S; ++pc)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int d = 16 * mt + c;
      vf[pc][mt] = *reinterpret_cast<const p16x8*>(stg + pc * PSTR + XA_TILE + d * 64 + ((g ^ vsw(d)) << 4));
    }
}

// The running sum of the online softmax, whose rounding depends on an fma-contraction decision, spelled out once for every kernel
// (every instantiation must return the same bits for the same (user, head) -- a user's result does not depend on the batch
// it is scored in -- and hipcc decides contraction per call site).
__device__ __forceinline__ float xa_l_update(float l, float alpha, float ps) { return __builtin_fmaf(l, alpha, ps); }

// bit j of the word = byte j of the 32 mask bytes at p != 0: a 32-key step's key bits
__device__ __forceinline__ uint32_t xa_pack32(const uint8_t* p32) {
  const uint4* p = reinterpret_cast<const uint4*>(p32);
  const uint4 a = p[0], c2 = p[1];
  const uint32_t w8[8] = {a.x, a.y, a.z, a.w, c2.x, c2.y, c2.z, c2.w};
  uint32_t bits = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) bits |= ((w8[i] >> (8 * j)) & 0xffu) ? (1u << (4 * i + j)) : 0u;
  return bits;
}
// Key-step setup of a user whose key bits fit two words per lane (<= 4096 keys): this lane's words kb0, kb1 (steps lane and lane + 64),
// either precomputed once per generate (gram_mask_key_bits) or packed here from the mask bytes mk, and the wave-uniform sets v0, v1 of
// the steps that hold a valid key.  A user with no valid key at all keeps every step: the reference's softmax over all-finfo.min
// scores is uniform over all S keys.
__device__ __forceinline__ void xa_key_steps(const uint32_t* __restrict__ key_bits, const uint8_t* __restrict__ mk, int b, int nsteps,
                                             int lane, uint32_t& kb0, uint32_t& kb1, unsigned long long& v0, unsigned long long& v1) {
  kb0 = 0, kb1 = 0;
  if (key_bits) {
    if (lane < nsteps) kb0 = key_bits[(size_t)b * 128 + lane];
    if (lane + 64 < nsteps) kb1 = key_bits[(size_t)b * 128 + 64 + lane];
  } else {
    if (lane < nsteps) kb0 = xa_pack32(mk + 32 * lane);
    if (lane + 64 < nsteps) kb1 = xa_pack32(mk + 32 * (lane + 64));
  }
  v0 = __ballot(kb0 != 0u), v1 = __ballot(kb1 != 0u);
  if ((v0 | v1) == 0ull) {
    v0 = nsteps >= 64 ? ~0ull : ((1ull << nsteps) - 1ull);
    v1 = nsteps > 64 ? ((nsteps >= 128 ? ~0ull : ((1ull << (nsteps - 64)) - 1ull))) : 0ull;
  }
  v0 = __builtin_amdgcn_readfirstlane((unsigned)v0) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(v0 >> 32)) << 32);
  v1 = __builtin_amdgcn_readfirstlane((unsigned)v1) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(v1 >> 32)) << 32);
}
// the word of key bits of `step` out of the two words per lane (steps lane and lane + 64) that every wave holds (wave-uniform)
__device__ __forceinline__ uint32_t xa_kword(uint32_t kb0, uint32_t kb1, int step) {
  return step < 64 ? (uint32_t)__builtin_amdgcn_readlane((int)kb0, step) : (uint32_t)__builtin_amdgcn_readlane((int)kb1, step - 64);
}

// S^T = K Q^T of the step, tile t of row tile nt, the piece products in the SplitTab order: lane (c, g) holds row 16 nt + c, keys
// 8g + 4t + j; masked keys = finfo.min (kbits: the step's word of key bits >> 8g)
template <int S, int NA>
__device__ __forceinline__ f32x4 xa_scores(const p16x8 (&kf)[S][2][2], const p16x8 (&qf)[S][NA][2], int nt, int t, uint32_t kbits) {
  using T = SplitTab<S>;
  f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int pr = 0; pr < T::NP; ++pr) {
    a = mfma16(kf[T::A[pr]][t][0], qf[T::B[pr]][nt][0], a);
    a = mfma16(kf[T::A[pr]][t][1], qf[T::B[pr]][nt][1], a);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = ((kbits >> (4 * t + j)) & 1u) ? a[j] : GRAM_FMIN;
  return a;
}
// the step's row maximum folded into m: returns the new maximum, alpha = the factor that rescales what was summed under the old one
__device__ __forceinline__ float xa_row_max(const f32x4 (&s)[2], float& m, float& alpha) {
  float tm = fmaxf(fmaxf(fmaxf(s[0][0], s[0][1]), fmaxf(s[0][2], s[0][3])),
                   fmaxf(fmaxf(s[1][0], s[1][1]), fmaxf(s[1][2], s[1][3])));
  tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
  tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
  const float mn = fmaxf(m, tm);
  alpha = __expf(m - mn);
  m = mn;
  return mn;
}
// First half of a 32-key step for the first NL of the caller's row tiles: scores, online softmax (m, l; O rescaled), and
// pf = exp(S^T - max) as pieces, the B operand of O^T += V^T P^T.  kword: the step's word of key bits; g = lane >> 4.
template <int NL, int S, int NA, int MT>
__device__ __forceinline__ void xa_step_qk(uint32_t kword, int g, const p16x8 (&kf)[S][2][2], const p16x8 (&qf)[S][NA][2],
                                           p16x8 (&pf)[S][NA], float (&m)[MT], float (&l)[MT], f32x4 (&o)[4][MT]) {
  const uint32_t kbits = kword >> (8 * g);  // this lane's keys 8g + 4t + j
#pragma unroll
  for (int nt = 0; nt < NL; ++nt) {
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) s[t] = xa_scores(kf, qf, nt, t, kbits);
    float alpha;
    const float mn = xa_row_max(s, m[nt], alpha);
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float e = __expf(s[t][j] - mn);
        ps += e;
#pragma unroll
        for (int pc = 0; pc < S; ++pc) {
          const p16 eb = (p16)e;
          pf[pc][nt][4 * t + j] = eb;
          e -= (float)eb;
        }
      }
    l[nt] = xa_l_update(l[nt], alpha, ps);
    // (One round-1 build of cross_attn_kernel returned wrong values in dims 48-63; the cause was not this scaling -- whose packed
    // multiply was blamed at the time -- but accumulators read by the loop's back-edge copies 2-7 wait states after their
    // MFMA, through branches the compiler's hazard padding did not cover: DESIGN.md §4.3.  tools/check_isa_hazards.py
    // checks every build for that, across the control-flow graph.)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) o[mt][nt] *= alpha;
  }
}
// Second half: O^T += V^T P^T for the same tiles
template <int NL, int S, int NA, int MT>
__device__ __forceinline__ void xa_step_pv(const p16x8 (&vf)[S][4], const p16x8 (&pf)[S][NA], f32x4 (&o)[4][MT]) {
  using T = SplitTab<S>;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < NL; ++nt)
#pragma unroll
      for (int pr = 0; pr < T::NP; ++pr) o[mt][nt] = mfma16(vf[T::A[pr]][mt], pf[T::B[pr]][nt], o[mt][nt]);
}

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
