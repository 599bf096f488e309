// xattn_probs.hip -- the cross-attention PROBABILITIES of Q query rows per user over that user's K bank (gram_cross_attn_probs_split):
// what HF returns as `cross_attentions` (gram_t5_modeling.py:600-603,629), which dec_attn.hip's online-softmax kernel never forms.
//
//     probs[b][h][i][s] = softmax_s(q[b*Q + i] . k[b][h][s] + (mask[b][s] ? 0 : finfo.min)),  f32 [B][H][Q][S]
//
// A sibling of cross_attn_kernel (dec_attn.hip) without V: the same operand pieces, the scores and the online (max, sum) of xattn_tile.h
// (xa_scores in the three-product order, xa_row_max, xa_l_update), the same K tiles through LDS-DMA with the same swizzle (ksw) and the
// same key bits, so the numbers describe the attention the decoder applied.  The key-step setup, the DMA and the fragment reads stay
// spelled out here: through the shared functions this kernel's schedule changes, and it did not time inside the parent's spread.
// A row's normaliser (max, sum) is only known after the last key, so the bank's K is swept TWICE: sweep 1 keeps (m, l) per row,
// sweep 2 recomputes the scores -- the same MFMAs on the same data: the same bits -- and stores exp(s - m) * (1 / l).  Nothing the
// kernel writes is read back.
//
// Mapping: ONE wave per (head, user, tile of 32 query rows); grid (H, B, ceil(Q / 32)).  The tile is fixed -- one instantiation per
// piece mode -- and a query row is one MFMA column, so a row's bits depend on nothing but that row, its user's K and mask: not on Q,
// B or the other rows (rows past Q are zero queries that store nothing).  No atomics.  Fully masked 32-key steps are not fetched; their
// outputs are written as zeros.  A user without a valid key keeps every step: scores all finfo.min, probabilities uniform 1 / S.
#include "common.h"
#include "prof.h"
#include "xattn_tile.h"

namespace {

constexpr int XP_NT = 2;       // 16-row MFMA tiles per wave: 32 query rows per workgroup
constexpr int XP_ROWS = XP_NT * 16;

template <int S>
__global__ __launch_bounds__(64) void cross_attn_probs_kernel(const p16* __restrict__ q, const p16* __restrict__ kbank,
                                                              const uint8_t* __restrict__ mask, float* __restrict__ probs, int Q, int H,
                                                              int Sk, long q_pstride, long bank_pstride,
                                                              const uint32_t* __restrict__ key_bits) {
  constexpr int NT = XP_NT;
  __shared__ __attribute__((aligned(16))) char smem[S * XA_TILE];  // the one stage: this step's K tile of every piece

  const int h = blockIdx.x, b = blockIdx.y, row0 = blockIdx.z * XP_ROWS;
  const int lane = threadIdx.x;
  const int c = lane & 15, g = lane >> 4;
  const int inner = H * 64;
  const char* kb = reinterpret_cast<const char*>(kbank + ((size_t)b * H + h) * Sk * 64);
  const uint8_t* mk = mask + (size_t)b * Sk;
  float* prow[NT];  // this lane's output row (query row0 + 16 nt + c), nullptr past Q
  p16x8 qf[S][NT][2];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int i = row0 + 16 * nt + c;
    prow[nt] = i < Q ? probs + (((size_t)b * H + h) * Q + i) * Sk : nullptr;
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd)
        qf[pc][nt][kd] = i < Q ? ld_global_b128(q + pc * q_pstride + ((size_t)b * Q + i) * inner + h * 64 + 32 * kd + 8 * g) : zero_bf16x8();
  }
  // this lane's two words of key bits (steps lane and lane + 64), precomputed (gram_mask_key_bits) or packed here from the mask bytes
  const int nsteps = Sk >> 5;
  uint32_t kb0 = 0, kb1 = 0;
  if (key_bits) {
    if (lane < nsteps) kb0 = key_bits[(size_t)b * 128 + lane];
    if (lane + 64 < nsteps) kb1 = key_bits[(size_t)b * 128 + 64 + lane];
  } else {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int st = lane + 64 * half;
      uint32_t bits = 0;
      if (st < nsteps) {
        const uint4* p = reinterpret_cast<const uint4*>(mk + 32 * st);
        const uint4 a = p[0], c2 = p[1];
        const uint32_t w8[8] = {a.x, a.y, a.z, a.w, c2.x, c2.y, c2.z, c2.w};
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) bits |= ((w8[i] >> (8 * j)) & 0xffu) ? (1u << (4 * i + j)) : 0u;
      }
      if (half == 0) kb0 = bits; else kb1 = bits;
    }
  }
  // the steps that hold a valid key; a user with none keeps every step (the reference's softmax over all-finfo.min scores is uniform)
  unsigned long long v0 = __ballot(kb0 != 0u), v1 = __ballot(kb1 != 0u);
  if ((v0 | v1) == 0ull) {
    v0 = nsteps >= 64 ? ~0ull : ((1ull << nsteps) - 1ull);
    v1 = nsteps > 64 ? ((nsteps >= 128 ? ~0ull : ((1ull << (nsteps - 64)) - 1ull))) : 0ull;
  }
  v0 = __builtin_amdgcn_readfirstlane((unsigned)v0) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(v0 >> 32)) << 32);
  v1 = __builtin_amdgcn_readfirstlane((unsigned)v1) | ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(v1 >> 32)) << 32);
  auto valid = [&](int s) -> bool { return ((s < 64 ? (v0 >> s) : (v1 >> (s - 64))) & 1ull) != 0ull; };
  auto next = [&](int s) -> int {
    for (s = s + 1; s < nsteps; ++s)
      if (valid(s)) return s;
    return nsteps;
  };

  // the skipped steps' outputs: zeros (lane: keys 8g .. 8g+7 of the step, as in sweep 2)
  for (int s = 0; s < nsteps; ++s) {
    if (valid(s)) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      if (prow[nt]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) *reinterpret_cast<f32x4*>(prow[nt] + (size_t)s * 32 + 8 * g + 4 * t) = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
  }

  // per-lane byte offsets of this lane's 16 B in each of the 4 DMA instructions of a (step, piece)
  uint32_t koff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 8 * i + (lane >> 3);  // key row of the tile; the lane lands at position lane & 7 and fetches chunk pos ^ ksw
    koff[i] = (uint32_t)(kr * 128 + (((lane & 7) ^ ksw(kr)) << 4));
  }
  const uint32_t stage0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  auto issue_k = [&](int step) {
#pragma unroll
    for (int pc = 0; pc < S; ++pc) {
      const char* kbase = kb + (size_t)pc * bank_pstride * 2 + (size_t)step * (32 * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) dma16_nt(stage0 + pc * XA_TILE + i * 1024, koff[i], kbase);
    }
  };
  const int krow = 8 * (c >> 2) + (c & 3);  // + 4t: key row of S^T tile t this lane feeds
  p16x8 kf[S][2][2];
  auto read_k = [&]() {
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd) {
          const int r = krow + 4 * t;
          kf[pc][t][kd] = *reinterpret_cast<const p16x8*>(smem + pc * XA_TILE + r * 128 + (((g + 4 * kd) ^ ksw(r)) << 4));
        }
  };
  // S^T = K Q^T of the step for row tile nt (xa_scores): lane (c, g) holds row 16 nt + c, keys 8g + 4t + j; masked keys = finfo.min
  auto scores = [&](int step, int nt, f32x4 (&s)[2]) {
    const uint32_t kbits = xa_kword(kb0, kb1, step) >> (8 * g);
#pragma unroll
    for (int t = 0; t < 2; ++t) s[t] = xa_scores(kf, qf, nt, t, kbits);
  };

  // ordinary loads (query fragments, key bits) are retired here: the waits of the sweeps see DMA instructions and stores only
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) asm volatile("" : "+v"(qf[pc][nt][kd]));  // (hipcc's own wait for the loads goes HERE)

  // One stage, re-filled as soon as its fragments are in registers: the next step's tiles fly during this step's arithmetic.
  // Every wait is vmcnt(0): in sweep 2 the counter also holds the step's stores, and nothing here is counted past them.
  auto sweep = [&](auto&& math) {
    int cur = next(-1);
    if (cur < nsteps) issue_k(cur);
    while (cur < nsteps) {
      const int nxt = next(cur);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's K tiles have landed
      read_k();
      if (nxt < nsteps) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the fragments are in registers before their tiles are re-filled
        issue_k(nxt);
      }
      math(cur);
      cur = nxt;
    }
  };

  // sweep 1: (max, sum of exp) per row, online
  float m[NT], l[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    m[nt] = GRAM_FMIN;
    l[nt] = 0.f;
  }
  sweep([&](int step) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 s[2];
      scores(step, nt, s);
      float alpha;
      const float mn = xa_row_max(s, m[nt], alpha);
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) ps += __expf(s[t][j] - mn);
      l[nt] = xa_l_update(l[nt], alpha, ps);
    }
  });
  float inv[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    float lt = l[nt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    inv[nt] = 1.f / lt;
  }
  // sweep 2: the same scores again, normalised and stored (8 consecutive keys per lane: two 16-B stores)
  sweep([&](int step) {
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 s[2];
      scores(step, nt, s);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f32x4 p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = __expf(s[t][j] - m[nt]) * inv[nt];
        if (prow[nt]) *reinterpret_cast<f32x4*>(prow[nt] + (size_t)step * 32 + 8 * g + 4 * t) = p;
      }
    }
  });
}

}  // namespace

extern "C" int gram_cross_attn_probs_split(const void* q, const void* k_layer, const uint8_t* mask, float* probs, int B, int Q, int H,
                                           int S, int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits,
                                           void* stream) {
  if (!q || !k_layer || !mask || !probs || B < 1 || B > 65535 || Q < 1 || H < 1 || S < 32 || (S & 31) || S > 4096 || pieces < 1 ||
      pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && (q_pstride < (int64_t)B * Q * H * 64 || bank_pstride < (int64_t)H * S * 64)) return GRAM_E_ARG;
  if ((reinterpret_cast<uintptr_t>(mask) & 15) || (reinterpret_cast<uintptr_t>(k_layer) & 15) || (reinterpret_cast<uintptr_t>(q) & 15) ||
      (reinterpret_cast<uintptr_t>(probs) & 15))
    return GRAM_E_ARG;
  const int64_t tiles = ((int64_t)Q + XP_ROWS - 1) / XP_ROWS;
  if (tiles > 65535) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_CROSS_ATTN, st, 4.0 * B * H * S * 64 * pieces);  // K twice, every piece
  const dim3 grid(H, B, (unsigned)tiles);
  if (pieces == 2)
    hipLaunchKernelGGL(cross_attn_probs_kernel<2>, grid, dim3(64), 0, st, (const p16*)q, (const p16*)k_layer, mask, probs, Q, H, S,
                       (long)q_pstride, (long)bank_pstride, key_bits);
  else
    hipLaunchKernelGGL(cross_attn_probs_kernel<1>, grid, dim3(64), 0, st, (const p16*)q, (const p16*)k_layer, mask, probs, Q, H, S,
                       (long)q_pstride, (long)bank_pstride, key_bits);
  GRAM_CHECK_LAUNCH();
  return 0;
}
