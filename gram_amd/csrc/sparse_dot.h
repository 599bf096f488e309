// sparse_dot.h -- the dot product of one hidden row with one lm_head row that every sparse logit of the path is computed with:
// the Trie-constrained search step (beam.hip) and the teacher-forced label log-probs (tf_attn.hip) include this one definition, so a
// label's logit is the same function, and the same bits, as the beam search's logit of that token.
#pragma once

#include "common.h"

namespace {

// h[row] . E[tok] on 8 lanes (sub = lane & 7): the same sums in the same order wherever a candidate is computed -- inside the search
// step's workgroup or, for a handful of users, by sparse_logits_kernel's many workgroups (launch_search_step)
__device__ __forceinline__ float sparse_dot(bool act, int lr, int tok, int sub, const p16* __restrict__ hd, const p16* __restrict__ emb,
                                            const float* __restrict__ emb32, int d, int pieces) {
  const int per = d >> 3;  // elements per lane
    float acc = 0.f;
    if (act && emb32) {
      // two-piece mode (gram_split_t): h = fp32 sum of its pieces (smallest first; the row is interleaved, [2 d]), E = the fp32 lm_head row
      const p16* hrow = hd + (size_t)lr * d * pieces;
      const int c0 = sub * per;
      auto hoff = [&](int n, int pc) { return pieces == 2 ? inter_off(n, pc) : n; };
      const f32x4* ep = reinterpret_cast<const f32x4*>(emb32 + (size_t)tok * d + sub * per);
      int i = 0;
      if (pieces <= 2) {
        // 32 elements per lane and trip, every load of the trip in flight together (one 8-element step per trip is a dependent
        // round trip each: 12 of them per candidate at d = 768); same sums in the same order as the loop below
        for (; i + 32 <= per; i += 32) {
          p16x8 hb0[4], hb1[4];
          f32x4 ev[8];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            hb0[u] = ld_global_b128(hrow + hoff(c0 + i + 8 * u, 0));
            hb1[u] = pieces == 2 ? ld_global_b128(hrow + hoff(c0 + i + 8 * u, 1)) : zero_bf16x8();
            ev[2 * u] = ep[(i >> 2) + 2 * u];
            ev[2 * u + 1] = ep[(i >> 2) + 2 * u + 1];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            float hv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) hv[e] = pieces == 2 ? (0.f + (float)hb1[u][e]) + (float)hb0[u][e] : 0.f + (float)hb0[u][e];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += hv[e] * ev[2 * u][e];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += hv[4 + e] * ev[2 * u + 1][e];
          }
        }
      }
      for (; i < per; i += 8) {
        float hv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int pc = pieces - 1; pc >= 0; --pc) {
          const p16x8 hb = ld_global_b128(hrow + hoff(c0 + i, pc));
#pragma unroll
          for (int e = 0; e < 8; ++e) hv[e] += (float)hb[e];
        }
        const f32x4 e0 = ep[i >> 2], e1 = ep[(i >> 2) + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += hv[e] * e0[e];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += hv[4 + e] * e1[e];
      }
    } else if (act) {
      const p16* hp = hd + (size_t)lr * d + sub * per;
      const p16* ep = emb + (size_t)tok * d + sub * per;
      int i = 0;
      for (; i + 32 <= per; i += 32) {  // 8 loads in flight per lane (one load pair per iteration is a dependent round trip each)
        p16x8 hv[4], ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          hv[u] = ld_global_b128(hp + i + 8 * u);
          ev[u] = ld_global_b128(ep + i + 8 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc += (float)hv[u][e] * (float)ev[u][e];  // same order as the scalar loop
      }
      for (; i < per; i += 8) {
        const p16x8 hv = ld_global_b128(hp + i), ev = ld_global_b128(ep + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += (float)hv[e] * (float)ev[e];
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    return acc;
  }

}  // namespace
