// tf_attn.hip -- the kernels of the teacher-forced decoder pass (gram_teacher_forced): the decoder over whole label sequences at
// once instead of one token per step.
//
// (1) dec_self_attn_tf_kernel: causal self-attention of all T <= 64 positions of a decoder sequence over the same sequence
//     (T5Attention.forward self branch with the causal mask and the unidirectional relative bias of layer 0,
//     gram_t5_modeling.py:586-593; T5ForConditionalGeneration_GRAM.forward passes no decoder mask, gram_t5.py:181-263).
//     q|k|v straight from the QKV GEMM's planar output: no cache, no ancestor table.  One workgroup per (sequence, head); the
//     sequence's keys and values (fp32 sums of their pieces) sit in LDS, 16 lanes per query, 4 dims per lane.
//     VALU, not MFMA: the ids of the "split" / "t5_token" types are ~10 tokens, so a 16x16 tile would be mostly padding, and the
//     kernel is bound by reading the q|k|v rows once (T * 64 * 2 flops per key against 3 * 128 B per row and piece).  The
//     arithmetic of a row is self_attn_row.h's, the one text that dec_attn.hip's stepped kernel and tree_attn.hip's kernel call
//     too: a teacher-forced position and a cached decode step over the same prefix give the same bits by construction.
// (2) the cross-attention of Q = C * T query rows per user over that user's bank: dec_attn.hip's cross_attn_kernel takes <= 64 rows
//     per user, so Q <= 64 calls it directly (K = Q) and Q > 64 calls its live-row form once per group of <= 64 rows, with offset
//     q / out pointers and a row table that maps (user, row of the group) to b * Q + row.  Each group re-reads the bank.
// (3) label_logprob_kernel: token_logp = h . E[label] - lse with dec_attn's sibling beam.hip's sparse_dot (sparse_dot.h: the same
//     function, the same bits as a beam-search logit), seq_logp = the sum over the sequence in position order (no float atomics).
#include "common.h"
#include "prof.h"
#include "self_attn_row.h"
#include "sparse_dot.h"

namespace {

template <int S>
__global__ __launch_bounds__(256) void dec_self_attn_tf_kernel(const p16* __restrict__ qkv, const float* __restrict__ bias,
                                                               p16* __restrict__ out, int T, int H, long qkv_ps) {
  __shared__ float ks[GRAM_MAX_DEC_LEN][16][4], vs[GRAM_MAX_DEC_LEN][16][4];  // [position][lane of the 16][dim]
  const int sq = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
  const int inner = H * 64, l16 = tid & 15, grp = tid >> 4, ngrp = blockDim.x >> 4;
  const size_t row0 = (size_t)sq * T;
  // keys and values of the sequence, summed over their pieces once
  for (int idx = tid; idx < T * 16; idx += blockDim.x) {
    const int j = idx >> 4, c = idx & 15;
    const p16* row = qkv + (row0 + j) * 3 * inner + h * 64 + 4 * c;
    sa_load<S>(row + inner, qkv_ps, ks[j][c]);
    sa_load<S>(row + 2 * inner, qkv_ps, vs[j][c]);
  }
  __syncthreads();
  // every 16-lane group walks its queries t = grp, grp + ngrp, ... (the loop bound is uniform per group: the lane sums stay whole)
  for (int t = grp; t < T; t += ngrp) {
    float qf[4], m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
    sa_load<S>(qkv + (row0 + t) * 3 * inner + h * 64 + 4 * l16, qkv_ps, qf);
    for (int j = 0; j <= t; ++j)  // causal: positions 0..t, in order
      sa_step(qf, ks[j][l16], vs[j][l16], bias[h * GRAM_MAX_DEC_LEN + (t - j)], m, l, acc);
    sa_store<S>(out + (row0 + t) * inner * S, h * 64 + 4 * l16, l, acc);
  }
}

// the row tables of the grouped cross-attention: users[b] = b; full[b * 64 + i] = b * Q + i; tail[b * kt + i] = b * Q + i
__global__ __launch_bounds__(64) void tf_rowmap_kernel(int32_t* __restrict__ users, int32_t* __restrict__ full, int32_t* __restrict__ tail,
                                                       int Q, int kt) {
  const int b = blockIdx.x, i = threadIdx.x;
  if (i == 0) users[b] = b;
  full[(size_t)b * 64 + i] = b * Q + i;
  if (i < kt) tail[(size_t)b * kt + i] = b * Q + i;
}

// One workgroup per sequence, 8 lanes per position (sparse_dot), 32 positions per trip
__global__ __launch_bounds__(256) void label_logprob_kernel(const p16* __restrict__ hd, const p16* __restrict__ emb,
                                                            const float* __restrict__ emb32, int d, const float* __restrict__ lse,
                                                            const int32_t* __restrict__ labels, int T, int V, int pieces,
                                                            float* __restrict__ token_logp, float* __restrict__ seq_logp) {
  __shared__ float s_lp[GRAM_MAX_DEC_LEN];
  const int sq = blockIdx.x, tid = threadIdx.x, sub = tid & 7;
  for (int t0 = 0; t0 < T; t0 += 32) {
    const int t = t0 + (tid >> 3);
    const size_t r = (size_t)sq * T + t;
    const int lab = t < T ? labels[r] : -1;
    const bool act = lab >= 0 && lab < V;  // (the host checks labels < V; an out-of-range one is never read)
    const float v = sparse_dot(act, (int)r, act ? lab : 0, sub, hd, emb, emb32, d, pieces);
    if (t < T && sub == 0) {
      const float lp = act ? v - lse[r] : 0.f;
      token_logp[r] = lp;
      s_lp[t] = lp;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;  // position order, starting from 0 like a beam's score: the same sum as the search's running beam score
    for (int t = 0; t < T; ++t)
      if (labels[(size_t)sq * T + t] >= 0) s += s_lp[t];
    seq_logp[sq] = s;
  }
}

}  // namespace

extern "C" int gram_dec_self_attn_tf_split(const void* qkv, const float* bias, void* out, int n_seq, int T, int H, int pieces,
                                           int64_t qkv_pstride, void* stream) {
  if (!qkv || !bias || !out || n_seq < 1 || T < 1 || T > GRAM_MAX_DEC_LEN || H < 1 || H > 16 || pieces < 1 || pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && qkv_pstride < (int64_t)n_seq * T * 3 * H * 64) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_DEC_SELF_ATTN, st, 2.0 * 3 * n_seq * T * H * 64 * pieces);  // q|k|v rows read once
  const int ngrp = T < 16 ? T : 16;
  const dim3 grid(n_seq, H), block((ngrp * 16 + 63) / 64 * 64);
  if (pieces == 2)
    hipLaunchKernelGGL(dec_self_attn_tf_kernel<2>, grid, block, 0, st, (const p16*)qkv, bias, (p16*)out, T, H, (long)qkv_pstride);
  else
    hipLaunchKernelGGL(dec_self_attn_tf_kernel<1>, grid, block, 0, st, (const p16*)qkv, bias, (p16*)out, T, H, (long)qkv_pstride);
  GRAM_CHECK_LAUNCH();
  return 0;
}

// the row tables of a grouped cross-attention over Q > GRAM_MAX_BEAMS rows per user (common.h; also xattn_long.hip's)
int gram_tf_rowmap(int32_t* rowmap, int B, int Q, void* stream) {
  int32_t* users = rowmap;
  int32_t* full = users + B;
  int32_t* tail = full + (size_t)B * GRAM_MAX_BEAMS;
  hipLaunchKernelGGL(tf_rowmap_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, users, full, tail, Q, Q % GRAM_MAX_BEAMS);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_cross_attn_rows_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                          int B, int Q, int H, int S, int pieces, int64_t q_pstride, int64_t bank_pstride,
                                          const uint32_t* key_bits, int32_t* rowmap, void* stream) {
  if (!q || !out || B < 1 || Q < 1 || H < 1 || pieces < 1 || pieces > GRAM_MAX_PIECES) return GRAM_E_ARG;
  if (Q <= GRAM_MAX_BEAMS)  // one call: rows b * Q + i are the kernel's own (user, beam) rows
    return gram_cross_attn_decode_split(q, k_layer, vt_layer, mask, out, B, Q, H, S, nullptr, nullptr, pieces, q_pstride, bank_pstride,
                                        key_bits, stream);
  if (!rowmap || (int64_t)B * Q > INT32_MAX) return GRAM_E_ARG;
  int32_t* users = rowmap;
  int32_t* full = users + B;
  int32_t* tail = full + (size_t)B * GRAM_MAX_BEAMS;
  const int e0 = gram_tf_rowmap(rowmap, B, Q, stream);
  if (e0) return e0;
  const size_t inner = (size_t)H * 64;
  for (int r0 = 0; r0 < Q; r0 += GRAM_MAX_BEAMS) {
    const int kc = Q - r0 < GRAM_MAX_BEAMS ? Q - r0 : GRAM_MAX_BEAMS;
    // q planar: row r0 of every piece is r0 * inner elements in (the pieces stay q_pstride apart); out: [rows][pieces * inner]
    const int e = gram_cross_attn_decode_split((const p16*)q + r0 * inner, k_layer, vt_layer, mask, (p16*)out + r0 * inner * pieces,
                                               B, kc, H, S, users, kc == GRAM_MAX_BEAMS ? full : tail, pieces, q_pstride, bank_pstride,
                                               key_bits, stream);
    if (e) return e;
  }
  return 0;
}

extern "C" int gram_label_logprob_split(const void* hidden, const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse,
                                        const int32_t* labels, int n_seq, int T, int V, int pieces, float* token_logp, float* seq_logp,
                                        void* stream) {
  if (!hidden || !lse || !labels || !token_logp || !seq_logp || n_seq < 1 || T < 1 || T > GRAM_MAX_DEC_LEN || V < 1 || d < 64 ||
      d % 64 || pieces < 1 || pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 ? !lm_head_f32 : !lm_head_bf16) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_LSE, st, 4.0 * n_seq * T * d);
  hipLaunchKernelGGL(label_logprob_kernel, dim3(n_seq), dim3(256), 0, st, (const p16*)hidden, (const p16*)lm_head_bf16,
                     pieces > 1 ? lm_head_f32 : nullptr, d, lse, labels, T, V, pieces, token_logp, seq_logp);
  GRAM_CHECK_LAUNCH();
  return 0;
}
