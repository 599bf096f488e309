// tree_attn.hip -- the kernels of the Trie-shaped decoder pass (gram_score_trie): one decoder row per internal Trie node instead of
// one per (candidate, position), so that every catalogue item is scored in one pass.
//
// (1) dec_self_attn_tree_kernel: causal self-attention where row i attends to the rows anc[i][0..pos[i]] of its user -- its
//     ancestors in the Trie and itself (T5Attention.forward self branch with the causal mask and the unidirectional relative bias of
//     layer 0, gram_t5_modeling.py:586-593, on the prefix the row stands for; gram_t5.py:181-263).  The arithmetic of a row is
//     self_attn_row.h's, the one text that tf_attn.hip's dec_self_attn_tf_kernel and dec_attn.hip's stepped kernel call too, so a
//     tree row, the same prefix in a teacher-forced sequence and the same prefix in a cached decode step give the same bits by
//     construction.  16 queries per workgroup; the ancestors' K/V rows are read through L2 (neighbouring rows are siblings and
//     cousins: the four queries of a wave mostly ask for the same lines).  No LDS, no barrier.
// (2) trie_row_edge_kernel / trie_leaf_kernel: log p of every edge below a row from the final hidden rows (sparse_dot.h: the dot
//     product of label_logprob_kernel and of the search step, the same bits), then per leaf the sum of the edge terms along its path in
//     position order, starting from 0.f -- label_logprob_kernel's sum.  One writer per output element: no float atomics.
// (3) trie_repeat_tokens_kernel: the Q decoder input tokens of the row table repeated for every user.
#include "common.h"
#include "prof.h"
#include "self_attn_row.h"
#include "sparse_dot.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int S>
__global__ __launch_bounds__(256) void dec_self_attn_tree_kernel(const p16* __restrict__ qkv, const int32_t* __restrict__ pos,
                                                                 const int32_t* __restrict__ anc, const float* __restrict__ bias,
                                                                 p16* __restrict__ out, int Q, int Tq, int H, long qkv_ps, int nblk) {
  const int b = blockIdx.x / nblk, blk = blockIdx.x % nblk, h = blockIdx.y, tid = threadIdx.x;
  const int inner = H * 64, l16 = tid & 15, grp = tid >> 4;
  const int i = blk * 16 + grp;
  if (i >= Q) return;  // (uniform per 16-lane group: the lane sums stay whole)
  const size_t row0 = (size_t)b * Q;
  // (a table entry outside its range is clamped, never followed out of the user's rows)
  const int t = clampi(pos[i], 0, Tq - 1);
  const int32_t* ai = anc + (size_t)i * Tq;
  const p16* row = qkv + (row0 + i) * 3 * inner + h * 64 + 4 * l16;
  float qf[4], m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  sa_load<S>(row, qkv_ps, qf);
  for (int j = 0; j <= t; ++j) {  // the ancestor at position j, in order; j == t: the row itself
    const int a = clampi(ai[j], 0, Q - 1);
    const p16* arow = qkv + (row0 + a) * 3 * inner + h * 64 + 4 * l16;
    float kj[4], vj[4];
    sa_load<S>(arow + inner, qkv_ps, kj);
    sa_load<S>(arow + 2 * inner, qkv_ps, vj);
    sa_step(qf, kj, vj, bias[h * GRAM_MAX_DEC_LEN + (t - j)], m, l, acc);
  }
  sa_store<S>(out + (row0 + i) * inner * S, h * 64 + 4 * l16, l, acc);
}

__global__ __launch_bounds__(256) void trie_repeat_tokens_kernel(const int32_t* __restrict__ tokens, int32_t* __restrict__ out, int Q,
                                                                 long total) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g < total) out[g] = tokens[g % Q];
}

// 8 lanes (sparse_dot) per (user, row i): the term of the edge INTO row i's node, predicted by the row of its parent
__global__ __launch_bounds__(256) void trie_row_edge_kernel(const p16* __restrict__ hd, const p16* __restrict__ emb,
                                                            const float* __restrict__ emb32, int d, const float* __restrict__ lse,
                                                            gram_trie_rows_t tr, int B, int V, int pieces, float* __restrict__ edge,
                                                            float* __restrict__ node_logp) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7, Q = tr.Q;
  const bool in = g < (long)B * Q;  // (uniform per 8-lane group)
  const int b = in ? (int)(g / Q) : 0, i = in ? (int)(g % Q) : 0;
  const int t = clampi(tr.pos[i], 0, tr.Tq - 1);
  const int tok = tr.tokens[i];
  const bool act = in && t >= 1 && tok >= 0 && tok < V;  // (position 0 is the start token: no edge term)
  const int parent = act ? clampi(tr.anc[(size_t)i * tr.Tq + t - 1], 0, Q - 1) : 0;
  const size_t r = (size_t)b * Q + parent;
  const float v = sparse_dot(act, (int)r, act ? tok : 0, sub, hd, emb, emb32, d, pieces);
  if (in && sub == 0) {
    const float lp = act ? v - lse[r] : 0.f;
    edge[g] = lp;
    const int n = tr.row_node[i];
    if (node_logp && n >= 0 && n < tr.n_nodes) node_logp[(size_t)b * tr.n_nodes + n] = lp;
  }
}

// 8 lanes per (user, node n): a leaf's own edge term, then lane 0 adds the terms along its path in position order
__global__ __launch_bounds__(256) void trie_leaf_kernel(const p16* __restrict__ hd, const p16* __restrict__ emb,
                                                        const float* __restrict__ emb32, int d, const float* __restrict__ lse,
                                                        gram_trie_rows_t tr, int B, int V, int pieces, const float* __restrict__ edge,
                                                        float* __restrict__ leaf_logp, float* __restrict__ node_logp) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7, Q = tr.Q;
  const bool in = g < (long)B * tr.n_nodes;
  const int b = in ? (int)(g / tr.n_nodes) : 0, n = in ? (int)(g % tr.n_nodes) : 0;
  const int rank = tr.node_leaf[n], i = tr.node_row[n], tok = tr.node_tok[n];
  const bool leaf = in && rank >= 0 && rank < tr.n_leaves && i >= 0 && i < Q;
  const bool act = leaf && tok >= 0 && tok < V;
  const size_t r = (size_t)b * Q + (leaf ? i : 0);
  const float v = sparse_dot(act, (int)r, act ? tok : 0, sub, hd, emb, emb32, d, pieces);
  if (!in || sub != 0) return;
  if (leaf) {
    const float lp = act ? v - lse[r] : 0.f;
    const int t = clampi(tr.pos[i], 0, tr.Tq - 1);
    const int32_t* ai = tr.anc + (size_t)i * tr.Tq;
    float s = 0.f;  // position order, starting from 0 like a beam's score (label_logprob_kernel's sum)
    for (int j = 1; j <= t; ++j) s += edge[(size_t)b * Q + clampi(ai[j], 0, Q - 1)];
    s += lp;
    leaf_logp[(size_t)b * tr.n_leaves + rank] = s;
    if (node_logp) node_logp[(size_t)b * tr.n_nodes + n] = lp;
  } else if (node_logp && i < 0) {
    node_logp[(size_t)b * tr.n_nodes + n] = 0.f;  // the root and the start token's node: nothing predicts them
  }
}

bool rows_ok(const gram_trie_rows_t* t) {
  return t && t->tokens && t->pos && t->anc && t->row_node && t->node_row && t->node_tok && t->node_leaf && t->Q >= 1 && t->Tq >= 1 &&
         t->Tq <= GRAM_MAX_DEC_LEN && t->n_nodes >= 3 && t->n_leaves >= 1 && t->n_leaves < t->n_nodes;
}

}  // namespace

extern "C" int gram_dec_self_attn_tree_split(const void* qkv, const int32_t* pos, const int32_t* anc, const float* bias, void* out, int B,
                                             int Q, int Tq, int H, int pieces, int64_t qkv_pstride, void* stream) {
  if (!qkv || !pos || !anc || !bias || !out || B < 1 || Q < 1 || Tq < 1 || Tq > GRAM_MAX_DEC_LEN || H < 1 || H > 16 || pieces < 1 ||
      pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  const int64_t nblk = ((int64_t)Q + 15) / 16;
  if ((int64_t)B * Q > INT32_MAX / 4 || (int64_t)B * nblk > INT32_MAX) return GRAM_E_ARG;
  if (pieces > 1 && qkv_pstride < (int64_t)B * Q * 3 * H * 64) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_DEC_SELF_ATTN, st, 2.0 * 3 * B * Q * H * 64 * pieces);  // q|k|v rows, each counted once
  const dim3 grid((unsigned)(B * nblk), H), block(256);
  if (pieces == 2)
    hipLaunchKernelGGL(dec_self_attn_tree_kernel<2>, grid, block, 0, st, (const p16*)qkv, pos, anc, bias, (p16*)out, Q, Tq, H,
                       (long)qkv_pstride, (int)nblk);
  else
    hipLaunchKernelGGL(dec_self_attn_tree_kernel<1>, grid, block, 0, st, (const p16*)qkv, pos, anc, bias, (p16*)out, Q, Tq, H,
                       (long)qkv_pstride, (int)nblk);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_trie_repeat_tokens(const int32_t* tokens, int32_t* out, int B, int Q, void* stream) {
  if (!tokens || !out || B < 1 || Q < 1 || (int64_t)B * Q > INT32_MAX / 4) return GRAM_E_ARG;
  const long total = (long)B * Q;
  hipLaunchKernelGGL(trie_repeat_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tokens, out, Q,
                     total);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_trie_leaf_logprob_split(const void* hidden, const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse,
                                            const gram_trie_rows_t* rows_host, int B, int V, int pieces, float* row_edge, float* leaf_logp,
                                            float* node_logp, void* stream) {
  if (!hidden || !lse || !row_edge || !leaf_logp || !rows_ok(rows_host) || B < 1 || V < 1 || d < 64 || d % 64 || pieces < 1 ||
      pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 ? !lm_head_f32 : !lm_head_bf16) return GRAM_E_ARG;
  const gram_trie_rows_t tr = *rows_host;
  if ((int64_t)B * tr.Q > INT32_MAX / 4 || (int64_t)B * tr.n_nodes > INT32_MAX / 4) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_LSE, st, 4.0 * B * (tr.n_nodes - 2) * d);
  const p16* emb = (const p16*)lm_head_bf16;
  const float* emb32 = pieces > 1 ? lm_head_f32 : nullptr;
  const long rows = (long)B * tr.Q, nodes = (long)B * tr.n_nodes;  // 32 eight-lane groups per workgroup
  hipLaunchKernelGGL(trie_row_edge_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, st, (const p16*)hidden, emb, emb32, d, lse, tr,
                     B, V, pieces, row_edge, node_logp);
  GRAM_CHECK_LAUNCH();
  hipLaunchKernelGGL(trie_leaf_kernel, dim3((unsigned)((nodes + 31) / 32)), dim3(256), 0, st, (const p16*)hidden, emb, emb32, d, lse, tr, B,
                     V, pieces, (const float*)row_edge, leaf_logp, node_logp);
  GRAM_CHECK_LAUNCH();
  return 0;
}
