// Recording stand-ins for every external that gram_amd/csrc/generate.hip calls: the gram_* kernel launchers and four HIP runtime
// calls.  Linked with the product's own generate.o (and driver.cpp) they turn a call into the C ABI into its launch train as text,
// one line per call: the entry's name, then every argument in order.  No GPU, no HIP runtime: the workspace is host memory.
// A pointer into the workspace prints as ws+<offset>, null as 0, any other pointer raw (the driver hands out fixed addresses);
// a struct argument prints its fields in braces.
#include <stdio.h>
#include <string.h>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/gram_hip.h"

char* g_ws = nullptr;  // the workspace of the running case (driver.cpp)
int64_t g_ws_bytes = 0;
std::vector<int> g_live_script;  // what the next gram_live_rows calls report: {live rows, users} per call
std::vector<int> g_tail_script;  // what the next gram_tail_forest call reports: {rows, entries, most rows of a user}

namespace {
void put(int v) { printf(" %d", v); }
void put(int64_t v) { printf(" %lld", (long long)v); }
void put(size_t v) { printf(" %zu", v); }
void put(float v) { printf(" %.9g", v); }
void put(const void* p) {
  const char* c = (const char*)p;
  if (!p) printf(" 0");
  else if (c >= g_ws && c < g_ws + g_ws_bytes) printf(" ws+%lld", (long long)(c - g_ws));
  else printf(" %p", p);
}
template <class... A>
void fields(A... a) {
  printf(" {");
  (put(a), ...);
  printf(" }");
}
void put(const gram_norm_fusion_t* n) {
  if (!n) return put((const void*)nullptr);
  fields(n->xb_out, n->ss_out, n->ss_in, n->nblk_in, n->d, n->eps, n->quarter, n->xs_in, n->xs_out);
}
void put(const gram_split_t* s) {
  if (!s) return put((const void*)nullptr);
  fields(s->pieces, s->c_interleaved, s->c_pstride, s->bank_pstride, s->out_scale);
}
void put(const gram_kv_bank_t* b) {
  if (!b) return put((const void*)nullptr);
  fields(b->k, b->vt, b->n_layers, b->B, b->H, b->S, b->passage_map, b->N, b->L);
}
void put(const gram_beam_state_t* s) {
  fields(s->B, s->K, s->Tmax, s->length_penalty, s->eos, s->pad, s->tokens, s->node, s->beam_scores, s->seq, s->anc, s->done, s->n_hyps,
         s->hyp_score, s->worst, s->hyp_len, s->hyp_tok, s->error, s->cand_logits, s->cand_logits_users, s->cand_logits_stride);
}
void put(const gram_trie_t* t) { fields(t->child_off, t->child_tok, t->child_node, t->n_nodes, t->n_edges, t->max_fanout, t->min_seq_len); }
void put(const gram_user_items_t* u) { fields(u->leaf_lo, u->leaf_hi, u->ranks, u->count, u->stride, u->mode); }
void put(const gram_user_mask_t* u) { fields(u->leaf_lo, u->leaf_hi, u->words, u->stride, u->n_leaves); }
void put(const gram_trie_rows_t* r) {
  fields(r->tokens, r->pos, r->anc, r->row_node, r->node_row, r->node_tok, r->node_leaf, r->Q, r->Tq, r->n_nodes, r->n_leaves);
}
void put(const gram_sample_params_t* p) { fields(p->temperature, p->top_k, p->top_p); }
void put(const gram_live_rows_t* l) { fields(l->rows, l->rowpos, l->users, l->tokens, l->counts); }
void put(const gram_trie_tail_t* t) { fields(t->sub_rows, t->d_tail, t->steps); }
void put(const gram_forest_t* f) {
  fields(f->tokens, f->pos, f->parent, f->root, f->node, f->user_off, f->ent_off, f->ent_users, f->ent_rows, f->rowpos, f->counts,
         f->slot, f->lvl_rows, f->lvl_tokens, f->lvl_anc, f->cap_rows, f->cap_entries, f->n_levels);
}
template <class... A>
int rec(const char* name, A... a) {
  fputs(name, stdout);
  (put(a), ...);
  putchar('\n');
  return 0;
}
}  // namespace

void trace_line(const char* name, int64_t v) { rec(name, v); }

#define REC(...) return rec(__func__, __VA_ARGS__)
extern "C" {
int gram_gemm_stream_max_m(void) { return 512; }  // the product default
int gram_gemm_bf16_split(const void* A, const void* W, void* C, int M, int N, int kc, int lda, int ldc, int epi, const gram_kv_bank_t* bank,
                         const gram_norm_fusion_t* nf, const gram_split_t* sp, void* st) {
  REC(A, W, C, M, N, kc, lda, ldc, epi, bank, nf, sp, st);
}
int gram_gemm_bf16_lse_split(const void* A, const void* W, float* logits, float* lse_part, int M, int N, int kc, int lda, int ldc,
                             const gram_split_t* sp, void* st) {
  REC(A, W, logits, lse_part, M, N, kc, lda, ldc, sp, st);
}
int gram_row_rscale_xs(const float* ss, float* rs, const float* xs_in, float* xs_out, int M, int nblk, int d, float eps, void* st) {
  REC(ss, rs, xs_in, xs_out, M, nblk, d, eps, st);
}
int gram_embed_ex_xs(const float* table, const void* ids, int i64, float* x, void* xb, float* ss, float* xs_out, int nblk, int rows, int d,
                     int pieces, void* st) {
  REC(table, ids, i64, x, xb, ss, xs_out, nblk, rows, d, pieces, st);
}
int gram_embed_i64(const float* table, const int64_t* ids, float* x, int rows, int d, void* st) { REC(table, ids, x, rows, d, st); }
int gram_embed_i32(const float* table, const int32_t* ids, float* x, int rows, int d, void* st) { REC(table, ids, x, rows, d, st); }
int gram_rmsnorm_bf16_split(const float* x, const float* w, void* out, int rows, int d, float eps, float scale, const float* pos, int N, int L,
                            const int32_t* pmap, int pieces, void* st) {
  REC(x, w, out, rows, d, eps, scale, pos, N, L, pmap, pieces, st);
}
int gram_enc_self_attn_split(const void* qkv, const float* bias, const uint8_t* mask, void* out, int P, int L, int H, int pieces, int64_t ps,
                             void* st) {
  REC(qkv, bias, mask, out, P, L, H, pieces, ps, st);
}
int gram_enc_self_attn_rows_split(const void* table, const int64_t* ids, const float* bias, const uint8_t* mask, void* out, int P, int L, int H,
                                  int pieces, int64_t ps, void* st) {
  REC(table, ids, bias, mask, out, P, L, H, pieces, ps, st);
}
int gram_enc_self_attn_long_split(const void* qkv, const float* bias, const uint8_t* mask, void* out, int P, int L, int H, int pieces,
                                  int64_t ps, void* st) {
  REC(qkv, bias, mask, out, P, L, H, pieces, ps, st);
}
int gram_enc_self_attn_long_rows_split(const void* table, const int64_t* ids, const float* bias, const uint8_t* mask, void* out, int P, int L,
                                       int H, int pieces, int64_t ps, void* st) {
  REC(table, ids, bias, mask, out, P, L, H, pieces, ps, st);
}
int gram_iota_i32(int32_t* out, int n, void* st) { REC(out, n, st); }
int gram_gather_passage_x(const float* cache_x, const int32_t* slot, float* x, int n, int L, int cache_L, int d, void* st) {
  REC(cache_x, slot, x, n, L, cache_L, d, st);
}
int gram_mask_key_bits(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* st) { REC(mask, key_bits, B, S, st); }
int gram_dec_self_attn_split(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias, void* out, int R, int n_rows,
                             const int32_t* rows, int H, int t, int Tmax, int pieces, int64_t qkv_ps, int64_t cache_ps, void* st) {
  REC(qkv, kcache, vcache, anc, bias, out, R, n_rows, rows, H, t, Tmax, pieces, qkv_ps, cache_ps, st);
}
int gram_dec_self_attn_rows_split(const void* table, const int32_t* qkv_rows, void* kcache, void* vcache, const int32_t* anc, const float* bias,
                                  void* out, int R, int n_rows, const int32_t* rows, int H, int t, int Tmax, int pieces, int64_t qkv_ps,
                                  int64_t cache_ps, void* st) {
  REC(table, qkv_rows, kcache, vcache, anc, bias, out, R, n_rows, rows, H, t, Tmax, pieces, qkv_ps, cache_ps, st);
}
int gram_cross_attn_decode_split(const void* q, const void* k, const void* vt, const uint8_t* mask, void* out, int B, int K, int H, int S,
                                 const int32_t* users, const int32_t* rowpos, int pieces, int64_t q_ps, int64_t bank_ps,
                                 const uint32_t* key_bits, void* st) {
  REC(q, k, vt, mask, out, B, K, H, S, users, rowpos, pieces, q_ps, bank_ps, key_bits, st);
}
int gram_mask_key_bits_long(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* st) { REC(mask, key_bits, B, S, st); }
int64_t gram_cross_attn_long_scratch_bytes(int rows, int H, int S) {  // (the product's size: a query, not a launch -- nothing recorded)
  return S <= GRAM_MAX_FUSED_LEN ? 0 : (int64_t)rows * H * ((S + 4095) / 4096) * 68 * 4;
}
int gram_cross_attn_long_split(const void* q, const void* k, const void* vt, const uint8_t* mask, void* out, int B, int K, int H, int S,
                               const int32_t* users, const int32_t* rowpos, int pieces, int64_t q_ps, int64_t bank_ps,
                               const uint32_t* key_bits, float* scratch, void* st) {
  REC(q, k, vt, mask, out, B, K, H, S, users, rowpos, pieces, q_ps, bank_ps, key_bits, scratch, st);
}
int gram_cross_attn_rows_long_split(const void* q, const void* k, const void* vt, const uint8_t* mask, void* out, int B, int Q, int H, int S,
                                    int pieces, int64_t q_ps, int64_t bank_ps, const uint32_t* key_bits, float* scratch, int32_t* rowmap,
                                    void* st) {
  REC(q, k, vt, mask, out, B, Q, H, S, pieces, q_ps, bank_ps, key_bits, scratch, rowmap, st);
}
int gram_dec_self_attn_tf_split(const void* qkv, const float* bias, void* out, int n_seq, int T, int H, int pieces, int64_t qkv_ps, void* st) {
  REC(qkv, bias, out, n_seq, T, H, pieces, qkv_ps, st);
}
int gram_cross_attn_rows_split(const void* q, const void* k, const void* vt, const uint8_t* mask, void* out, int B, int Q, int H, int S,
                               int pieces, int64_t q_ps, int64_t bank_ps, const uint32_t* key_bits, int32_t* rowmap, void* st) {
  REC(q, k, vt, mask, out, B, Q, H, S, pieces, q_ps, bank_ps, key_bits, rowmap, st);
}
int gram_label_logprob_split(const void* hidden, const void* lm16, const float* lm32, int d, const float* lse, const int32_t* labels, int n_seq,
                             int T, int V, int pieces, float* token_logp, float* seq_logp, void* st) {
  REC(hidden, lm16, lm32, d, lse, labels, n_seq, T, V, pieces, token_logp, seq_logp, st);
}
int gram_dec_self_attn_tree_split(const void* qkv, const int32_t* pos, const int32_t* anc, const float* bias, void* out, int B, int Q, int Tq,
                                  int H, int pieces, int64_t qkv_ps, void* st) {
  REC(qkv, pos, anc, bias, out, B, Q, Tq, H, pieces, qkv_ps, st);
}
int gram_trie_repeat_tokens(const int32_t* tokens, int32_t* out, int B, int Q, void* st) { REC(tokens, out, B, Q, st); }
int gram_trie_leaf_logprob_split(const void* hidden, const void* lm16, const float* lm32, int d, const float* lse, const gram_trie_rows_t* rows,
                                 int B, int V, int pieces, float* row_edge, float* leaf_logp, float* node_logp, void* st) {
  REC(hidden, lm16, lm32, d, lse, rows, B, V, pieces, row_edge, leaf_logp, node_logp, st);
}
int gram_cross_attn_probs_split(const void* q, const void* k, const uint8_t* mask, float* probs, int B, int Q, int H, int S, int pieces,
                                int64_t q_ps, int64_t bank_ps, const uint32_t* key_bits, void* st) {
  REC(q, k, mask, probs, B, Q, H, S, pieces, q_ps, bank_ps, key_bits, st);
}
int gram_cross_attn_token_scores_split(const void* q, const void* k, float* acc, int B, int Q, int H, int S, int pieces, int64_t q_ps,
                                       int64_t bank_ps, const uint32_t* key_bits, int first, void* st) {
  REC(q, k, acc, B, Q, H, S, pieces, q_ps, bank_ps, key_bits, first, st);
}
int gram_xattn_head_sum(const float* probs, float* acc, int B, int Q, int H, int S, int first, void* st) {
  REC(probs, acc, B, Q, H, S, first, st);
}
int gram_xattn_passage_scores(const float* acc, const uint8_t* mask, float* scores, int B, int Q, int N, int L, float denom, void* st) {
  REC(acc, mask, scores, B, Q, N, L, denom, st);
}
int gram_lse_combine(const float* lse_part, float* lse, int M, int nblk, void* st) { REC(lse_part, lse, M, nblk, st); }
int gram_beam_init(const gram_beam_state_t* s, const gram_trie_t* trie, int start, void* st) { REC(s, trie, start, st); }
int gram_beam_init_groups(const gram_beam_state_t* s, const gram_trie_t* trie, int start, int num_groups, void* st) {
  REC(s, trie, start, num_groups, st);
}
int gram_beam_step_groups_sparse(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32,
                                 int d, const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, int pieces,
                                 int num_groups, float diversity_penalty, const gram_user_items_t* items, void* st) {
  if (!items) REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, num_groups, diversity_penalty, (const void*)items, st);
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, num_groups, diversity_penalty, items, st);
}
int gram_beam_step_bias_sparse(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32,
                               int d, const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, int pieces,
                               const float* phi, int64_t phi_stride, const gram_user_items_t* items, void* st) {
  if (!items) REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, phi, phi_stride, (const void*)items, st);
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, phi, phi_stride, items, st);
}
int gram_beam_step_sparse(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, int d, const float* lse,
                          int V, int cur_len, int rows_per_user, void* st) {
  REC(s, trie, hidden, lm16, d, lse, V, cur_len, rows_per_user, st);
}
int gram_beam_step_sparse_live(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, int d,
                               const float* lse, int V, int cur_len, const int32_t* rowpos, void* st) {
  REC(s, trie, hidden, lm16, d, lse, V, cur_len, rowpos, st);
}
int gram_beam_step_sparse_split(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const float* lm32, int d,
                                const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, int pieces, void* st) {
  REC(s, trie, hidden, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, st);
}
int gram_beam_step_sparse_items(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, int d,
                                const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, const gram_user_items_t* items,
                                void* st) {
  REC(s, trie, hidden, lm16, d, lse, V, cur_len, rows_per_user, rowpos, items, st);
}
int gram_beam_step_sparse_split_items(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const float* lm32, int d,
                                      const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, int pieces,
                                      const gram_user_items_t* items, void* st) {
  REC(s, trie, hidden, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, items, st);
}
int gram_greedy_step_items(const gram_beam_state_t* s, const gram_trie_t* trie, const float* logits, int V, int cur_len,
                           const gram_user_items_t* items, void* st) {
  REC(s, trie, logits, V, cur_len, items, st);
}
int gram_beam_step_sparse_mask(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32,
                               int d, const float* lse, int V, int cur_len, int rows_per_user, const int32_t* rowpos, int pieces,
                               const gram_user_mask_t* mask, void* st) {
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, mask, st);
}
int gram_greedy_step_mask(const gram_beam_state_t* s, const gram_trie_t* trie, const float* logits, int V, int cur_len,
                          const gram_user_mask_t* mask, void* st) {
  REC(s, trie, logits, V, cur_len, mask, st);
}
int gram_greedy_step(const gram_beam_state_t* s, const gram_trie_t* trie, const float* logits, int V, int cur_len, void* st) {
  REC(s, trie, logits, V, cur_len, st);
}
int gram_greedy_finalize(const gram_beam_state_t* s, int max_length, int64_t* sequences, int32_t* width, void* st) {
  REC(s, max_length, sequences, width, st);
}
int gram_beam_finalize(const gram_beam_state_t* s, int nret, int max_length, int64_t* sequences, float* scores, int32_t* width, void* st) {
  REC(s, nret, max_length, sequences, scores, width, st);
}
int gram_sample_capacity(void) { return 8192; }  // the product default (a query, not a launch -- nothing recorded)
int gram_sample_step(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32, int d,
                     const float* lse, int V, int cur_len, int rows_per_user, int pieces, const gram_sample_params_t* prm, const float* u,
                     int u_stride, float* sample_lp, float* model_lp, void* st) {
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, pieces, prm, u, u_stride, sample_lp, model_lp, st);
}
int gram_sample_step_items(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32, int d,
                           const float* lse, int V, int cur_len, int rows_per_user, int pieces, const gram_sample_params_t* prm,
                           const float* u, int u_stride, float* sample_lp, float* model_lp, const gram_user_items_t* items, void* st) {
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, pieces, prm, u, u_stride, sample_lp, model_lp, items, st);
}
int gram_sample_finalize(const gram_beam_state_t* s, int max_length, const float* model_lp, const float* sample_lp, int64_t* sequences,
                         float* seq_logprobs, float* sample_logprobs, int32_t* width, void* st) {
  REC(s, max_length, model_lp, sample_lp, sequences, seq_logprobs, sample_logprobs, width, st);
}
int gram_sbs_capacity(void) { return 4096; }  // the product default (a query, not a launch -- nothing recorded)
int gram_sbs_init(const gram_beam_state_t* s, const gram_trie_t* trie, int start, uint64_t seed, const int64_t* user_keys, float* sample_lp,
                  float* model_lp, uint64_t* path, void* st) {
  REC(s, trie, start, (int64_t)seed, user_keys, sample_lp, model_lp, path, st);
}
int gram_sbs_step(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32, int d,
                  const float* lse, int V, int cur_len, int rows_per_user, int pieces, float temperature, uint64_t seed, float* sample_lp,
                  float* model_lp, uint64_t* path, void* st) {
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, pieces, temperature, (int64_t)seed, sample_lp, model_lp, path, st);
}
int gram_sbs_step_items(const gram_beam_state_t* s, const gram_trie_t* trie, const void* hidden, const void* lm16, const float* lm32, int d,
                        const float* lse, int V, int cur_len, int rows_per_user, int pieces, float temperature, uint64_t seed,
                        float* sample_lp, float* model_lp, uint64_t* path, const gram_user_items_t* items, void* st) {
  REC(s, trie, hidden, lm16, lm32, d, lse, V, cur_len, rows_per_user, pieces, temperature, (int64_t)seed, sample_lp, model_lp, path, items,
      st);
}
int gram_sbs_finalize(const gram_beam_state_t* s, int max_length, const float* model_lp, const float* sample_lp, int64_t* sequences,
                      float* seq_logprobs, float* sample_logprobs, float* perturbed, int32_t* width, void* st) {
  REC(s, max_length, model_lp, sample_lp, sequences, seq_logprobs, sample_logprobs, perturbed, width, st);
}
int gram_live_rows(const gram_beam_state_t* s, const gram_trie_t* trie, const gram_live_rows_t* out, void* st) {
  // the scripted counts of this call: {live rows, users owning one}, two entries of g_live_script per call
  for (int i = 0; i < 2; ++i) {
    out->counts[i] = g_live_script.empty() ? 0 : g_live_script.front();
    if (!g_live_script.empty()) g_live_script.erase(g_live_script.begin());
  }
  REC(s, trie, out, out->counts[0], out->counts[1], st);
}
int gram_tail_forest(const gram_beam_state_t* s, const gram_trie_t* trie, const gram_trie_tail_t* tail, const gram_forest_t* f, int t,
                     void* st) {
  for (int i = 0; i < 4 + 2 * GRAM_TAIL_MAX_STEPS; ++i) {  // the scripted counts: rows, entries, most rows, 0, rows per (group, level)
    f->counts[i] = g_tail_script.empty() ? 0 : g_tail_script.front();
    if (!g_tail_script.empty()) g_tail_script.erase(g_tail_script.begin());
  }
  REC(s, trie, tail, f, t, f->counts[0], f->counts[1], st);
}
int gram_tail_rowpos(const gram_beam_state_t* s, const gram_trie_t* trie, const gram_forest_t* f, void* st) { REC(s, trie, f, st); }
int gram_scatter_rows(const void* src, const int32_t* rows, void* dst, int n, int row_bytes, int dst_rows, void* st) {
  REC(src, rows, dst, n, row_bytes, dst_rows, st);
}
int gram_dec_self_attn_forest_split(const void* qkv, const int32_t* qkv_rows, const void* kcache, const void* vcache, const int32_t* anc,
                                    const int32_t* pos, const int32_t* parent, const int32_t* root, const float* bias, void* out, int n_rows,
                                    int R, int H, int t0, int Tmax, int nlev, int pieces, int64_t qkv_ps, int64_t cache_ps, void* st) {
  REC(qkv, qkv_rows, kcache, vcache, anc, pos, parent, root, bias, out, n_rows, R, H, t0, Tmax, nlev, pieces, qkv_ps, cache_ps, st);
}
int gram_cross_attn_entries_split(const void* q, const void* k, const void* vt, const uint8_t* mask, void* out, int n_entries, int K, int H,
                                  int S, const int32_t* ent_users, const int32_t* ent_rows, int pieces, int64_t q_ps, int64_t bank_ps,
                                  const uint32_t* key_bits, void* st) {
  REC(q, k, vt, mask, out, n_entries, K, H, S, ent_users, ent_rows, pieces, q_ps, bank_ps, key_bits, st);
}

hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t st) { return (hipError_t)rec(__func__, dst, value, bytes, (void*)st); }
hipError_t hipMemset2DAsync(void* dst, size_t pitch, int value, size_t width, size_t height, hipStream_t st) {
  return (hipError_t)rec(__func__, dst, pitch, value, width, height, (void*)st);
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  if (kind != hipMemcpyDeviceToHost) return (hipError_t)rec(__func__, dst, src, bytes, (int)kind, (void*)st);
  memcpy(dst, src, bytes);  // (the destination is the caller's stack: printed by name, not by address)
  printf("hipMemcpyAsync host");
  return (hipError_t)rec("", src, bytes, (int)kind, (void*)st);
}
hipError_t hipStreamSynchronize(hipStream_t st) { return (hipError_t)rec(__func__, (void*)st); }
}
