// launch_trace <case>: prints the launch train of one call into the C ABI of generate.hip on a tiny model (vocab 256, d 128, d_ff 256,
// 2 heads, 2 + 2 layers), recorded by stub.cpp.  launch_trace --list names the cases.  tests/test_launch_train.py compares every
// case with tests/golden/launch_train/<case>.txt.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "../../include/gram_hip.h"

extern char* g_ws;
extern int64_t g_ws_bytes;
extern std::vector<int> g_live_script;
extern std::vector<int> g_tail_script;
void trace_line(const char* name, int64_t v);

namespace {
// every pointer that is not in the workspace (weights, inputs, outputs, the stream) is a fixed fake address, 16 MiB from the last
uintptr_t g_next = 0x100000000;
template <class T = void>
T* fake() {
  g_next += 0x1000000;
  return (T*)g_next;
}

enum Entry { GENERATE, ENCODE_FUSED, ENCODE_PASSAGES, DECODE_STEP, TEACHER_FORCED, SCORE_TRIE, SBS };
enum Live { OFF, NONE, SOME, ALL };  // live rows off, or on with gram_live_rows reporting no row, some rows, every row
struct Case {
  const char* name;
  Entry entry;
  int pieces, fold, B, N, L, K, T;  // K: beams, or sequences per user of the teacher-forced pass; T: max_length (SCORE_TRIE: K * T rows per user)
  Live live;
  bool comp, capped, logits;  // a gram_compaction_t with cached passages; every stage capped to one piece; teacher-forced logits stored
  bool tables;                // the handle has token tables: the trace starts with their build (workspace offsets: the build's scratch)
  int attn;                   // gram_teacher_forced_ex: 1 = every layer's probabilities, 2 = one layer of scratch + token and passage scores;
                              // 3 = gram_teacher_forced_scores: token and passage scores, the heads summed inside the kernel
  bool items;                 // gram_generate_items: per-user item filters (gram_user_items_t)
  int max_L;                  // != 0: gram_model_set_max_passage_len first (a long-mode handle: the tiled encoder attention at every L)
  int max_S;                  // != 0: gram_model_set_max_fused_len first (the long cross-attention at every S; the model takes 40 passages)
  int tail_rows;              // != 0: gram_generate_tail with d_tail = 2 and two steps left; gram_tail_forest reports this many rows
  int forest_attn;            // 1: gram_debug_set_tail_forest_attn(1) first (0: the default -- forests this small keep the level train)
  int groups;                 // != 0: gram_generate_groups with this many beam groups and diversity_penalty = 0.5
  int bias;                   // != 0: gram_generate_bias; 1: one row of potentials shared by all users, 2: a row of 40 per user
  bool umask;                 // gram_generate_mask: per-user item masks (gram_user_mask_t)
};
const Case kCases[] = {
    {"generate_p1_folded", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME},
    {"generate_p1_unfolded", GENERATE, 1, 0, 2, 3, 32, 4, 4, SOME},
    {"generate_p2", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME},
    {"generate_p2_capped", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, true},
    {"generate_greedy", GENERATE, 1, 1, 2, 3, 32, 1, 4, SOME},
    {"generate_rows_640", GENERATE, 1, 1, 40, 1, 32, 16, 4, SOME},       // 512 < rows < 32 768: neither quarter nor pre_rs
    {"generate_rows_32768", GENERATE, 1, 1, 1024, 1, 32, 32, 4, ALL},    // pre_rs in the encoder and in the decoder (every row live)
    {"generate_live_off", GENERATE, 1, 1, 2, 3, 32, 4, 4, OFF},
    {"generate_live_none", GENERATE, 1, 1, 2, 3, 32, 4, 4, NONE},
    {"generate_live_all", GENERATE, 1, 1, 2, 3, 32, 4, 4, ALL},
    {"generate_comp", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, true},
    {"encode_fused", ENCODE_FUSED, 1, 1, 2, 3, 32, 4, 4},
    {"encode_passages", ENCODE_PASSAGES, 1, 1, 6, 1, 32, 1, 2},
    {"decode_step", DECODE_STEP, 1, 1, 2, 3, 32, 4, 4},
    {"tf_folded", TEACHER_FORCED, 1, 1, 2, 3, 32, 3, 4},
    {"tf_folded_logits", TEACHER_FORCED, 1, 1, 2, 3, 32, 3, 4, OFF, false, false, true},
    {"tf_folded_comp", TEACHER_FORCED, 1, 1, 2, 3, 32, 3, 4, OFF, true},
    {"tf_folded_comp_logits", TEACHER_FORCED, 1, 1, 2, 3, 32, 3, 4, OFF, true, false, true},
    {"tf_unfolded", TEACHER_FORCED, 1, 0, 2, 3, 32, 3, 4},
    {"tf_unfolded_logits", TEACHER_FORCED, 1, 0, 2, 3, 32, 3, 4, OFF, false, false, true},
    {"tf_unfolded_comp", TEACHER_FORCED, 1, 0, 2, 3, 32, 3, 4, OFF, true},
    {"tf_unfolded_comp_logits", TEACHER_FORCED, 1, 0, 2, 3, 32, 3, 4, OFF, true, false, true},
    {"tf_p2", TEACHER_FORCED, 2, 1, 2, 3, 32, 3, 4},
    // handles with token tables: layer 0 of the encoder and of a decode step reads them; a capped stage and the teacher-forced pass keep the GEMM
    {"generate_p1_tables", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, true},
    {"generate_p2_tables", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, true},
    {"generate_p2_capped_tables", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, true, false, true},
    {"generate_greedy_tables", GENERATE, 1, 1, 2, 3, 32, 1, 4, SOME, false, false, false, true},
    {"generate_rows_32768_tables", GENERATE, 1, 1, 1024, 1, 32, 32, 4, ALL, false, false, false, true},
    {"generate_comp_tables", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, true, false, false, true},
    {"encode_passages_tables", ENCODE_PASSAGES, 1, 1, 6, 1, 32, 1, 2, OFF, false, false, false, true},
    {"decode_step_tables", DECODE_STEP, 1, 1, 2, 3, 32, 4, 4, OFF, false, false, false, true},
    {"tf_p2_tables", TEACHER_FORCED, 2, 1, 2, 3, 32, 3, 4, OFF, false, false, false, true},
    // gram_teacher_forced_ex with attention outputs: the train of tf_folded / tf_p2 plus, per layer, the probabilities and their head sum
    {"tf_attn_probs", TEACHER_FORCED, 1, 1, 2, 3, 32, 3, 4, OFF, false, false, false, false, 1},
    {"tf_p2_attn_scores", TEACHER_FORCED, 2, 1, 2, 3, 32, 3, 4, OFF, false, false, false, false, 2},
    // gram_generate_items: the train of generate_p2 with every search step in its per-user-filter form
    {"generate_p2_items", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, true},
    // gram_score_trie over Q = 12 rows per user: the train of tf_folded / tf_p2 (the same 24 rows) with the tokens repeated per user,
    // the tree self-attention in every layer and the Trie reduction in place of the label log-probs
    {"score_trie_folded", SCORE_TRIE, 1, 1, 2, 3, 32, 3, 4},
    {"score_trie_p2", SCORE_TRIE, 2, 1, 2, 3, 32, 3, 4},
    // long-mode handles (gram_model_set_max_passage_len(256)): the trains of generate_p1_folded / generate_p2_tables with the long
    // encoder attention in place of the short one, at L = 32 and at a length a default handle refuses
    {"generate_long_32", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 256},
    {"generate_long_160", GENERATE, 1, 1, 2, 3, 160, 4, 4, SOME, false, false, false, false, 0, false, 256},
    {"generate_p2_tables_long_160", GENERATE, 2, 1, 2, 3, 160, 4, 4, SOME, false, false, false, true, 0, false, 256},
    // handles with a raised fused limit (gram_model_set_max_fused_len(16384)): the train of generate_p1_folded with the long key bits and
    // the long cross-attention in place of the short ones, then N * L = 21 * 224 = 4704 -- a context a default handle refuses -- through
    // generate, the teacher-forced pass and the Trie pass
    {"generate_fused_32", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 16384},
    {"generate_fused_4704", GENERATE, 2, 1, 2, 21, 224, 4, 4, SOME, false, false, false, false, 0, false, 256, 16384},
    {"tf_fused_4704", TEACHER_FORCED, 2, 1, 2, 21, 224, 3, 4, OFF, false, false, false, false, 0, false, 256, 16384},
    {"score_trie_fused_4704", SCORE_TRIE, 2, 1, 2, 21, 224, 3, 4, OFF, false, false, false, false, 0, false, 256, 16384},
    // gram_generate_tail (d_tail = 2, two steps left; capacity 5/4 * 8 * 2 = 20 rows): the trains of generate_p1_folded /
    // generate_p2_tables up to step 1, then the forest, ONE decoder pass over its 11 rows in 2 entries and two search steps; a forest
    // of 21 rows goes on step by step (generate_p1_folded's train behind the forest's count); a raised fused limit never builds one
    {"generate_tail_p1", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 11},
    {"generate_tail_p2_tables", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, true, 0, false, 0, 0, 11},
    {"generate_tail_over", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 21},
    {"generate_tail_fused_32", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 16384, 11},
    // gram_teacher_forced_scores on a raised handle: the trains of tf_p2 (with the long key bits and cross-attention) and tf_fused_4704
    // plus, per layer, the head-summed token scores; the passage scores behind the last layer
    {"tf_scores_fused_96", TEACHER_FORCED, 2, 1, 2, 3, 32, 3, 4, OFF, false, false, false, false, 3, false, 0, 16384},
    {"tf_scores_fused_4704", TEACHER_FORCED, 2, 1, 2, 21, 224, 3, 4, OFF, false, false, false, false, 3, false, 256, 16384},
    // the forest self-attention forced on: the trains of generate_tail_p2_tables / generate_tail_p1 with ONE self-attention launch per
    // layer over the 11 rows in place of the launches per group and level and their scatters (the forest's tables stay what they
    // were); then max_length = 3, which ends inside the tail: the rows of level 1 are left to the memset in front of the launch
    {"generate_tail_forest_p2_tables", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, true, 0, false, 0, 0, 11, 1},
    {"generate_tail_forest_p1", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 11, 1},
    {"generate_tail_forest_cut", GENERATE, 2, 1, 2, 3, 32, 4, 3, SOME, false, false, false, false, 0, false, 0, 0, 11, 1},
    // gram_generate_groups (2 groups of 2 beams): the train of generate_p2 with the group init and the group step in the search's place
    {"generate_groups_p2", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 0, 0, 2},
    // gram_generate_sbs / gram_generate_sbs_items (K = 4 rows per user): the encoder and the decode steps of generate_live_off with
    // the stochastic beam search's init, step and finalize in the search's place, step 0 on one decoder row per user; the three
    // per-row arrays lie behind gram_workspace_bytes
    {"generate_sbs_p2", SBS, 2, 1, 2, 3, 32, 4, 4},
    {"generate_sbs_p1_items", SBS, 1, 1, 2, 3, 32, 4, 4, OFF, false, false, false, false, 0, true},
    // gram_generate_bias: the train of generate_p2_items (per-user potentials, item filters) and of generate_live_off (one shared
    // row) with the biased step in the search step's place
    {"generate_bias_p2_items", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, true, 0, 0, 0, 0, 0, 2},
    {"generate_bias_p1", GENERATE, 1, 1, 2, 3, 32, 4, 4, OFF, false, false, false, false, 0, false, 0, 0, 0, 0, 0, 1},
    // gram_generate_mask: the trains of gram_generate_items at the same shapes (two pieces, one piece, greedy) with every step in
    // its per-user-mask form (tests/test_item_mask_host.py compares each pair call for call)
    {"generate_p2_mask", GENERATE, 2, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 0, 0, 0, 0, true},
    {"generate_p1_items", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, true},
    {"generate_p1_mask", GENERATE, 1, 1, 2, 3, 32, 4, 4, SOME, false, false, false, false, 0, false, 0, 0, 0, 0, 0, 0, true},
    {"generate_greedy_items", GENERATE, 1, 1, 2, 3, 32, 1, 4, SOME, false, false, false, false, 0, true},
    {"generate_greedy_mask", GENERATE, 1, 1, 2, 3, 32, 1, 4, SOME, false, false, false, false, 0, false, 0, 0, 0, 0, 0, 0, true},
};

gram_model_t* make_model(int pieces, int fold, int max_passages) {
  enum { NL = 2 };
  static const float* ln[5][NL];
  static const void* w[10][NL];
  static float scales[10 * NL + 2];
  gram_model_desc_t d{};
  d.vocab = 256, d.d_model = 128, d.d_ff = 256, d.n_heads = 2, d.n_enc_layers = d.n_dec_layers = NL, d.max_passages = max_passages;
  d.tie_word_embeddings = d.use_position_embedding = 1, d.fold_norm = fold, d.eps = 1e-6f, d.pieces = pieces;
  d.embed_f32 = fake<float>(), d.lm_head_bf16 = fake(), d.pos_emb_f32 = fake<float>(), d.enc_bias_f32 = fake<float>();
  d.dec_bias_f32 = fake<float>(), d.enc_final_ln = fake<float>(), d.dec_final_ln = fake<float>();
  d.dec_wkv_x_all = fake(), d.lm_head_f32 = fake<float>();
  for (auto& a : ln)
    for (auto& p : a) p = fake<float>();
  for (auto& a : w)
    for (auto& p : a) p = fake();
  for (int i = 0; i < 10 * NL + 2; ++i) scales[i] = (float)(1 << (i + 1));  // a different out_scale for every weight
  d.enc_ln1 = ln[0], d.enc_ln2 = ln[1], d.dec_ln1 = ln[2], d.dec_ln2 = ln[3], d.dec_ln3 = ln[4];
  d.enc_wqkv = w[0], d.enc_wo = w[1], d.enc_wi = w[2], d.enc_wo2 = w[3], d.dec_wqkv = w[4], d.dec_wo = w[5];
  d.dec_wq_x = w[6], d.dec_wo_x = w[7], d.dec_wi = w[8], d.dec_wo2 = w[9];
  d.w_scales = scales;
  return gram_model_create(&d);
}

int run(const Case& c) {
  gram_model_t* m = make_model(c.pieces, c.fold, c.max_S ? 40 : 5);
  if (!m) return GRAM_E_ARG;
  if (c.max_L) trace_line("gram_model_set_max_passage_len", gram_model_set_max_passage_len(m, c.max_L));
  if (c.max_S) trace_line("gram_model_set_max_fused_len", gram_model_set_max_fused_len(m, c.max_S));
  void* st = fake();
  const int64_t* ids = fake<int64_t>();
  const uint8_t* mask = fake<uint8_t>();
  const gram_compaction_t comp{c.B * c.N - 1, fake<int32_t>(), fake<int64_t>(), fake<uint8_t>(), 2, 16, fake<float>(), fake<int32_t>()};
  const gram_trie_t trie{fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), 40, 39, 3, /*min_seq_len=*/2};  // live rows from step 1 on
  const int B = c.B, N = c.N, L = c.L, K = c.K, T = c.T, R = B * K;
  if (c.capped) {
    const int32_t caps[GRAM_STAGE_COUNT] = {1, 1, 1, 1, 1, 1, 1, 1};
    gram_debug_set_stage_pieces(caps, GRAM_STAGE_COUNT);
  }
  if (c.tables) {
    trace_line("gram_token_tables_bytes", gram_token_tables_bytes(m));
    g_ws_bytes = gram_token_tables_workspace_bytes(m);
    trace_line("gram_token_tables_workspace_bytes", g_ws_bytes);
    g_ws = (char*)calloc(g_ws_bytes, 1);
    trace_line("gram_model_build_token_tables", gram_model_build_token_tables(m, fake(), gram_token_tables_bytes(m), g_ws, g_ws_bytes, st));
  }
  gram_debug_set_live_rows(c.live != OFF);
  if (c.live == SOME) g_live_script = {R - 1, B, R / 2, (B + 1) / 2};
  if (c.live == ALL) g_live_script = {R, B, R, B};
  trace_line("gram_workspace_bytes", gram_workspace_bytes(m, B, N, L, K, T));
  trace_line("gram_workspace_bytes_tf", gram_workspace_bytes_tf(m, B, N, L, K, T));
  trace_line("gram_workspace_encoder_x_offset", gram_workspace_encoder_x_offset(m, B, N, L, K, T));
  g_ws_bytes = c.entry == TEACHER_FORCED ? gram_workspace_bytes_tf(m, B, N, L, K, T) : gram_workspace_bytes(m, B, N, L, K, T);
  if (c.entry == SCORE_TRIE) {
    g_ws_bytes = gram_workspace_bytes_trie(m, B, N, L, K * T);
    trace_line("gram_workspace_bytes_trie", g_ws_bytes);
  }
  if (c.entry == SBS) {
    g_ws_bytes = gram_workspace_bytes_sbs(m, B, N, L, K, T, trie.max_fanout);
    trace_line("gram_workspace_bytes_sbs", g_ws_bytes);
  }
  gram_trie_tail_t tail{nullptr, 2, 2};
  if (c.tail_rows) {
    tail.sub_rows = fake<int32_t>();  // (only here: the other cases' fake addresses stay what their goldens recorded)
    // rows, entries, most rows of a user, 0; then the even users' levels (4 and rows - 7) and, 16 entries on, the odd users' (3 and 0)
    g_tail_script = {c.tail_rows, (c.tail_rows + 63) / 64 + 1, c.tail_rows - 3, 0, 4, c.tail_rows - 7};
    g_tail_script.resize(4 + GRAM_TAIL_MAX_STEPS, 0);
    g_tail_script.push_back(3);
    gram_debug_set_tail_pass(1);  // (whatever GRAM_TAIL_PASS says in the caller's environment)
    if (c.forest_attn) gram_debug_set_tail_forest_attn(1);
    g_ws_bytes = gram_workspace_bytes_tail(m, B, N, L, K, T, tail.steps);
    trace_line("gram_workspace_bytes_tail", g_ws_bytes);
  }
  g_ws = (char*)calloc(g_ws_bytes, 1);  // zeroed, and touched only where a stub writes: a large case costs address space alone
  int32_t width = -1;
  void* io[5] = {fake(), fake(), fake(), fake(), fake()};  // the remaining inputs and outputs of the entry, in its argument order
  switch (c.entry) {
    case GENERATE:
      if (c.bias) {
        // (the filter's tables first, as in the items case below: the addresses of generate_p2_items; the potentials behind them)
        const gram_user_items_t items{c.items ? fake<int32_t>() : nullptr, c.items ? fake<int32_t>() : nullptr,
                                      c.items ? fake<int32_t>() : nullptr, c.items ? fake<int32_t>() : nullptr, 64, GRAM_ITEMS_EXCLUDE};
        return gram_generate_bias(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, fake<float>(),
                                  c.bias == 2 ? trie.n_nodes : 0, c.items ? &items : nullptr, g_ws, g_ws_bytes, (int64_t*)io[0],
                                  (float*)io[1], &width, st);
      }
      if (c.groups)
        return gram_generate_groups(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, c.groups, 0.5f, nullptr, g_ws,
                                    g_ws_bytes, (int64_t*)io[0], (float*)io[1], &width, st);
      if (c.umask) {  // (27 leaves: one record, in a row of two)
        const gram_user_mask_t um{fake<int32_t>(), fake<int32_t>(), fake<uint32_t>(), 2, 27};
        return gram_generate_mask(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, &um, g_ws, g_ws_bytes,
                                  (int64_t*)io[0], (float*)io[1], &width, st);
      }
      if (c.items) {
        const gram_user_items_t items{fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), 64, GRAM_ITEMS_EXCLUDE};
        return gram_generate_items(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, &items, g_ws, g_ws_bytes,
                                   (int64_t*)io[0], (float*)io[1], &width, st);
      }
      if (c.tail_rows)
        return gram_generate_tail(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, &tail, g_ws, g_ws_bytes,
                                  (int64_t*)io[0], (float*)io[1], &width, st);
      return gram_generate_ex(m, ids, mask, B, N, L, K, K, T, 1.f, &trie, c.comp ? &comp : nullptr, g_ws, g_ws_bytes, (int64_t*)io[0],
                              (float*)io[1], &width, st);
    case SBS: {
      const int64_t* user_keys = fake<int64_t>();  // (only here: the other cases' fake addresses stay what their goldens recorded)
      float* perturbed = fake<float>();
      const uint64_t seed = 0x0123456789abcdefull;
      if (c.items) {
        const gram_user_items_t items{fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), 64, GRAM_ITEMS_EXCLUDE};
        return gram_generate_sbs_items(m, ids, mask, B, N, L, K, T, &trie, c.comp ? &comp : nullptr, &items, 0.5f, seed, user_keys, g_ws,
                                       g_ws_bytes, (int64_t*)io[0], (float*)io[1], (float*)io[2], perturbed, &width, st);
      }
      return gram_generate_sbs(m, ids, mask, B, N, L, K, T, &trie, c.comp ? &comp : nullptr, 0.5f, seed, user_keys, g_ws, g_ws_bytes,
                               (int64_t*)io[0], (float*)io[1], (float*)io[2], perturbed, &width, st);
    }
    case ENCODE_FUSED:
      return gram_encode_fused(m, ids, mask, B, N, L, g_ws, g_ws_bytes, K, T, io[0], st);
    case ENCODE_PASSAGES:
      return gram_encode_passages(m, ids, mask, B, L, g_ws, g_ws_bytes, (float*)io[0], st);
    case DECODE_STEP:
      return gram_decode_step(m, (int32_t*)io[0], (int32_t*)io[1], mask, B, N, L, K, T, /*t=*/1, g_ws, g_ws_bytes, (float*)io[2], st);
    case TEACHER_FORCED:
      if (c.attn == 3) {
        const gram_xattn_scores_t scores{fake<float>(), fake<float>()};
        return gram_teacher_forced_scores(m, ids, mask, B, N, L, nullptr, (int32_t*)io[0], (int32_t*)io[1], K, T, g_ws, g_ws_bytes, nullptr,
                                          (float*)io[3], (float*)io[4], &scores, st);
      }
      if (c.attn) {
        const gram_xattn_out_t attn = c.attn == 1 ? gram_xattn_out_t{fake<float>(), nullptr, nullptr, nullptr}
                                                  : gram_xattn_out_t{nullptr, fake<float>(), fake<float>(), fake<float>()};
        return gram_teacher_forced_ex(m, ids, mask, B, N, L, nullptr, (int32_t*)io[0], (int32_t*)io[1], K, T, g_ws, g_ws_bytes, nullptr,
                                      (float*)io[3], (float*)io[4], &attn, st);
      }
      return gram_teacher_forced(m, ids, mask, B, N, L, c.comp ? &comp : nullptr, (int32_t*)io[0], (int32_t*)io[1], K, T, g_ws, g_ws_bytes,
                                 c.logits ? (float*)io[2] : nullptr, (float*)io[3], (float*)io[4], st);
    case SCORE_TRIE: {
      const gram_trie_rows_t rows{fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), fake<int32_t>(), fake<int32_t>(),
                                  fake<int32_t>(), K * T, T, trie.n_nodes, 27};
      return gram_score_trie(m, ids, mask, B, N, L, c.comp ? &comp : nullptr, &trie, &rows, g_ws, g_ws_bytes, (float*)io[3], (float*)io[4], st);
    }
  }
  return GRAM_E_ARG;
}
}  // namespace

int main(int argc, char** argv) {
  for (const Case& c : kCases) {
    if (argc == 2 && !strcmp(argv[1], "--list")) puts(c.name);
    if (argc == 2 && !strcmp(argv[1], c.name)) {
      trace_line("return", run(c));
      return 0;
    }
  }
  return argc == 2 && !strcmp(argv[1], "--list") ? 0 : 2;
}
