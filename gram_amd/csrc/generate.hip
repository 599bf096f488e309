// generate.hip -- host-side orchestration of the scoring path behind the C ABI: the model
// handle, the workspace carve, and the encode -> fuse -> bank -> decode-loop launch sequences.
// Nothing here allocates device memory or synchronises (except the optional 4-byte width read
// at the end of gram_generate); every launch goes to the caller's stream, so the whole
// generate() is one stream-ordered launch train.
//
// Reference call graph being replaced:
//   GRAM.generate gram.py:74-107 -> EncoderWrapper.forward gram.py:200-256 -> T5Stack (encoder)
//   gram_t5_modeling.py:1037-1296 -> HF beam_search -> per step
//   T5ForConditionalGeneration_GRAM.forward gram_t5.py:118-287 -> T5Stack (decoder) -> lm_head.
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "common.h"
#include "prof.h"

struct gram_model {
  gram_model_desc_t d;
  std::vector<const float*> enc_ln1, enc_ln2, dec_ln1, dec_ln2, dec_ln3;
  std::vector<const void*> enc_wqkv, enc_wo, enc_wi, enc_wo2, dec_wqkv, dec_wo, dec_wq_x, dec_wo_x, dec_wi, dec_wo2;
  // 1 / (power-of-two factor a weight matrix was scaled by) = the out_scale of its GEMM (gram_model_desc_t.w_scales)
  std::vector<float> s_enc_wqkv, s_enc_wo, s_enc_wi, s_enc_wo2, s_dec_wqkv, s_dec_wo, s_dec_wq_x, s_dec_wo_x, s_dec_wi, s_dec_wo2;
  float s_wkv = 1.f, s_lm = 1.f;
  // layer 0's q|k|v per token (gram_model_build_token_tables), [pieces][vocab][3 * inner] each; null: none, layer 0 runs its QKV GEMM
  const p16 *enc_qkv0 = nullptr, *dec_qkv0 = nullptr;
  // longest passage the whole-path entry points take (gram_model_set_max_passage_len); above GRAM_MAX_PASSAGE_LEN the encoder's
  // self-attention is the long kernel at every L
  int max_L = GRAM_MAX_PASSAGE_LEN;
  // longest fused context N * L they take (gram_model_set_max_fused_len); above GRAM_MAX_FUSED_LEN the cross-attention is the long
  // form (xattn_long.hip) at every S
  int max_S = GRAM_MAX_FUSED_LEN;
  bool long_xattn() const { return max_S > GRAM_MAX_FUSED_LEN; }
};

namespace {

struct Carve {
  char* base;
  int64_t off;
  explicit Carve(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(int64_t n) {
    off = (off + 255) & ~(int64_t)255;
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * (int64_t)sizeof(T);
    return p;
  }
};

// The folded-norm partial sums of squares are [rows][d / 64] floats, or -- "quarter" layout of the streaming small-M GEMM, chosen per
// CALL from the rows that call works on (all of them, the compacted encoder rows, the live rows of a late decode step) --
// [rows_of_the_call][d / 16] with rows_of_the_call <= gram_gemm_stream_max_m() <= kStreamRowsLimit.  The buffer holds the larger of
// the two for every count the full row number allows, whatever GRAM_GEMM_STREAM_MAXM says.
constexpr int64_t kStreamRowsLimit = GRAM_STREAM_MAX_M_LIMIT;  // (common.h: gram_gemm_stream_max_m() never exceeds it)
inline int64_t ss_floats(int64_t rows, int64_t d) {
  const int64_t q = (rows < kStreamRowsLimit ? rows : kStreamRowsLimit) * (d / 16), full = rows * (d / 64);
  return q > full ? q : full;
}
// The per-row buffers of one T5 stack (the encoder's passages * L rows, the decoder's rows), in carve order
struct Rows {
  float* x;      // [rows][d]        residual stream (fp32)
  p16* h;        // [rows][d]        normed activations -- folded norm: the 16-bit copy of x -- the A operand of the in-GEMMs
  p16* qkv;      // [rows][3*inner]
  p16* attn;     // [rows][inner]
  p16* qx;       // [rows][inner]    decoder only: the cross-attention's queries
  p16* u;        // [rows][d_ff]
  float* ss;     // [rows][d/64]     folded-norm partial sums of squares (16-column partials for a small-M call: ss_floats)
  float* rs;     // [rows]           1/rms per row
  float* xs[2];  // [rows] x 2       per-row power-of-two factors of the 16-bit copy of x (gram_norm_fusion_t.xs_in / xs_out), ping-pong
  int64_t ps_qkv, ps_qx;  // two-piece mode: elements between the planar pieces of qkv and of qx
};
struct Workspace {
  Rows enc, dec;
  // fused bank
  p16* bank_k;     // [layers][B][H][S][64]
  p16* bank_vt;    // [layers][B][H][S/32][64][32]
  // decoder
  p16* kcache;     // [layers][Tmax][R][inner]
  p16* vcache;
  float* logits;    // [R][V]
  float* lse;       // [R]
  float* lse_part;  // [R][V/64][2]
  // beam state
  gram_beam_state_t beam;
  gram_live_rows_t live;
  int32_t* width;
  uint32_t* key_bits;  // [B][128]  the cross-attention's bit view of the mask (gram_mask_key_bits), once per generate
                       // (a handle with a raised fused limit: [B][GRAM_KEY_BITS_LONG_STRIDE], gram_mask_key_bits_long)
  float* xa_scratch;   // such a handle only: the long cross-attention's partials (gram_cross_attn_long_scratch_bytes)
  int32_t* rowmap;     // teacher-forced pass only: gram_cross_attn_rows_split's row tables [B * (1 + 2 * GRAM_MAX_BEAMS)]
  int64_t bytes;
  // the tail pass (gram_generate_tail; carve_tail): the forest and its decoder rows, BEHIND `bytes` -- nothing above moves
  gram_forest_t forest;
  Rows tail;
  float *tail_lse, *tail_lse_part;
  int64_t tail_bytes;  // 0: not carved
  // two-piece mode (gram_split_t): what a GEMM reads (h, attn, u) is ONE interleaved buffer of twice the row length;
  // what only attention kernels read (qkv, qx, the bank, the cache) is `pieces` planar copies, these many elements apart
  int pieces;
  int64_t ps_bank, ps_cache;
};

Rows take_rows(Carve& cv, const gram_model_desc_t& c, int64_t P, int64_t rows, bool decoder) {
  const int64_t d = c.d_model, inner = (int64_t)c.n_heads * 64;
  Rows r{};
  r.ps_qkv = rows * 3 * inner;
  r.ps_qx = rows * inner;
  r.x = cv.take<float>(rows * d);
  r.h = cv.take<p16>(P * rows * d);
  r.qkv = cv.take<p16>(P * r.ps_qkv);
  r.attn = cv.take<p16>(P * rows * inner);
  if (decoder) r.qx = cv.take<p16>(P * r.ps_qx);
  r.u = cv.take<p16>(P * rows * c.d_ff);
  r.ss = cv.take<float>(ss_floats(rows, d));
  r.rs = cv.take<float>(rows);
  r.xs[0] = cv.take<float>(rows);
  r.xs[1] = cv.take<float>(rows);
  return r;
}
// the key bits of B users, and on a handle with a raised fused limit the long cross-attention's scratch for `rows` (user, row) slots
void take_key_bits(Carve& cv, Workspace& w, const gram_model* m, int64_t B, int64_t rows, int S) {
  if (!m->long_xattn()) {
    w.key_bits = cv.take<uint32_t>(B * 128);
    return;
  }
  w.key_bits = cv.take<uint32_t>(B * GRAM_KEY_BITS_LONG_STRIDE);
  const int64_t n = gram_cross_attn_long_scratch_bytes((int)rows, m->d.n_heads, S) / (int64_t)sizeof(float);
  w.xa_scratch = n > 0 ? cv.take<float>(n) : nullptr;  // (S <= 4096: one segment, nothing to merge)
}
void take_bank(Carve& cv, Workspace& w, const gram_model_desc_t& c, int64_t B, int64_t S) {
  w.ps_bank = c.n_dec_layers * B * c.n_heads * S * 64;
  w.bank_k = cv.take<p16>(w.pieces * w.ps_bank);
  w.bank_vt = cv.take<p16>(w.pieces * w.ps_bank);
}

Workspace carve(const gram_model* m, void* ws, int B, int N, int L, int K, int Tmax) {
  const gram_model_desc_t& c = m->d;
  const int64_t inner = (int64_t)c.n_heads * 64, V = c.vocab, R = (int64_t)B * K, nl = c.n_dec_layers;
  Carve cv(ws);
  Workspace w{};
  const int64_t P = w.pieces = c.pieces > 1 ? c.pieces : 1;
  w.enc = take_rows(cv, c, P, (int64_t)B * N * L, false);
  take_bank(cv, w, c, B, (int64_t)N * L);
  w.dec = take_rows(cv, c, P, R, true);
  w.ps_cache = nl * Tmax * R * inner;
  w.kcache = cv.take<p16>(P * w.ps_cache);
  w.vcache = cv.take<p16>(P * w.ps_cache);
  w.logits = cv.take<float>(R * V);
  w.lse = cv.take<float>(R);
  w.lse_part = cv.take<float>(R * (V / 64) * 2);
  gram_beam_state_t& s = w.beam;
  s.B = B;
  s.K = K;
  s.Tmax = Tmax;
  s.length_penalty = 1.f;
  s.eos = 1;
  s.pad = 0;
  s.tokens = cv.take<int32_t>(R);
  s.node = cv.take<int32_t>(R);
  s.beam_scores = cv.take<float>(R);
  s.seq = cv.take<int32_t>(R * Tmax);
  s.anc = cv.take<int32_t>((int64_t)Tmax * R);
  s.done = cv.take<int32_t>(B);
  s.n_hyps = cv.take<int32_t>(B);
  s.hyp_score = cv.take<double>((int64_t)B * (K + 1));
  s.worst = cv.take<double>(B);
  s.hyp_len = cv.take<int32_t>((int64_t)B * (K + 1));
  s.hyp_tok = cv.take<int32_t>((int64_t)B * (K + 1) * Tmax);
  s.error = cv.take<int32_t>(4);
  // scratch of the small-batch sparse-logits kernel (gram_beam_state_t.cand_logits): 16 384 >= any K * max_fanout of the one-shot search step (wider steps stream: no scratch)
  s.cand_logits_users = B < 16 ? B : 16;
  s.cand_logits_stride = 16384;
  s.cand_logits = cv.take<float>((int64_t)s.cand_logits_users * s.cand_logits_stride);
  w.live.rows = cv.take<int32_t>(R);
  w.live.rowpos = cv.take<int32_t>(R);
  w.live.users = cv.take<int32_t>(B);
  w.live.tokens = cv.take<int32_t>(R);
  w.live.counts = cv.take<int32_t>(4);
  w.width = cv.take<int32_t>(4);
  take_key_bits(cv, w, m, B, R, N * L);
  w.bytes = (cv.off + 255) & ~(int64_t)255;
  return w;
}

// The forest of the tail pass behind a carve()d workspace: capacity 5/4 * B * K * steps rows (measured on the bench: 0.81 * B * K *
// steps on average over 4096 users, 0.93 for the largest user -- which is what a call of one user needs: 80 of its 125 at B = 1), one cross-attention entry per 64 rows of a
// user (so at most cap_rows / 64 + B), the decoder's per-row buffers for that many rows and their LSE partials.
void carve_tail(const gram_model* m, void* ws, Workspace& w, int B, int K, int steps) {
  const gram_model_desc_t& c = m->d;
  const int64_t V = c.vocab, R = (int64_t)B * K;
  Carve cv(ws);
  cv.off = w.bytes;
  const int64_t cap = (5 * R * steps + 3) / 4, ents = cap / GRAM_TAIL_ENTRY_ROWS + B;
  gram_forest_t& f = w.forest;
  f.cap_rows = (int32_t)cap;
  f.cap_entries = (int32_t)ents;
  f.tokens = cv.take<int32_t>(cap);
  f.pos = cv.take<int32_t>(cap);
  f.parent = cv.take<int32_t>(cap);
  f.root = cv.take<int32_t>(cap);
  f.node = cv.take<int32_t>(cap);
  f.user_off = cv.take<int32_t>(B + 1);
  f.ent_off = cv.take<int32_t>(B + 1);
  f.ent_users = cv.take<int32_t>(ents);
  f.ent_rows = cv.take<int32_t>(ents * GRAM_TAIL_ENTRY_ROWS);
  f.rowpos = cv.take<int32_t>(R);
  f.counts = cv.take<int32_t>(4 + 2 * GRAM_TAIL_MAX_STEPS);
  f.n_levels = steps;
  f.slot = cv.take<int32_t>(cap);
  f.lvl_rows = cv.take<int32_t>(2 * cap * steps);
  f.lvl_tokens = cv.take<int32_t>(2 * cap * steps);
  f.lvl_anc = cv.take<int32_t>(2 * (int64_t)steps * GRAM_MAX_DEC_LEN * R);
  w.tail = take_rows(cv, c, w.pieces, cap, true);
  w.tail_lse = cv.take<float>(cap);
  w.tail_lse_part = cv.take<float>(cap * (V / 64) * 2);
  w.tail_bytes = (cv.off + 255) & ~(int64_t)255;
}
inline bool tail_shape_ok(int B, int K, int steps) {
  return steps >= 1 && steps <= GRAM_TAIL_MAX_STEPS && 5 * (int64_t)B * K * steps / 4 + 1 <= INT32_MAX / 4;
}

int check_shapes(const gram_model* m, int B, int N, int L, int K, int Tmax) {
  if (!m || B < 1 || N < 1 || N > m->d.max_passages || L < 32 || L > m->max_L || (L & 31) || N * L > m->max_S || K < 1 ||
      K > GRAM_MAX_BEAMS || Tmax < 2 || Tmax > GRAM_MAX_DEC_LEN)
    return GRAM_E_ARG;
  return 0;
}

constexpr int kPrecomputedRsRows = 32768;  // = the row count from which gemm.hip dispatches to the ping-pong kernel

#define TRY(x)            \
  do {                    \
    int e__ = (x);        \
    if (e__) return e__;  \
  } while (0)

// Sensitivity sweeps (gram_debug_set_stage_pieces): stage s computes on its first g_stage_cap[s] pieces only.  Implemented by ZEROING
// the upper piece of the stage's activation operands before they are consumed (a zero piece contributes exact zeros to every product
// it enters, so the arithmetic is that of one piece; the kernels and their cost are unchanged) -- the weights' upper piece is
// zeroed by the caller when it expands them.  Debug only: every cap costs a memset per use.
int g_stage_cap[GRAM_STAGE_COUNT] = {99, 99, 99, 99, 99, 99, 99, 99};
// planar buffer: `pieces` copies, ps elements apart
int cap_planar(const Workspace& w, void* buf, int64_t ps, int stage, void* st) {
  if (w.pieces < 2 || g_stage_cap[stage] >= 2) return 0;
  hipError_t e = hipMemsetAsync((p16*)buf + (size_t)ps, 0, (size_t)ps * sizeof(p16), (hipStream_t)st);
  return e == hipSuccess ? 0 : (int)e;
}
// interleaved buffer [rows][cols / 32][2][32]: piece 1 = the second 64 B of every 128 B
int cap_inter(const Workspace& w, void* buf, int64_t rows, int64_t cols, int stage, void* st) {
  if (w.pieces < 2 || g_stage_cap[stage] >= 2) return 0;
  hipError_t e = hipMemset2DAsync((char*)buf + 64, 128, 0, 64, (size_t)(rows * cols / 32), (hipStream_t)st);
  return e == hipSuccess ? 0 : (int)e;
}

// One Linear of the path.  Two-piece mode: A is the interleaved [M][2 kc] buffer, W the interleaved weight; a 16-bit C is written
// planar (c_kind 1: c_ps elements apart -- an attention kernel reads it) or interleaved (c_kind 2: [M][2 N], the next GEMM's A);
// the xb copy of a residual epilogue (nf) is always interleaved, the bank planar.
enum { C_NONE = 0, C_PLANAR = 1, C_INTER = 2 };
int linear(const Workspace& w, const void* A, const void* W, float out_scale, void* C, int c_kind, int64_t c_ps, int M, int N, int kc, int epi,
           const gram_kv_bank_t* bank, const gram_norm_fusion_t* nf, void* st) {
  const int P = w.pieces;
  const gram_split_t sp{P, c_kind == C_INTER, c_ps, w.ps_bank, out_scale};
  return gram_gemm_bf16_split(A, W, C, M, N, kc, P * kc, c_kind == C_INTER ? P * N : N, epi, bank, nf, &sp, st);
}

// The chain of T5LayerNorms of one stack over n rows of r: the embedding, "the norm in front of this consumer GEMM" and "the fusion
// struct of a residual GEMM".  Folded (gram_norm_fusion_t): r.h holds xb = the 16-bit copy of x, r.ss the per-row sum-of-squares
// partials; both are refreshed by every residual GEMM's epilogue.  Unfolded (one piece only: gram_model_create insists on fold_norm in
// the two-piece mode; the A/B and debugging path): a norm kernel with the layer's gain, and no fusion struct anywhere.
struct NormChain {
  const gram_model_desc_t& c;
  const Workspace& w;
  const Rows& r;
  const int n, d;
  void* const st;
  // few rows (one short user, a late decode step): the streaming GEMM and its 16-column partials (gram_norm_fusion_t.quarter); the
  // embedding writes 64-column ones
  const int quarter;
  // big problems (the ping-pong GEMMs, M >= kPrecomputedRsRows) take 1/rms precomputed per row by one tiny kernel per norm; below
  // that the consumer GEMM adds the partials itself (same order, same bits) and the launch is saved -- a small batch is a chain of
  // ~1 500 dependent launches and nothing else
  const bool pre_rs;
  // The 16-bit copy of the residual stream carries a power-of-two factor per row (gram_norm_fusion_t.xs_in / xs_out): T5's stream
  // leaves the IEEE-half range in trained checkpoints.  Norm point p: the producer before it scaled the copy by xs[p & 1]; the
  // consumer divides its row scale by that and publishes the factor of the NEXT producer in xs[(p + 1) & 1].  One norm point per
  // consumer, counted across the layers of the stack.
  int np = 0;

  NormChain(const gram_model* m, const Workspace& w, const Rows& r, int n, void* st)
      : c(m->d), w(w), r(r), n(n), d(c.d_model), st(st),
        quarter(c.fold_norm && n <= gram_gemm_stream_max_m() && d % 128 == 0 && (c.n_heads * 64) % 128 == 0 && c.d_ff % 128 == 0),
        pre_rs(n >= kPrecomputedRsRows) {}

  // want_xb false: the first consumer reads a token table, not the 16-bit copy (the copy's row factor is still published)
  int embed(const void* ids, int ids_are_i64, bool want_xb = true) {
    if (c.fold_norm)
      return gram_embed_ex_xs(c.embed_f32, ids, ids_are_i64, r.x, want_xb ? r.h : nullptr, r.ss, r.xs[0], d / 64, n, d, w.pieces, st);
    return ids_are_i64 ? gram_embed_i64(c.embed_f32, (const int64_t*)ids, r.x, n, d, st)
                       : gram_embed_i32(c.embed_f32, (const int32_t*)ids, r.x, n, d, st);
  }
  // The norm in front of a consumer GEMM: launches what has to run before it (big path: 1/rms / xs and the next factor; unfolded: the
  // norm itself) and returns in *pnf what the GEMM takes, nf or null.  The first consumer after the embedding reads 64-column partials.
  // no_gemm (folded norm, from_embed): a token table stands in for the consumer GEMM, so what that GEMM does besides its product on
  // the small path -- publishing the next producer's row factor -- is left to the big path's kernel (same order, same bits)
  int norm(const float* gain, bool from_embed, gram_norm_fusion_t& nf, const gram_norm_fusion_t** pnf, bool no_gemm = false) {
    float *const xs_in = r.xs[np & 1], *const xs_out = r.xs[(np + 1) & 1];
    ++np;
    *pnf = c.fold_norm ? &nf : nullptr;
    if (!c.fold_norm) return gram_rmsnorm_bf16_split(r.x, gain, r.h, n, d, c.eps, 1.f, nullptr, 1, 1, nullptr, 1, st);
    if (pre_rs || no_gemm) {
      nf = gram_norm_fusion_t{nullptr, nullptr, r.rs, 0, d, c.eps, 0, nullptr, nullptr};
      return gram_row_rscale_xs(r.ss, r.rs, xs_in, xs_out, n, d / 64, d, c.eps, st);
    }
    nf = gram_norm_fusion_t{nullptr, nullptr, r.ss, d / 64, d, c.eps, from_embed ? 0 : quarter, xs_in, xs_out};
    return 0;
  }
  // the fusion struct of the residual GEMM behind that consumer
  const gram_norm_fusion_t* residual(gram_norm_fusion_t& nf) const {
    if (!c.fold_norm) return nullptr;
    nf = gram_norm_fusion_t{r.h, r.ss, nullptr, 0, 0, 0.f, quarter, r.xs[np & 1], nullptr};
    return &nf;
  }
};

// One sublayer: x += W_out (mixer(W_in norm(x))).  The in-GEMM writes `mid` -- planar pieces mid_ps apart for an attention kernel,
// interleaved for a GEMM -- and the residual GEMM reads `a`: the mixer's output, or mid itself where there is no mixer (the FFN).
struct Sublayer {
  int stage;          // gram_stage of every operand below
  const float* gain;  // of the norm (unfolded path; folded into w_in otherwise)
  const void* w_in;
  float s_in;
  p16* mid;
  int mid_kind;  // C_PLANAR / C_INTER
  int64_t mid_ps;
  int n_mid, epi;
  const p16* a;
  int k_out;
  const void* w_out;
  float s_out;
  bool mid_from_table = false;  // layer 0 of a stack whose handle has token tables: the mixer reads q|k|v rows by token, no in-GEMM
};
template <typename Mixer>
int sublayer(NormChain& nc, const Sublayer& s, bool from_embed, Mixer mixer) {
  const Workspace& w = nc.w;
  const Rows& r = nc.r;
  const int n = nc.n, d = nc.d;
  void* const st = nc.st;
  gram_norm_fusion_t nf;
  const gram_norm_fusion_t* pnf;
  TRY(nc.norm(s.gain, from_embed, nf, &pnf, s.mid_from_table));
  if (!s.mid_from_table) {  // (a table is used only where the stage has no cap: token_table())
    TRY(cap_inter(w, r.h, n, d, s.stage, st));
    // (the unfolded path has one piece, and has always declared its in-GEMM's C planar with stride 0)
    TRY(linear(w, r.h, s.w_in, s.s_in, s.mid, pnf ? s.mid_kind : C_PLANAR, pnf ? s.mid_ps : 0, n, s.n_mid, d, s.epi, nullptr, pnf, st));
    if (s.mid_kind == C_PLANAR) TRY(cap_planar(w, s.mid, s.mid_ps, s.stage, st));
    else TRY(cap_inter(w, s.mid, n, s.n_mid, s.stage, st));
  }
  if (s.a != s.mid) {
    TRY(mixer());
    TRY(cap_inter(w, r.attn, n, s.k_out, s.stage, st));
  }
  return linear(w, s.a, s.w_out, s.s_out, r.x, C_NONE, 0, n, d, s.k_out, GRAM_EPI_F32_ADD, nullptr, nc.residual(nf), st);
}
inline int no_mixer() { return 0; }

// Layer-0 q|k|v per token (gram_hip.h, gram_model_build_token_tables).  A stack reads its table where the handle has one, the switch is
// on and the stage runs uncapped (gram_debug_set_stage_pieces zeroes operand pieces in front of the GEMM the table replaces).
int g_token_tables = -1;  // -1: the GRAM_TOKEN_TABLES environment variable decides (default on)
const p16* token_table(const gram_model* m, const p16* table, int stage) {
  if (!table || !m->d.fold_norm || g_stage_cap[stage] < 2) return nullptr;
  if (g_token_tables >= 0) return g_token_tables ? table : nullptr;
  const char* e = getenv("GRAM_TOKEN_TABLES");
  return e && e[0] == '0' ? nullptr : table;
}
inline int64_t token_table_elems(const gram_model_desc_t& c) {  // of one table, padded to the carve's 256 B
  const int64_t P = c.pieces > 1 ? c.pieces : 1;
  return (P * c.vocab * 3 * c.n_heads * 64 + 127) & ~(int64_t)127;
}

// The encoder layers on P passages (ids/mask [P][L]); leaves the residual stream in w.enc.x rows [0, P*L).
int encoder_layers(const gram_model* m, const Workspace& w, const int64_t* ids, const uint8_t* mask, int L, int P, void* st) {
  const gram_model_desc_t& c = m->d;
  const int inner = c.n_heads * 64, F = c.d_ff;
  const Rows& r = w.enc;
  NormChain nc(m, w, r, P * L, st);
  const p16* const table = token_table(m, m->enc_qkv0, GRAM_STAGE_ENC_ATTN);
  TRY(nc.embed(ids, 1, !table));
  for (int i = 0; i < c.n_enc_layers; ++i) {
    const p16* const tab = i == 0 ? table : nullptr;
    TRY(sublayer(nc, {GRAM_STAGE_ENC_ATTN, m->enc_ln1[i], m->enc_wqkv[i], m->s_enc_wqkv[i], r.qkv, C_PLANAR, r.ps_qkv, 3 * inner,
                      GRAM_EPI_BF16, r.attn, inner, m->enc_wo[i], m->s_enc_wo[i], tab != nullptr},
                 i == 0, [&] {  // (unfolded: stride 0, as for the GEMM in front)
                   if (m->max_L > GRAM_MAX_PASSAGE_LEN) {  // a long-mode handle: the tiled kernel at every L
                     if (tab)
                       return gram_enc_self_attn_long_rows_split(tab, ids, c.enc_bias_f32, mask, r.attn, P, L, c.n_heads, w.pieces,
                                                                 (int64_t)c.vocab * 3 * inner, st);
                     return gram_enc_self_attn_long_split(r.qkv, c.enc_bias_f32, mask, r.attn, P, L, c.n_heads, w.pieces,
                                                          c.fold_norm ? r.ps_qkv : 0, st);
                   }
                   if (tab)
                     return gram_enc_self_attn_rows_split(tab, ids, c.enc_bias_f32, mask, r.attn, P, L, c.n_heads, w.pieces,
                                                          (int64_t)c.vocab * 3 * inner, st);
                   return gram_enc_self_attn_split(r.qkv, c.enc_bias_f32, mask, r.attn, P, L, c.n_heads, w.pieces,
                                                   c.fold_norm ? r.ps_qkv : 0, st);
                 }));
    TRY(sublayer(nc, {GRAM_STAGE_ENC_FFN, m->enc_ln2[i], m->enc_wi[i], m->s_enc_wi[i], r.u, C_INTER, 0, F, GRAM_EPI_BF16_RELU, r.u, F,
                      m->enc_wo2[i], m->s_enc_wo2[i]},
                 false, no_mixer));
  }
  return 0;
}

struct CachedPassages {  // gram_compaction_t's cache fields
  int n;
  int cache_L;
  const float* x;
  const int32_t* slot;
};

// P passages (all B*N, or the active ones with their flat indices in pmap): the first P - cached.n go through the
// encoder (ids/mask [P - cached.n][L]), the rest take their residual-stream rows from the passage cache.
int encode(const gram_model* m, const Workspace& w, const int64_t* ids, const uint8_t* mask, const uint8_t* full_mask, int B, int N,
           int L, int P, const int32_t* pmap, const CachedPassages& cached, void* st) {
  const gram_model_desc_t& c = m->d;
  const int d = c.d_model, inner = c.n_heads * 64, H = c.n_heads;
  const int Pe = P - cached.n, Me = P * L;
  if (m->long_xattn()) TRY(gram_mask_key_bits_long(full_mask, w.key_bits, B, N * L, st));
  else TRY(gram_mask_key_bits(full_mask, w.key_bits, B, N * L, st));
  if (Pe > 0) TRY(encoder_layers(m, w, ids, mask, L, Pe, st));
  if (cached.n > 0) TRY(gram_gather_passage_x(cached.x, cached.slot, w.enc.x + (size_t)Pe * L * d, cached.n, L, cached.cache_L, d, st));
  // final norm + per-passage position embedding = the late fusion (gram.py:238-255); the
  // (B*N, L, d) -> (B, N*L, d) view is free: rows are already user-major.
  TRY(gram_rmsnorm_bf16_split(w.enc.x, c.enc_final_ln, w.enc.h, Me, d, c.eps, 1.f, c.use_position_embedding ? c.pos_emb_f32 : nullptr, N, L,
                              pmap, w.pieces, st));
  // every decoder layer's cross K/V in ONE GEMM, scattered into the beam-shared bank
  gram_kv_bank_t bank{w.bank_k, w.bank_vt, c.n_dec_layers, B, H, N * L, pmap, N, L};
  TRY(linear(w, w.enc.h, c.dec_wkv_x_all, m->s_wkv, nullptr, C_NONE, 0, Me, c.n_dec_layers * 2 * inner, d, GRAM_EPI_KV_BANK, &bank, nullptr, st));
  TRY(cap_planar(w, w.bank_k, w.ps_bank, GRAM_STAGE_BANK_K, st));
  TRY(cap_planar(w, w.bank_vt, w.ps_bank, GRAM_STAGE_BANK_V, st));
  return 0;
}

int check_compaction(const gram_compaction_t* comp, int B, int N) {
  if (!comp) return 0;
  const int n_enc = comp->n_active - comp->n_cached;
  if (comp->n_active < B || comp->n_active > B * N || !comp->passage_map || comp->n_cached < 0 || n_enc < 0) return GRAM_E_ARG;
  if (n_enc > 0 && (!comp->ids || !comp->mask)) return GRAM_E_ARG;
  if (comp->n_cached > 0 && (!comp->cache_x || !comp->cache_slot || comp->cache_L < 1)) return GRAM_E_ARG;
  return 0;
}

// encode() on every passage (comp NULL), or on the active passages only: the padded ones leave their bank positions untouched (never read)
int encode_call(const gram_model* m, const Workspace& w, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                const gram_compaction_t* comp, void* st) {
  if (comp)
    return encode(m, w, comp->ids, comp->mask, mask, B, N, L, comp->n_active, comp->passage_map,
                  CachedPassages{comp->n_cached, comp->cache_L, comp->cache_x, comp->cache_slot}, st);
  return encode(m, w, input_ids, mask, mask, B, N, L, B * N, nullptr, CachedPassages{0, 0, nullptr, nullptr}, st);
}
struct LiveStep {  // host view of gram_live_rows_t after the counts came back
  int n_rows, n_users;
  const int32_t *rows, *rowpos, *users;
};

// The decoder layers on n rows (tokens i32 [n]).  self_attn(i) and cross_attn(i) launch layer i's attention from w.dec.qkv / w.dec.qx
// into w.dec.attn: one position over the cache and one row per beam (decode_step), or whole sequences (decoder_tf).
// qkv0_from_table: self_attn(0) reads the rows `tokens` of the decoder's token table instead of w.dec.qkv.
template <typename SelfAttn, typename CrossAttn>
int decoder_layers(const gram_model* m, const Workspace& w, const int32_t* tokens, int n, bool qkv0_from_table, SelfAttn self_attn,
                   CrossAttn cross_attn, void* st) {
  const gram_model_desc_t& c = m->d;
  const int inner = c.n_heads * 64, F = c.d_ff;
  const Rows& r = w.dec;
  NormChain nc(m, w, r, n, st);
  TRY(nc.embed(tokens, 0, !qkv0_from_table));
  for (int i = 0; i < c.n_dec_layers; ++i) {
    TRY(sublayer(nc, {GRAM_STAGE_DEC_SELF, m->dec_ln1[i], m->dec_wqkv[i], m->s_dec_wqkv[i], r.qkv, C_PLANAR, r.ps_qkv, 3 * inner,
                      GRAM_EPI_BF16, r.attn, inner, m->dec_wo[i], m->s_dec_wo[i], i == 0 && qkv0_from_table},
                 i == 0, [&] { return self_attn(i); }));
    TRY(sublayer(nc, {GRAM_STAGE_DEC_CROSS, m->dec_ln2[i], m->dec_wq_x[i], m->s_dec_wq_x[i], r.qx, C_PLANAR, r.ps_qx, inner,
                      GRAM_EPI_BF16, r.attn, inner, m->dec_wo_x[i], m->s_dec_wo_x[i]},
                 false, [&] { return cross_attn(i); }));
    TRY(sublayer(nc, {GRAM_STAGE_DEC_FFN, m->dec_ln3[i], m->dec_wi[i], m->s_dec_wi[i], r.u, C_INTER, 0, F, GRAM_EPI_BF16_RELU, r.u, F,
                      m->dec_wo2[i], m->s_dec_wo2[i]},
                 false, no_mixer));
  }
  return 0;
}

// Final norm with the tied-embedding scale, then the lm_head GEMM on n decoder rows: with lse_part the log-softmax normaliser partials
// come straight from the accumulators and logits may be NULL (not stored); without, plain fp32 logits.
int lm_head(const gram_model* m, const Workspace& w, int n, float* logits, float* lse_part, void* st) {
  const gram_model_desc_t& c = m->d;
  const int d = c.d_model, V = c.vocab;
  const float scale = c.tie_word_embeddings ? 1.0f / sqrtf((float)d) : 1.f;  // gram_t5.py:249-252
  TRY(gram_rmsnorm_bf16_split(w.dec.x, c.dec_final_ln, w.dec.h, n, d, c.eps, scale, nullptr, 1, 1, nullptr, w.pieces, st));
  TRY(cap_inter(w, w.dec.h, n, d, GRAM_STAGE_LM_HEAD, st));
  const gram_split_t sp{w.pieces, 0, 0, 0, m->s_lm};
  if (lse_part) return gram_gemm_bf16_lse_split(w.dec.h, c.lm_head_bf16, logits, lse_part, n, V, d, w.pieces * d, V, &sp, st);
  return gram_gemm_bf16_split(w.dec.h, c.lm_head_bf16, logits, n, V, d, w.pieces * d, V, GRAM_EPI_F32, nullptr, nullptr, &sp, st);
}

// K = beams per user in THIS step's rows (1 for the compact step 0), R_cache = rows of the cache slots.
// live != NULL: the step runs on live->n_rows compact rows (tokens = their tokens), see gram_live_rows_t.
int decode_step(const gram_model* m, const Workspace& w, const int32_t* tokens, const int32_t* anc, const uint8_t* mask, int B,
                int N, int L, int K, int R_cache, int Tmax, int t, float* logits, float* lse_part, const LiveStep* live,
                void* st) {
  const gram_model_desc_t& c = m->d;
  const int inner = c.n_heads * 64, H = c.n_heads;
  const int R = live ? live->n_rows : B * K, S = N * L;
  const size_t bank_layer = (size_t)B * H * S * 64;
  const size_t cache_layer = (size_t)Tmax * R_cache * inner;
  const Rows& r = w.dec;
  const p16* const table = token_table(m, m->dec_qkv0, GRAM_STAGE_DEC_SELF);
  TRY(decoder_layers(
      m, w, tokens, R, table != nullptr,
      [&](int i) {
        if (i == 0 && table)
          return gram_dec_self_attn_rows_split(table, tokens, w.kcache, w.vcache, anc, c.dec_bias_f32, r.attn, live ? R_cache : R, R,
                                               live ? live->rows : nullptr, H, t, Tmax, w.pieces, (int64_t)c.vocab * 3 * inner,
                                               w.ps_cache, st);
        return gram_dec_self_attn_split(r.qkv, w.kcache + i * cache_layer, w.vcache + i * cache_layer, anc, c.dec_bias_f32, r.attn,
                                        live ? R_cache : R, R, live ? live->rows : nullptr, H, t, Tmax, w.pieces, r.ps_qkv, w.ps_cache, st);
      },
      [&](int i) {
        if (m->long_xattn())
          return gram_cross_attn_long_split(r.qx, w.bank_k + i * bank_layer, w.bank_vt + i * bank_layer, mask, r.attn,
                                            live ? live->n_users : B, K, H, S, live ? live->users : nullptr,
                                            live ? live->rowpos : nullptr, w.pieces, r.ps_qx, w.ps_bank, w.key_bits, w.xa_scratch, st);
        return gram_cross_attn_decode_split(r.qx, w.bank_k + i * bank_layer, w.bank_vt + i * bank_layer, mask, r.attn,
                                            live ? live->n_users : B, K, H, S, live ? live->users : nullptr, live ? live->rowpos : nullptr,
                                            w.pieces, r.ps_qx, w.ps_bank, w.key_bits, st);
      },
      st));
  return lm_head(m, w, R, logits, lse_part, st);
}

// The search mode of a whole-path call; all of it empty: the plain search of gram_generate_ex.
struct SearchMode {
  const gram_user_items_t* items = nullptr;  // per-user item lists (gram_generate_items; optional beside groups or potentials)
  const gram_user_mask_t* umask = nullptr;   // per-user item masks (gram_generate_mask): they come alone
  const gram_trie_tail_t* tail = nullptr;    // the tail pass (gram_generate_tail): the plain search only
  int num_groups = 0;                        // > 0: group beam search (gram_generate_groups), its init and its step
  float diversity_penalty = 0.f;
  const float* phi = nullptr;                // the biased search (gram_generate_bias): the caller's potentials (gram_item_bias_table)
  int64_t phi_stride = 0;                    //   and their row stride
};

// the search step on the hidden states decode_step left in w.dec.h (rowpos: live-row step, else NULL)
int search_step(const gram_model* m, const Workspace& w, const gram_trie_t* trie, int cur_len, int rows_per_user, const int32_t* rowpos,
                const SearchMode& sm, void* st) {
  const gram_model_desc_t& c = m->d;
  const gram_user_items_t* items = sm.items;
  if (sm.umask)
    return gram_beam_step_sparse_mask(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.lm_head_f32, c.d_model, w.lse, c.vocab, cur_len,
                                      rows_per_user, rowpos, w.pieces, sm.umask, st);
  if (sm.phi)
    return gram_beam_step_bias_sparse(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.lm_head_f32, c.d_model, w.lse, c.vocab, cur_len,
                                      rows_per_user, rowpos, w.pieces, sm.phi, sm.phi_stride, items, st);
  if (sm.num_groups)
    return gram_beam_step_groups_sparse(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.lm_head_f32, c.d_model, w.lse, c.vocab, cur_len,
                                        rows_per_user, rowpos, w.pieces, sm.num_groups, sm.diversity_penalty, items, st);
  if (items) {
    if (w.pieces > 1)
      return gram_beam_step_sparse_split_items(&w.beam, trie, w.dec.h, c.lm_head_f32, c.d_model, w.lse, c.vocab, cur_len, rows_per_user,
                                               rowpos, w.pieces, items, st);
    return gram_beam_step_sparse_items(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.d_model, w.lse, c.vocab, cur_len, rows_per_user, rowpos,
                                       items, st);
  }
  if (w.pieces > 1)
    return gram_beam_step_sparse_split(&w.beam, trie, w.dec.h, c.lm_head_f32, c.d_model, w.lse, c.vocab, cur_len, rows_per_user, rowpos,
                                       w.pieces, st);
  if (rowpos) return gram_beam_step_sparse_live(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.d_model, w.lse, c.vocab, cur_len, rowpos, st);
  return gram_beam_step_sparse(&w.beam, trie, w.dec.h, c.lm_head_bf16, c.d_model, w.lse, c.vocab, cur_len, rows_per_user, st);
}

// Which self-attention the tail pass runs (gram_debug_set_tail_forest_attn).  The forest kernel is one launch per layer where the
// step-wise kernel is two per user group and level; it is taken by default from kForestAttnMinRows forest rows on, which -- like
// kTailMinBankBytes below -- is no performance crossover: the launch-train goldens and the suite's small calls with the pass forced
// on pin the level-by-level train (their forests hold up to a few thousand rows), the calls of 2049 users and the bench (330 010
// rows) lie above it.
int g_tail_forest_attn = -1;  // -1: the GRAM_TAIL_FOREST_ATTN environment variable decides, then the size
constexpr int kForestAttnMinRows = 16384;
bool tail_forest_attn_wanted(int n_rows) {
  if (g_tail_forest_attn >= 0) return g_tail_forest_attn != 0;  // (forced either way)
  const char* e = getenv("GRAM_TAIL_FOREST_ATTN");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  return n_rows >= kForestAttnMinRows;
}

// The tail pass (gram_generate_tail): decode_step's layers ONCE over the n_rows rows of the forest in w.forest -- embedding by row
// token, layer 0's q|k|v from the token table as decode_step reads it, the forest self-attention over cache and in-pass ancestors,
// the cross-attention per entry of <= 64 rows -- then the lm_head with its LSE partials.  `w` is the call's workspace with w.dec /
// w.lse / w.lse_part pointing at the forest's buffers (tail_view), so the replayed search steps read them like any step's.
int tail_pass(const gram_model* m, const Workspace& w, const uint8_t* mask, int B, int N, int L, int K, int Tmax, int t0, int n_rows,
              int n_entries, const int32_t* lvl_n, void* st) {
  const gram_model_desc_t& c = m->d;
  const int inner = c.n_heads * 64, H = c.n_heads, S = N * L, R = B * K;
  const size_t bank_layer = (size_t)B * H * S * 64;
  const size_t cache_layer = (size_t)Tmax * R * inner;
  const Rows& r = w.dec;
  const gram_forest_t& f = w.forest;
  const p16* const table = token_table(m, m->dec_qkv0, GRAM_STAGE_DEC_SELF);
  // levels the call's steps can read (a max_length that ends inside the tail leaves the deeper rows without attention)
  int nlev = f.n_levels, cut = 0;
  for (int g = 0; g < 2; ++g)
    for (int l = 0; l < f.n_levels; ++l)
      if (lvl_n[g * GRAM_TAIL_MAX_STEPS + l] > 0 && t0 + l >= Tmax - 1) cut = 1, nlev = l < nlev ? l : nlev;
  const bool forest_attn = tail_forest_attn_wanted(n_rows);
  TRY(decoder_layers(
      m, w, f.tokens, n_rows, table != nullptr,
      [&](int i) {
        if (cut) {
          hipError_t e = hipMemsetAsync(r.attn, 0, (size_t)n_rows * inner * w.pieces * sizeof(p16), (hipStream_t)st);
          if (e != hipSuccess) return (int)e;
        }
        // The forest kernel: every row in one launch, its in-pass ancestors read from their own q|k|v rows, the result written by row.
        if (forest_attn) {
          if (i == 0 && table)
            return gram_dec_self_attn_forest_split(table, f.tokens, w.kcache, w.vcache, w.beam.anc, f.pos, f.parent, f.root, c.dec_bias_f32,
                                                   r.attn, n_rows, R, H, t0, Tmax, nlev, w.pieces, (int64_t)c.vocab * 3 * inner, w.ps_cache,
                                                   st);
          return gram_dec_self_attn_forest_split(r.qkv, nullptr, w.kcache + i * cache_layer, w.vcache + i * cache_layer, w.beam.anc, f.pos,
                                                 f.parent, f.root, c.dec_bias_f32, r.attn, n_rows, R, H, t0, Tmax, nlev, w.pieces, r.ps_qkv,
                                                 w.ps_cache, st);
        }
        // The step-wise kernel, level by level: the level's rows gathered by slot (qkv_rows), their k and v written to the cache rows
        // of that position (no step reads them any more), the result -- compact, in the cross-attention's query buffer, free until its
        // GEMM -- put back by row.
        // (two groups of users, one after the other: the second reuses the first's cache rows, which nothing reads any more)
        for (int g = 0; g < 2; ++g)
          for (int l = 0; l < nlev; ++l) {
            const int n = lvl_n[g * GRAM_TAIL_MAX_STEPS + l];
            if (n < 1) continue;
            const size_t tab = ((size_t)g * f.n_levels + l) * f.cap_rows;
            const int32_t* const rows_l = f.lvl_rows + tab;
            const int32_t* const anc_l = f.lvl_anc + ((size_t)g * f.n_levels + l) * Tmax * R;
            if (i == 0 && table)
              TRY(gram_dec_self_attn_rows_split(table, f.lvl_tokens + tab, w.kcache, w.vcache, anc_l, c.dec_bias_f32, r.qx, R, n, nullptr, H,
                                                t0 + l, Tmax, w.pieces, (int64_t)c.vocab * 3 * inner, w.ps_cache, st));
            else
              TRY(gram_dec_self_attn_rows_split(r.qkv, rows_l, w.kcache + i * cache_layer, w.vcache + i * cache_layer, anc_l, c.dec_bias_f32,
                                                r.qx, R, n, nullptr, H, t0 + l, Tmax, w.pieces, r.ps_qkv, w.ps_cache, st));
            TRY(gram_scatter_rows(r.qx, rows_l, r.attn, n, inner * w.pieces * (int)sizeof(p16), n_rows, st));
          }
        return 0;
      },
      [&](int i) {
        return gram_cross_attn_entries_split(r.qx, w.bank_k + i * bank_layer, w.bank_vt + i * bank_layer, mask, r.attn, n_entries, K, H, S,
                                             f.ent_users, f.ent_rows, w.pieces, r.ps_qx, w.ps_bank, w.key_bits, st);
      },
      st));
  TRY(lm_head(m, w, n_rows, nullptr, w.lse_part, st));
  return gram_lse_combine(w.lse_part, w.lse, n_rows, c.vocab / 64, st);
}
Workspace tail_view(const Workspace& w) {
  Workspace v = w;
  v.dec = w.tail;
  v.lse = w.tail_lse;
  v.lse_part = w.tail_lse_part;
  return v;
}

int g_tail_pass = -1;  // -1: the GRAM_TAIL_PASS environment variable decides (default on)
int g_tail_cap = 0;    // gram_debug_set_tail_capacity
int g_tail_level_cap = 0;  // gram_debug_set_tail_level_capacity
int32_t g_tail_last[4] = {0, 0, 0, 0};  // gram_debug_tail_last
// Which calls take the pass by default.  Measured (profiles/tail_pass_bench_ab.txt) the pass is faster at every batch tried -- B = 1:
// 17.5 -> 13.3 ms per generate, 64: 52.3 -> 44.5, 256: 110.3 -> 104.3, 4096: -33 ms -- so this is NOT a performance crossover.  The
// limit is there because the suite's tests of small calls pin the step-wise train (launches per kind, rows per GEMM, rows per
// self-attention step), and a default that replaced that train under them would need most of them rewritten.  So by default the
// pass is taken where one layer's bank holds 256 MB or more (large evaluation batches; the bench's holds 9.66 GB);
// GRAM_TAIL_PASS=1 or gram_debug_set_tail_pass(1) takes it at any size, which is what a latency-bound caller wants.
constexpr double kTailMinBankBytes = 256.0 * 1024 * 1024;
bool tail_wanted(const gram_model* m, int B, int N, int L) {
  if (g_tail_pass >= 0) return g_tail_pass != 0;  // (forced either way)
  const char* e = getenv("GRAM_TAIL_PASS");
  if (e && e[0] == '0') return false;
  if (e && e[0] == '1') return true;
  const int P = m->d.pieces > 1 ? m->d.pieces : 1;
  return 4.0 * B * m->d.n_heads * N * L * 64 * P >= kTailMinBankBytes;  // K + V^T, 16 bits, every piece
}

}  // namespace

extern "C" int gram_debug_set_tail_pass(int on) {
  g_tail_pass = on;
  return 0;
}
extern "C" int gram_debug_set_tail_forest_attn(int on) {
  g_tail_forest_attn = on;
  return 0;
}
extern "C" int gram_tail_pass_wanted(const gram_model_t* m, int B, int N, int L) {
  if (!m || B < 1 || N < 1 || L < 1) return GRAM_E_ARG;
  return tail_wanted(m, B, N, L) ? 1 : 0;
}
extern "C" int gram_debug_set_tail_capacity(int rows) {
  g_tail_cap = rows < 0 ? 0 : rows;
  return 0;
}
extern "C" int gram_debug_workspace_beam_state(const gram_model_t* m, void* workspace, int B, int N, int L, int K, int max_length,
                                               gram_beam_state_t* out) {
  if (!workspace || !out || check_shapes(m, B, N, L, K, max_length)) return GRAM_E_ARG;
  *out = carve(m, workspace, B, N, L, K, max_length).beam;
  return 0;
}
extern "C" int gram_debug_set_tail_level_capacity(int rows) {
  g_tail_level_cap = rows < 0 ? 0 : rows;
  return 0;
}
extern "C" int gram_debug_tail_last(int32_t* out4) {
  if (!out4) return GRAM_E_ARG;
  memcpy(out4, g_tail_last, sizeof(g_tail_last));
  return 0;
}

extern "C" int gram_abi_version(void) { return GRAM_ABI_VERSION; }
extern "C" int gram_piece_format(void) { return GRAM_PIECE_FORMAT; }

extern "C" int gram_debug_set_stage_pieces(const int32_t* caps, int n) {
  if (caps && n != GRAM_STAGE_COUNT) return GRAM_E_ARG;
  for (int i = 0; i < GRAM_STAGE_COUNT; ++i) g_stage_cap[i] = caps ? (caps[i] < 1 ? 1 : caps[i]) : 99;
  return 0;
}

static int g_live_rows = -1;  // -1: the GRAM_LIVE_ROWS environment variable decides (default on)
extern "C" int gram_debug_set_live_rows(int on) {
  g_live_rows = on;
  return 0;
}
extern "C" int gram_debug_set_token_tables(int on) {
  g_token_tables = on;
  return 0;
}

extern "C" gram_model_t* gram_model_create(const gram_model_desc_t* d) {
  // (x % 128 alone lets 0 and negative multiples through)
  if (!d || d->vocab < 128 || d->d_model < 128 || d->d_ff < 128 || d->vocab % 128 || d->d_model % 128 || d->d_ff % 128 ||
      d->n_heads < 1 || d->n_heads > 16 ||
      (d->n_heads * 64) % 128 || d->d_model > 1024 || d->n_enc_layers < 1 || d->n_dec_layers < 1)
    return nullptr;
  if (d->pieces < 0 || d->pieces > GRAM_MAX_PIECES || (d->pieces > 1 && (!d->lm_head_f32 || !d->fold_norm))) return nullptr;
  gram_model* m = new gram_model();
  m->d = *d;
  // the descriptor's per-layer arrays are copied into, and then point at, storage the handle owns
  auto own = [](auto& v, auto& p, int n) {
    v.assign(p, p + n);
    p = v.data();
  };
  gram_model_desc_t& c = m->d;
  own(m->enc_ln1, c.enc_ln1, c.n_enc_layers);
  own(m->enc_ln2, c.enc_ln2, c.n_enc_layers);
  own(m->enc_wqkv, c.enc_wqkv, c.n_enc_layers);
  own(m->enc_wo, c.enc_wo, c.n_enc_layers);
  own(m->enc_wi, c.enc_wi, c.n_enc_layers);
  own(m->enc_wo2, c.enc_wo2, c.n_enc_layers);
  own(m->dec_ln1, c.dec_ln1, c.n_dec_layers);
  own(m->dec_ln2, c.dec_ln2, c.n_dec_layers);
  own(m->dec_ln3, c.dec_ln3, c.n_dec_layers);
  own(m->dec_wqkv, c.dec_wqkv, c.n_dec_layers);
  own(m->dec_wo, c.dec_wo, c.n_dec_layers);
  own(m->dec_wq_x, c.dec_wq_x, c.n_dec_layers);
  own(m->dec_wo_x, c.dec_wo_x, c.n_dec_layers);
  own(m->dec_wi, c.dec_wi, c.n_dec_layers);
  own(m->dec_wo2, c.dec_wo2, c.n_dec_layers);
  {
    const float* ws = d->w_scales;
    auto take = [&](std::vector<float>& v, int n) {
      v.assign(n, 1.f);
      if (ws) {
        for (int i = 0; i < n; ++i) v[i] = 1.f / ws[i];
        ws += n;
      }
    };
    take(m->s_enc_wqkv, d->n_enc_layers);
    take(m->s_enc_wo, d->n_enc_layers);
    take(m->s_enc_wi, d->n_enc_layers);
    take(m->s_enc_wo2, d->n_enc_layers);
    take(m->s_dec_wqkv, d->n_dec_layers);
    take(m->s_dec_wo, d->n_dec_layers);
    take(m->s_dec_wq_x, d->n_dec_layers);
    take(m->s_dec_wo_x, d->n_dec_layers);
    take(m->s_dec_wi, d->n_dec_layers);
    take(m->s_dec_wo2, d->n_dec_layers);
    if (ws) {
      m->s_wkv = 1.f / ws[0];
      m->s_lm = 1.f / ws[1];
    }
    m->d.w_scales = nullptr;  // (consumed)
  }
  return m;
}

extern "C" int gram_model_set_max_passage_len(gram_model_t* m, int Lmax) {
  if (!m || Lmax < GRAM_MAX_PASSAGE_LEN || Lmax > GRAM_MAX_LONG_PASSAGE_LEN || (Lmax & 31)) return GRAM_E_ARG;
  m->max_L = Lmax;
  return 0;
}

extern "C" int gram_model_set_max_fused_len(gram_model_t* m, int Smax) {
  if (!m || Smax < GRAM_MAX_FUSED_LEN || Smax > GRAM_MAX_LONG_FUSED_LEN || (Smax & 31)) return GRAM_E_ARG;
  m->max_S = Smax;
  return 0;
}

extern "C" void gram_model_destroy(gram_model_t* m) {
  if (!m) return;
  delete m;
}

// ---- token tables (gram_model_build_token_tables) ------------------------------------------------------------------------------------
namespace {

// scratch of the build: what the embedding and the norm of `vocab` rows write, and the ids 0 .. vocab-1
struct TableScratch {
  Rows rows;
  int32_t* ids;
  int64_t bytes;
};
TableScratch carve_tables(const gram_model_desc_t& c, void* ws) {
  const int64_t P = c.pieces > 1 ? c.pieces : 1, V = c.vocab, d = c.d_model;
  Carve cv(ws);
  TableScratch t{};
  t.rows.x = cv.take<float>(V * d);
  t.rows.h = cv.take<p16>(P * V * d);
  t.rows.ss = cv.take<float>(ss_floats(V, d));
  t.rows.rs = cv.take<float>(V);
  t.rows.xs[0] = cv.take<float>(V);
  t.rows.xs[1] = cv.take<float>(V);
  t.ids = cv.take<int32_t>(V);
  t.bytes = (cv.off + 255) & ~(int64_t)255;
  return t;
}

// one stack's table by the path's own launches: the embedding of every token, the first norm, the layer-0 QKV GEMM writing planar pieces
int build_table(const gram_model* m, const Workspace& w, const TableScratch& t, const float* gain, const void* wqkv, float s_wqkv,
                p16* table, void* st) {
  const gram_model_desc_t& c = m->d;
  const int V = c.vocab, inner = c.n_heads * 64;
  NormChain nc(m, w, t.rows, V, st);
  TRY(nc.embed(t.ids, 0));
  gram_norm_fusion_t nf;
  const gram_norm_fusion_t* pnf;
  TRY(nc.norm(gain, true, nf, &pnf));
  return linear(w, t.rows.h, wqkv, s_wqkv, table, C_PLANAR, (int64_t)V * 3 * inner, V, 3 * inner, c.d_model, GRAM_EPI_BF16, nullptr, pnf, st);
}

}  // namespace

extern "C" int64_t gram_token_tables_bytes(const gram_model_t* m) {
  if (!m) return GRAM_E_ARG;
  return m->d.fold_norm ? 2 * token_table_elems(m->d) * (int64_t)sizeof(p16) : 0;
}

extern "C" int64_t gram_token_tables_workspace_bytes(const gram_model_t* m) {
  if (!m) return GRAM_E_ARG;
  return m->d.fold_norm ? carve_tables(m->d, nullptr).bytes : 0;
}

extern "C" int gram_model_build_token_tables(gram_model_t* m, void* tables, int64_t tables_bytes, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
  if (!m || !m->d.fold_norm || !tables || (reinterpret_cast<uintptr_t>(tables) & 255)) return GRAM_E_ARG;
  if (tables_bytes < gram_token_tables_bytes(m)) return GRAM_E_ARG;
  const gram_model_desc_t& c = m->d;
  const TableScratch t = carve_tables(c, workspace);
  if (!workspace || workspace_bytes < t.bytes) return GRAM_E_WORKSPACE;
  Workspace w{};
  w.pieces = c.pieces > 1 ? c.pieces : 1;
  m->enc_qkv0 = m->dec_qkv0 = nullptr;
  p16* const enc = (p16*)tables;
  p16* const dec = enc + token_table_elems(c);
  TRY(gram_iota_i32(t.ids, c.vocab, stream));
  TRY(build_table(m, w, t, m->enc_ln1[0], m->enc_wqkv[0], m->s_enc_wqkv[0], enc, stream));
  TRY(build_table(m, w, t, m->dec_ln1[0], m->dec_wqkv[0], m->s_dec_wqkv[0], dec, stream));
  m->enc_qkv0 = enc;
  m->dec_qkv0 = dec;
  return 0;
}

extern "C" int64_t gram_workspace_bytes(const gram_model_t* m, int B, int N, int L, int K, int max_length) {
  if (check_shapes(m, B, N, L, K, max_length)) return GRAM_E_ARG;
  return carve(m, nullptr, B, N, L, K, max_length).bytes;
}

extern "C" int64_t gram_workspace_encoder_x_offset(const gram_model_t* m, int B, int N, int L, int K, int max_length) {
  if (check_shapes(m, B, N, L, K, max_length)) return GRAM_E_ARG;
  const Workspace w = carve(m, (void*)256, B, N, L, K, max_length);  // (any non-null base: only the offset is wanted)
  return (int64_t)((const char*)w.enc.x - (const char*)256);
}

extern "C" int gram_encode_fused(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                                 void* workspace, int64_t workspace_bytes, int K, int max_length, void* enc_out_bf16,
                                 void* stream) {
  TRY(check_shapes(m, B, N, L, K, max_length));
  Workspace w = carve(m, workspace, B, N, L, K, max_length);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, nullptr, stream));
  if (enc_out_bf16) {  // (split modes: all the pieces, [pieces][B*N*L][d])
    hipError_t e = hipMemcpyAsync(enc_out_bf16, w.enc.h, (size_t)w.pieces * B * N * L * m->d.d_model * sizeof(p16), hipMemcpyDeviceToDevice,  // (interleaved rows)
                                  (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
  }
  return 0;
}

extern "C" int gram_encode_passages(const gram_model_t* m, const int64_t* ids, const uint8_t* mask, int P, int L, void* workspace,
                                    int64_t workspace_bytes, float* x_out, void* stream) {
  TRY(check_shapes(m, P, 1, L, 1, 2));
  if (!ids || !mask || !x_out) return GRAM_E_ARG;
  Workspace w = carve(m, workspace, P, 1, L, 1, 2);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  TRY(encoder_layers(m, w, ids, mask, L, P, stream));
  hipError_t e = hipMemcpyAsync(x_out, w.enc.x, (size_t)P * L * m->d.d_model * sizeof(float), hipMemcpyDeviceToDevice,
                                (hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int gram_decode_step(const gram_model_t* m, const int32_t* tokens, const int32_t* anc, const uint8_t* mask, int B, int N,
                                int L, int K, int max_length, int t, void* workspace, int64_t workspace_bytes, float* logits,
                                void* stream) {
  TRY(check_shapes(m, B, N, L, K, max_length));
  if (t < 0 || t >= max_length - 1 || !logits) return GRAM_E_ARG;
  Workspace w = carve(m, workspace, B, N, L, K, max_length);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  return decode_step(m, w, tokens, anc, mask, B, N, L, K, B * K, max_length, t, logits, nullptr, nullptr, stream);
}

extern "C" int gram_generate(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                             int nret, int max_length, float length_penalty, const gram_trie_t* trie, void* workspace,
                             int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream) {
  return gram_generate_ex(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, nullptr, workspace, workspace_bytes,
                          sequences, scores, width_host, stream);
}

namespace {
// encode -> search -> finalize of one generate() on `stream`.
// (Replaying a small batch's launch train from a HIP graph was built in round 2 and measured in three rounds -- B = 1: 20.1 vs 20.2 ms,
// 14.1 vs 12.8 ms, 11.5 vs 10.65 ms eager: the chain is bound by the GPU-side dependency between ~950 tiny kernels, not by the host's
// launch cost, and a captured train cannot take the live-row step, whose row counts travel through the host -- and removed in round 4.)
int generate_body(const gram_model* m, Workspace& w, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                  int max_length, const gram_trie_t* trie, const gram_compaction_t* comp, const SearchMode& sm, int64_t* sequences,
                  float* scores, void* stream) {
  const gram_trie_tail_t* tail = sm.tail;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, comp, stream));
  // group beam search (gram_generate_groups): its init and its search step, the same loop (a -inf beam has no node, so
  // gram_live_rows' liveness test holds unchanged); the caller passes no tail
  // the biased search (gram_generate_bias): the plain init and the biased search step, the same loop; no tail either
  if (sm.num_groups) TRY(gram_beam_init_groups(&w.beam, trie, /*decoder_start_token_id=*/0, sm.num_groups, stream));
  else TRY(gram_beam_init(&w.beam, trie, /*decoder_start_token_id=*/0, stream));
  if (K == 1) {  // HF: num_beams == 1 -> greedy_search (raw logits, no hypotheses, no scores)
    for (int t = 0; t + 1 < max_length; ++t) {
      TRY(decode_step(m, w, w.beam.tokens, w.beam.anc, mask, B, N, L, 1, B, max_length, t, w.logits, nullptr, nullptr, stream));
      if (sm.umask) TRY(gram_greedy_step_mask(&w.beam, trie, w.logits, m->d.vocab, t + 1, sm.umask, stream));
      else if (sm.items) TRY(gram_greedy_step_items(&w.beam, trie, w.logits, m->d.vocab, t + 1, sm.items, stream));
      else TRY(gram_greedy_step(&w.beam, trie, w.logits, m->d.vocab, t + 1, stream));
    }
    TRY(gram_greedy_finalize(&w.beam, max_length, sequences, w.width, stream));
  } else {
    static const bool live_rows_env = [] {
      const char* e = getenv("GRAM_LIVE_ROWS");
      return !(e && e[0] == '0');
    }();
    const bool live_rows = g_live_rows < 0 ? live_rows_env : g_live_rows != 0;  // (the live-row step needs a host round trip)
    // The tail pass (tail != NULL: generate_call carved its buffers): at step t_tail the beams hold d_tail tokens, and every decoder
    // state the remaining steps can ask for is a row of the forest below them.  One pass computes them all; the steps from t_tail on
    // are then search steps alone, each beam reading the forest row of its node.  A forest over capacity (or an empty one) leaves
    // the loop as it is.  The forest's counts (rows, entries, rows per group and level: 144 bytes) cost the call one host round
    // trip -- a hipStreamSynchronize of its own: at t_tail the loop makes no live-row read the counts could ride in.
    const int t_tail = tail ? tail->d_tail - 1 : -1;
    bool replay = false;
    Workspace wt = w;
    if (tail) {
      wt = tail_view(w);
      if (g_tail_cap > 0 && g_tail_cap < wt.forest.cap_rows) wt.forest.cap_rows = g_tail_cap;
    }
    // fixed max_length-1 steps: finished users are padded exactly as BeamSearchScorer.process
    // pads them, so skipping HF's all-done early exit changes nothing and needs no host sync
    for (int t = 0; t + 1 < max_length; ++t) {
      if (t == t_tail) {
        int32_t counts[4 + 2 * GRAM_TAIL_MAX_STEPS] = {0};
        TRY(gram_tail_forest(&w.beam, trie, tail, &wt.forest, t, stream));
        hipError_t e = hipMemcpyAsync(counts, wt.forest.counts, sizeof(counts), hipMemcpyDeviceToHost, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
        if (counts[0] < 0 || counts[1] < 0) return GRAM_E_BEAM;
        g_tail_last[1] = counts[0], g_tail_last[2] = counts[1], g_tail_last[3] = counts[2];
        bool fits = counts[0] >= 1 && counts[0] <= wt.forest.cap_rows && counts[1] >= 1 && counts[1] <= wt.forest.cap_entries;
        const int level_cap = g_tail_level_cap > 0 && g_tail_level_cap < B * K ? g_tail_level_cap : B * K;  // (slots are cache rows)
        for (int l = 0; l < 2 * GRAM_TAIL_MAX_STEPS; ++l) fits = fits && counts[4 + l] >= 0 && counts[4 + l] <= level_cap;
        if (fits) {
          TRY(tail_pass(m, wt, mask, B, N, L, K, max_length, t, counts[0], counts[1], counts + 4, stream));
          replay = true;
          g_tail_last[0] = 1;
        }
      }
      if (replay) {
        TRY(gram_tail_rowpos(&w.beam, trie, &wt.forest, stream));
        TRY(search_step(m, wt, trie, t + 1, K, wt.forest.rowpos, SearchMode{}, stream));
        continue;
      }
      // step 0: every beam of a user holds the same start token and an empty cache, so the decoder,
      // the cross-attention and the lm_head run on ONE row per user (HF runs K identical rows);
      // gram_beam_step reads that shared row and points every beam's slot-0 ancestor at it
      const int Kt = t == 0 ? 1 : K;
      // From the step after the shortest candidate's EOS on, beams have left the Trie (gram_live_rows_t): the decoder
      // runs on the live rows only.  This costs the loop's one host round trip per such step (8 bytes), which is why
      // it is tried only where the Trie says rows can be dead -- with ids of l or l+1 pieces, the last step.
      if (live_rows && t >= 1 && trie->min_seq_len >= 2 && t >= trie->min_seq_len - 1) {
        int32_t counts[2] = {0, 0};
        TRY(gram_live_rows(&w.beam, trie, &w.live, stream));
        hipError_t e = hipMemcpyAsync(counts, w.live.counts, sizeof(counts), hipMemcpyDeviceToHost, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
        if (counts[0] < 0 || counts[0] > B * K || counts[1] < 0 || counts[1] > B) return GRAM_E_BEAM;
        if (counts[0] < B * K) {
          if (counts[0] > 0) {
            const LiveStep live{counts[0], counts[1], w.live.rows, w.live.rowpos, w.live.users};
            TRY(decode_step(m, w, w.live.tokens, w.beam.anc, mask, B, N, L, K, B * K, max_length, t, nullptr, w.lse_part, &live,
                            stream));
            TRY(gram_lse_combine(w.lse_part, w.lse, counts[0], m->d.vocab / 64, stream));
          }  // else: no beam can be extended; the search step below reads no decoder row
          TRY(search_step(m, w, trie, t + 1, K, w.live.rowpos, sm, stream));
          continue;
        }
      }
      // the [rows][V] logits are never written: LSE partials from the lm_head epilogue + sparse logits in the beam kernel
      TRY(decode_step(m, w, w.beam.tokens, w.beam.anc, mask, B, N, L, Kt, B * K, max_length, t, nullptr, w.lse_part, nullptr,
                      stream));
      TRY(gram_lse_combine(w.lse_part, w.lse, B * Kt, m->d.vocab / 64, stream));
      TRY(search_step(m, w, trie, t + 1, Kt, nullptr, sm, stream));
    }
    TRY(gram_beam_finalize(&w.beam, nret, max_length, sequences, scores, w.width, stream));
  }
  return 0;
}

}  // namespace

// The end of a whole-path call: with width_host, the returned width and the device's error flag come back (the call's one stream
// synchronise) and the flag becomes the return code.
static int read_width_and_error(const Workspace& w, int32_t* width_host, void* stream) {
  if (!width_host) return 0;
  int32_t host[2] = {0, 0};
  hipError_t e = hipMemcpyAsync(&host[0], w.width, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&host[1], w.beam.error, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  *width_host = host[0];
  if (host[1] == 4) return GRAM_E_NONFINITE;
  if (host[1] != 0) return GRAM_E_BEAM;
  return 0;
}

// every whole-path beam-search entry point: gram_generate_ex's call in the search mode sm (checked by the entry point)
static int generate_call(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                         int max_length, float length_penalty, const gram_trie_t* trie, const gram_compaction_t* comp, SearchMode sm,
                         void* workspace, int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream) {
  TRY(check_shapes(m, B, N, L, K, max_length));
  TRY(check_compaction(comp, B, N));
  if (!trie || nret < 1 || nret > K || !sequences || (!scores && K != 1)) return GRAM_E_ARG;
  Workspace w = carve(m, workspace, B, N, L, K, max_length);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  // the tail pass where the Trie has a tail inside this call's steps and the call is one it covers (beam search, no item filters,
  // the short cross-attention); everything else is the step-wise train, launch for launch
  memset(g_tail_last, 0, sizeof(g_tail_last));  // (gram_debug_tail_last speaks of the last generate call of any kind)
  if (sm.tail) {
    const bool on = sm.tail->d_tail >= 2 && sm.tail->d_tail < max_length && sm.tail->sub_rows && K > 1 && !sm.items &&
                    !m->long_xattn() && tail_shape_ok(B, K, sm.tail->steps) && tail_wanted(m, B, N, L);
    if (on) {
      carve_tail(m, workspace, w, B, K, sm.tail->steps);
      if (workspace_bytes < w.tail_bytes) return GRAM_E_WORKSPACE;
    } else {
      sm.tail = nullptr;
    }
  }
  w.beam.length_penalty = length_penalty;
  TRY(generate_body(m, w, input_ids, mask, B, N, L, K, nret, max_length, trie, comp, sm, sequences, scores, stream));
  return read_width_and_error(w, width_host, stream);
}

extern "C" int gram_generate_ex(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                const gram_compaction_t* comp, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                                float* scores, int32_t* width_host, void* stream) {
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, SearchMode{}, workspace,
                       workspace_bytes, sequences, scores, width_host, stream);
}

extern "C" int64_t gram_workspace_bytes_tail(const gram_model_t* m, int B, int N, int L, int K, int max_length, int steps) {
  if (check_shapes(m, B, N, L, K, max_length) || !tail_shape_ok(B, K, steps)) return GRAM_E_ARG;
  Workspace w = carve(m, nullptr, B, N, L, K, max_length);
  carve_tail(m, nullptr, w, B, K, steps);
  return w.tail_bytes;
}

extern "C" int gram_generate_tail(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                  int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                  const gram_compaction_t* comp, const gram_trie_tail_t* tail, void* workspace,
                                  int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream) {
  SearchMode sm;
  sm.tail = tail;
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, sm, workspace, workspace_bytes,
                       sequences, scores, width_host, stream);
}

// the per-user lists of every whole-path entry that takes them (gram_user_items_t): every array present, stride and mode in range
static bool items_ok(const gram_user_items_t* items) {
  return items && items->leaf_lo && items->leaf_hi && items->ranks && items->count && items->stride >= 1 &&
         items->stride <= GRAM_MAX_USER_ITEMS && (items->mode == GRAM_ITEMS_EXCLUDE || items->mode == GRAM_ITEMS_ALLOW);
}

extern "C" int gram_generate_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                   int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                   const gram_compaction_t* comp, const gram_user_items_t* items, void* workspace,
                                   int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream) {
  if (!items_ok(items)) return GRAM_E_ARG;
  SearchMode sm;
  sm.items = items;
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, sm, workspace, workspace_bytes,
                       sequences, scores, width_host, stream);
}

// per-user item masks: gram_generate_items' call with the masks in the lists' place (no tail pass)
extern "C" int gram_generate_mask(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                  int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                  const gram_compaction_t* comp, const gram_user_mask_t* umask, void* workspace,
                                  int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream) {
  if (!umask || !umask->leaf_lo || !umask->leaf_hi || !umask->words || umask->n_leaves < 1 ||
      umask->stride < (int64_t)umask->n_leaves / 32 + 1 || (reinterpret_cast<uintptr_t>(umask->words) & 7))
    return GRAM_E_ARG;
  SearchMode sm;
  sm.umask = umask;
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, sm, workspace, workspace_bytes,
                       sequences, scores, width_host, stream);
}

// group beam search: gram_generate_ex's call with the group init and the group step; items may be NULL
extern "C" int gram_generate_groups(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                    int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                    const gram_compaction_t* comp, int num_groups, float diversity_penalty,
                                    const gram_user_items_t* items, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                                    float* scores, int32_t* width_host, void* stream) {
  if (K < 2 || num_groups < 1 || num_groups > K || K % num_groups != 0 || !(diversity_penalty >= 0.f && diversity_penalty < INFINITY))
    return GRAM_E_ARG;
  if (items && !items_ok(items)) return GRAM_E_ARG;
  SearchMode sm;
  sm.items = items, sm.num_groups = num_groups, sm.diversity_penalty = diversity_penalty;
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, sm, workspace, workspace_bytes,
                       sequences, scores, width_host, stream);
}

// beam search with per-item score biases: gram_generate_ex's call with the biased search step; items may be NULL.
// The potentials are the caller's tensor (gram_item_bias_table): the workspace is gram_generate_ex's.
extern "C" int gram_generate_bias(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K,
                                  int nret, int max_length, float length_penalty, const gram_trie_t* trie,
                                  const gram_compaction_t* comp, const float* phi, int64_t phi_stride, const gram_user_items_t* items,
                                  void* workspace, int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host,
                                  void* stream) {
  if (K < 2 || !trie || !phi || (phi_stride != 0 && phi_stride < trie->n_nodes)) return GRAM_E_ARG;
  if (items && !items_ok(items)) return GRAM_E_ARG;
  SearchMode sm;
  sm.items = items, sm.phi = phi, sm.phi_stride = phi_stride;
  return generate_call(m, input_ids, mask, B, N, L, K, nret, max_length, length_penalty, trie, comp, sm, workspace, workspace_bytes,
                       sequences, scores, width_host, stream);
}

// ---- Trie-constrained sampling (gram_sample) ------------------------------------------------------------------------
namespace {

// What sampling needs beyond carve()'s layout, BEHIND `bytes` (nothing above moves): the two per-row accumulators and, for a Trie whose
// fan-out exceeds what the sampling step holds on chip, the streamed candidates of every row.
struct SampleScratch {
  float *model_lp, *sample_lp;  // [B * R]
  int64_t bytes;
};
SampleScratch carve_sample(Workspace& w, void* ws, int B, int R, int max_fanout) {
  Carve cv(ws);
  cv.off = w.bytes;
  SampleScratch s{};
  const int64_t rows = (int64_t)B * R;
  s.model_lp = cv.take<float>(rows);
  s.sample_lp = cv.take<float>(rows);
  if (max_fanout > gram_sample_capacity()) {
    w.beam.cand_logits_users = (int32_t)rows;
    w.beam.cand_logits_stride = max_fanout;
    w.beam.cand_logits = cv.take<float>(rows * max_fanout);
  }
  s.bytes = (cv.off + 255) & ~(int64_t)255;
  return s;
}
inline bool sample_shape_ok(int B, int R, int max_fanout) {
  return max_fanout >= 0 && (int64_t)B * R <= INT32_MAX / GRAM_MAX_DEC_LEN && (int64_t)B * R * max_fanout <= ((int64_t)1 << 40);
}

// encode -> R sampled rows per user -> finalize, next to generate_body: the same encode_call / decode_step / gram_lse_combine launches
// with the search step replaced by the sampling step.  A user's R rows share its bank as K beams do; step 0 runs on one decoder row
// per user; no row is ever reordered, so the ancestor table stays gram_beam_init's identity.  Finished rows keep being decoded.
int sample_body(const gram_model* m, Workspace& w, const SampleScratch& s, const int64_t* input_ids, const uint8_t* mask, int B, int N,
                int L, int R, int max_length, const gram_trie_t* trie, const gram_compaction_t* comp, const gram_user_items_t* items,
                const gram_sample_params_t* prm, const float* uniforms, int64_t* sequences, float* seq_logprobs, float* sample_logprobs,
                void* stream) {
  const gram_model_desc_t& c = m->d;
  const size_t rows = (size_t)B * R;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, comp, stream));
  TRY(gram_beam_init(&w.beam, trie, /*decoder_start_token_id=*/0, stream));
  // the rows' "finished" lengths live in the unused hypothesis heap (gram_hip.h); they and the accumulators start at zero
  hipError_t e = hipMemsetAsync(w.beam.hyp_len, 0, rows * sizeof(int32_t), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(s.model_lp, 0, rows * sizeof(float), (hipStream_t)stream);
  if (e == hipSuccess) e = hipMemsetAsync(s.sample_lp, 0, rows * sizeof(float), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  for (int t = 0; t + 1 < max_length; ++t) {
    const int Kt = t == 0 ? 1 : R;
    TRY(decode_step(m, w, w.beam.tokens, w.beam.anc, mask, B, N, L, Kt, B * R, max_length, t, nullptr, w.lse_part, nullptr, stream));
    TRY(gram_lse_combine(w.lse_part, w.lse, B * Kt, c.vocab / 64, stream));
    const void* const lm16 = w.pieces > 1 ? nullptr : c.lm_head_bf16;  // (the search step's operands: search_step)
    if (items)
      TRY(gram_sample_step_items(&w.beam, trie, w.dec.h, lm16, c.lm_head_f32, c.d_model, w.lse, c.vocab, t + 1, Kt, w.pieces, prm,
                                 uniforms + t, max_length - 1, s.sample_lp, s.model_lp, items, stream));
    else
      TRY(gram_sample_step(&w.beam, trie, w.dec.h, lm16, c.lm_head_f32, c.d_model, w.lse, c.vocab, t + 1, Kt, w.pieces, prm, uniforms + t,
                           max_length - 1, s.sample_lp, s.model_lp, stream));
  }
  return gram_sample_finalize(&w.beam, max_length, s.model_lp, s.sample_lp, sequences, seq_logprobs, sample_logprobs, w.width, stream);
}

int sample_call(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
                const gram_trie_t* trie, const gram_compaction_t* comp, const gram_user_items_t* items, const gram_sample_params_t* prm,
                const float* uniforms, void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
                float* sample_logprobs, int32_t* width_host, void* stream) {
  TRY(check_shapes(m, B, N, L, R, max_length));
  TRY(check_compaction(comp, B, N));
  if (!trie || !prm || !uniforms || !sequences || !seq_logprobs || !sample_logprobs || !mask || (!comp && !input_ids) ||
      !sample_shape_ok(B, R, trie->max_fanout))
    return GRAM_E_ARG;
  if (!(prm->temperature > 0.f) || prm->top_k < 0 || !(prm->top_p > 0.f) || !(prm->top_p <= 1.f)) return GRAM_E_ARG;
  Workspace w = carve(m, workspace, B, N, L, R, max_length);
  const SampleScratch s = carve_sample(w, workspace, B, R, trie->max_fanout);
  if (!workspace || workspace_bytes < s.bytes) return GRAM_E_WORKSPACE;
  memset(g_tail_last, 0, sizeof(g_tail_last));  // (gram_debug_tail_last speaks of the last generate call of any kind)
  TRY(sample_body(m, w, s, input_ids, mask, B, N, L, R, max_length, trie, comp, items, prm, uniforms, sequences, seq_logprobs,
                  sample_logprobs, stream));
  return read_width_and_error(w, width_host, stream);
}

}  // namespace

extern "C" int64_t gram_workspace_bytes_sample(const gram_model_t* m, int B, int N, int L, int R, int max_length, int max_fanout) {
  if (check_shapes(m, B, N, L, R, max_length) || !sample_shape_ok(B, R, max_fanout)) return GRAM_E_ARG;
  Workspace w = carve(m, nullptr, B, N, L, R, max_length);
  return carve_sample(w, nullptr, B, R, max_fanout).bytes;
}

extern "C" int gram_sample(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
                           const gram_trie_t* trie, const gram_compaction_t* comp, const gram_sample_params_t* params,
                           const float* uniforms, void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
                           float* sample_logprobs, int32_t* width_host, void* stream) {
  return sample_call(m, input_ids, mask, B, N, L, R, max_length, trie, comp, nullptr, params, uniforms, workspace, workspace_bytes,
                     sequences, seq_logprobs, sample_logprobs, width_host, stream);
}

extern "C" int gram_sample_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R,
                                 int max_length, const gram_trie_t* trie, const gram_compaction_t* comp, const gram_user_items_t* items,
                                 const gram_sample_params_t* params, const float* uniforms, void* workspace, int64_t workspace_bytes,
                                 int64_t* sequences, float* seq_logprobs, float* sample_logprobs, int32_t* width_host, void* stream) {
  if (!items_ok(items)) return GRAM_E_ARG;
  return sample_call(m, input_ids, mask, B, N, L, R, max_length, trie, comp, items, params, uniforms, workspace, workspace_bytes,
                     sequences, seq_logprobs, sample_logprobs, width_host, stream);
}

// ---- sampling without replacement (gram_generate_sbs) --------------------------------------------------------------
namespace {

// Behind carve_sample's layout (whose two accumulators are phi and the model's log-probability here): the rows' path words and,
// where a user's candidates exceed what the step holds on chip, 2 * max_fanout words per row instead of the sampling step's max_fanout.
struct SbsScratch {
  SampleScratch s;
  uint64_t* path;  // [B * R]
  int64_t bytes;
};
SbsScratch carve_sbs(Workspace& w, void* ws, int B, int R, int max_fanout) {
  SbsScratch x{};
  x.s = carve_sample(w, ws, B, R, /*max_fanout=*/0);
  Carve cv(ws);
  cv.off = x.s.bytes;
  const int64_t rows = (int64_t)B * R;
  x.path = cv.take<uint64_t>(rows);
  if ((int64_t)R * max_fanout > gram_sbs_capacity()) {
    w.beam.cand_logits_users = (int32_t)rows;
    w.beam.cand_logits_stride = 2 * (int64_t)max_fanout;
    w.beam.cand_logits = cv.take<float>(rows * 2 * max_fanout);
  }
  x.bytes = (cv.off + 255) & ~(int64_t)255;
  return x;
}

// sample_body's train -- the same encode_call / decode_step / gram_lse_combine launches -- with the stochastic beam search's init,
// step and finalize.  Rows are reordered, so the step advances the ancestor table as the beam search does.
int sbs_call(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
             const gram_trie_t* trie, const gram_compaction_t* comp, const gram_user_items_t* items, float temperature, uint64_t seed,
             const int64_t* user_keys, void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
             float* sample_logprobs, float* perturbed, int32_t* width_host, void* stream) {
  TRY(check_shapes(m, B, N, L, R, max_length));
  TRY(check_compaction(comp, B, N));
  if (!trie || !user_keys || !sequences || !seq_logprobs || !sample_logprobs || !perturbed || !mask || (!comp && !input_ids) ||
      trie->max_fanout > INT32_MAX / 2 || !sample_shape_ok(B, R, 2 * trie->max_fanout))
    return GRAM_E_ARG;
  if (!(temperature > 0.f) || !(temperature < 3.0e38f)) return GRAM_E_ARG;
  Workspace w = carve(m, workspace, B, N, L, R, max_length);
  const SbsScratch x = carve_sbs(w, workspace, B, R, trie->max_fanout);
  if (!workspace || workspace_bytes < x.bytes) return GRAM_E_WORKSPACE;
  memset(g_tail_last, 0, sizeof(g_tail_last));  // (gram_debug_tail_last speaks of the last generate call of any kind)
  const gram_model_desc_t& c = m->d;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, comp, stream));
  TRY(gram_sbs_init(&w.beam, trie, /*decoder_start_token_id=*/0, seed, user_keys, x.s.sample_lp, x.s.model_lp, x.path, stream));
  for (int t = 0; t + 1 < max_length; ++t) {
    const int Kt = t == 0 ? 1 : R;
    TRY(decode_step(m, w, w.beam.tokens, w.beam.anc, mask, B, N, L, Kt, B * R, max_length, t, nullptr, w.lse_part, nullptr, stream));
    TRY(gram_lse_combine(w.lse_part, w.lse, B * Kt, c.vocab / 64, stream));
    const void* const lm16 = w.pieces > 1 ? nullptr : c.lm_head_bf16;  // (the search step's operands: search_step)
    if (items)
      TRY(gram_sbs_step_items(&w.beam, trie, w.dec.h, lm16, c.lm_head_f32, c.d_model, w.lse, c.vocab, t + 1, Kt, w.pieces, temperature,
                              seed, x.s.sample_lp, x.s.model_lp, x.path, items, stream));
    else
      TRY(gram_sbs_step(&w.beam, trie, w.dec.h, lm16, c.lm_head_f32, c.d_model, w.lse, c.vocab, t + 1, Kt, w.pieces, temperature, seed,
                        x.s.sample_lp, x.s.model_lp, x.path, stream));
  }
  TRY(gram_sbs_finalize(&w.beam, max_length, x.s.model_lp, x.s.sample_lp, sequences, seq_logprobs, sample_logprobs, perturbed, w.width,
                        stream));
  return read_width_and_error(w, width_host, stream);
}

}  // namespace

extern "C" int64_t gram_workspace_bytes_sbs(const gram_model_t* m, int B, int N, int L, int R, int max_length, int max_fanout) {
  if (check_shapes(m, B, N, L, R, max_length) || max_fanout < 0 || max_fanout > INT32_MAX / 2 || !sample_shape_ok(B, R, 2 * max_fanout))
    return GRAM_E_ARG;
  Workspace w = carve(m, nullptr, B, N, L, R, max_length);
  return carve_sbs(w, nullptr, B, R, max_fanout).bytes;
}

extern "C" int gram_generate_sbs(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R,
                                 int max_length, const gram_trie_t* trie, const gram_compaction_t* comp, float temperature, uint64_t seed,
                                 const int64_t* user_keys, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                                 float* seq_logprobs, float* sample_logprobs, float* perturbed_scores, int32_t* width_host,
                                 void* stream) {
  return sbs_call(m, input_ids, mask, B, N, L, R, max_length, trie, comp, nullptr, temperature, seed, user_keys, workspace,
                  workspace_bytes, sequences, seq_logprobs, sample_logprobs, perturbed_scores, width_host, stream);
}

extern "C" int gram_generate_sbs_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R,
                                       int max_length, const gram_trie_t* trie, const gram_compaction_t* comp,
                                       const gram_user_items_t* items, float temperature, uint64_t seed, const int64_t* user_keys,
                                       void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
                                       float* sample_logprobs, float* perturbed_scores, int32_t* width_host, void* stream) {
  if (!items_ok(items)) return GRAM_E_ARG;
  return sbs_call(m, input_ids, mask, B, N, L, R, max_length, trie, comp, items, temperature, seed, user_keys, workspace, workspace_bytes,
                  sequences, seq_logprobs, sample_logprobs, perturbed_scores, width_host, stream);
}

// ---- teacher-forced decoder pass (gram_teacher_forced) -----------------------------------------------------------------------------
namespace {

int check_shapes_tf(const gram_model* m, int B, int N, int L, int C, int T) {
  if (!m || B < 1 || N < 1 || N > m->d.max_passages || L < 32 || L > m->max_L || (L & 31) || N * L > m->max_S || C < 1 ||
      T < 1 || T > GRAM_MAX_DEC_LEN || (int64_t)B * C * T > INT32_MAX / 4)
    return GRAM_E_ARG;
  return 0;
}

// The bank and the small tables first; then the encoder's buffers, and the decoder's R = B*C*T rows IN THE SAME BYTES: the encoder's
// activations are dead once the bank GEMM has read w.enc.h (stream order), and the two together would be most of a large call's workspace.
Workspace carve_tf(const gram_model* m, void* ws, int B, int N, int L, int C, int T) {
  const gram_model_desc_t& c = m->d;
  const int64_t V = c.vocab, R = (int64_t)B * C * T;
  Carve cv(ws);
  Workspace w{};
  const int64_t P = w.pieces = c.pieces > 1 ? c.pieces : 1;
  take_key_bits(cv, w, m, B, (int64_t)B * ((int64_t)C * T < GRAM_MAX_BEAMS ? C * T : GRAM_MAX_BEAMS), N * L);
  w.rowmap = cv.take<int32_t>((int64_t)B * (1 + 2 * GRAM_MAX_BEAMS));
  take_bank(cv, w, c, B, (int64_t)N * L);
  const int64_t shared = cv.off;
  w.enc = take_rows(cv, c, P, (int64_t)B * N * L, false);
  const int64_t enc_end = cv.off;
  cv.off = shared;
  w.dec = take_rows(cv, c, P, R, true);
  w.lse = cv.take<float>(R);
  w.lse_part = cv.take<float>(R * (V / 64) * 2);
  const int64_t end = cv.off > enc_end ? cv.off : enc_end;
  w.bytes = (end + 255) & ~(int64_t)255;
  return w;
}

// The decoder layers over R = B * Q rows (Q = C * T per user): decode_step's, with the stepped self-attention replaced by the
// whole-sequence one and the cross-attention taking all Q rows of a user; then the lm_head with its LSE partials (logits stored when
// given) and their combination.  attn != NULL (gram_teacher_forced_ex): every layer's cross-attention is followed by its probabilities
// (xattn_probs.hip, on the same r.qx and K bank) and their head sum; the passage scores follow the last layer.  These launches only read
// what the pass computes.  sc != NULL (gram_teacher_forced_scores): every layer's cross-attention is followed by the head-summed
// probabilities (xattn_scores.hip) accumulated into sc->token_scores; no per-head buffer, any S the handle takes.
// tree != NULL (gram_score_trie): the Q rows of a user are the rows of a Trie, each attending to its ancestors (T is not used).
int decoder_tf(const gram_model* m, const Workspace& w, const int32_t* tokens, const uint8_t* mask, int B, int N, int L, int Q, int T,
               float* logits, const gram_xattn_out_t* attn, const gram_xattn_scores_t* sc, const gram_trie_rows_t* tree, void* st) {
  const gram_model_desc_t& c = m->d;
  const int H = c.n_heads, R = B * Q, S = N * L;
  const size_t bank_layer = (size_t)B * H * S * 64;
  const Rows& r = w.dec;
  TRY(decoder_layers(
      m, w, tokens, R, /*qkv0_from_table=*/false,
      [&](int) {
        if (tree)
          return gram_dec_self_attn_tree_split(r.qkv, tree->pos, tree->anc, c.dec_bias_f32, r.attn, B, Q, tree->Tq, H, w.pieces, r.ps_qkv,
                                               st);
        return gram_dec_self_attn_tf_split(r.qkv, c.dec_bias_f32, r.attn, R / T, T, H, w.pieces, r.ps_qkv, st);
      },
      [&](int i) {
        if (m->long_xattn())
          TRY(gram_cross_attn_rows_long_split(r.qx, w.bank_k + i * bank_layer, w.bank_vt + i * bank_layer, mask, r.attn, B, Q, H, S,
                                              w.pieces, r.ps_qx, w.ps_bank, w.key_bits, w.xa_scratch, w.rowmap, st));
        else
          TRY(gram_cross_attn_rows_split(r.qx, w.bank_k + i * bank_layer, w.bank_vt + i * bank_layer, mask, r.attn, B, Q, H, S, w.pieces,
                                         r.ps_qx, w.ps_bank, w.key_bits, w.rowmap, st));
        if (sc)
          TRY(gram_cross_attn_token_scores_split(r.qx, w.bank_k + i * bank_layer, sc->token_scores, B, Q, H, S, w.pieces, r.ps_qx,
                                                 w.ps_bank, w.key_bits, /*first=*/i == 0, st));
        if (!attn) return 0;
        float* p = attn->probs ? attn->probs + (size_t)i * B * H * Q * S : attn->layer_probs;
        // (the probabilities read the short form's key bits; a handle that carved the long form's lets the kernel pack them from the mask)
        TRY(gram_cross_attn_probs_split(r.qx, w.bank_k + i * bank_layer, mask, p, B, Q, H, S, w.pieces, r.ps_qx, w.ps_bank,
                                        m->long_xattn() ? nullptr : w.key_bits, st));
        return attn->token_scores ? gram_xattn_head_sum(p, attn->token_scores, B, Q, H, S, /*first=*/i == 0, st) : 0;
      },
      st));
  if (attn && attn->passage_scores)
    TRY(gram_xattn_passage_scores(attn->token_scores, mask, attn->passage_scores, B, Q, N, L, (float)(c.n_dec_layers * H), st));
  if (sc && sc->passage_scores)
    TRY(gram_xattn_passage_scores(sc->token_scores, mask, sc->passage_scores, B, Q, N, L, (float)(c.n_dec_layers * H), st));
  TRY(lm_head(m, w, R, logits, w.lse_part, st));
  return gram_lse_combine(w.lse_part, w.lse, R, c.vocab / 64, st);
}

}  // namespace

extern "C" int64_t gram_workspace_bytes_tf(const gram_model_t* m, int B, int N, int L, int C, int T) {
  if (check_shapes_tf(m, B, N, L, C, T)) return GRAM_E_ARG;
  return carve_tf(m, nullptr, B, N, L, C, T).bytes;
}

extern "C" int gram_teacher_forced(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                                   const gram_compaction_t* comp, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                                   void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp,
                                   void* stream) {
  return gram_teacher_forced_ex(m, input_ids, mask, B, N, L, comp, dec_ids, labels, C, T, workspace, workspace_bytes, logits, token_logp,
                                seq_logp, nullptr, stream);
}

namespace {
// the teacher-forced pass with either kind of attention output (at most one of attn, sc); every check before any launch
int teacher_forced_run(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                       const gram_compaction_t* comp, const int32_t* dec_ids, const int32_t* labels, int C, int T, void* workspace,
                       int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp, const gram_xattn_out_t* attn,
                       const gram_xattn_scores_t* sc, void* stream) {
  TRY(check_shapes_tf(m, B, N, L, C, T));
  if (!mask || !dec_ids || !labels || !token_logp || !seq_logp || (!comp && !input_ids)) return GRAM_E_ARG;
  // the attention outputs are the caller's memory: one layer of probabilities at least, and the passage scores are a reduction of the
  // token scores
  if (attn && ((!attn->probs && !attn->layer_probs) || (attn->passage_scores && !attn->token_scores))) return GRAM_E_ARG;
  if (attn && N * L > GRAM_MAX_FUSED_LEN) return GRAM_E_ARG;  // probabilities stop at 4096 keys (gram_cross_attn_probs_split)
  TRY(check_compaction(comp, B, N));  // (as gram_generate_ex)
  Workspace w = carve_tf(m, workspace, B, N, L, C, T);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  const gram_model_desc_t& c = m->d;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, comp, stream));
  TRY(decoder_tf(m, w, dec_ids, mask, B, N, L, C * T, T, logits, attn, sc, nullptr, stream));
  return gram_label_logprob_split(w.dec.h, c.lm_head_bf16, c.lm_head_f32, c.d_model, w.lse, labels, B * C, T, c.vocab, w.pieces,
                                  token_logp, seq_logp, stream);
}
}  // namespace

extern "C" int gram_teacher_forced_ex(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                                      const gram_compaction_t* comp, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                                      void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp,
                                      const gram_xattn_out_t* attn, void* stream) {
  return teacher_forced_run(m, input_ids, mask, B, N, L, comp, dec_ids, labels, C, T, workspace, workspace_bytes, logits, token_logp,
                            seq_logp, attn, nullptr, stream);
}

// The head-summed scores read the long form's key bits, which only a raised handle's workspace holds (the carve is not changed for
// this call); the kernel takes 16 heads at most.
extern "C" int gram_teacher_forced_scores(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                                          const gram_compaction_t* comp, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                                          void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp,
                                          const gram_xattn_scores_t* scores, void* stream) {
  if (!m || !scores || !scores->token_scores || !m->long_xattn() || m->d.n_heads > 16) return GRAM_E_ARG;
  if (reinterpret_cast<uintptr_t>(scores->token_scores) & 15) return GRAM_E_ARG;
  if (B > 65535 || ((int64_t)C * T + 31) / 32 > 65535) return GRAM_E_ARG;  // (the kernel's grid: users, tiles of 32 rows)
  return teacher_forced_run(m, input_ids, mask, B, N, L, comp, dec_ids, labels, C, T, workspace, workspace_bytes, logits, token_logp,
                            seq_logp, nullptr, scores, stream);
}

// ---- every catalogue item in one decoder pass over the Trie (gram_score_trie) ------------------------------------------------------
namespace {

struct TrieScratch {
  int32_t* tokens;  // [B * Q]  the row table's tokens repeated per user
  float* edge;      // [B * Q]  gram_trie_leaf_logprob_split's row_edge
};

// carve_tf's layout with R = B * Q rows, then the two row tables of the pass
Workspace carve_trie(const gram_model* m, void* ws, int B, int N, int L, int Q, TrieScratch& ts) {
  Workspace w = carve_tf(m, ws, B, N, L, Q, 1);
  Carve cv(ws);
  cv.off = w.bytes;
  ts.tokens = cv.take<int32_t>((int64_t)B * Q);
  ts.edge = cv.take<float>((int64_t)B * Q);
  w.bytes = (cv.off + 255) & ~(int64_t)255;
  return w;
}

}  // namespace

extern "C" int64_t gram_workspace_bytes_trie(const gram_model_t* m, int B, int N, int L, int Q) {
  if (check_shapes_tf(m, B, N, L, Q, 1)) return GRAM_E_ARG;
  TrieScratch ts;
  return carve_trie(m, nullptr, B, N, L, Q, ts).bytes;
}

extern "C" int gram_score_trie(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                               const gram_compaction_t* comp, const gram_trie_t* trie, const gram_trie_rows_t* rows, void* workspace,
                               int64_t workspace_bytes, float* leaf_logp, float* node_logp, void* stream) {
  if (!rows || !trie || rows->Q < 1) return GRAM_E_ARG;
  const int Q = rows->Q;
  TRY(check_shapes_tf(m, B, N, L, Q, 1));
  if (!mask || !leaf_logp || (!comp && !input_ids)) return GRAM_E_ARG;
  if (!rows->tokens || !rows->pos || !rows->anc || !rows->row_node || !rows->node_row || !rows->node_tok || !rows->node_leaf ||
      rows->Tq < 1 || rows->Tq > GRAM_MAX_DEC_LEN || rows->n_nodes != trie->n_nodes || rows->n_nodes < 3 || rows->n_leaves < 1 ||
      rows->n_leaves >= rows->n_nodes || (int64_t)B * rows->n_nodes > INT32_MAX / 4)
    return GRAM_E_ARG;
  TRY(check_compaction(comp, B, N));  // (as gram_generate_ex)
  TrieScratch ts;
  Workspace w = carve_trie(m, workspace, B, N, L, Q, ts);
  if (!workspace || workspace_bytes < w.bytes) return GRAM_E_WORKSPACE;
  const gram_model_desc_t& c = m->d;
  TRY(encode_call(m, w, input_ids, mask, B, N, L, comp, stream));
  TRY(gram_trie_repeat_tokens(rows->tokens, ts.tokens, B, Q, stream));
  TRY(decoder_tf(m, w, ts.tokens, mask, B, N, L, Q, 1, nullptr, nullptr, nullptr, rows, stream));
  return gram_trie_leaf_logprob_split(w.dec.h, c.lm_head_bf16, c.lm_head_f32, c.d_model, w.lse, rows, B, c.vocab, w.pieces, ts.edge,
                                      leaf_logp, node_logp, stream);
}
