/*
 * gram_hip.h -- C ABI of libgram_hip.so: GRAM's multi-granular late-fusion generative scoring
 * path on MI355X (gfx950), hand-written HIP kernels.
 *
 * The reference (zhaodong-liu/GRAM) is pure Python and has no FFI; its seam for this path is
 *   src/model/gram.py:74-107        GRAM.generate(input_ids, attention_mask, max_length, **hf_kwargs)
 *   src/runner/single_runner_gram.py:641-651   the call site (beam=K, top-K, Trie closure)
 * Each entry point below names the reference function(s) it replaces.  INTEGRATION.md shows the
 * ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, nothing allocates,
 *     nothing synchronises (except gram_generate's final 4-byte width read when asked)
 *   - "bf16" in a name or a comment = the library's 16-bit operand type, row-major: IEEE HALF in the default build, bfloat16 only in
 *     the `make PIECE=bf16` A/B build (gram_piece_format() tells; the names predate the switch).  Every `_bf16` entry point has an
 *     `_f16` alias (end of this header) that runs only in a library built on IEEE half -- bind those.
 *   - "inner" = n_heads * 64; d_kv must be 64
 *   - return value: 0 on success, >0 a hipError_t, <0 an argument error (GRAM_E_*)
 */
#ifndef GRAM_HIP_H
#define GRAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRAM_ABI_VERSION 7

#define GRAM_E_ARG (-1)       /* bad shape / unsupported size                           */
#define GRAM_E_WORKSPACE (-2) /* workspace too small (see gram_workspace_bytes)          */
#define GRAM_E_BEAM (-3)      /* device beam bookkeeping flagged an impossible state      */
#define GRAM_E_NONFINITE (-4) /* a returned score is NaN or +inf: an activation left the range of the 16-bit pieces (IEEE half:
                                 |x| <= 65 504) -- use the bfloat16 build (make PIECE=bf16)             */

#define GRAM_MAX_BEAMS 64      /* K <= 64 (reference default 50, headline 20)             */
#define GRAM_MAX_DEC_LEN 64    /* max_length <= 64 (reference: the longest candidate, 8..12, for the "split" / "t5_token" id
                                  types, 50 for "term": single_runner_gram.py:629-637); also the row stride of dec_bias_f32 */
#define GRAM_MAX_PASSAGE_LEN 128 /* L <= 128 on a default handle (arguments.py:293-298), L % 32 == 0 */
#define GRAM_MAX_LONG_PASSAGE_LEN 512 /* L <= 512 on a handle raised by gram_model_set_max_passage_len */
#define GRAM_MAX_FUSED_LEN 4096       /* S = N * L <= 4096 on a default handle */
#define GRAM_MAX_LONG_FUSED_LEN 16384 /* S <= 16 384 on a handle raised by gram_model_set_max_fused_len */

/* ---- GEMM epilogues ------------------------------------------------------------------ */
enum gram_epilogue {
  GRAM_EPI_BF16 = 0,      /* C_bf16[m][n]  = acc                                          */
  GRAM_EPI_BF16_RELU = 1, /* C_bf16[m][n]  = max(acc, 0)        (T5DenseActDense wi+ReLU) */
  GRAM_EPI_F32_ADD = 2,   /* C_f32[m][n]  += acc                (residual add)            */
  GRAM_EPI_F32 = 3,       /* C_f32[m][n]   = acc                (lm_head logits)          */
  GRAM_EPI_KV_BANK = 4,   /* scatter into the fused K bank / V^T bank (see below)         */
  GRAM_EPI_F32_LSE = 5    /* GRAM_EPI_F32 + per-(row, 64-column block) softmax partials       */
};

/* Fused cross-attention KV bank for B users, S = N*L fused tokens, n_layers decoder layers:
 *   k  : [layer][b][h][s][64]   bf16   (key rows contiguous: streamed 128 B per key)
 *   vt : [layer][b][h][s/32][64][32] bf16 (V transposed and blocked by 32 keys: the 64 x 32 tile of a 32-key step is 4 KiB
 *                                    contiguous, fetched as whole 128-B lines like a K tile; S % 32 == 0)
 * Beam-invariant: ONE copy per user, shared by the user's K beams (the reference replicates it
 * K times and index_select-s it every step: gram_t5_modeling.py:531-549, gram_t5.py:320-348). */
typedef struct {
  void* k;
  void* vt;
  int32_t n_layers, B, H, S;
  /* optional compaction of fully padded passages: GEMM row m belongs to compact passage p = m / L, which is
   * passage n = passage_map[p] % N of user b = passage_map[p] / N (S = N*L).  NULL = rows are b*S + s. */
  const int32_t* passage_map;
  int32_t N, L;
} gram_kv_bank_t;

/* C[M,N] (+)= A[M,K] @ W[N,K]^T, bf16 operands, fp32 accumulate on MFMA.
 * Replaces every nn.Linear on the path (gram_t5_modeling.py:300-301,369-372; gram_t5.py:254).
 * N % 128 == 0, K % 64 == 0, any M >= 1.  For GRAM_EPI_KV_BANK, C is ignored, `bank` is used,
 * rows m = b*S + s and columns n = (layer*2 + which)*inner + h*64 + d. */
int gram_gemm_bf16(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldc,
                   int epilogue, const gram_kv_bank_t* bank_host, void* stream);

/* T5LayerNorm folded into the GEMMs on either side of it (no separate norm pass over the residual stream):
 *   producer (GRAM_EPI_F32_ADD):  besides x += acc it writes xb = bf16(x) and, per row and 64-column block,
 *                                 the partial sum of squares ss_out[m][n/64] (deterministic: no atomics)
 *   consumer (GRAM_EPI_BF16[_RELU]): A is xb, W has the norm gain folded in (W[n][k] * g[k]), and every output
 *                                 row is scaled by rsqrt(sum_b ss_in[m][b] / d + eps) before ReLU / rounding,
 * which equals Linear(T5LayerNorm(x)) (gram_t5_modeling.py:262-276 followed by :300-301 / :369-372). */
typedef struct {
  void* xb_out;        /* producer: bf16 [M][ldc] copy of the updated residual, or NULL            */
  float* ss_out;       /* producer: f32 [M][N/64] partial sums of squares, or NULL                 */
  const float* ss_in;  /* consumer: f32 [M][nblk_in] partials of the rows of A, or NULL            */
  int32_t nblk_in;     /* consumer: d_model / 64, or 0 if ss_in already holds 1/rms per row        */
  int32_t d;           /* consumer: d_model (the mean is over d elements)                          */
  float eps;
  int32_t quarter;     /* != 0: the partials cover 16 columns each -- ss_out [M][N/16], ss_in [M][4*nblk_in] -- and a block's
                          sum is (q0 + q1) + (q2 + q3), which is how the 64-column epilogues add it up themselves: same bits.
                          The layout of the small-M streaming GEMM (one 16-column n-tile per workgroup); only legal for
                          M <= gram_gemm_stream_max_m() and K % 128 == 0 (GRAM_E_ARG otherwise)                  */
  /* Range of the 16-bit copy.  T5's residual stream is unnormalised and leaves the IEEE-half range in trained checkpoints (the
   * reference's own T5 carries the fp16 clamp for it: gram_t5_modeling.py:773-776,803-808,824-827), so xb is stored as the pieces
   * of x[m] * xs[m], xs[m] a POWER OF TWO per row (exact), and the consumer's row scale is divided by it (exact):
   *   producer: xs_in f32 [M] -- xb_out[m] = pieces(x[m] * xs_in[m]); NULL = 1
   *   consumer: xs_in f32 [M] -- the factor the producer of A applied: every output row is scaled by rsqrt(..) / xs_in[m].  Ignored
   *             when nblk_in == 0 (ss_in then already holds rsqrt(..) / xs: gram_row_rscale_xs).
   *             xs_out f32 [M] or NULL -- the workgroups of the first n-tile also write the factor for the NEXT producer from the
   *             partials they have just added up: with typ^2 = (smallest 64-column partial of row m) / 64 -- the ordinary magnitude
   *             of the row; the few outlier features of a T5 row dominate its rms but not its quietest block -- the power of two
   *             that puts typ * xs into [2^-2, 2^-1), capped so that sqrt(sum of squares) * xs <= 2^10, clamped to [2^-40, 2^20].
   *             Two IEEE-half pieces then hold 22 bits of every element down to half the ordinary magnitude (error floor 2^-23 of
   *             it below) and up to 1.3e5 times it.  xs_out must not alias xs_in. */
  const float* xs_in;
  float* xs_out;
} gram_norm_fusion_t;
/* Largest M the streaming small-M GEMM takes (0: switched off, GRAM_GEMM_STREAM=0 or a forced variant). */
int gram_gemm_stream_max_m(void);
int gram_gemm_bf16_ex(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldc, int epilogue,
                      const gram_kv_bank_t* bank_host, const gram_norm_fusion_t* nf_host, void* stream);
/* rs[m] = rsqrt(sum_b ss[m][b] / d + eps); a consumer may take it directly with nblk_in = 0 (ss_in = rs). */
int gram_row_rscale(const float* ss, float* rs, int M, int nblk, int d, float eps, void* stream);
/* The same with the row factors of the 16-bit copy (gram_norm_fusion_t): rs[m] = rsqrt(..) / xs_in[m] (xs_in NULL = 1) and, when
 * xs_out is given, xs_out[m] = the factor for the next producer (see xs_out above).  xs_out may not alias xs_in. */
int gram_row_rscale_xs(const float* ss, float* rs, const float* xs_in, float* xs_out, int M, int nblk, int d, float eps, void* stream);
/* embed_tokens for the folded path: x (f32), xb = bf16(x), ss[m][b] = the sum of squares of 64-column block b when nblk * 64 == d
 * (any other nblk, or a d that is no multiple of 64: the row's total in ss[m][0], zeros behind it). */
int gram_embed_ex(const float* table, const void* ids, int ids_are_i64, float* x, void* xb, float* ss, int nblk, int rows,
                  int d, void* stream);

/* ---- two-piece operands: fp32-class arithmetic on the 16-bit MFMA ("f16x3" / "bf16x3") --------------------------------
 * The reference computes in fp32 end to end (no autocast / half anywhere in src/; fp32 softmax gram_t5_modeling.py:608).
 * One 16-bit piece per value moves Recall@5/NDCG@5 by ~5e-3 (bf16) on a 2 048-user population -- 50x the 1e-4 bound.  With
 * gram_split_t.pieces = 2 a value v travels as TWO 16-bit numbers
 *     p0 = r16(v),  p1 = r16(v - p0)              (r16 = round to the library's 16-bit type, gram_piece_format())
 * and a product a*w is evaluated on the 16-bit MFMA as three piece products accumulated in fp32, smallest first:
 *     a0*w1 + a1*w0 + a0*w0          relative error ~2^-22 with IEEE-half pieces (11 significant bits each), ~2^-18 with bf16
 * Layouts.  GEMM operands are INTERLEAVED: a logical [rows][K] matrix is stored as [rows][K/32][2][32] -- the two pieces of a
 * 32-column block side by side, 128 B -- so that one 64-column k-tile of the physical [rows][2K] matrix carries everything the
 * three products of that block need and is fetched once (inter(n, p) = (n / 32) * 64 + p * 32 + n % 32).  This holds for every
 * activation a GEMM reads (the normed / copied residual stream, attention outputs, the FFN intermediate) and for every weight
 * matrix.  What only attention kernels read -- Q/K/V rows, the KV bank, the self-attention cache -- stays PLANAR: `pieces`
 * copies of the plain layout, `*_pstride` elements apart.  pieces = 1 is the plain path (every *_split entry point accepts
 * split = NULL). */
#define GRAM_MAX_PIECES 2
typedef struct {
  int32_t pieces;         /* 1 or 2                                                                                   */
  int32_t c_interleaved;  /* a 16-bit C (GRAM_EPI_BF16[_RELU]) is written interleaved ([M][ldc >= 2N]) instead of planar  */
  int64_t c_pstride;      /* planar 16-bit C: elements between its pieces                                              */
  int64_t bank_pstride;   /* elements between the pieces of gram_kv_bank_t.k and .vt                                   */
  float out_scale;        /* every result is acc * out_scale; 0 = 1.  Must be a power of two (GRAM_E_ARG otherwise): the
                             inverse of the factor the caller scaled W by (gram_model_desc_t.w_scales)                  */
} gram_split_t;
/* gram_gemm_bf16_ex on two-piece operands: A is the interleaved [M][lda >= 2 kc] matrix, W the interleaved [N][2 kc] one, kc the
 * LOGICAL reduction length; 16-bit results are written as pieces (C planar or interleaved as split says; gram_norm_fusion_t.xb_out
 * always interleaved, [M][2 ldc]; the bank planar), fp32 results (residual stream, logits, LSE) as fp32. */
int gram_gemm_bf16_split(const void* A, const void* W, void* C, int M, int N, int kc, int lda, int ldc, int epilogue,
                         const gram_kv_bank_t* bank_host, const gram_norm_fusion_t* nf_host, const gram_split_t* split_host,
                         void* stream);
int gram_gemm_bf16_lse_split(const void* A, const void* W, float* logits, float* lse_part, int M, int N, int kc, int lda,
                             int ldc, const gram_split_t* split_host, void* stream);

/* The other kernels on two-piece operands.  Masks, bias tables, fp32 tensors and integer state are as in the plain entry points.
 * Outputs that feed a GEMM (xb, the norm's out, the attention outputs) are interleaved ([rows][2 * cols]) when pieces = 2; Q/K/V
 * inputs, the bank and the cache are planar, *_pstride elements apart. */
int gram_embed_ex_split(const float* table, const void* ids, int ids_are_i64, float* x, void* xb, float* ss, int nblk, int rows,
                        int d, int pieces, void* stream);
/* ... with the row factor of the 16-bit copy (gram_norm_fusion_t.xs_in of the consumer that follows): xs_out[m] = the factor of the
 * row's OWN rms, xb = pieces(x * xs_out[m]).  xs_out NULL = gram_embed_ex_split.  xb NULL: the 16-bit copy is
 * not written -- x, ss and xs_out are (the first consumer reads a token table instead: gram_model_build_token_tables). */
int gram_embed_ex_xs(const float* table, const void* ids, int ids_are_i64, float* x, void* xb, float* ss, float* xs_out, int nblk,
                     int rows, int d, int pieces, void* stream);
int gram_rmsnorm_bf16_split(const float* x, const float* w, void* out_bf16, int rows, int d, float eps, float scale,
                            const float* pos, int N, int L, const int32_t* passage_map, int pieces, void* stream);
int gram_enc_self_attn_split(const void* qkv, const float* bias, const uint8_t* mask, void* out, int P, int L, int H,
                             int pieces, int64_t qkv_pstride, void* stream);
/* ... with the q|k|v rows taken from a per-token table (gram_model_build_token_tables) instead of a per-row buffer: row `row` of
 * passage p is qkv_table + ids[p * L + row] * 3 * inner, ids i64 [P][L], every id a row of the table; qkv_pstride = elements
 * between the table's pieces.  Same bits as gram_enc_self_attn_split on the gathered rows. */
int gram_enc_self_attn_rows_split(const void* qkv_table, const int64_t* ids, const float* bias, const uint8_t* mask, void* out,
                                  int P, int L, int H, int pieces, int64_t qkv_pstride, void* stream);
/* Encoder self-attention for passages of up to GRAM_MAX_LONG_PASSAGE_LEN tokens: gram_enc_self_attn_split's operands and conventions
 * (planar q|k|v pieces, output interleaved at two pieces, unscaled scores, u8 key mask with finfo.min, fp32 softmax) for any
 * L = 32 n, 32 <= L <= 512.  One workgroup per (head, passage, block of 128 queries) walks the keys in tiles of 128 with an online
 * softmax.  The bias table stays [H][255]: the index is clamp(key - query, -127, 127) + 127, which is T5's bucket function wherever
 * relative_attention_max_distance <= 128 (the caller checks).  A key tile without a valid key is not fetched when the passage has a
 * valid key; a passage without one gets the uniform row over its L keys.  A row's bits depend on the row's passage alone -- its
 * tokens and valid keys -- not on L, P or the passage's place in the batch; they are NOT those of gram_enc_self_attn_split at
 * L <= 128 (another summation order).  A null pointer, a misaligned qkv / out or a piece stride shorter than the rows:
 * GRAM_E_ARG before any launch. */
int gram_enc_self_attn_long_split(const void* qkv, const float* bias, const uint8_t* mask, void* out, int P, int L, int H,
                                  int pieces, int64_t qkv_pstride, void* stream);
/* ... with the q|k|v rows taken from a per-token table (gram_enc_self_attn_rows_split's contract).  Same bits as
 * gram_enc_self_attn_long_split on the gathered rows. */
int gram_enc_self_attn_long_rows_split(const void* qkv_table, const int64_t* ids, const float* bias, const uint8_t* mask, void* out,
                                       int P, int L, int H, int pieces, int64_t qkv_pstride, void* stream);
/* users/rowpos NULL: all B users, rows b*K + beam; else the live-row form (gram_cross_attn_decode_live, B = n_users).
 * key_bits: gram_mask_key_bits(mask) computed once per generate (the mask is the same for every head, layer and step), or
 * NULL: every workgroup packs its user's bits from the mask bytes itself. */
int gram_cross_attn_decode_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out, int B,
                                 int K, int H, int S, const int32_t* users, const int32_t* rowpos, int pieces,
                                 int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, void* stream);
/* key_bits u32 [B][128]: bit j of word st = mask[b][32*st + j] != 0 (st < S/32). */
int gram_mask_key_bits(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* stream);
/* ---- cross-attention over up to GRAM_MAX_LONG_FUSED_LEN fused keys (the form a handle raised by gram_model_set_max_fused_len runs) ----
 * key_bits for the long form, u32 [B][GRAM_KEY_BITS_LONG_STRIDE]: words 0 .. GRAM_KEY_BITS_LONG_WORDS-1 of a row are the step words
 * (bit j of word st = mask[b][32*st + j] != 0, zero for st >= S/32), word GRAM_KEY_BITS_LONG_WORDS is the number of nonzero step
 * words (the user's valid 32-key steps; 0 = no valid key), the rest of the row is zero.  Any S = 32 n, 32 <= S <= 16 384; mask
 * 16-byte aligned.  The bits belong to the S they were packed for. */
#define GRAM_KEY_BITS_LONG_WORDS 512
#define GRAM_KEY_BITS_LONG_STRIDE 528
int gram_mask_key_bits_long(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* stream);
/* Bytes of fp32 scratch gram_cross_attn_long_split needs for `rows` = B * K (user, beam) slots: one unnormalised partial
 * (O[64], m, l: 68 floats) per slot, head and segment of 4096 keys; 0 for S <= 4096 (one segment stores directly).  GRAM_E_ARG for
 * rows or H < 1 or an S the kernel does not take. */
int64_t gram_cross_attn_long_scratch_bytes(int rows, int H, int S);
/* gram_cross_attn_decode_split's operands and conventions (planar Q pieces, K bank [s][64], V^T bank blocked by 32 keys, unscaled
 * scores, masked keys at finfo.min, fp32 softmax, output interleaved at two pieces, users/rowpos NULL or the live-row form) for any
 * S = 32 n, 32 <= S <= 16 384.  Split-key: a user's valid 32-key steps, counted in key order, are cut into segments of 128; one
 * workgroup per (head, user, segment) writes an unnormalised partial softmax to `scratch`, and a second kernel folds a row's
 * partials in ascending segment order (launched only for S > 4096; a user whose valid steps fit one segment is stored by that
 * segment).  No atomics, one fixed summation order.  A row's bits depend on its query row and on the user's valid steps in order:
 * not on B, the user's place in the batch, K, the live-row form, or where the masked steps lie between the valid ones (the
 * batch's L and N) -- and they are NOT gram_cross_attn_decode_split's bits.  Fully masked steps are never fetched and masked keys
 * contribute exactly nothing, whatever the bank holds there; a user without a valid key gets the uniform row over exactly S keys.
 * key_bits: gram_mask_key_bits_long of the same mask and S (required; `mask` itself is not read).  scratch: 16-byte aligned,
 * gram_cross_attn_long_scratch_bytes(B * K, H, S) bytes, may be NULL for S <= 4096.  GRAM_E_ARG before any launch: a null q / k_layer /
 * vt_layer / out / key_bits, a misaligned pointer, S out of range, K > GRAM_MAX_BEAMS, or (two pieces) q_pstride < B*K*H*64 in the
 * all-rows form or bank_pstride < H*S*64. */
int gram_cross_attn_long_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out, int B, int K,
                               int H, int S, const int32_t* users, const int32_t* rowpos, int pieces, int64_t q_pstride,
                               int64_t bank_pstride, const uint32_t* key_bits, float* scratch, void* stream);
/* rows NULL: all R rows; else the live-row form (gram_dec_self_attn_live). */
int gram_dec_self_attn_split(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias, void* out,
                             int R, int n_rows, const int32_t* rows, int H, int t, int Tmax, int pieces, int64_t qkv_pstride,
                             int64_t cache_pstride, void* stream);
/* ... with the new token's q|k|v taken from a per-token table: compact row r reads qkv_table + qkv_rows[r] * 3 * inner (qkv_rows
 * i32 [n_rows]: the step's token array, every entry a row of the table).  Cache writes, ancestor reads and `rows` are unchanged. */
int gram_dec_self_attn_rows_split(const void* qkv_table, const int32_t* qkv_rows, void* kcache, void* vcache, const int32_t* anc,
                                  const float* bias, void* out, int R, int n_rows, const int32_t* rows, int H, int t, int Tmax,
                                  int pieces, int64_t qkv_pstride, int64_t cache_pstride, void* stream);
/* lm_head with the log-softmax normaliser fused: logits as GRAM_EPI_F32, plus for every row and every
 * 64-column block the pair (max, sum exp(x - max)) in lse_part f32 [M][N/64][2]; gram_lse_combine folds
 * them into lse[M] = log sum_v exp(logits[m][v]) without re-reading the logits (gram_row_lse does).
 * logits may be NULL: then only the partials are produced (see gram_beam_step_sparse). */
int gram_gemm_bf16_lse(const void* A, const void* W, float* logits, float* lse_part, int M, int N, int K, int lda,
                       int ldc, void* stream);
int gram_lse_combine(const float* lse_part, float* lse, int M, int nblk, void* stream);

/* x[row][:] = table[ids[row]][:]   (embed_tokens, gram_t5_modeling.py:1091). */
int gram_embed_i64(const float* table, const int64_t* ids, float* x, int rows, int d, void* stream);
int gram_embed_i32(const float* table, const int32_t* ids, float* x, int rows, int d, void* stream);

/* T5LayerNorm (gram_t5_modeling.py:262-276) with the two fusions the path needs:
 *   out_bf16[row][i] = bf16( x[row][i] * rsqrt(mean(x^2)+eps) * w[i] * scale
 *                            + (pos ? pos[(row / L) % N][i] : 0) )
 * scale = d_model^-0.5 for the tied lm_head (gram_t5.py:249-252); pos = per-passage position
 * embedding of the late fusion (gram.py:238-249). */
int gram_rmsnorm_bf16(const float* x, const float* w, void* out_bf16, int rows, int d, float eps,
                      float scale, const float* pos, int N, int L, void* stream);
/* same, for compacted passages: the passage of row r is passage_map[r / L] % N (see gram_kv_bank_t) */
int gram_rmsnorm_bf16_map(const float* x, const float* w, void* out_bf16, int rows, int d, float eps, float scale,
                          const float* pos, int N, int L, const int32_t* passage_map, void* stream);

/* Encoder self-attention for P passages of L tokens (T5Attention.forward, bidirectional,
 * gram_t5_modeling.py:479-631): unscaled QK^T + bucketed relative bias + key mask, fp32
 * softmax, @V.  qkv: bf16 [P*L][3*inner] (q|k|v); bias: f32 [H][255] indexed by
 * (key - query + 127); mask: u8 [P][L] (1 = valid); out: bf16 [P*L][inner]. */
int gram_enc_self_attn(const void* qkv, const float* bias, const uint8_t* mask, void* out, int P,
                       int L, int H, void* stream);

/* Late-fusion cross-attention for one decoder layer and one decode step (the fusion read:
 * T5Attention.forward cross branch, gram_t5_modeling.py:531-534,547-549,572-622; zero position
 * bias :577-582; mask :1145-1147).  q: bf16 [B*K][inner] (row = b*K + beam); k/vt: that layer's
 * slices of the bank; mask: u8 [B][S]; out: bf16 [B*K][inner].  S % 32 == 0, K <= 64. */
int gram_cross_attn_decode(const void* q, const void* k_layer, const void* vt_layer,
                           const uint8_t* mask, void* out, int B, int K, int H, int S, void* stream);

/* Decoder causal self-attention for the token at position t with a slot cache and beam-parent
 * indirection instead of the reference's torch.cat + index_select (gram_t5_modeling.py:536-540,
 * 586-593; gram_t5.py:320-348).  qkv: bf16 [R][3*inner]; kcache/vcache: bf16 [Tmax][R][inner]
 * (this layer); anc: i32 [Tmax][R], anc[j][r] = row whose step-j K/V is r's ancestor (j < t);
 * bias: f32 [H][GRAM_MAX_DEC_LEN] indexed by distance t-j.  Writes this step's k,v into slot t. */
int gram_dec_self_attn(const void* qkv, void* kcache, void* vcache, const int32_t* anc,
                       const float* bias, void* out, int R, int H, int t, int Tmax, void* stream);

/* lse[r] = log(sum_v exp(logits[r][v]))   (the normaliser of HF's log_softmax in beam_search).
 * A logit of -inf adds nothing; a row of -inf throughout gives -inf. */
int gram_row_lse(const float* logits, float* lse, int R, int V, void* stream);

/* Flat Trie in HBM (CSR), built from generation_trie.py:5-68's nested dict by
 * gram_amd.utils.generation_trie.FlatTrie.  Children of node n are
 * child_tok/child_node[child_off[n] .. child_off[n+1]), sorted by token.  Node 0 is the root. */
typedef struct {
  const int32_t* child_off;
  const int32_t* child_tok;
  const int32_t* child_node;
  int32_t n_nodes, n_edges, max_fanout; /* max_fanout: the largest child count of a node, <= the vocabulary; any value is supported.
                                           The search step holds all K * max_fanout candidates of a user on chip at once while
                                           K * max_fanout <= 16 384 (and they fit the LDS beside the call's [K][Tmax] tables),
                                           and streams them through a fixed-size array beyond that: the same results either way */
  int32_t min_seq_len; /* shortest candidate sequence, start token and EOS included; 0 = unknown (gram_generate then
                          never tries the live-row compaction below) */
} gram_trie_t;

/* Beam-search state for B users x K beams (HF transformers 4.26 beam_search + BeamSearchScorer
 * + BeamHypotheses state, kept on the device).  All arrays are caller-allocated. */
typedef struct {
  int32_t B, K, Tmax;      /* Tmax = max_length                                           */
  float length_penalty;
  int32_t eos, pad;
  int32_t* tokens;         /* [R]        next decoder input token per row                  */
  int32_t* node;           /* [R]        Trie node of each beam's prefix, -1 = not in Trie */
  float* beam_scores;      /* [R]                                                        */
  int32_t* seq;            /* [R][Tmax]  input_ids of each beam                           */
  int32_t* anc;            /* [Tmax][R]  self-attention ancestor table                    */
  int32_t* done;           /* [B]                                                        */
  int32_t* n_hyps;         /* [B]                                                        */
  double* hyp_score;       /* [B][K+1]   length-normalised score (Python float semantics);
                              one spare slot: BeamHypotheses.add appends, then drops the worst */
  double* worst;           /* [B]                                                        */
  int32_t* hyp_len;        /* [B][K+1]                                                   */
  int32_t* hyp_tok;        /* [B][K+1][Tmax]                                             */
  int32_t* error;          /* [1]        set non-zero on an impossible state              */
  /* optional scratch (NULL / 0 = off): with B <= cand_logits_users (and <= 16) users a sparse search step computes its candidates'
   * logits with a kernel of its own over many CUs before the per-user search kernel runs -- one workgroup per user pulls up to
   * K * fan-out lm_head rows through ONE CU, most of a one-user step.  f32 [cand_logits_users][cand_logits_stride],
   * cand_logits_stride >= the power of two >= K * max_fanout.  Same values either way.  Used by the one-shot search step only
   * (K * max_fanout <= 16 384, gram_trie_t): a wider step streams its candidates and computes their logits itself, so the scratch
   * never has to be larger than [16][16 384]. */
  float* cand_logits;
  int32_t cand_logits_users;
  int64_t cand_logits_stride;
} gram_beam_state_t;

/* decoder_input_ids = [[start]]*B*K ; beam_scores = [0,-1e9,...] (HF 4.26 beam_search init). */
int gram_beam_init(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, int start_token,
                   void* stream);

/* One search step, cur_len = number of tokens already in each beam:
 *   log_softmax (via lse) -> PrefixConstrainedLogitsProcessor (Trie children; -inf elsewhere)
 *   -> + beam_scores -> top-2K over K*V (ties: lower flat index first) -> BeamSearchScorer.process
 *   -> next tokens / scores / parents, sequences and the ancestor table advanced in place.
 * Replaces HF 4.26 beam_search's per-step body and generation_trie.py:89-95's per-beam Python
 * callback (one D2H sync per beam per step in the reference).
 * rows_per_user = K normally (logits/lse have one row per beam); 1 when the K beams of a user share
 * one logits row and one self-attention cache row (step 0, where all beams are identical). */
int gram_beam_step(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits,
                   const float* lse, int V, int cur_len, int rows_per_user, void* stream);

/* Same step without a materialised logits tensor: the logits of the allowed tokens are recomputed inside the
 * kernel as hidden[row] . lm_head[tok] (bf16 operands, fp32 accumulate), `lse` coming from
 * gram_gemm_bf16_lse(logits = NULL) + gram_lse_combine.  hidden: bf16 [rows][d] (the lm_head A operand). */
int gram_beam_step_sparse(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                          const void* lm_head_bf16, int d, const float* lse, int V, int cur_len, int rows_per_user,
                          void* stream);

/* Live rows.  When a beam emits EOS its hypothesis moves to the heap and HF refills the slot with a -inf candidate
 * (BeamSearchScorer.process); such a row, and every row of a finished user, can only produce -inf candidates from then
 * on, so nothing downstream reads its decoder output -- but the reference still runs the decoder on it.  With item
 * ids of l or l+1 pieces most rows of the last step are in that state.  gram_live_rows compacts the
 * others (ascending, so grouped by user); the *_live variants of the per-row kernels then work on compact rows while
 * the self-attention cache, the ancestor table, the bank and the beam state keep their original indexing.
 * Results are bit-identical to running every row (every kernel of the step is row-independent). */
typedef struct {
  int32_t* rows;   /* [R]  original row of compact row i                                   */
  int32_t* rowpos; /* [R]  compact row of original row r, -1 = not live                    */
  int32_t* users;  /* [B]  users owning at least one live row, ascending                   */
  int32_t* tokens; /* [R]  decoder input token of compact row i                            */
  int32_t* counts; /* [2]  number of live rows, number of such users                       */
} gram_live_rows_t;
int gram_live_rows(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const gram_live_rows_t* out_host,
                   void* stream);
/* gram_dec_self_attn on n_rows compact rows: qkv/out [n_rows][..] compact, cache/anc rows = rows[i] of R. */
int gram_dec_self_attn_live(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias,
                            void* out, int R, int n_rows, const int32_t* rows, int H, int t, int Tmax, void* stream);
/* gram_cross_attn_decode for the n_users users in `users`; q/out rows = rowpos[user*K + beam] (skipped if -1). */
int gram_cross_attn_decode_live(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask,
                                void* out, int n_users, const int32_t* users, const int32_t* rowpos, int K, int H,
                                int S, void* stream);
/* gram_beam_step_sparse with hidden/lse indexed by compact row (all B users are stepped). */
int gram_beam_step_sparse_live(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                               const void* lm_head_bf16, int d, const float* lse, int V, int cur_len,
                               const int32_t* rowpos, void* stream);

/* gram_beam_step_sparse[_live] with the hidden state as pieces (interleaved [rows][2 d] when pieces = 2): the allowed logits are
 * h . E[tok] in fp32, h the fp32 sum of the pieces and E the FP32 lm_head table [V][d] (rowpos NULL: rows b*K + beam,
 * rows_per_user as in gram_beam_step). */
int gram_beam_step_sparse_split(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                                const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                const int32_t* rowpos, int pieces, void* stream);

/* ---- per-user item filters: every user searches its own view of the shared Trie ------------------------------------------------
 * User b has an item set A_b, a subset of the candidate list the Trie was built from: A_b = its list (GRAM_ITEMS_ALLOW) or every
 * candidate but its list (GRAM_ITEMS_EXCLUDE).  The search step then offers a child token iff some item of A_b lies below it --
 * exactly what HF's PrefixConstrainedLogitsProcessor does with prefix_allowed_tokens_fn(Trie(A_b)) for that user alone; everything
 * else is -inf, and the -inf fillers are still the lowest token ids of beam 0 that are not offered.
 * Mechanism: the Trie's leaves are numbered in lexicographic order of their sequences (the leaf RANK), so the leaves below node n
 * are the contiguous ranks [leaf_lo[n], leaf_hi[n]).  A user's list travels as its distinct leaf ranks in ascending order; node n
 * is alive for the user iff the number c of its ranks inside [leaf_lo[n], leaf_hi[n]) -- two binary searches -- is > 0 (allow) or
 * < leaf_hi[n] - leaf_lo[n] (exclude).  Two candidates that spell the same sequence share a leaf: listing either lists the sequence.
 * All arrays are caller-allocated; gram_workspace_bytes does not change. */
#define GRAM_MAX_USER_ITEMS 4096 /* entries of one user's list (the preparation kernel sorts them in 16 KB of LDS) */
#define GRAM_ITEMS_EXCLUDE 0
#define GRAM_ITEMS_ALLOW 1
typedef struct {
  const int32_t* leaf_lo; /* [n_nodes]   first leaf rank below (or at) each node                            */
  const int32_t* leaf_hi; /* [n_nodes]   one past the last                                                  */
  const int32_t* ranks;   /* [B][stride] each user's leaf ranks, ascending and distinct                     */
  const int32_t* count;   /* [B]         how many of them                                                   */
  int32_t stride;         /* 1 .. GRAM_MAX_USER_ITEMS                                                       */
  int32_t mode;           /* GRAM_ITEMS_EXCLUDE or GRAM_ITEMS_ALLOW                                         */
} gram_user_items_t;

/* A call's lists -> gram_user_items_t.ranks / .count.  items i32 [B][M]: indices into the candidate list, -1 = padding (dropped);
 * item_rank i32 [n_items]: leaf rank of every candidate (an index outside [0, n_items) is dropped like padding: the caller
 * validates).  One workgroup per user maps, sorts and de-duplicates in LDS.  1 <= M <= stride <= GRAM_MAX_USER_ITEMS. */
int gram_user_items_prepare(const int32_t* item_rank, int n_items, const int32_t* items, int B, int M, int32_t* ranks,
                            int32_t* count, int stride, void* stream);

/* gram_beam_step_sparse / gram_beam_step_sparse_live (rowpos != NULL: the live-row form, rows_per_user must be K) with the lists. */
int gram_beam_step_sparse_items(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                                const void* lm_head_bf16, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                const int32_t* rowpos, const gram_user_items_t* items_host, void* stream);
/* gram_beam_step_sparse_split with the lists (rowpos != NULL: rows_per_user must be K, as above). */
int gram_beam_step_sparse_split_items(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                                      const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                      const int32_t* rowpos, int pieces, const gram_user_items_t* items_host, void* stream);
/* gram_greedy_step with the lists: the argmax runs over the alive children. */
int gram_greedy_step_items(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits, int V, int cur_len,
                           const gram_user_items_t* items_host, void* stream);
/* Every entry point that takes the lists returns GRAM_E_ARG before any launch for items_host == NULL, a NULL array, a stride
 * outside 1 .. GRAM_MAX_USER_ITEMS or an unknown mode.  (Sets of more than GRAM_MAX_USER_ITEMS entries: the masks below.) */

/* ---- per-user item masks: a user's item set of ANY size -----------------------------------------------------------
 * The second representation of A_b (above): a bitset over the leaf ranks with a running count beside every word.  User b owns
 * `stride` records of two 32-bit words {bits, before}, of which W = n_leaves / 32 + 1 are in use: bit j of record w's `bits` says
 * that the leaf of rank 32 w + j is kept (ranks >= n_leaves: 0), `before` is the number of kept leaves in the records < w.  The kept
 * leaves below rank x are  count(x) = before[x >> 5] + popcount(bits[x >> 5] & ((1u << (x & 31)) - 1))  -- the last record always
 * exists, so x = n_leaves indexes inside the row -- and node n is alive for the user iff count(leaf_hi[n]) - count(leaf_lo[n]) > 0:
 * two 8-byte loads whatever the set's size, at 2 bits per leaf.  The semantics are GRAM_ITEMS_ALLOW's with the same set: exactly
 * what HF's PrefixConstrainedLogitsProcessor does with prefix_allowed_tokens_fn(Trie(A_b)) for that user alone, -inf fillers
 * included.  All arrays are caller-allocated; gram_workspace_bytes does not change. */
typedef struct gram_user_mask gram_user_mask_t;
struct gram_user_mask {
  const int32_t* leaf_lo; /* [n_nodes]         first leaf rank below (or at) each node (gram_user_items_t's table)  */
  const int32_t* leaf_hi; /* [n_nodes]         one past the last                                                    */
  const uint32_t* words;  /* [B][stride][2]    = {bits, before}; 8-byte aligned                                     */
  int64_t stride;         /* records per user, >= n_leaves / 32 + 1                                                 */
  int32_t n_leaves;       /* >= 1                                                                                   */
}; /* (40 bytes; its ctypes mirror is checked by tests/test_item_mask_host.py) */
/* Records of one user's row: n_leaves / 32 + 1 (GRAM_E_ARG for n_leaves < 1). */
int64_t gram_user_mask_words(int n_leaves);
/* A call's masks -> gram_user_mask_t.words and count[b] = the number of leaves user b keeps.  mask u8: row b at mask + b *
 * mask_stride, n_items bytes, non-zero = the user may get the candidate (what `M[b] != 0` is in torch); leaf_item i32 [n_leaves]:
 * the candidate that names the leaf of every leaf rank (gram_item_bias_table's table; a value outside [0, n_items): no candidate
 * names the leaf, its bit is 0).  One launch, one workgroup per user, one pass over the leaf ranks; no atomics, the same words in
 * any geometry; records [n_leaves / 32 + 1, stride) are left untouched.  1 <= n_leaves <= 2^24, mask_stride >= n_items >= 1. */
int gram_user_mask_prepare(const uint8_t* mask, int64_t mask_stride, int B, int n_items, const int32_t* leaf_item, int n_leaves,
                           uint32_t* words, int64_t stride, int32_t* count, void* stream);
/* gram_beam_step_sparse / _live / _split with the masks: lm_head_bf16 / lm_head_f32 / pieces as in gram_beam_step_groups_sparse
 * (pieces == 1 reads lm_head_bf16; two pieces, or no lm_head_bf16, lm_head_f32), rowpos != NULL: the live-row form, rows_per_user
 * must be K.  The same launch forms as gram_beam_step_sparse_items (one-shot, chunked, the scratch logits of <= 16 users), and in
 * GRAM_ITEMS_ALLOW mode with the same sets the same state bit for bit. */
int gram_beam_step_sparse_mask(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                               const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                               int rows_per_user, const int32_t* rowpos, int pieces, const gram_user_mask_t* mask_host, void* stream);
/* gram_greedy_step with the masks: the argmax runs over the alive children (gram_greedy_step_items with the same sets). */
int gram_greedy_step_mask(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits, int V, int cur_len,
                          const gram_user_mask_t* mask_host, void* stream);
/* Every entry point that takes the masks returns GRAM_E_ARG before any launch, the state untouched, for mask_host == NULL, a NULL
 * array, words not 8-byte aligned, n_leaves < 1 or a stride below gram_user_mask_words(n_leaves). */

/* HF 4.26 greedy_search (generate with num_beams == 1; BASELINE configs[0]) on the same state with K = 1:
 * argmax of the RAW logits over the Trie children (first maximum), finished users emit pad; finalize copies
 * the sequences (i64 [B][max_length]) and reports the width HF would return (it stops once all rows hit EOS). */
int gram_greedy_step(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits, int V,
                     int cur_len, void* stream);
int gram_greedy_finalize(const gram_beam_state_t* st_host, int max_length, int64_t* sequences, int32_t* out_width,
                         void* stream);

/* BeamSearchScorer.finalize: sequences int64 [B*nret][Tmax] (0-padded, EOS appended when it
 * fits), scores f32 [B*nret], out_width[0] = min(max hyp len + 1, max_length). */
int gram_beam_finalize(const gram_beam_state_t* st_host, int nret, int max_length, int64_t* sequences,
                       float* scores, int32_t* out_width, void* stream);

/* Item index of each returned sequence.  Every hypothesis of a Trie-constrained search is a root-to-leaf path of the candidate Trie,
 * so what the runner does next per user -- tokenizer.batch_decode of the K generated id rows and a string comparison with the decoded
 * target (single_runner_gram.py:657-673, evaluate.py:5-22) -- needs only WHICH candidate each row spells: the strings come from one
 * batch_decode of the candidate list per evaluation.  sequences i64 [rows][T] as gram_beam_finalize / gram_generate wrote them (start
 * token first, 0-padded); node_item i32 [n_nodes]: candidate index of a leaf node (the first one if several candidates share a
 * sequence), anything for inner nodes.  out_item i32 [rows]: the index, or -1 when the row is not a candidate sequence followed by
 * padding (the -inf filler beams HF returns when fewer than nret hypotheses finished): the caller decodes those rows itself. */
int gram_trie_item_index(const gram_trie_t* trie_host, const int32_t* node_item, const int64_t* sequences, int rows, int T,
                         int32_t* out_item, void* stream);

/* ---- whole-path entry points ---------------------------------------------------------- */
typedef struct {
  int32_t vocab, d_model, d_ff, n_heads, n_enc_layers, n_dec_layers, max_passages;
  int32_t tie_word_embeddings, use_position_embedding;
  int32_t fold_norm; /* 1: enc_wqkv/enc_wi/dec_wqkv/dec_wq_x/dec_wi carry their layer-norm gain (gram_norm_fusion_t path) */
  float eps;
  const float* embed_f32;      /* [V][d]      shared.weight                                */
  const void* lm_head_bf16;    /* [V][d]      lm_head.weight                               */
  const float* pos_emb_f32;    /* [max_passages][d] or NULL                                */
  const float* enc_bias_f32;   /* [H][255]    encoder relative bias, layer-0 table         */
  const float* dec_bias_f32;   /* [H][GRAM_MAX_DEC_LEN] decoder relative bias by distance  */
  const float* enc_final_ln;   /* [d]                                                     */
  const float* dec_final_ln;   /* [d]                                                     */
  /* per-layer arrays (HOST arrays of device pointers) */
  const float* const* enc_ln1; /* [n_enc]  layer.0.layer_norm                              */
  const void* const* enc_wqkv; /* [n_enc]  bf16 [3*inner][d]  (q;k;v rows concatenated)    */
  const void* const* enc_wo;   /* [n_enc]  bf16 [d][inner]                                 */
  const float* const* enc_ln2; /* [n_enc]                                                 */
  const void* const* enc_wi;   /* [n_enc]  bf16 [d_ff][d]                                  */
  const void* const* enc_wo2;  /* [n_enc]  bf16 [d][d_ff]                                  */
  const float* const* dec_ln1; /* [n_dec]                                                 */
  const void* const* dec_wqkv; /* [n_dec]  bf16 [3*inner][d]                               */
  const void* const* dec_wo;   /* [n_dec]  bf16 [d][inner]                                 */
  const float* const* dec_ln2; /* [n_dec]                                                 */
  const void* const* dec_wq_x; /* [n_dec]  bf16 [inner][d]   EncDecAttention.q             */
  const void* const* dec_wo_x; /* [n_dec]  bf16 [d][inner]   EncDecAttention.o             */
  const float* const* dec_ln3; /* [n_dec]                                                 */
  const void* const* dec_wi;   /* [n_dec]  bf16 [d_ff][d]                                  */
  const void* const* dec_wo2;  /* [n_dec]  bf16 [d][d_ff]                                  */
  const void* dec_wkv_x_all;   /* bf16 [n_dec*2*inner][d]: per layer k rows then v rows     */
  /* two-piece mode (gram_split_t): pieces = 2 ("f16x3" / "bf16x3"); 0 / 1 = one piece.  Then EVERY 16-bit weight above is the
   * interleaved two-piece matrix [out][in / 32][2][32] and lm_head_f32 [V][d] must be given too (the beam kernel's sparse
   * logits).  fold_norm must be 1. */
  int32_t pieces;
  const float* lm_head_f32;
  /* Power-of-two factors the 16-bit weight matrices above were multiplied by before they were rounded (HOST array, or NULL = all
   * 1): [enc_wqkv x n_enc][enc_wo x n_enc][enc_wi x n_enc][enc_wo2 x n_enc][dec_wqkv x n_dec][dec_wo][dec_wq_x][dec_wo_x][dec_wi]
   * [dec_wo2 x n_dec][dec_wkv_x_all][lm_head]  (4 n_enc + 6 n_dec + 2 floats).  Every GEMM multiplies its result by the inverse
   * (gram_split_t.out_scale).  Used by the f16 build (gram_piece_format() == 1): an IEEE-half low piece of a small weight would
   * otherwise be subnormal and lose bits; bf16 has fp32's exponent range and needs none. */
  const float* w_scales;
} gram_model_desc_t;

typedef struct gram_model gram_model_t;

/* Copies the descriptor (not the weights).  Mirrors create_model("gram", config) +
 * load_state_dict (src/model/__init__.py:9-24, gram.py:162-165).
 * NULL for a shape the kernels do not cover: vocab, d_model and d_ff are positive multiples of 128, d_model <= 1024, n_heads even
 * and <= 16 (inner = 64 n_heads, independent of d_model), at least one layer per stack, pieces 0..2; two pieces need lm_head_f32
 * and fold_norm (tests/test_model_shapes_host.py). */
gram_model_t* gram_model_create(const gram_model_desc_t* desc_host);
void gram_model_destroy(gram_model_t* m);

/* Longest passage the handle's whole-path entry points take (default GRAM_MAX_PASSAGE_LEN).  Lmax must be a multiple of 32 in
 * [GRAM_MAX_PASSAGE_LEN, GRAM_MAX_LONG_PASSAGE_LEN] (GRAM_E_ARG otherwise).  A handle with Lmax > 128 runs the long encoder
 * self-attention (gram_enc_self_attn_long[_rows]_split) at EVERY L, so that a passage's bits never depend on the padded length of
 * the batch it landed in; a handle at 128 launches exactly what it always launched.  Every whole-path entry point and workspace
 * query returns GRAM_E_ARG for L > Lmax or N * L above the handle's fused limit (gram_model_set_max_fused_len; 4096 by default)
 * before any launch.  The caller guarantees that the encoder's bias is
 * constant beyond distance +-127 (relative_attention_max_distance <= 128) before raising the limit. */
int gram_model_set_max_passage_len(gram_model_t* m, int Lmax);

/* Longest fused context S = N * L the handle's whole-path entry points take (default GRAM_MAX_FUSED_LEN).  Smax must be a multiple
 * of 32 in [GRAM_MAX_FUSED_LEN, GRAM_MAX_LONG_FUSED_LEN] (GRAM_E_ARG otherwise, the limit unchanged).  A handle with Smax > 4096 runs
 * the long cross-attention (gram_mask_key_bits_long, gram_cross_attn_long_split, gram_cross_attn_rows_long_split) at EVERY S -- in the
 * decode step's all-rows and live-row forms, the teacher-forced pass and gram_score_trie -- so that a user's bits never depend on
 * whether its batch crossed 4096; its workspaces hold the wider key bits and the long form's scratch.  A handle at 4096 launches
 * exactly what it always launched.  Cross-attention probabilities stay limited to 4096 keys: gram_teacher_forced_ex with attention
 * outputs returns GRAM_E_ARG for N * L > 4096 on any handle. */
int gram_model_set_max_fused_len(gram_model_t* m, int Smax);

/* Layer-0 q|k|v per TOKEN.  T5 has no absolute positions: the first sublayer of each stack norms the raw embedding row of a token
 * (row-local) and multiplies it by layer 0's W_qkv, so its q|k|v row depends on the token id and the weights only.  The two tables
 * (encoder, decoder: shared embedding, own W_qkv), each [pieces][vocab][3 * inner] 16-bit planar pieces, are computed once per
 * handle by the path's own launches (embedding of ids 0 .. vocab-1, the folded norm, the layer-0 QKV GEMM: the same bits a row
 * holding that token gets today); generate / encode / decode-step calls on a handle that has them read layer 0's q|k|v from the
 * tables and launch no layer-0 QKV GEMM.  The teacher-forced pass keeps its GEMM.  A handle without tables behaves as before.
 * gram_token_tables_bytes: bytes of both tables (0: no tables for this model -- unfolded norms);
 * gram_token_tables_workspace_bytes: scratch of the build (free again once the build's launches have run);
 * gram_model_build_token_tables: launches the build on `stream` into caller-owned memory (256-B aligned) that must outlive the
 * handle's use, and records the tables in the handle. */
int gram_iota_i32(int32_t* out, int n, void* stream); /* out[i] = i, i < n: the build's token ids */
int64_t gram_token_tables_bytes(const gram_model_t* m);
int64_t gram_token_tables_workspace_bytes(const gram_model_t* m);
int gram_model_build_token_tables(gram_model_t* m, void* tables, int64_t tables_bytes, void* workspace, int64_t workspace_bytes,
                                  void* stream);

/* Bytes of scratch gram_generate needs for this problem size (256-B aligned carve). */
int64_t gram_workspace_bytes(const gram_model_t* m, int B, int N, int L, int K, int max_length);

/* EncoderWrapper.forward + the fused-bank projection (gram.py:200-256; gram_t5_modeling.py
 * T5Stack encoder role; cross K/V projection :531-534 for every decoder layer at once).
 * input_ids i64 [B][N][L], mask u8 [B][N][L].  Writes the bank into the workspace; when
 * enc_out_bf16 != NULL also copies the fused encoder states there (tests): [B*N*L][d], or in the two-piece mode the
 * interleaved [B*N*L][2 d]. */
int gram_encode_fused(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N,
                      int L, void* workspace, int64_t workspace_bytes, int K, int max_length,
                      void* enc_out_bf16, void* stream);

/* One cached decoder step for all B*K rows at position t, using the bank a preceding
 * gram_encode_fused left in the same workspace (T5ForConditionalGeneration_GRAM.forward with
 * encoder_outputs given, gram_t5.py:181-254).  tokens i32 [B*K]; anc as in gram_dec_self_attn;
 * logits f32 [B*K][V] (device, caller-owned). */
int gram_decode_step(const gram_model_t* m, const int32_t* tokens, const int32_t* anc, const uint8_t* mask,
                     int B, int N, int L, int K, int max_length, int t, void* workspace,
                     int64_t workspace_bytes, float* logits, void* stream);

/* GRAM.generate (gram.py:74-107) with the runner's kwargs (single_runner_gram.py:641-651):
 * encoder -> late fusion -> bank -> max_length-1 constrained beam-search steps -> finalize.
 * sequences i64 [B*nret][max_length], scores f32 [B*nret]; *width_host receives
 * min(max hyp len + 1, max_length) (the column count HF returns) if non-NULL, which costs one
 * stream synchronise.  Returns GRAM_E_BEAM if the device flagged an impossible beam state.
 * K == 1 follows HF's dispatch to greedy_search: `scores` may be NULL and is not written. */
int gram_generate(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                  int K, int nret, int max_length, float length_penalty, const gram_trie_t* trie_host,
                  void* workspace, int64_t workspace_bytes, int64_t* sequences, float* scores,
                  int32_t* width_host, void* stream);

/* Ragged batches: the Collator pads every user to the batch's largest passage count with fully masked passages
 * (Collator.py:410-436); the encoder need not run on those.  The caller passes the n_active passages that have
 * at least one valid token, gathered contiguously (ids/mask [n_active][L]), and their flat indices
 * passage_map[p] = b*N + n (ascending).  `mask` stays the full (B,N,L) mask: the cross-attention skips the
 * untouched bank positions of the padded passages.  Every user must keep >= 1 active passage. */
typedef struct {
  int32_t n_active;
  const int32_t* passage_map; /* device, i32 [n_active] */
  const int64_t* ids;         /* device, i64 [n_active - n_cached][L] */
  const uint8_t* mask;        /* device, u8  [n_active - n_cached][L] */
  /* Passage cache (all zero = off).  An item passage's encoder output depends neither on the
   * user nor on the slot it sits in: EncoderWrapper runs every passage on its own and adds the slot's position
   * embedding afterwards (gram.py:238-255).  The LAST n_cached entries of passage_map skip the encoder: their
   * residual-stream rows (gram_encode_passages) are gathered from cache_x[cache_slot[i]] instead; rows at
   * positions >= cache_L are zero-filled (they are padding, masked in the cross-attention).  passage_map need
   * not be ascending.  Results are bit-identical to encoding the passages in place. */
  int32_t n_cached;
  int32_t cache_L;            /* rows per cached passage */
  const float* cache_x;       /* device, f32 [slots][cache_L][d_model] */
  const int32_t* cache_slot;  /* device, i32 [n_cached] */
} gram_compaction_t;
int gram_generate_ex(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                     int K, int nret, int max_length, float length_penalty, const gram_trie_t* trie_host,
                     const gram_compaction_t* compaction_host, void* workspace, int64_t workspace_bytes,
                     int64_t* sequences, float* scores, int32_t* width_host, void* stream);

/* gram_generate_ex with per-user item filters (gram_user_items_t, prepared by gram_user_items_prepare on the same stream): every
 * search step and the greedy step take the lists; everything else -- the encoder, the decoder, the workspace, the live-row
 * compaction -- is gram_generate_ex's.  The caller guarantees every user at least one item.  GRAM_E_ARG for bad lists as above. */
int gram_generate_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                        int max_length, float length_penalty, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                        const gram_user_items_t* items_host, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                        float* scores, int32_t* width_host, void* stream);

/* gram_generate_ex with per-user item masks (gram_user_mask_t, prepared by gram_user_mask_prepare on the same stream): every search
 * step and the greedy step take the masks -- gram_generate_items' call with the masks in the lists' place: the same workspace
 * (gram_workspace_bytes), the same step-wise launch train, the same live-row compaction, no tail pass.  Stands for HF's generate
 * with prefix_allowed_tokens_fn(Trie(A_b)) per user, for sets of any size.  The caller guarantees every user at least one item
 * (gram_user_mask_prepare's count).  GRAM_E_ARG for bad masks as above. */
int gram_generate_mask(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                       int max_length, float length_penalty, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                       const gram_user_mask_t* mask_host, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                       float* scores, int32_t* width_host, void* stream);

/* ---- Group (diverse) beam search: HF 4.26 `group_beam_search` + HammingDiversityLogitsProcessor on a Trie ----------
 * K beams = num_groups groups of gs = K / num_groups; group g owns beams [g gs, (g + 1) gs) of every user.  The state is the plain
 * search's gram_beam_state_t: ONE hypothesis heap of capacity K and one done flag per user, shared by its groups.
 * One step, for every user and for g = 0 .. num_groups - 1 in order:
 *   a done user's group gets score 0 and token pad; otherwise candidate (beam k of the group, child token v of its Trie node) scores
 *     s = logit[row k][v] - lse[row k];  s = s - diversity_penalty * c_v;  s = s + beam_scores[k]       (fp32, one rounding each),
 *   c_v = the beams of groups 0 .. g - 1 of this user whose token chosen in THIS step is v (nothing is subtracted where c_v = 0 or
 *   the penalty is 0); the best 2 gs of the group's candidates, ties to the lower k * V + v, padded with -inf fillers on the
 *   group's first beam, go through BeamSearchScorer.process with group size gs (EOS at rank < gs -> the user's heap; the other
 *   candidates fill the group's gs slots; fewer than gs is error 1), and done |= heap.is_done(the group's best score, cur_len) --
 *   so a user can finish at group g of a step: its later groups are padded in the same step.
 * Then all K rows advance at once.  gram_beam_finalize is the plain search's.  num_groups == 1 with diversity_penalty == 0 is the
 * plain step bit for bit.  GRAM_E_ARG, before any launch: num_groups < 1, > K or not a divisor of K; a penalty that is negative or
 * not finite. */
/* gram_beam_init for a group search: the first beam of every GROUP starts at score 0, the others at -1e9. */
int gram_beam_init_groups(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, int start_token, int num_groups,
                          void* stream);
/* One group step on dense logits f32 [B * rows_per_user][V] (as gram_beam_step; for tests on given logits). */
int gram_beam_step_groups(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits, const float* lse, int V,
                          int cur_len, int rows_per_user, int num_groups, float diversity_penalty, void* stream);
/* One group step on hidden states (the sparse logits of gram_beam_step_sparse).  lm_head_bf16 / lm_head_f32 / pieces as in
 * gram_sample_step; rowpos as in gram_beam_step_sparse_live (NULL: rows in place); items_host: per-user item filters or NULL.
 * A group's candidates are held in LDS up to 16 384 of them and streamed through the 4 096-key array beyond (or under
 * gram_debug_set_beam_chunked(1) / gram_debug_set_beam_chunk_capacity): the same results bit for bit. */
int gram_beam_step_groups_sparse(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                                 const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                                 int rows_per_user, const int32_t* rowpos, int pieces, int num_groups, float diversity_penalty,
                                 const gram_user_items_t* items_host, void* stream);
/* generate(num_beam_groups = num_groups, diversity_penalty): gram_generate_ex's arguments, workspace (gram_workspace_bytes) and
 * launch train -- encoder, bank, the shared step-0 row, the live-row compaction -- with gram_beam_init_groups and the group step in
 * the search's place; the tail pass is not taken.  items_host: per-user item filters (as gram_generate_items) or NULL.
 * sequences_scores include the accumulated penalties, as in HF; two groups can return the same sequence.  K >= 2. */
int gram_generate_groups(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                         int max_length, float length_penalty, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                         int num_groups, float diversity_penalty, const gram_user_items_t* items_host, void* workspace,
                         int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream);

/* ---- Beam search with per-item score biases: generate(item_bias=) -------------------------------------------------
 * Every item carries a bias T[r][item], r = 0 (one row shared by all users) or the user.  The biases are pushed up the Trie as
 * POTENTIALS phi f32 [rows][n_nodes]: a leaf's potential is its item's bias, an internal node's the largest potential below it
 * (lookahead) or 0, the root's and the start node's 0.  The candidate that moves beam k from its node p along a Trie edge to child c
 * then scores, fp32 with one rounding per operation,
 *     s = (logit - lse) + (phi[r][c] - phi[r][p]);   s = s + beam_scores[k]
 * and everything else is the plain search on these scores.  Along a path the edge terms telescope: a finished item's sum is its
 * sum of log-probabilities + T[r][item].
 *
 * gram_item_bias_table: the potentials, one launch.  bias f32: row r at bias + r * bias_stride, n_items entries (rows == 1: the
 * stride is not read); leaf_item i32 [n_leaves]: the candidate that names the leaf of every leaf rank (a value outside [0, n_items):
 * the leaf carries no bias); leaf_lo / leaf_hi i32 [n_nodes]: the leaf-rank range below every node (gram_user_items_t's tables);
 * start_token: the root's child under it is the start node; lookahead != 0: internal nodes take the max, else 0.  Writes
 * phi[rows][trie->n_nodes].  The max is taken over a total order of the floats (-0 below +0): the same bits in any order. */
int gram_item_bias_table(const float* bias, int64_t bias_stride, int rows, int n_items, const int32_t* leaf_item, int n_leaves,
                         const int32_t* leaf_lo, const int32_t* leaf_hi, const gram_trie_t* trie_host, int start_token, int lookahead,
                         float* phi, void* stream);
/* One biased step on dense logits f32 [B * rows_per_user][V] (as gram_beam_step; for tests on given logits).  phi_stride: elements
 * between the rows of two users, >= n_nodes, or 0: one row shared by all users.  items_host: per-user item filters or NULL. */
int gram_beam_step_bias(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const float* logits, const float* lse, int V,
                        int cur_len, int rows_per_user, const float* phi, int64_t phi_stride, const gram_user_items_t* items_host,
                        void* stream);
/* One biased step on hidden states (the sparse logits of gram_beam_step_sparse).  lm_head_bf16 / lm_head_f32 / pieces as in
 * gram_beam_step_groups_sparse; rowpos as in gram_beam_step_sparse_live (NULL: rows in place); items_host: per-user item filters
 * or NULL.  The one-shot and the chunked form are chosen as for gram_beam_step_sparse and return the same bits. */
int gram_beam_step_bias_sparse(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                               const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                               int rows_per_user, const int32_t* rowpos, int pieces, const float* phi, int64_t phi_stride,
                               const gram_user_items_t* items_host, void* stream);
/* generate(item_bias=): gram_generate_ex's arguments, workspace (gram_workspace_bytes) and step-wise launch train -- encoder, bank,
 * the shared step-0 row, the live-row compaction -- with the biased step in the search step's place; the tail pass is not taken.
 * phi / phi_stride: the caller's potentials (gram_item_bias_table), read by every step.  items_host: per-user item filters (as
 * gram_generate_items) or NULL; the potentials are over the shared Trie and ignore them.  K >= 2. */
int gram_generate_bias(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                       int max_length, float length_penalty, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                       const float* phi, int64_t phi_stride, const gram_user_items_t* items_host, void* workspace,
                       int64_t workspace_bytes, int64_t* sequences, float* scores, int32_t* width_host, void* stream);

/* ---- Trie-constrained sampling: HF 4.26 `sample` restated for a Trie ------------------------------------------------
 * The state is a gram_beam_state_t with K = R samples per user; nothing is ever reordered, so anc keeps the identity gram_beam_init
 * wrote (except slot 0 at the compact step 0, below).  Sampling leaves the hypothesis heap unused and keeps its per-row "finished"
 * there: hyp_len[row] (row < B * R) = the length at which the row drew EOS, 0 = still running; the caller zeroes hyp_len[0, B * R)
 * before the first step.  done / n_hyps / beam_scores are not touched.
 * One step, for every row at Trie node n with children c_0 < ... < c_{F-1} in token order (with the lists: the alive ones only):
 *   z_i = hidden[row] . lm_head[c_i] (fp32; the search step's sparse logit: the same function, the same bits), y_i = z_i / temperature;
 *   top_k (0 = off): k' = min(max(top_k, 1), F), child i is kept iff y_i >= the k'-th largest y (ties at the threshold all stay);
 *   top_p (< 1; over what top_k kept): w_i = exp(y_i - y_max), child i stays iff sum_{j kept, y_j <= y_i} w_j > (1 - top_p) * sum_kept w
 *     (the maximum always stays; equal y stay or go together);
 *   draw: W = sum of the kept w, the row takes the first kept child in token order whose running sum exceeds u * W (none, by rounding:
 *     the last kept child) -- inverse-CDF sampling;
 *   sample_logprob[row] += (y_i - y_max) - log W;  model_logprob[row] += z_i - lse[row].
 * A row that draws EOS is finished: from then on it emits pad, its node is -1 and its accumulators do not move.  Every sum is fp32 in
 * an order fixed by the row's own (alive) children, so a row's draw depends on its node, its hidden row, its u and the parameters
 * only -- not on B, R or the other rows.  A row without any child is error 1 (GRAM_E_BEAM), non-finite logits / lse error 4. */
struct gram_sample_params {
  float temperature; /* > 0                                   */
  int32_t top_k;     /* >= 0; 0 = off                          */
  float top_p;       /* in (0, 1]; 1 = off                     */
};
typedef struct gram_sample_params gram_sample_params_t; /* (layout against its ctypes mirror: tests/test_sample_host.py) */

/* One sampling step (cur_len = tokens already in each row).  hidden / lm_head_bf16 / lm_head_f32 / d / pieces as in
 * gram_beam_step_sparse (pieces == 1: lm_head_bf16) and gram_beam_step_sparse_split (pieces == 2, or lm_head_bf16 NULL: lm_head_f32).
 * rows_per_user = R normally; 1 at the compact step 0 (hidden and lse hold one row per user), which also sets anc[0][row] = user.
 * u: row r's uniform in [0, 1) at u[r * u_stride].  Writes tokens, node, seq[row][cur_len], hyp_len and the two accumulators
 * (f32 [B * R] each).  A row's candidates are held on chip up to 8 192 of them (32 KB of LDS: four workgroups per CU); a Trie with
 * max_fanout above that streams them through st->cand_logits, which must then hold f32 [B * R][cand_logits_stride >= max_fanout]
 * (cand_logits_users >= B * R; GRAM_E_ARG otherwise) -- the same results bit for bit. */
int gram_sample_step(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16, const void* lm_head_bf16,
                     const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                     const gram_sample_params_t* params_host, const float* u, int u_stride, float* sample_logprob,
                     float* model_logprob, void* stream);
/* gram_sample_step with per-user item filters: a row's children are those alive for its user (gram_user_items_t). */
int gram_sample_step_items(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                           const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                           int rows_per_user, int pieces, const gram_sample_params_t* params_host, const float* u, int u_stride,
                           float* sample_logprob, float* model_logprob, const gram_user_items_t* items_host, void* stream);
/* sequences i64 [B * R][max_length] (pad behind a finished row), the two accumulators copied to seq_logprobs / sample_logprobs
 * f32 [B * R] (a non-finite one is error 4), *out_width (device) = 1 + the longest row capped at max_length, as gram_greedy_finalize. */
int gram_sample_finalize(const gram_beam_state_t* st_host, int max_length, const float* model_logprob, const float* sample_logprob,
                         int64_t* sequences, float* seq_logprobs, float* sample_logprobs, int32_t* out_width, void* stream);
/* Candidates of a row the sampling step holds on chip (8 192, or what gram_debug_set_sample_capacity lowered it to). */
int gram_sample_capacity(void);
/* TEST hook: lowers that capacity (0 = the default), so that the streamed form is reachable at small fan-outs.  Results do not
 * depend on it.  Process-wide. */
int gram_debug_set_sample_capacity(int candidates);

/* Bytes of scratch gram_sample needs: gram_workspace_bytes(m, B, N, L, R, max_length) -- the layout is unchanged -- plus, behind it,
 * the two accumulators and, where max_fanout exceeds gram_sample_capacity(), the streamed candidates [B * R][max_fanout]. */
int64_t gram_workspace_bytes_sample(const gram_model_t* m, int B, int N, int L, int R, int max_length, int max_fanout);

/* generate(do_sample=True, num_beams=1, num_return_sequences=R): encoder -> late fusion -> bank (shared by a user's R samples as by
 * K beams) -> max_length - 1 steps of decoder + gram_sample_step (step 0 on one decoder row per user) -> gram_sample_finalize.
 * uniforms f32 [B][R][max_length - 1] (device): row (b, r) consumes uniforms[b][r][t] at step t.  sequences i64 [B * R][max_length],
 * seq_logprobs (the model's full-vocabulary log-probability of each row, what gram_teacher_forced sums) and sample_logprobs (under the
 * distribution drawn from) f32 [B * R]; width_host as in gram_generate.  Finished rows keep being decoded. */
int gram_sample(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
                const gram_trie_t* trie_host, const gram_compaction_t* compaction_host, const gram_sample_params_t* params_host,
                const float* uniforms, void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
                float* sample_logprobs, int32_t* width_host, void* stream);
/* gram_sample with per-user item filters (as gram_generate_items). */
int gram_sample_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
                      const gram_trie_t* trie_host, const gram_compaction_t* compaction_host, const gram_user_items_t* items_host,
                      const gram_sample_params_t* params_host, const float* uniforms, void* workspace, int64_t workspace_bytes,
                      int64_t* sequences, float* seq_logprobs, float* sample_logprobs, int32_t* width_host, void* stream);

/* ---- Sampling without replacement: stochastic beam search (Kool, van Hoof, Welling, ICML 2019) on a Trie ------------
 * R DISTINCT items per user, in the order of sampling without replacement (Plackett-Luce) from the distribution gram_sample draws from
 * with top_k and top_p off: p(child) = softmax over the row's (alive) children of y = z / temperature.  The state is a
 * gram_beam_state_t with K = R rows per user; rows ARE reordered, as in beam search.  Per row, beside the state's own arrays:
 *   beam_scores[row]  G, the perturbed score (-inf: a dead row);      hyp_len[row] (row < B * R) > 0: finished at that length;
 *   sample_logprob    phi, the log-probability of the prefix under that distribution;      model_logprob   sum of z - lse[row];
 *   path              a 64-bit word that names the prefix to the random number generator.
 * Uniforms are Philox4x32-10 words with key (seed low word, seed high word): root w = philox(user_key low, user_key high, 0, 0),
 * path = (w0, w1), u = ((w2 >> 8) + 0.5) 2^-24, phi = 0, G = -log(-log u); the child with token tok chosen at the step that writes
 * position cur_len: w = philox(path low, path high, tok, cur_len), path = (w0, w1), u from w2.  So a draw depends on (seed, user key,
 * token prefix) only.  One step, for every live row (G = T) over its alive children in token order, fp32:
 *   lse_k = log sum exp y;  phi_c = phi + (y_c - lse_k);  G~_c = phi_c - log(-log u_c);  Z = max_c G~_c;
 *   v = (T - G~_c) + log1p(-exp(G~_c - Z));  G_c = (T - max(0, v)) - log1p(exp(-|v|)), and G_c = T exactly where G~_c = Z.
 * A finished row is one candidate, itself; a dead row none.  The R candidates with the largest G become the new rows in descending
 * order of G (ties: the lower row * V + token); sequences, ancestors, node and the four words move with them; a row that takes EOS is
 * finished; fewer than R candidates leave dead rows (no error).  The sum's order is fixed by a row's own alive children (sbs.hip), so
 * a user's rows do not depend on B, on the other users or on where the candidates are held, and the rows of R' < R are the first R'
 * rows of R.  Non-finite logits, lse or scores are error 4. */
/* gram_beam_init, then the root words: row 0 of every user live, the others dead.  user_keys i64 [B] (device). */
int gram_sbs_init(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, int start_token, uint64_t seed,
                  const int64_t* user_keys, float* sample_logprob, float* model_logprob, uint64_t* path, void* stream);
/* One step (cur_len = tokens already in each row); operands as gram_sample_step.  rows_per_user = R, or 1 at step 0 (hidden and lse
 * hold one row per user).  A user's candidates are held on chip up to 4 096 of them; where R * max_fanout exceeds
 * gram_sbs_capacity() st->cand_logits must hold f32 [B * R][cand_logits_stride >= 2 * max_fanout] (GRAM_E_ARG otherwise) -- the same
 * results bit for bit. */
int gram_sbs_step(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16, const void* lm_head_bf16,
                  const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                  float temperature, uint64_t seed, float* sample_logprob, float* model_logprob, uint64_t* path, void* stream);
/* gram_sbs_step with per-user item filters: bit for bit the unfiltered step on the Trie of the user's alive items. */
int gram_sbs_step_items(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const void* hidden_bf16,
                        const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                        int rows_per_user, int pieces, float temperature, uint64_t seed, float* sample_logprob, float* model_logprob,
                        uint64_t* path, const gram_user_items_t* items_host, void* stream);
/* sequences i64 [B * R][max_length], seq_logprobs (model), sample_logprobs (phi), perturbed_scores (G) f32 [B * R]; a dead row is the
 * start token followed by pad with -inf in all three; NaN / +inf anywhere is error 4; *out_width as gram_sample_finalize. */
int gram_sbs_finalize(const gram_beam_state_t* st_host, int max_length, const float* model_logprob, const float* sample_logprob,
                      int64_t* sequences, float* seq_logprobs, float* sample_logprobs, float* perturbed_scores, int32_t* out_width,
                      void* stream);
/* Candidates of a user the step holds on chip (4 096, or what gram_debug_set_sbs_capacity lowered it to). */
int gram_sbs_capacity(void);
/* TEST hook: lowers that capacity (0 = the default).  Results do not depend on it.  Process-wide. */
int gram_debug_set_sbs_capacity(int candidates);
/* Bytes of scratch gram_generate_sbs needs: gram_workspace_bytes(m, B, N, L, R, max_length) plus, behind it, the three per-row arrays
 * and, where R * max_fanout exceeds gram_sbs_capacity(), the streamed candidates [B * R][2 * max_fanout]. */
int64_t gram_workspace_bytes_sbs(const gram_model_t* m, int B, int N, int L, int R, int max_length, int max_fanout);
/* generate(do_sample=True, replacement=False, num_return_sequences=R): gram_sample's launch train with gram_sbs_init / gram_sbs_step /
 * gram_sbs_finalize in the sampling step's place (step 0 on one decoder row per user; finished and dead rows keep being decoded). */
int gram_generate_sbs(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R, int max_length,
                      const gram_trie_t* trie_host, const gram_compaction_t* compaction_host, float temperature, uint64_t seed,
                      const int64_t* user_keys, void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs,
                      float* sample_logprobs, float* perturbed_scores, int32_t* width_host, void* stream);
/* gram_generate_sbs with per-user item filters (as gram_generate_items). */
int gram_generate_sbs_items(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int R,
                            int max_length, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                            const gram_user_items_t* items_host, float temperature, uint64_t seed, const int64_t* user_keys,
                            void* workspace, int64_t workspace_bytes, int64_t* sequences, float* seq_logprobs, float* sample_logprobs,
                            float* perturbed_scores, int32_t* width_host, void* stream);

/* ---- the tail pass: the chain-like lower levels of the Trie decoded in one pass per user forest ---------------------
 * Once a user's beams stand on prefixes of length d_tail (start token counted), every decoder state the remaining search steps can
 * ask for belongs to a known forest: the beams' nodes and their descendants that have children.  gram_generate_tail builds that
 * forest on the device after the search step that reaches d_tail (gram_tail_forest), runs the decoder ONCE over its rows -- the
 * cross-attention reads a user's bank once per 64 forest rows instead of once per step -- and replays the remaining search steps on
 * the stored hidden states (gram_tail_rowpos maps each beam to its forest row; no decoder launch in between).  Sequences, scores
 * and the beam state after every step are gram_generate_ex's bit for bit: every kernel of the pass is row-independent, the
 * self-attention is the step-wise kernel (level by level) or the forest kernel, which calls the same row arithmetic
 * (gram_dec_self_attn_forest_split), and the cross-attention is the step-wise kernel's template. */
#define GRAM_TAIL_MAX_STEPS 16  /* decode steps one pass replaces at most (a forest row walks that many parents at most) */
#define GRAM_TAIL_ENTRY_ROWS 64 /* forest rows of one cross-attention entry: the four 16-row tiles of the entry kernel        */
typedef struct {
  const int32_t* sub_rows; /* device, i32 [n_nodes]: decoder rows of node n's subtree = n and its descendants that have children;
                              0 for a leaf (FlatTrie.tail_tables)                                                              */
  int32_t d_tail;          /* switch depth: the pass starts when the beams hold d_tail tokens; 0 = this Trie has no tail       */
  int32_t steps;           /* decode steps left from there: (depth of the deepest node with children) - d_tail + 1             */
} gram_trie_tail_t;
/* The forest of one call (device arrays, carved from the workspace by gram_generate_tail).  Rows are user-major; inside a user
 * depth-major: the live beams in beam order, then level by level the children that have children, parents in row order, children
 * in token order. */
typedef struct {
  int32_t* tokens;    /* [cap_rows]  decoder input token of the row                                                  */
  int32_t* pos;       /* [cap_rows]  decoder position of the row                                                     */
  int32_t* parent;    /* [cap_rows]  forest row of the parent prefix, -1 for a beam's own row                        */
  int32_t* root;      /* [cap_rows]  beam row b * K + k whose subtree the row belongs to (its cache and anc column)  */
  int32_t* node;      /* [cap_rows]  Trie node of the row's prefix                                                   */
  int32_t* user_off;  /* [B + 1]     rows of user b: [user_off[b], user_off[b + 1])                                  */
  int32_t* ent_off;   /* [B + 1]     cross-attention entries of user b (one per 64 rows)                             */
  int32_t* ent_users; /* [cap_entries]       user of each entry                                                      */
  int32_t* ent_rows;  /* [cap_entries][64]   forest rows of each entry, -1 = none                                    */
  int32_t* rowpos;    /* [B * K]     forest row of each beam in the coming search step, -1 = the beam is not live    */
  int32_t* counts;    /* [4 + 2 * GRAM_TAIL_MAX_STEPS]  rows, entries, most rows of one user, 0, then the rows of every level of
                         the even users [GRAM_TAIL_MAX_STEPS] and of the odd users [GRAM_TAIL_MAX_STEPS]                 */
  /* Small forests (gram_debug_set_tail_forest_attn; large ones read pos / parent / root above, gram_dec_self_attn_forest_split):
   * the self-attention of the pass is the step-wise kernel, run level by level: level l (position t + l) takes its rows gathered
   * by SLOT -- a row's index among the rows of its level, which is also the cache row the kernel writes its k and v to -- and an
   * ancestor table of its own: column s holds, for positions < t, what the beam's column of gram_beam_state_t.anc holds, and from
   * t on the slots of the row's ancestors in the forest.  A level of the forest may hold more rows than the cache has per position
   * (B * K): the users go in two groups, even and odd, each with its own slots and tables, run one after the other.  (Slots are
   * handed out per user and level in the order the users' threads arrive: they differ from run to run, the results do not.) */
  int32_t* slot;       /* [cap_rows]                slot of the row at its level, within its user's group               */
  int32_t* lvl_rows;   /* [2][n_levels][cap_rows]   forest row of every slot                                            */
  int32_t* lvl_tokens; /* [2][n_levels][cap_rows]   its token (layer 0 reads the token table by it)                     */
  int32_t* lvl_anc;    /* [2][n_levels][Tmax][B*K]  the ancestor tables                                                 */
  int32_t cap_rows, cap_entries, n_levels, pad_;
} gram_forest_t;
/* counts and offsets (one workgroup), the rows, slots and entries (one thread per user), the ancestor tables (one thread per row).
 * A forest of more than cap_rows rows or cap_entries entries writes its counts only: the caller reads them and goes on step by
 * step (as it does when a group's level holds more than B * K rows: a level's slots are cache rows).  t = position of the beams' rows.
 * A user holds the rows tail->sub_rows promises for its live beams (at most cap_rows + 1 are counted per user).  A table that
 * promises more rows than the Trie holds below those beams sets st->error[0] = 3 -- a soft flag, as every beam-state error -- and
 * the rows promised and not found become harmless copies of a start row behind the user's real rows: pad token, pos t, parent -1,
 * root b * K, node -1, slots of level 0 like any row's; no beam's gram_tail_rowpos points at one.
 * What is written: counts [4 + 2 * GRAM_TAIL_MAX_STEPS], user_off and ent_off [B + 1] always; for a forest that fits, the row arrays
 * and slot [counts[0]], ent_users and ent_rows [counts[1]], per (group, level < n_levels) the first counts[4 + ...] cells of lvl_rows
 * and lvl_tokens, and of lvl_anc the columns of the slots < B * K: the positions < t and those of the row's ancestors (< Tmax), not
 * the row's own.  A row at level >= n_levels gets slot -1 and no table cell.  rowpos is gram_tail_rowpos's.  Nothing else is touched. */
int gram_tail_forest(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const gram_trie_tail_t* tail_host,
                     const gram_forest_t* forest_host, int t, void* stream);
/* forest.rowpos for the coming search step: the forest row whose node is the beam's (the first of its user's rows), -1 for a beam
 * that is not live.  A live beam whose node none of its user's rows holds sets st->error[0] = 3 and gets row 0. */
int gram_tail_rowpos(const gram_beam_state_t* st_host, const gram_trie_t* trie_host, const gram_forest_t* forest_host, void* stream);
/* dst row rows[i] = src row i, for i < n: rows of row_bytes bytes (a multiple of 16); an index outside [0, dst_rows) is skipped.  The
 * tail pass runs its self-attention level by level with the step-wise kernel, on the level's rows gathered by slot, and puts the
 * results back with this. */
int gram_scatter_rows(const void* src, const int32_t* rows, void* dst, int n, int row_bytes, int dst_rows, void* stream);
/* The self-attention of the tail pass in one launch over all n_rows forest rows (forest_attn.hip): row i at position p = pos[i],
 * t0 <= p < min(t0 + nlev, Tmax), attends in position order the cache rows (j, anc[j * R + root[i]]) of the positions j < t0
 * (anc: gram_beam_state_t.anc; root clamped to [0, R)), then the k and v columns of the q|k|v rows of its ancestors at the positions
 * t0 .. p - 1 -- parent[] walked from i, every index clamped to [0, n_rows) -- then its own, and writes row i of out.  qkv and
 * qkv_rows as gram_dec_self_attn_rows_split's: the pass's q|k|v buffer [n_rows][3 * inner] (qkv_rows NULL), or a per-token table
 * and the forest's tokens.  A row at any other position is left alone, rows >= n_rows too, and the cache is only read.  A row's bits
 * are those of the level-by-level train of gram_dec_self_attn_rows_split + gram_scatter_rows over gram_tail_forest's tables: both
 * kernels call the one row arithmetic of self_attn_row.h on the same pieces in the same order. */
int gram_dec_self_attn_forest_split(const void* qkv, const int32_t* qkv_rows, const void* kcache, const void* vcache, const int32_t* anc,
                                    const int32_t* pos, const int32_t* parent, const int32_t* root, const float* bias, void* out,
                                    int n_rows, int R, int H, int t0, int Tmax, int nlev, int pieces, int64_t qkv_pstride,
                                    int64_t cache_pstride, void* stream);
/* gram_cross_attn_decode_split's live-row form over entries: workgroup row e serves user ent_users[e] and the up to 64 rows
 * ent_rows[e * 64 ..] of q / out (-1: none).  K is the beam count of the search whose bits are restated (it selects the one- or
 * two-wave split of the keys, as gram_cross_attn_decode_split does): a row gets the bits that call gives it. */
int gram_cross_attn_entries_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                  int n_entries, int K, int H, int S, const int32_t* ent_users, const int32_t* ent_rows, int pieces,
                                  int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, void* stream);
/* Workspace of gram_generate_tail: gram_workspace_bytes plus the forest's decoder rows and tables, carved BEHIND it (nothing of
 * gram_workspace_bytes's layout moves).  Capacity: 5/4 * B * K * steps rows (a forest of the average Beauty node holds 1.04 rows
 * per replaced step and beam), about 38 KB per row at T5-base in the two-piece mode. */
int64_t gram_workspace_bytes_tail(const gram_model_t* m, int B, int N, int L, int K, int max_length, int steps);
/* gram_generate_ex with the tail pass.  tail_host NULL, d_tail 0, K = 1, a handle with a raised fused limit, a call for which
 * gram_tail_pass_wanted says 0 or a forest over capacity: exactly gram_generate_ex's launches.  Otherwise workspace_bytes must be
 * gram_workspace_bytes_tail's. */
int gram_generate_tail(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L, int K, int nret,
                       int max_length, float length_penalty, const gram_trie_t* trie_host, const gram_compaction_t* compaction_host,
                       const gram_trie_tail_t* tail_host, void* workspace, int64_t workspace_bytes, int64_t* sequences,
                       float* scores, int32_t* width_host, void* stream);

/* The encoder layers alone on P independent passages (T5Stack encoder role, gram_t5_modeling.py:1037-1296, up to
 * but excluding final_layer_norm): x_out f32 [P][L][d_model] is the residual stream the final norm, the position
 * embedding and the bank projection consume.  ids i64 [P][L], mask u8 [P][L].  Workspace as for
 * gram_workspace_bytes(m, P, 1, L, 1, 2).  Feeds gram_compaction_t.cache_x. */
int gram_encode_passages(const gram_model_t* m, const int64_t* ids, const uint8_t* mask, int P, int L,
                         void* workspace, int64_t workspace_bytes, float* x_out, void* stream);
/* Byte offset, inside a workspace carved for (B, N, L, K, max_length), of the encoder's fp32 residual stream [passages * L][d_model]
 * (before final_layer_norm) as the last gram_generate[_ex] / gram_encode_fused on that workspace left it: rows [p*L, (p+1)*L) belong to
 * compact passage p (the order of gram_compaction_t.ids; b*N + n without a compaction).  It is what gram_encode_passages copies out,
 * so a caller can add the passages a generate() has just encoded to its passage cache (gram_compaction_t.cache_x) without encoding
 * them a second time.  < 0: GRAM_E_ARG. */
int64_t gram_workspace_encoder_x_offset(const gram_model_t* m, int B, int N, int L, int K, int max_length);
/* x[i][l][:] = l < cache_L ? cache_x[slot[i]][l][:] : 0 for i < n, l < L (d % 4 == 0). */
int gram_gather_passage_x(const float* cache_x, const int32_t* slot, float* x, int n, int L, int cache_L, int d,
                          void* stream);

/* ---- teacher-forced decoder pass (forward(labels) loss, sequence scores) ---------------------------------------------------
 * T5ForConditionalGeneration_GRAM.forward with labels (gram_t5.py:181-263, reached through GRAM.forward gram.py:50-60): the decoder
 * runs once over whole sequences -- decoder_input_ids = _shift_right(labels) (gram_t5_modeling.py:935-964), causal self-attention
 * only (no decoder mask), cross-attention over the late-fused encoder states, final norm with the tied-embedding scale, lm_head --
 * instead of one token per step.  The reference's CrossEntropyLoss(ignore_index=-100) (gram_t5.py:256-260) and a candidate's
 * log p(item | user) are sums of the per-token log-probs returned here.
 * Rows are user-major (b, c, t): B users x C sequences per user x T positions, R = B * C * T. */

/* Bytes of scratch gram_teacher_forced needs for this problem size; < 0: GRAM_E_ARG. */
int64_t gram_workspace_bytes_tf(const gram_model_t* m, int B, int N, int L, int C, int T);

/* The encoder as gram_generate_ex runs it (compaction_host as there: ragged batches and the passage cache; NULL = every passage),
 * then the decoder over the R rows.  dec_ids i32 [R] (decoder input tokens, in [0, vocab)), labels i32 [R] (< vocab; < 0 = ignored:
 * token_logp 0, not counted in seq_logp).  logits f32 [R][vocab] or NULL (not materialised); token_logp f32 [R] = log_softmax(logits)
 * [label]; seq_logp f32 [B * C] = the sum of a sequence's token_logp in position order.  T <= GRAM_MAX_DEC_LEN, C >= 1; shapes are
 * checked before any launch (GRAM_E_ARG). */
int gram_teacher_forced(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                        const gram_compaction_t* compaction_host, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                        void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp, void* stream);

/* Causal self-attention of n_seq decoder sequences of T <= 64 positions, every position at once (T5Attention.forward self branch,
 * unidirectional relative bias of layer 0 and causal mask, gram_t5_modeling.py:586-593).  qkv: planar pieces [n_seq * T][3 * inner]
 * (row = seq * T + t), qkv_pstride elements apart; bias f32 [H][GRAM_MAX_DEC_LEN] by distance; out as gram_dec_self_attn_split's
 * (interleaved [rows][2 * inner] when pieces = 2). */
int gram_dec_self_attn_tf_split(const void* qkv, const float* bias, void* out, int n_seq, int T, int H, int pieces,
                                int64_t qkv_pstride, void* stream);

/* Cross-attention of Q query rows per user (row = b * Q + i) over that user's bank (gram_cross_attn_decode_split's arguments with
 * K = Q).  Q <= GRAM_MAX_BEAMS is one gram_cross_attn_decode_split call; above, one call per group of <= GRAM_MAX_BEAMS rows, which
 * needs rowmap: device scratch i32 [B * (1 + 2 * GRAM_MAX_BEAMS)] (may be NULL when Q <= GRAM_MAX_BEAMS). */
int gram_cross_attn_rows_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out, int B, int Q,
                               int H, int S, int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits,
                               int32_t* rowmap, void* stream);
/* The same over up to 16 384 fused keys: gram_cross_attn_long_split with K = Q for Q <= GRAM_MAX_BEAMS, one live-row call of it per
 * group of <= GRAM_MAX_BEAMS rows above (same bits as those calls made by hand).  key_bits: gram_mask_key_bits_long; scratch:
 * gram_cross_attn_long_scratch_bytes(B * min(Q, GRAM_MAX_BEAMS), H, S) bytes, reused by every group; rowmap as above.  GRAM_E_ARG
 * before any launch: gram_cross_attn_long_split's cases, a NULL rowmap for Q > GRAM_MAX_BEAMS, or (two pieces) q_pstride < B*Q*H*64. */
int gram_cross_attn_rows_long_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out, int B,
                                    int Q, int H, int S, int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits,
                                    float* scratch, int32_t* rowmap, void* stream);

/* Label log-probs from the final hidden rows: token_logp[r] = hidden[r] . E[labels[r]] - lse[r] for labels[r] >= 0 (0 otherwise),
 * the dot product being gram_beam_step_sparse_split's (E = lm_head_f32 when pieces = 2, lm_head_bf16 when 1), lse from
 * gram_gemm_bf16_lse_split + gram_lse_combine; seq_logp[s] = sum over t of token_logp[s * T + t] with labels >= 0, in position
 * order (deterministic: no atomics).  hidden as the lm_head GEMM's A operand ([R][pieces * d], interleaved when pieces = 2). */
int gram_label_logprob_split(const void* hidden, const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse,
                             const int32_t* labels, int n_seq, int T, int V, int pieces, float* token_logp, float* seq_logp,
                             void* stream);

/* ---- cross-attention probabilities and per-passage scores (GRAM.get_crossattention_scores) ---------------------------------
 * HF's `cross_attentions` (T5Attention.forward's attn_weights, gram_t5_modeling.py:600-603,629) and the reference's reduction of
 * them to one score per passage (src/model/gram.py:109-138), for the teacher-forced pass. */

/* probs f32 [B][H][Q][S]: probs[b][h][i][s] = softmax over s of (q[b*Q + i] . k[b][h][s] + (mask[b][s] ? 0 : finfo(float32).min)),
 * scores unscaled.  q, k_layer, mask, pieces, the strides and key_bits as gram_cross_attn_rows_split takes them (the same operand
 * pieces and product order as the cross-attention kernel), any Q >= 1, B <= 65535.  Masked keys of a user with a valid key are
 * exactly 0.0; a user without one gets 1 / S everywhere.  A row's bits depend on that row, its user's K and mask only.
 * S % 32 == 0, S <= 4096, pieces 1 or 2, pointers 16-byte aligned: otherwise GRAM_E_ARG before any launch. */
int gram_cross_attn_probs_split(const void* q, const void* k_layer, const uint8_t* mask, float* probs, int B, int Q, int H, int S,
                                int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, void* stream);

/* acc[b][i][s] = (first ? 0 : acc[b][i][s]) + the sum over h, in head order, of probs[b][h][i][s]; acc f32 [B][Q][S], S % 4 == 0. */
int gram_xattn_head_sum(const float* probs, float* acc, int B, int Q, int H, int S, int first, void* stream);

/* scores[b][i][n] = (sum over l with mask[b][n][l] != 0 of acc[b][i][n*L + l]) / (count(b, n) * denom), count = the passage's valid
 * keys; NaN when count == 0 (the reference's 0 / 0).  mask u8 [B][N][L], scores f32 [B][Q][N]; fixed summation order. */
int gram_xattn_passage_scores(const float* acc, const uint8_t* mask, float* scores, int B, int Q, int N, int L, float denom,
                              void* stream);

/* Attention outputs of gram_teacher_forced_ex, all caller-owned device memory (Q = C * T rows per user, S = N * L keys). */
typedef struct {
  float* probs;          /* [n_dec_layers][B][H][Q][S]: every layer's probabilities, or NULL                            */
  float* layer_probs;    /* [B][H][Q][S]: scratch for one layer; required when probs == NULL                             */
  float* token_scores;   /* [B][Q][S]: the sum over layers and heads, or NULL                                            */
  float* passage_scores; /* [B][Q][N]: gram_xattn_passage_scores of token_scores, denom = n_dec_layers * H; or NULL      */
} gram_xattn_out_t;

/* gram_teacher_forced with the cross-attention probabilities of the pass.  attn_host == NULL: gram_teacher_forced itself (which is
 * this call).  Otherwise every decoder layer's cross-attention is followed by gram_cross_attn_probs_split on the same queries and
 * K bank and, with token_scores, gram_xattn_head_sum; gram_xattn_passage_scores follows the last layer.  The workspace and every
 * other output are those of gram_teacher_forced.  probs and layer_probs both NULL, or passage_scores without token_scores:
 * GRAM_E_ARG before any launch. */
int gram_teacher_forced_ex(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                           const gram_compaction_t* compaction_host, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                           void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp,
                           const gram_xattn_out_t* attn_host, void* stream);

/* The token scores without the per-head tensor, over up to GRAM_MAX_LONG_FUSED_LEN fused keys:
 *   acc[b][i][s] = (first ? 0 : acc[b][i][s]) + the sum over h, in head order, of softmax_s(q[b*Q + i] . k[b][h][s] + masked)[s],
 * acc f32 [B][Q][S]: gram_cross_attn_probs_split's probabilities (the same operands, product order and online normaliser) summed over
 * the heads on chip -- what gram_cross_attn_probs_split + gram_xattn_head_sum leave in acc, with nothing of size H * Q * S in
 * between.  key_bits is required: gram_mask_key_bits_long of the same mask and S (the mask bytes are not read).  S % 32 == 0,
 * 32 <= S <= GRAM_MAX_LONG_FUSED_LEN, Q >= 1, H <= 16, B <= 65535, pieces 1 or 2.  No atomics, one fixed order for every sum: a row's
 * valid keys depend on that row, the user's valid 32-key steps in key order (each with its word of bits), `first` and the old value
 * only -- not on B, Q, the user's place in the batch or where the fully masked steps lie.  Fully masked steps are not fetched: with
 * `first` their keys are written as 0.0, otherwise left alone; masked keys of a valid step add exactly 0.0 whatever the bank holds; a
 * user without a valid key gets H / S everywhere.  GRAM_E_ARG before any launch: a NULL or not 16-byte aligned q, k_layer, acc or
 * key_bits, a size out of range, (two pieces) q_pstride < B*Q*H*64 or bank_pstride < H*S*64, more than 65535 tiles of 32 rows. */
int gram_cross_attn_token_scores_split(const void* q, const void* k_layer, float* acc, int B, int Q, int H, int S, int pieces,
                                       int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, int first, void* stream);

/* Score outputs of gram_teacher_forced_scores, caller-owned device memory (Q = C * T rows per user, S = N * L keys). */
typedef struct {
  float* token_scores;   /* [B][Q][S]: sum over decoder layers and heads; required                                       */
  float* passage_scores; /* [B][Q][N]: gram_xattn_passage_scores of it, denom = n_dec_layers * H; or NULL                */
} gram_xattn_scores_t;

/* gram_teacher_forced with the token (and passage) scores of the pass at every S the handle takes, without a per-head buffer: every
 * decoder layer's cross-attention is followed by gram_cross_attn_token_scores_split on the same queries and K bank (first = layer 0);
 * gram_xattn_passage_scores follows the last layer.  Needs a handle raised by gram_model_set_max_fused_len (its workspace holds the
 * long key bits): a default handle, scores_host == NULL, a NULL or not 16-byte aligned token_scores, more than 16 heads, B > 65535 or
 * more than 65535 tiles of 32 rows get GRAM_E_ARG before any launch.
 * The workspace and every other output are those of gram_teacher_forced. */
int gram_teacher_forced_scores(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                               const gram_compaction_t* compaction_host, const int32_t* dec_ids, const int32_t* labels, int C, int T,
                               void* workspace, int64_t workspace_bytes, float* logits, float* token_logp, float* seq_logp,
                               const gram_xattn_scores_t* scores_host, void* stream);

/* ---- every catalogue item in one decoder pass over the Trie (GRAM.score_all_items) -----------------------------------------
 * The teacher-forced pass above spends one decoder row per (candidate, position); two candidates that share an id prefix share every
 * decoder state along it (a teacher-forced row depends on its prefix only: gram_t5.py:181-263 with the causal self-attention of
 * gram_t5_modeling.py:586-593).  Here the rows of a user are the INTERNAL NODES of the flat Trie below the root -- one per distinct
 * proper prefix -- each attending to its ancestors, and a leaf's log p(item | user) is the sum of the edge terms along its path.
 * Rows are user-major (b, i): B users x Q rows, R = B * Q. */

/* The row tables of a Trie (gram_amd.utils.generation_trie.FlatTrie.decoder_rows), device pointers.  Row order follows node order, so
 * every depth is contiguous; row 0 is the root's only child, the decoder start token. */
typedef struct {
  const int32_t* tokens;    /* [Q]       decoder input of the row: its node's own token                                        */
  const int32_t* pos;       /* [Q]       position t of the row = depth of its node - 1                                         */
  const int32_t* anc;       /* [Q][Tq]   row of the ancestor at every position j <= pos[i]; anc[i][pos[i]] = i; rest unused    */
  const int32_t* row_node;  /* [Q]       Trie node of the row                                                                  */
  const int32_t* node_row;  /* [n_nodes] row of the node's PARENT (the row that predicts the node); -1: the root and row 0's   */
  const int32_t* node_tok;  /* [n_nodes] token on the edge into the node                                                       */
  const int32_t* node_leaf; /* [n_nodes] leaf rank (FlatTrie.leaf_ranges) of a leaf, -1 elsewhere                              */
  int32_t Q, Tq;            /* rows; Tq = max pos + 1 <= GRAM_MAX_DEC_LEN                                                      */
  int32_t n_nodes, n_leaves;
} gram_trie_rows_t;

/* Causal self-attention of Q rows per user where row i (global row b * Q + i) attends to the rows anc[i][0 .. pos[i]] of the same
 * user (T5Attention.forward self branch with the causal mask, gram_t5_modeling.py:586-593, on the prefix row i stands for).  qkv:
 * planar pieces [B * Q][3 * inner], qkv_pstride elements apart; bias f32 [H][GRAM_MAX_DEC_LEN] by distance pos[i] - j; out as
 * gram_dec_self_attn_tf_split's (interleaved [rows][2 * inner] when pieces = 2).  The expression is gram_dec_self_attn_tf_split's: a
 * tree row and the same prefix there give the same bits.  pos / anc entries out of range are clamped, not followed.  A null pointer,
 * Tq outside 1..GRAM_MAX_DEC_LEN, H outside 1..16, pieces outside 1..2 or a piece stride shorter than the rows: GRAM_E_ARG before
 * any launch. */
int gram_dec_self_attn_tree_split(const void* qkv, const int32_t* pos, const int32_t* anc, const float* bias, void* out, int B, int Q,
                                  int Tq, int H, int pieces, int64_t qkv_pstride, void* stream);

/* out i32 [B * Q]: out[b * Q + i] = tokens[i], the decoder inputs of gram_score_trie's rows. */
int gram_trie_repeat_tokens(const int32_t* tokens, int32_t* out, int B, int Q, void* stream);

/* Item scores from the final hidden rows (the lm_head and log-softmax of gram_t5.py:181-263 at the Trie's tokens only).  For every edge (row i -> child node c with token tok):
 * term[b][c] = hidden[b * Q + i] . E[tok] - lse[b * Q + i], the dot product being gram_label_logprob_split's (E = lm_head_f32 when
 * pieces = 2, lm_head_bf16 when 1); leaf_logp[b][rank] = the sum of the terms along the leaf's path in position order, starting from
 * 0.f -- the sum gram_label_logprob_split and the beam's running score make (one writer per element, no atomics).  Two launches: the
 * terms of the edges into rows go to row_edge (device scratch f32 [B * Q]), then every leaf adds its own term to those of its path.
 * leaf_logp f32 [B][n_leaves] by leaf rank; node_logp f32 [B][n_nodes] or NULL: the term of the edge into every node (0 for the
 * root and row 0's node).  hidden and lse as gram_label_logprob_split takes them. */
int gram_trie_leaf_logprob_split(const void* hidden, const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse,
                                 const gram_trie_rows_t* rows_host, int B, int V, int pieces, float* row_edge, float* leaf_logp,
                                 float* node_logp, void* stream);

/* Bytes of scratch gram_score_trie needs: gram_workspace_bytes_tf's layout with R = B * Q rows (and the same shape checks with B * Q
 * in place of B * C * T), plus the repeated tokens and the edge terms, [B * Q] each.  < 0: GRAM_E_ARG. */
int64_t gram_workspace_bytes_trie(const gram_model_t* m, int B, int N, int L, int Q);

/* log p(item | user) of every leaf of the Trie -- T5ForConditionalGeneration_GRAM.forward with labels (gram_t5.py:181-263) for every
 * candidate at once, each shared prefix computed once: the encoder as gram_generate_ex runs it, the decoder layers over the B * Q rows of
 * rows_host (the decoder inputs are rows_host->tokens repeated per user by gram_trie_repeat_tokens: the caller passes no token
 * tensor) with gram_dec_self_attn_tree_split as the self-attention and gram_cross_attn_rows_split as the cross-attention, the lm_head
 * with its LSE partials (no logits), gram_lse_combine, gram_trie_leaf_logprob_split.  trie_host: the Trie the tables were built from
 * (its n_nodes must equal rows_host's).  leaf_logp f32 [B][n_leaves], node_logp f32 [B][n_nodes] or NULL.  Shapes and pointers are
 * checked before any launch (GRAM_E_ARG). */
int gram_score_trie(const gram_model_t* m, const int64_t* input_ids, const uint8_t* mask, int B, int N, int L,
                    const gram_compaction_t* compaction_host, const gram_trie_t* trie_host, const gram_trie_rows_t* rows_host,
                    void* workspace, int64_t workspace_bytes, float* leaf_logp, float* node_logp, void* stream);

/* ---- live per-kernel timing (bench.py) ------------------------------------------------ */
enum gram_kernel_kind {
  GRAM_K_GEMM = 0,          /* work = 2*M*N*K flops per launch                              */
  GRAM_K_ENC_ATTN = 1,      /* work = 4*P*H*L*L*64 flops                                   */
  GRAM_K_CROSS_ATTN = 2,    /* work = algorithmic HBM bytes: B*H*S*64*2(K,V)*2 B           */
  GRAM_K_DEC_SELF_ATTN = 3, /* work = bytes of cached K/V read                              */
  GRAM_K_ROWOPS = 4,        /* embed / rmsnorm: work = bytes moved                          */
  GRAM_K_LSE = 5,           /* work = R*V*4 bytes                                          */
  GRAM_K_BEAM = 6,          /* work = 0                                                    */
  GRAM_K_COUNT = 7
};
/* Record a HIP-event pair around every launch of the selected kinds, on the launch stream.
 * kind_mask = OR of (1 << kind); 0 disables and frees the pool.  Not thread-safe. */
int gram_prof_enable(uint32_t kind_mask, int max_events);
int gram_prof_reset(void);
/* Sum of event-measured durations (ms), launch count and summed `work` for one kind; waits for
 * the recorded events.  dropped = launches not recorded because the pool was full. */
int gram_prof_collect(int kind, double* total_ms, int64_t* launches, double* work, int64_t* dropped);

/* Diagnostic, OFF by default (the product path runs without it): on != 0 makes every workgroup of the persistent ping-pong GEMM stamp
 * s_memtime / s_memrealtime around its tile loop (two atomics per workgroup and launch) for gram_prof_pp_clock.  Not thread-safe. */
int gram_prof_pp_clock_enable(int on);
/* Time-weighted shader clock (GHz) the chip held inside the persistent ping-pong GEMM launches since the last reset (while enabled,
 * see above): every workgroup of those kernels adds its s_memtime / s_memrealtime differences around its tile loop to two device counters.  The MFMA peak a
 * power-limited chip can be priced against is 2.5 PFLOP/s x this / 2.4 (bench.py's roofline).  Synchronises the device; reset != 0
 * zeroes the counters after reading.  ghz may be NULL. */
int gram_prof_pp_clock(double* ghz, int reset);

/* Tuning hook: force a GEMM staging variant (0 = register-staged double buffer, 1 = LDS-DMA
 * single buffer, -1 = automatic per problem size).  Used by tests/bench_gemm.py.  1000 + s: start stagger of the persistent kernel.
 * 2000 + n (n <= 63; 2000 = off): TEST hook, honoured by the chaos build only (make CHAOS=1; the product kernels carry no test code) --
 * wave group 1 of the persistent ping-pong kernel enters its prologue n x 512 cycles late, which turns a round-4 race of that prologue
 * (fixed) into a deterministic test. */
int gram_debug_set_gemm_variant(int variant);

/* Calibration probe (bench.py): one streaming read of `bytes` (16-B aligned) through every CU; nothing is
 * written unless a 32-bit fold of the data hits one magic value (sink may be NULL). */
int gram_debug_stream_read(const void* src, size_t bytes, void* sink, void* stream);
/* variants of the probe (tests/bench_stream.py): 0 = gram_debug_stream_read's kernel, 1 contiguous 16-KiB chunks per workgroup, 2 nontemporal,
 * 3 eight loads in flight, 4 LDS-DMA, 5 = 1 + nontemporal; wgs = workgroups of 256 threads */
int gram_debug_stream_read_variant(const void* src, size_t bytes, void* sink, int variant, int wgs, void* stream);

/* A/B hook (bench.py): 0 = decode every row in every step like the reference, 1 = live-row compaction (gram_live_rows_t),
 * -1 = what the GRAM_LIVE_ROWS environment variable says (default 1).  Results are bit-identical either way. */
int gram_debug_set_live_rows(int on);
/* A/B hook: 0 = layer 0's QKV GEMMs run as on a handle without token tables, 1 = the tables are read where the handle has them,
 * -1 = what the GRAM_TOKEN_TABLES environment variable says (default 1).  Results are bit-identical either way.  Process-wide. */
int gram_debug_set_token_tables(int on);
/* A/B hook: 0 = gram_generate_tail decodes step by step like gram_generate_ex, 1 = the tail pass wherever the Trie has a tail,
 * -1 (default) = what the GRAM_TAIL_PASS environment variable says (0: never, 1: wherever the Trie has a tail), and without it by
 * size: the pass where one layer's bank holds at least 256 MB.  The pass is faster at every batch size measured; the default keeps
 * small calls on the step-wise train because the suite pins that train there.
 * Results are bit-identical either way.  Process-wide. */
int gram_debug_set_tail_pass(int on);
/* A/B hook: which self-attention the tail pass runs.  0 = the step-wise kernel level by level (gram_dec_self_attn_rows_split +
 * gram_scatter_rows per user group and level), 1 = gram_dec_self_attn_forest_split, one launch per layer, -1 (default) = what the
 * GRAM_TAIL_FOREST_ATTN environment variable says (0 / 1), and without it by size: the forest kernel for forests of at least
 * 16 384 rows.  Not a performance crossover: the suite pins the launch train of small calls.  Results are
 * bit-identical either way.  Process-wide. */
int gram_debug_set_tail_forest_attn(int on);
/* 1 if gram_generate_tail would take the tail pass for a call of this shape on a Trie with a tail (the switch and the size rule
 * above), 0 if not: what a caller sizes its workspace by.  < 0: GRAM_E_ARG. */
int gram_tail_pass_wanted(const gram_model_t* m, int B, int N, int L);
/* TEST hook: the forest may hold at most `rows` rows (0 = what the workspace was carved for), so that the over-capacity fallback is
 * reachable with small Tries.  Process-wide. */
int gram_debug_set_tail_capacity(int rows);
/* TEST hook: a group's level of the forest may hold at most `rows` rows (0 = the cache's B * K rows per position), so that the
 * level fallback is reachable with small Tries.  Process-wide. */
int gram_debug_set_tail_level_capacity(int rows);
/* What the last gram_generate[_ex / _items / _tail] of this process did: out[0] = 1 if the tail pass ran (0: step by step), out[1] = forest rows,
 * out[2] = cross-attention entries, out[3] = most rows of one user (the three counts are 0 when no forest was built). */
int gram_debug_tail_last(int32_t* out4);
/* TEST hook: where gram_generate[_ex / _items / _tail] keeps its beam state inside a workspace carved for (B, N, L, K, max_length):
 * *out gets the device pointers and sizes (length_penalty is the carve's default), so a test can read the state a call left. */
int gram_debug_workspace_beam_state(const gram_model_t* m, void* workspace, int B, int N, int L, int K, int max_length,
                                    gram_beam_state_t* out);
/* A/B hook (tests/bench_wide_trie.py): which form of the Trie-constrained search step runs.  -1 (default) and 0 = by shape: the
 * one-shot kernel where all K * max_fanout candidates fit on chip, the chunked kernel otherwise; 1 = always the chunked kernel.
 * Results are bit-identical either way.  Process-wide. */
int gram_debug_set_beam_chunked(int mode);
/* TEST hook: the chunked search step takes at most `candidates` fresh candidates per selection round (0 = default: what its key
 * array holds, 4 096 - P, P = the power of two >= 2K, >= 64), so that chunk boundaries are reachable with small Tries.  Results do
 * not depend on it.  Process-wide. */
int gram_debug_set_beam_chunk_capacity(int candidates);
/* Sensitivity sweeps over the split modes (tests/precision_population.py --sweep): stage s of a generate() computes on the first
 * caps[s] pieces of its operands only (the upper pieces of its activation operands are zeroed before use; the caller zeroes the
 * upper pieces of that stage's weights when it expands them).  caps NULL = no caps.  n must be GRAM_STAGE_COUNT. */
enum gram_stage {
  GRAM_STAGE_ENC_ATTN = 0,  /* encoder QKV GEMM, self-attention, O GEMM                    */
  GRAM_STAGE_ENC_FFN = 1,   /* encoder wi / wo GEMMs                                       */
  GRAM_STAGE_BANK_K = 2,    /* the stored K bank (and the K rows of the bank projection)    */
  GRAM_STAGE_BANK_V = 3,    /* the stored V^T bank (and the V rows of the bank projection)  */
  GRAM_STAGE_DEC_SELF = 4,  /* decoder QKV GEMM, cached self-attention, O GEMM             */
  GRAM_STAGE_DEC_CROSS = 5, /* decoder cross-attention q GEMM, the query side, O GEMM      */
  GRAM_STAGE_DEC_FFN = 6,   /* decoder wi / wo GEMMs                                       */
  GRAM_STAGE_LM_HEAD = 7,   /* final hidden state: lm_head GEMM (LSE) and the sparse logits */
  GRAM_STAGE_COUNT = 8
};
int gram_debug_set_stage_pieces(const int32_t* caps, int n);

/* `_f16` aliases of the entry points whose historical names say `_bf16`: same arguments; they forward in a library built on IEEE half
 * (gram_piece_format() == 1, the default) and return GRAM_E_ARG in the bfloat16 A/B build, so a binding by name cannot hand the
 * kernels the wrong 16-bit type. */
int gram_gemm_f16(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldc, int epilogue,
                  const gram_kv_bank_t* bank_host, void* stream);
int gram_gemm_f16_ex(const void* A, const void* W, void* C, int M, int N, int K, int lda, int ldc, int epilogue,
                     const gram_kv_bank_t* bank_host, const gram_norm_fusion_t* nf_host, void* stream);
int gram_gemm_f16_split(const void* A, const void* W, void* C, int M, int N, int kc, int lda, int ldc, int epilogue,
                        const gram_kv_bank_t* bank_host, const gram_norm_fusion_t* nf_host, const gram_split_t* split_host, void* stream);
int gram_gemm_f16_lse(const void* A, const void* W, float* logits, float* lse_part, int M, int N, int K, int lda, int ldc, void* stream);
int gram_gemm_f16_lse_split(const void* A, const void* W, float* logits, float* lse_part, int M, int N, int kc, int lda, int ldc,
                            const gram_split_t* split_host, void* stream);
int gram_rmsnorm_f16(const float* x, const float* w, void* out_f16, int rows, int d, float eps, float scale, const float* pos, int N,
                     int L, void* stream);
int gram_rmsnorm_f16_map(const float* x, const float* w, void* out_f16, int rows, int d, float eps, float scale, const float* pos,
                         int N, int L, const int32_t* passage_map, void* stream);
int gram_rmsnorm_f16_split(const float* x, const float* w, void* out_f16, int rows, int d, float eps, float scale, const float* pos,
                           int N, int L, const int32_t* passage_map, int pieces, void* stream);

int gram_abi_version(void);
/* 16-bit operand type this build of the library computes on: 0 = bfloat16, 1 = IEEE half ("f16": make PIECE=f16).  Every "bf16"
 * pointer of this header is a pointer to that type. */
int gram_piece_format(void);

#ifdef __cplusplus
}
#endif
#endif /* GRAM_HIP_H */
