// dec_attn.hip -- the two decoder attention kernels of one decode step.
//
// (1) cross_attn_kernel: late-fusion cross-attention, THE HBM-bound kernel of the path.
//     Reference: T5Attention.forward cross branch, gram_t5_modeling.py:531-534,547-549,572-622
//     (zero position bias :577-582, additive mask :1145-1147), called per layer per step on
//     K-times replicated K/V.  Here ONE bank per user is streamed ONCE per (layer, step) and
//     shared by all of the user's beams: algorithmic bytes = 2 * S * 64 * 2 B per (user, head)
//     and bf16 piece of the bank.
//
//     Mapping: one workgroup per (user, head); two waves for K <= 32, one above (measured: launch_cross()); wave w
//     owns the valid 32-key steps w, w + NW, ...  A step's K rows (32 x 128 B) and V^T rows (64 x 64 B) of every bf16 piece are
//     brought into the wave's PRIVATE stage in LDS by LDS-DMA (global_load_lds, 16 B per lane, no staging registers).  There is
//     ONE stage per wave, consumed and re-filled in halves: the next step's K tiles fly during this step's S^T and softmax, its
//     V^T tiles during O^T += V^T P^T.  Waves never synchronise inside the loop (counted s_waitcnt vmcnt only).  The DMA writes
//     LDS linearly, so the bank-conflict swizzles are applied to the per-lane SOURCE chunk.  S^T = K Q^T puts a beam on a lane
//     column, so the online softmax is in-register + two cross-lane steps, and exp(S^T) is directly the B operand of
//     O^T = V^T P^T (same row-permutation trick as enc_attn.hip).  Two waves merge their (m, l, O) partials through LDS
//     (aliasing the stages) at the end; one wave's accumulators are the result.
//
// (2) dec_self_attn_kernel: causal self-attention of the newest token over <= 32 cached
//     positions with beam-parent indirection (anc table) instead of the reference's
//     torch.cat + index_select of the whole cache (gram_t5_modeling.py:536-540,
//     gram_t5.py:320-348); unidirectional relative bias, last query row (:586-593).  The arithmetic of a row is self_attn_row.h's,
//     the one text that tf_attn.hip's and tree_attn.hip's self-attention kernels call too: a cached decode step and the same
//     prefix in a teacher-forced sequence or in the Trie pass give the same bits by construction.
//
// Both kernels take their bf16 operands as 1 or 2 pieces (GRAM_MAX_PIECES; gram_split_t in gram_hip.h).
#include <type_traits>

#include "common.h"
#include "prof.h"
#include "self_attn_row.h"
#include "xattn_tile.h"

namespace {

// The merge of the cross-attention, whose rounding depends on an fma-contraction decision, spelled out once (xa_l_update: xattn_tile.h)
// (every instantiation of the kernel must return the same bits for the same (user, head) -- a user's result does not depend on the batch
// it is scored in -- and hipcc decides contraction per call site).
// merge of the two partial softmaxes (m, l, O) of a (user, head): weights and 1 / l
__device__ __forceinline__ void xa_merge_w(float m0, float m1, float l0, float l1, float& w0, float& w1, float& inv) {
  const float M = fmaxf(fmaxf(GRAM_FMIN, m0), m1);
  w0 = __expf(m0 - M);
  w1 = __expf(m1 - M);
  inv = 1.f / __builtin_fmaf(l1, w1, l0 * w0);
}
__device__ __forceinline__ f32x4 xa_merge_o(f32x4 o0, f32x4 o1, float w0, float w1, float inv) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = __builtin_fmaf(o1[e], w1, o0[e] * w0) * inv;
  return r;
}

// NT = 16-beam tiles; LIVE: live-row step (gram_live_rows_t); S = bf16 pieces; NW = waves per workgroup (1: a wave owns the whole
// (user, head) and nothing is merged)
template <int NT, bool LIVE, int S, int NW>
__global__ __launch_bounds__(NW * 64) void cross_attn_kernel(
    const p16* __restrict__ q, const p16* __restrict__ kbank, const p16* __restrict__ vtbank,
    const uint8_t* __restrict__ mask, p16* __restrict__ out, int K, int H, int Sk, const int32_t* __restrict__ users,
    const int32_t* __restrict__ rowpos, long q_pstride, long bank_pstride, const uint32_t* __restrict__ key_bits) {
  constexpr int NB = NT * 16;                     // padded beams
  static_assert(NW == 1 || NW == 2, "the merge is written for two waves");
  constexpr int PSTR = 2 * XA_TILE;               // piece stride inside the stage: K tile | V^T tile
  constexpr int STAGE = S * PSTR;                 // per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm_m = reinterpret_cast<float*>(smem);   // [NW][NB]     (the merge buffers alias the stages)
  float* sm_l = sm_m + NW * NB;                   // [NW][NB]
  float* sm_o = sm_l + NW * NB;                   // [NW][NB][64]

  // live-row step (users != NULL): workgroup y serves user users[y]; q/out rows are the compact rows rowpos[b*K + beam]
  // (-1 = beam not live: zero query, nothing stored)
  const int h = blockIdx.x, b = LIVE ? users[blockIdx.y] : blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int inner = H * 64;
  const char* kb = reinterpret_cast<const char*>(kbank + ((size_t)b * H + h) * Sk * 64);
  const char* vt = reinterpret_cast<const char*>(vtbank + ((size_t)b * H + h) * 64 * Sk);
  const uint8_t* mk = mask + (size_t)b * Sk;

  p16x8 qf[S][NT][2];  // query fragments
  f32x4 o[4][NT];
  float m[NT], l[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    m[nt] = GRAM_FMIN;
    l[nt] = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) o[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // query fragments (lane: beam 16 nt + c, dims 32 kd + 8 g ..+7 of the head; zeros for a beam that has no row): requested first, in
  // parallel with the key bits, and retired with them by the wait in front of the loop -- the counted waits of the loop must see DMA
  // instructions only.  (The load and, below, its fence are spelled out in each kernel: as shared functions they cost this one registers)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int qrow = xa_row<LIVE>(b, K, 16 * nt + c, rowpos);
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd)
        qf[pc][nt][kd] = qrow >= 0 ? ld_global_b128(q + pc * q_pstride + (size_t)qrow * inner + h * 64 + 32 * kd + 8 * g) : zero_bf16x8();
  }
  // Fully masked 32-key steps (padded passages / padded tails) are never fetched: the algorithmic
  // traffic is proportional to the VALID fused keys.  One word of key bits per step (S <= 4096 -> <= 128 steps);
  // the valid steps are dealt round-robin to the waves.  A user with no valid key at all keeps
  // every step: the reference's softmax over all-finfo.min scores is uniform over all S keys.
  const int nsteps = Sk >> 5;
  // this lane's two words of key bits (steps lane and lane + 64), either precomputed once per generate (gram_mask_key_bits) or
  // packed here from the mask bytes; every wave holds all of them, so a step's word is one v_readlane away
  uint32_t kb0, kb1;
  unsigned long long v0, v1;
  xa_key_steps(key_bits, mk, b, nsteps, lane, kb0, kb1, v0, v1);
  int ord = 0;  // ordinal of the next valid step (wave-uniform scalar state)
  // (the dealing is spelled out here and in cross_attn_runs_kernel: as a shared function it costs their instantiations one to three SGPRs)
  auto next = [&](int s) -> int {
    for (s = s + 1; s < nsteps; ++s) {
      const unsigned long long bit = (s < 64 ? (v0 >> s) : (v1 >> (s - 64))) & 1ull;
      if (bit) {
        const bool mine = ord == wave;
        ord = ord + 1 == NW ? 0 : ord + 1;
        if (mine) return s;
      }
    }
    return nsteps;
  };

  // per-lane byte offsets of this lane's 16 B in each of the 4 + 4 DMA instructions of a (step, piece)
  // (spelled out in each kernel: computed by shared functions, the bf16 build's <1, ., 2, 2> takes three VGPRs more)
  uint32_t koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 8 * i + (lane >> 3);  // key row of the tile; the lane lands at position lane & 7 and fetches chunk pos ^ ksw
    koff[i] = (uint32_t)(kr * 128 + (((lane & 7) ^ ksw(kr)) << 4));
    const int d = 16 * i + (lane >> 2);  // V^T row; position lane & 3
    voff[i] = (uint32_t)(d * 64 + (((lane & 3) ^ vsw(d)) << 4));
  }
  const uint32_t stage0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * STAGE;
  auto issue_k = [&](int step) { xa_issue_k<S, PSTR>(stage0, kb, bank_pstride, step, koff); };
  auto issue_v = [&](int step) { xa_issue_v<S, PSTR>(stage0, vt, bank_pstride, step, voff); };
  p16x8 kf[S][2][2], vf[S][4];  // the step's K / V^T fragments
  auto read_k = [&]() { xa_read_k<S, PSTR>(smem + wave * STAGE, c, g, kf); };
  auto read_v = [&]() { xa_read_v<S, PSTR>(smem + wave * STAGE, c, g, vf); };
  p16x8 pf[S][NT];  // exp(S^T - max) of the step, as pieces: the B operand of O^T += V^T P^T

  // the shared 32-key step (xattn_tile.h) on this kernel's registers.  (Through lambdas: called from the loop directly, hipcc promotes
  // the arrays they capture to registers before it unrolls, and reschedules whole kernels.)
  auto step_qk = [&](int step) { xa_step_qk<NT>(xa_kword(kb0, kb1, step), g, kf, qf, pf, m, l, o); };
  auto step_pv = [&]() { xa_step_pv<NT>(vf, pf, o); };

  // Everything the first DMAs depend on (the key bits) is in; ordinary loads, the query fragments among them, are retired so that the
  // counted waits below see DMA instructions only.
  wait_vm<0>();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) asm volatile("" : "+v"(qf[pc][nt][kd]));  // (hipcc's own wait for the loads goes HERE)
  // One stage per wave, consumed and re-filled in HALVES: the K tiles of step s+1 are requested as soon as the K fragments of step
  // s are in registers (and fly during S^T, softmax), its V^T tiles as soon as the V^T fragments of step s are (and fly during
  // O^T += V^T P^T and the next S^T): the wave always has a half-stage in flight, where waiting for the whole stage and
  // re-filling it after the reads left nothing in flight for a few hundred cycles of every step.
  int cur = next(-1);
  if (cur < nsteps) {
    issue_k(cur);
    issue_v(cur);
  }
  while (cur < nsteps) {
    const int nxt = next(cur);
    wait_vm<4 * S>();  // all but the newest half-stage (this step's V^T tiles): its K tiles have landed
    read_k();
    if (nxt < nsteps) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the K fragments are in registers before their tiles are re-filled
      issue_k(nxt);
    }
    step_qk(cur);
    if (nxt < nsteps) wait_vm<4 * S>();  // (newest: the next step's K tiles)
    else wait_vm<0>();
    read_v();
    if (nxt < nsteps) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      issue_v(nxt);
    }
    step_pv();
    cur = nxt;
  }

  if constexpr (NW == 1) {
    // one wave owns the whole (user, head): its accumulators are the result (lane: beam 16 nt + c, dims 16 mt + 4 g ..+3)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float lt = l[nt];
      lt += __shfl_xor(lt, 16, 64);
      lt += __shfl_xor(lt, 32, 64);
      const float inv = 1.f / lt;
      const int orow = xa_row<LIVE>(b, K, 16 * nt + c, rowpos);
      if (orow >= 0) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) xa_store<S>(out, orow, inner, h * 64 + 16 * mt + 4 * g, o[mt][nt] * inv);
      }
    }
    return;
  }
  // merge the two waves' partials (the stages are dead once both waves are past their loops)
  gram_sync();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    float lt = l[nt];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const int beam = 16 * nt + c;
    if (g == 0) {
      sm_m[wave * NB + beam] = m[nt];
      sm_l[wave * NB + beam] = lt;
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
      *reinterpret_cast<f32x4*>(sm_o + ((size_t)(wave * NB + beam)) * 64 + 16 * mt + 4 * g) = o[mt][nt];
  }
  gram_sync();
  for (int idx = tid; idx < K * 16; idx += NW * 64) {
    const int beam = idx >> 4, d4 = (idx & 15) * 4;
    float w0, w1, inv2;
    xa_merge_w(sm_m[beam], sm_m[NB + beam], sm_l[beam], sm_l[NB + beam], w0, w1, inv2);
    const f32x4 v = xa_merge_o(*reinterpret_cast<const f32x4*>(sm_o + ((size_t)beam) * 64 + d4),
                         *reinterpret_cast<const f32x4*>(sm_o + ((size_t)(NB + beam)) * 64 + d4), w0, w1, inv2);
    int orow = b * K + beam;  // (beam < K here; through xa_row() hipcc keeps the comparison and reschedules the merge)
    if constexpr (LIVE) orow = rowpos[orow];
    if (orow >= 0) xa_store<S>(out, orow, inner, h * 64 + d4, v);
  }
}

// The entry form of the tail pass (gram_cross_attn_entries_split): the rows of a user's forest, 64 table slots per entry
// (gram_forest_t.ent_rows, -1 = none).  One workgroup per (head, run of consecutive entries that name one user): the workgroup of an
// entry whose predecessor names the same user returns at once, the run's leader serves the run two entries (eight 16-row tiles) at a
// time and sweeps the user's bank slice once per pair.  2 * NW waves: wave (p, w) owns the valid key steps the step-wise kernel deals
// to wave w of NW and the live tiles -- tiles with a row in any of their 16 slots -- of ordinal p, p + 2, ... of the pair, at most
// four; a tile without a row costs nothing.  The two waves (0, w) and (1, w) of a key split consume the same steps and share a ring
// of two stages: one brings a step's K tiles, the other its V^T tiles, one step ahead, and one workgroup barrier per step hands the
// stages over (gram_sync(): the chaos build screens it).  The form with a private stage and a counted-wait pipeline per wave, as in
// cross_attn_kernel, was measured too: its second request for a line is not reliably an L2 hit (13.8 GB per launch from beyond the
// L2 against 10.7 GB here) and it was 0.4 ms per launch slower (profiles/xattn_entries_bench_ab.txt).
// A row's arithmetic is the step-wise kernel's: both call the one 32-key step of xattn_tile.h (xa_step_qk, xa_step_pv) and the one
// merge of the two key-split partials (xa_merge_w, xa_merge_o), and deal the valid steps to the waves alike, so a row's bits are those
// of cross_attn_kernel<.., S, NW> whatever tile of whatever entry holds it.
constexpr int XA_RUN_MERGE = 4 * (4 * 64 * 16 + 2 * 64 * 4);  // LDS per half for the merge: O, m, l of wave (p, 1) (aliases the stages)
template <int S, int NW>
__global__ __launch_bounds__(2 * NW * 64, 2) void cross_attn_runs_kernel(
    const p16* __restrict__ q, const p16* __restrict__ kbank, const p16* __restrict__ vtbank, const uint8_t* __restrict__ mask,
    p16* __restrict__ out, int n_entries, int H, int Sk, const int32_t* __restrict__ ent_users, const int32_t* __restrict__ ent_rows,
    long q_pstride, long bank_pstride, const uint32_t* __restrict__ key_bits) {
  static_assert(NW == 1 || NW == 2, "the merge is written for two waves");
  constexpr int ER = GRAM_TAIL_ENTRY_ROWS;        // table slots per entry
  constexpr int MT = 4;                           // tiles per wave at most: half of a pair's eight
  static_assert(ER == 64, "a pair of entries is eight 16-row tiles");
  constexpr int PSTR = 2 * XA_TILE;               // piece stride inside the stage: K tile | V^T tile
  constexpr int STAGE = S * PSTR;                 // per wave
  constexpr int MERGE = XA_RUN_MERGE;
  static_assert(MERGE == MT * (4 * 64 * 16 + 2 * 64 * 4), "O, m, l of up to MT tiles, one slot per lane");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int h = blockIdx.x, lead = blockIdx.y;
  const int b = ent_users[lead];
  if (lead > 0 && ent_users[lead - 1] == b) return;  // served by the run's leader
  int run_end = lead + 1;
  while (run_end < n_entries && ent_users[run_end] == b) ++run_end;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = wv % NW, half = wv / NW;       // key split | which of the pair's live tiles
  const int c = lane & 15, g = lane >> 4;
  const int inner = H * 64;
  const char* kb = reinterpret_cast<const char*>(kbank + ((size_t)b * H + h) * Sk * 64);
  const char* vt = reinterpret_cast<const char*>(vtbank + ((size_t)b * H + h) * 64 * Sk);
  const uint8_t* mk = mask + (size_t)b * Sk;

  // the valid 32-key steps (xa_key_steps) and their dealing to the waves of a key split, as in cross_attn_kernel
  const int nsteps = Sk >> 5;
  uint32_t kb0, kb1;
  unsigned long long v0, v1;
  xa_key_steps(key_bits, mk, b, nsteps, lane, kb0, kb1, v0, v1);
  int ord = 0;  // ordinal of the next valid step (wave-uniform scalar state)
  auto next = [&](int s) -> int {
    for (s = s + 1; s < nsteps; ++s) {
      const unsigned long long bit = (s < 64 ? (v0 >> s) : (v1 >> (s - 64))) & 1ull;
      if (bit) {
        const bool mine = ord == wave;
        ord = ord + 1 == NW ? 0 : ord + 1;
        if (mine) return s;
      }
    }
    return nsteps;
  };

  // per-lane byte offsets of this lane's 16 B in each of the 4 + 4 DMA instructions of a (step, piece)
  uint32_t koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 8 * i + (lane >> 3);
    koff[i] = (uint32_t)(kr * 128 + (((lane & 7) ^ ksw(kr)) << 4));
    const int d = 16 * i + (lane >> 2);
    voff[i] = (uint32_t)(d * 64 + (((lane & 3) ^ vsw(d)) << 4));
  }
  // a key split's ring of two stages, shared by its two waves: wave (0, w) brings a step's K tiles, wave (1, w) its V^T tiles
  const uint32_t stage0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * 2 * STAGE;
  const int nvalid = __popcll(v0) + __popcll(v1);
  const int trips = (nvalid + NW - 1) / NW;  // key steps of wave (., 0): every wave of the workgroup meets this many barriers per sweep
  auto issue_k = [&](int step, int buf) { xa_issue_k<S, PSTR>(stage0 + buf * STAGE, kb, bank_pstride, step, koff); };
  auto issue_v = [&](int step, int buf) { xa_issue_v<S, PSTR>(stage0 + buf * STAGE, vt, bank_pstride, step, voff); };

  f32x4 o[4][MT];
  float m[MT], l[MT];
  // one sweep of the slice for this wave's NL live tiles `tiles` (four bits each) of the pair whose table slots start at `rows`:
  // the shared step with NT = NL
  auto sweep = [&](auto nl_c, const int32_t* __restrict__ rows, int tiles) __attribute__((always_inline)) {
    constexpr int NL = decltype(nl_c)::value;
    constexpr int NA = NL > 0 ? NL : 1;  // (NL = 0: this half of the pair holds no live tile; the wave brings its tiles all the same)
    // the first step's tiles are requested ahead of the query fragments: both are in flight together
    ord = 0;
    int cur = next(-1);
    if (cur < nsteps) {
      if (half == 0) issue_k(cur, 0);
      else issue_v(cur, 0);
    }
    p16x8 qf[S][NA][2];
#pragma unroll
    for (int nt = 0; nt < NL; ++nt) {
      const int qrow = rows[16 * ((tiles >> (4 * nt)) & 7) + c];
#pragma unroll
      for (int pc = 0; pc < S; ++pc)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd)
          qf[pc][nt][kd] = qrow >= 0 ? ld_global_b128(q + pc * q_pstride + (size_t)qrow * inner + h * 64 + 32 * kd + 8 * g) : zero_bf16x8();
    }
    p16x8 kf[S][2][2], vf[S][4];
    auto read_k = [&](int buf) { xa_read_k<S, PSTR>(smem + (wave * 2 + buf) * STAGE, c, g, kf); };
    auto read_v = [&](int buf) { xa_read_v<S, PSTR>(smem + (wave * 2 + buf) * STAGE, c, g, vf); };
    p16x8 pf[S][NA];
    // (through lambdas: see cross_attn_kernel)
    auto step_qk = [&](int step) { xa_step_qk<NL>(xa_kword(kb0, kb1, step), g, kf, qf, pf, m, l, o); };
    auto step_pv = [&]() { xa_step_pv<NL>(vf, pf, o); };
    wait_vm<0>();
#pragma unroll
    for (int nt = 0; nt < NL; ++nt)
#pragma unroll
      for (int pc = 0; pc < S; ++pc)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd) asm volatile("" : "+v"(qf[pc][nt][kd]));
    // A step's tiles are requested one step ahead, into the other stage of the ring.  One workgroup barrier per step: behind it the
    // step's tiles have landed (each partner has waited for its own) and every wave has the last step's fragments in registers, so
    // that stage is free for the next step's tiles.  A wave that has run out of steps -- the second key split may own one step fewer
    // -- goes on meeting the barriers.
    for (int it = 0; it < trips; ++it) {
      const int buf = it & 1;
      wait_vm<0>();
      gram_sync();
      const int nxt = cur < nsteps ? next(cur) : nsteps;
      if (nxt < nsteps) {
        if (half == 0) issue_k(nxt, buf ^ 1);
        else issue_v(nxt, buf ^ 1);
      }
      if constexpr (NL > 0) {
        if (cur < nsteps) {
          read_k(buf);
          step_qk(cur);
          read_v(buf);
          step_pv();
        }
      }
      cur = nxt;
    }
  };

  for (int e0 = lead; e0 < run_end; e0 += 2) {
    const int32_t* rows = ent_rows + (size_t)e0 * ER;
    const int ntiles = e0 + 1 < run_end ? 2 * (ER / 16) : ER / 16;
    // the pair's live tiles, dealt alternately to the two halves (wave-uniform: a ballot per tile)
    int nl = 0, tiles = 0, seen = 0;
#pragma unroll
    for (int t = 0; t < 2 * (ER / 16); ++t) {
      const int r = t < ntiles ? rows[16 * t + c] : -1;
      if (__ballot(r >= 0) != 0ull) {
        if ((seen & 1) == half) {
          tiles |= t << (4 * nl);
          ++nl;
        }
        ++seen;
      }
    }
    if (seen == 0) continue;  // (the same for every wave of the workgroup)
    nl = __builtin_amdgcn_readfirstlane(nl);
    tiles = __builtin_amdgcn_readfirstlane(tiles);
#pragma unroll
    for (int nt = 0; nt < MT; ++nt) {
      m[nt] = GRAM_FMIN;
      l[nt] = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) o[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    if (e0 != lead) gram_sync();  // the last pair's stages and merge buffers have been read
    switch (nl) {
      case 1: sweep(std::integral_constant<int, 1>{}, rows, tiles); break;
      case 2: sweep(std::integral_constant<int, 2>{}, rows, tiles); break;
      case 3: sweep(std::integral_constant<int, 3>{}, rows, tiles); break;
      case 4: sweep(std::integral_constant<int, 4>{}, rows, tiles); break;
      default: sweep(std::integral_constant<int, 0>{}, rows, tiles); break;
    }
    float* mg_o = reinterpret_cast<float*>(smem + half * MERGE);  // [MT][4][64 lanes] f32x4
    float* mg_m = mg_o + MT * 4 * 64 * 4;                         // [MT][64 lanes]
    float* mg_l = mg_m + MT * 64;
    if constexpr (NW == 2) gram_sync();  // every wave is past its loop: the stages are dead
#pragma unroll
    for (int nt = 0; nt < MT; ++nt) {
      if (nt < nl) {
        float lt = l[nt];
        lt += __shfl_xor(lt, 16, 64);
        lt += __shfl_xor(lt, 32, 64);
        l[nt] = lt;
        if constexpr (NW == 2) {
          if (wave == 1) {
            mg_m[nt * 64 + lane] = m[nt];
            mg_l[nt * 64 + lane] = lt;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<f32x4*>(mg_o + ((nt * 4 + mt) * 64 + lane) * 4) = o[mt][nt];
          }
        }
      }
    }
    if constexpr (NW == 2) gram_sync();
    if (wave == 0) {
#pragma unroll
      for (int nt = 0; nt < MT; ++nt) {
        if (nt < nl) {
          const int orow = rows[16 * ((tiles >> (4 * nt)) & 7) + c];
          if constexpr (NW == 2) {
            float w0, w1, inv2;
            xa_merge_w(m[nt], mg_m[nt * 64 + lane], l[nt], mg_l[nt * 64 + lane], w0, w1, inv2);
            if (orow >= 0) {
#pragma unroll
              for (int mt = 0; mt < 4; ++mt)
                xa_store<S>(out, orow, inner, h * 64 + 16 * mt + 4 * g,
                            xa_merge_o(o[mt][nt], *reinterpret_cast<const f32x4*>(mg_o + ((nt * 4 + mt) * 64 + lane) * 4), w0, w1, inv2));
            }
          } else {
            const float inv = 1.f / l[nt];
            if (orow >= 0) {
#pragma unroll
              for (int mt = 0; mt < 4; ++mt) xa_store<S>(out, orow, inner, h * 64 + 16 * mt + 4 * g, o[mt][nt] * inv);
            }
          }
        }
      }
    }
  }
}

// host side of one cross-attention launch
struct XaLaunch {
  const void *q, *k, *vt;
  const uint8_t* mask;
  void* out;
  int B, K, H, Sk;
  const int32_t *users, *rowpos;
  long q_ps, bank_ps;
  const uint32_t* key_bits;
  hipStream_t st;
};

// Two waves per (user, head) for one or two beam tiles, one wave for three or four (K > 32: the per-workgroup state is larger), ONE
// stage per wave: many small workgroups per CU hide the per-workgroup prologue and merge better than deeper rings or more waves do.
// Every alternative that was measured: DESIGN.md §4.2.
template <int NT, int S>
int launch_cross(const XaLaunch& a) {
  constexpr int NW = NT >= 3 ? 1 : 2;
  constexpr int NB = NT * 16;
  constexpr int stages = NW * S * 2 * XA_TILE, merge = NW == 1 ? 0 : (2 * NW * NB + NW * NB * 64) * 4;
  constexpr int smem = stages > merge ? stages : merge;
  static_assert(smem <= 160 * 1024, "the stages do not fit the LDS");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_kernel<NT, false, S, NW>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_kernel<NT, true, S, NW>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  if (a.users)
    hipLaunchKernelGGL((cross_attn_kernel<NT, true, S, NW>), dim3(a.H, a.B), dim3(NW * 64), smem, a.st, (const p16*)a.q, (const p16*)a.k,
                       (const p16*)a.vt, a.mask, (p16*)a.out, a.K, a.H, a.Sk, a.users, a.rowpos, a.q_ps, a.bank_ps, a.key_bits);
  else
    hipLaunchKernelGGL((cross_attn_kernel<NT, false, S, NW>), dim3(a.H, a.B), dim3(NW * 64), smem, a.st, (const p16*)a.q, (const p16*)a.k,
                       (const p16*)a.vt, a.mask, (p16*)a.out, a.K, a.H, a.Sk, a.users, a.rowpos, a.q_ps, a.bank_ps, a.key_bits);
  GRAM_CHECK_LAUNCH();
  return 0;
}

template <int S>
int launch_cross_nt(const XaLaunch& a) {
  switch ((a.K + 15) / 16) {
    case 1: return launch_cross<1, S>(a);
    case 2: return launch_cross<2, S>(a);
    case 3: return launch_cross<3, S>(a);
    default: return launch_cross<4, S>(a);
  }
}

// The entry form of the tail pass: one workgroup per entry is launched (the runs of a user's entries are not known on the host) and
// the leader of each run does the run's work; NW is what launch_cross picks for the search's K beams, because the split of the keys
// over the waves is part of a row's bits.
template <int S, int NW>
int launch_cross_entries(const XaLaunch& a) {
  constexpr int stages = NW * 2 * S * 2 * XA_TILE, merge = NW == 1 ? 0 : 2 * XA_RUN_MERGE;  // a ring of two stages per key split
  constexpr int smem = stages > merge ? stages : merge;
  static_assert(smem <= 160 * 1024, "the stages do not fit the LDS");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_runs_kernel<S, NW>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL((cross_attn_runs_kernel<S, NW>), dim3(a.H, a.B), dim3(2 * NW * 64), smem, a.st, (const p16*)a.q, (const p16*)a.k,
                     (const p16*)a.vt, a.mask, (p16*)a.out, a.B, a.H, a.Sk, a.users, a.rowpos, a.q_ps, a.bank_ps, a.key_bits);
  GRAM_CHECK_LAUNCH();
  return 0;
}

// key_bits[b][st] bit j = mask[b][32 st + j] != 0 (st < S/32 <= 128; rows are 128 words apart): the cross-attention's view of
// the mask, the same for every head, layer and decode step of a generate() -- computed once instead of per workgroup
__global__ __launch_bounds__(128) void mask_key_bits_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ bits, int Sk) {
  const int b = blockIdx.x, st = threadIdx.x;
  uint32_t w = 0;
  if (st < (Sk >> 5)) w = xa_pack32(mask + (size_t)b * Sk + 32 * st);
  bits[(size_t)b * 128 + st] = w;
}

// ---------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(256) void dec_self_attn_kernel(const p16* __restrict__ qkv, p16* __restrict__ kcache,
                                                            p16* __restrict__ vcache, const int32_t* __restrict__ anc,
                                                            const float* __restrict__ bias, p16* __restrict__ out, int R,
                                                            int H, int t, const int32_t* __restrict__ rows, long qkv_ps,
                                                            long cache_ps, const int32_t* __restrict__ qkv_rows) {
  // live-row step (rows != NULL): qkv/out are indexed by the compact row, the cache and the ancestor table by the
  // original row rows[compact]; R stays the row count of the cache
  // qkv_rows != NULL: qkv is a per-token table (gram_model_build_token_tables) and compact row rc reads its row qkv_rows[rc]
  // (giving each XCD a contiguous eighth of the rows, so that a user's beams share ancestors' cache rows in ONE L2, was measured:
  // 41.9 ms per step against 41.2 for the round-robin order below)
  const int rc = blockIdx.x, i = threadIdx.x;  // i: 16 threads per head, 4 dims each
  const int r = rows ? rows[rc] : rc;
  const int inner = H * 64, h = i >> 4;
  const p16* row = qkv + (size_t)(qkv_rows ? qkv_rows[rc] : rc) * 3 * inner + 4 * i;
  // the new position's pieces go to the cache as they are
  p16x4 q4[S], k4[S], v4[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) {
    q4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps);
    k4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps + inner);
    v4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps + 2 * inner);
    *reinterpret_cast<p16x4*>(kcache + pc * cache_ps + ((size_t)t * R + r) * inner + 4 * i) = k4[pc];
    *reinterpret_cast<p16x4*>(vcache + pc * cache_ps + ((size_t)t * R + r) * inner + 4 * i) = v4[pc];
  }
  float qf[4], kn[4], vn[4], m = -INFINITY, l = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  sa_sum<S>(q4, qf);
  sa_sum<S>(k4, kn);
  sa_sum<S>(v4, vn);
  auto attend = [&](int j, const float (&kj)[4], const float (&vj)[4]) {  // position j, in order
    sa_step(qf, kj, vj, bias[h * GRAM_MAX_DEC_LEN + (t - j)], m, l, acc);
  };
  // Cached positions in batches of U: the U ancestor indices go out together, then the 2 * S * U row loads they address -- two
  // round trips per batch.  (One position per loop trip was ancestor load -> row loads -> arithmetic, strictly in sequence:
  // 2 t dependent round trips per block, 7 us per block at the bench shape.)  The positions are still taken in order.
  constexpr int U = 8;
  for (int j0 = 0; j0 < t; j0 += U) {
    int a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = anc[(size_t)min(j0 + u, t - 1) * R + r];
    p16x4 kk[U][S], vv[U][S];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t off = ((size_t)min(j0 + u, t - 1) * R + a[u]) * inner + 4 * i;
#pragma unroll
      for (int pc = 0; pc < S; ++pc) {
        kk[u][pc] = ld_stream_b64(kcache + pc * cache_ps + off);
        vv[u][pc] = ld_stream_b64(vcache + pc * cache_ps + off);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u < t) {
        float kj[4], vj[4];
        sa_sum<S>(kk[u], kj);
        sa_sum<S>(vv[u], vj);
        attend(j0 + u, kj, vj);
      }
    }
  }
  attend(t, kn, vn);
  sa_store<S>(out + (size_t)rc * inner * S, 4 * i, l, acc);
}

}  // namespace

extern "C" int gram_cross_attn_entries_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                             int n_entries, int K, int H, int S, const int32_t* ent_users, const int32_t* ent_rows,
                                             int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits,
                                             void* stream) {
  if (!q || !out || !ent_users || !ent_rows || n_entries < 1 || K < 1 || K > GRAM_MAX_BEAMS || H < 1 || S < 32 || (S & 31) ||
      S > 4096 || pieces < 1 || pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && (q_pstride < 1 || bank_pstride < (int64_t)H * S * 64)) return GRAM_E_ARG;
  if ((reinterpret_cast<uintptr_t>(mask) & 15) || (reinterpret_cast<uintptr_t>(k_layer) & 15) || (reinterpret_cast<uintptr_t>(vt_layer) & 15))
    return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_CROSS_ATTN, st, 4.0 * n_entries * H * S * 64 * pieces);  // K + V^T, every piece, per entry
  const XaLaunch a{q, k_layer, vt_layer, mask, out, n_entries, GRAM_TAIL_ENTRY_ROWS, H, S, ent_users, ent_rows, (long)q_pstride,
                   (long)bank_pstride, key_bits, st};
  const bool one_wave = (K + 15) / 16 >= 3;  // launch_cross's choice for K beams
  if (pieces == 2) return one_wave ? launch_cross_entries<2, 1>(a) : launch_cross_entries<2, 2>(a);
  return one_wave ? launch_cross_entries<1, 1>(a) : launch_cross_entries<1, 2>(a);
}

extern "C" int gram_mask_key_bits(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* stream) {
  if (!mask || !key_bits || B < 1 || S < 32 || (S & 31) || S > 4096 || (reinterpret_cast<uintptr_t>(mask) & 15)) return GRAM_E_ARG;
  hipLaunchKernelGGL(mask_key_bits_kernel, dim3(B), dim3(128), 0, (hipStream_t)stream, mask, key_bits, S);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_cross_attn_decode_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                            int B, int K, int H, int S, const int32_t* users, const int32_t* rowpos, int pieces,
                                            int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, void* stream) {
  if (B < 1 || K < 1 || K > GRAM_MAX_BEAMS || H < 1 || S < 32 || (S & 31) || S > 4096 || pieces < 1 || pieces > GRAM_MAX_PIECES ||
      (users == nullptr) != (rowpos == nullptr))
    return GRAM_E_ARG;
  if (pieces > 1 && (q_pstride < 1 || bank_pstride < (int64_t)H * S * 64)) return GRAM_E_ARG;
  if ((reinterpret_cast<uintptr_t>(mask) & 15) || (reinterpret_cast<uintptr_t>(k_layer) & 15) || (reinterpret_cast<uintptr_t>(vt_layer) & 15))
    return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_CROSS_ATTN, st, 4.0 * B * H * S * 64 * pieces);  // K + V^T, bf16, every piece
  const XaLaunch a{q, k_layer, vt_layer, mask, out, B, K, H, S, users, rowpos, (long)q_pstride, (long)bank_pstride, key_bits, st};
  return pieces == 2 ? launch_cross_nt<2>(a) : launch_cross_nt<1>(a);
}

extern "C" int gram_cross_attn_decode(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                      int B, int K, int H, int S, void* stream) {
  return gram_cross_attn_decode_split(q, k_layer, vt_layer, mask, out, B, K, H, S, nullptr, nullptr, 1, 0, 0, nullptr, stream);
}

extern "C" int gram_cross_attn_decode_live(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                           int n_users, const int32_t* users, const int32_t* rowpos, int K, int H, int S,
                                           void* stream) {
  if (!users || !rowpos) return GRAM_E_ARG;
  return gram_cross_attn_decode_split(q, k_layer, vt_layer, mask, out, n_users, K, H, S, users, rowpos, 1, 0, 0, nullptr, stream);
}

extern "C" int gram_dec_self_attn_split(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias, void* out,
                                        int R, int n_rows, const int32_t* rows, int H, int t, int Tmax, int pieces,
                                        int64_t qkv_pstride, int64_t cache_pstride, void* stream) {
  return gram_dec_self_attn_rows_split(qkv, nullptr, kcache, vcache, anc, bias, out, R, n_rows, rows, H, t, Tmax, pieces, qkv_pstride,
                                       cache_pstride, stream);
}

extern "C" int gram_dec_self_attn_rows_split(const void* qkv, const int32_t* qkv_rows, void* kcache, void* vcache, const int32_t* anc,
                                             const float* bias, void* out, int R, int n_rows, const int32_t* rows, int H, int t,
                                             int Tmax, int pieces, int64_t qkv_pstride, int64_t cache_pstride, void* stream) {
  if (R < 1 || n_rows < 1 || n_rows > R || H < 1 || H > 16 || t < 0 || t >= Tmax || Tmax > GRAM_MAX_DEC_LEN || pieces < 1 ||
      pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && (qkv_pstride < 1 || cache_pstride < (int64_t)Tmax * R * H * 64)) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_DEC_SELF_ATTN, st, 4.0 * n_rows * H * 64 * (t + 1) * pieces);
  const dim3 grid(n_rows), block(H * 16);
  if (pieces == 2)
    hipLaunchKernelGGL(dec_self_attn_kernel<2>, grid, block, 0, st, (const p16*)qkv, (p16*)kcache, (p16*)vcache, anc, bias,
                       (p16*)out, R, H, t, rows, (long)qkv_pstride, (long)cache_pstride, qkv_rows);
  else
    hipLaunchKernelGGL(dec_self_attn_kernel<1>, grid, block, 0, st, (const p16*)qkv, (p16*)kcache, (p16*)vcache, anc, bias,
                       (p16*)out, R, H, t, rows, (long)qkv_pstride, (long)cache_pstride, qkv_rows);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_dec_self_attn(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias, void* out,
                                  int R, int H, int t, int Tmax, void* stream) {
  return gram_dec_self_attn_split(qkv, kcache, vcache, anc, bias, out, R, R, nullptr, H, t, Tmax, 1, 0, 0, stream);
}

extern "C" int gram_dec_self_attn_live(const void* qkv, void* kcache, void* vcache, const int32_t* anc, const float* bias,
                                       void* out, int R, int n_rows, const int32_t* rows, int H, int t, int Tmax, void* stream) {
  if (!rows) return GRAM_E_ARG;
  return gram_dec_self_attn_split(qkv, kcache, vcache, anc, bias, out, R, n_rows, rows, H, t, Tmax, 1, 0, 0, stream);
}
