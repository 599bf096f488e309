// xattn_scores.hip -- the cross-attention probabilities of Q query rows per user SUMMED OVER THE HEADS on chip and accumulated over
// layers (gram_cross_attn_token_scores_split): the token scores of GRAM.get_crossattention_scores without the per-head tensor, over
// fused contexts of up to GRAM_MAX_LONG_FUSED_LEN = 16 384 keys.
//
//     acc[b][i][s] = (first ? 0 : acc[b][i][s]) + sum over h, ascending, of softmax_s(q[b*Q + i] . k[b][h][s] + (valid ? 0 : finfo.min))[s]
//
// The arithmetic of a (head, row) is cross_attn_probs_kernel's (xattn_probs.hip): xa_scores in the three-product order, the online
// (max, sum) of xa_row_max / xa_l_update in sweep 1, exp(s - m) * (1 / l) of the recomputed scores in sweep 2.  The key bits are
// xattn_long.hip's: eight step words per lane (gram_mask_key_bits_long), one ballot per word, the user's valid steps walked in key order.
//
// Mapping: ONE workgroup per (user, tile of 32 query rows), grid (ceil(Q / 32), B), W = min(H, 8) waves; wave w owns head w and, with
// H > 8, head w + 8 (two ROUNDS), their query fragments in registers and two K stages of its own (LDS-DMA, each re-filled as soon as its
// fragments are in registers: two tiles in flight per wave -- a workgroup is paced by the latency of a tile, not by bandwidth).
// Sweep 1 needs no barrier: each wave runs (m, l) of its heads over the valid steps.  In sweep 2 the waves
// walk the valid steps together: per (step, round) every wave writes its head's 32 x 32 tile of probabilities into its exchange slot,
// a barrier, thread t adds the round's slots in head order into its register (kept across the rounds: the order is 0 .. H-1), after the
// last round adds the old acc value unless `first` and stores -- eight threads write one full 128-byte row segment -- and a second
// barrier frees the slots.  Nothing with a head dimension leaves the chip.
//
// What a row's bits depend on: the query row, the user's valid steps in key order each with its word of bits, `first` and the old
// value -- not B, Q, the user's place in the batch, the other rows or where the fully masked steps lie.  No atomics; one writer per
// element.  Fully masked steps are never fetched: with `first` their keys are written as 0.0, otherwise left alone.  Masked keys of a
// valid step have the score finfo.min whatever the bank holds there (a select, not arithmetic), so they add exp(finfo.min - m) = 0.0.
// A user without any valid key keeps every step and every head adds the uniform 1 / S.  Rows past Q are zero queries that store nothing.
#include "common.h"
#include "prof.h"
#include "xattn_tile.h"

namespace {

constexpr int XS_NT = 2;                              // 16-row MFMA tiles: 32 query rows per workgroup
constexpr int XS_ROWS = XS_NT * 16;
constexpr int XS_MAXW = 8;                            // waves per workgroup at most; heads w and w + 8 share wave w
constexpr int XS_MAX_HEADS = 2 * XS_MAXW;
constexpr int XS_STAGES = 2;                          // K stages per wave: two tiles in flight
constexpr int XS_SLOT = XS_ROWS * 32 * 4;             // one head's exchange slot: [32 rows][32 keys] f32
constexpr int XS_CHUNKS = XS_SLOT / 16;               // 16-B chunks of a slot (= of the output tile): 8 per row
constexpr int XS_STRIDE = GRAM_KEY_BITS_LONG_STRIDE;  // words between key_bits rows

__device__ __forceinline__ unsigned long long xs_uniform64(unsigned long long v) {
  return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
         ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
}
// a[i] of eight wave-uniform values by a wave-uniform index, without a dynamically indexed array (0 past the end)
__device__ __forceinline__ unsigned long long xs_sel8(const unsigned long long (&a)[8], int i) {
  unsigned long long r = 0ull;
#pragma unroll
  for (int j = 0; j < 8; ++j) r = i == j ? a[j] : r;
  return r;
}
// byte offset of 16-B chunk ch of row r inside an exchange slot: the writers of a tile (16 rows, one chunk) and the reducers (8 chunks
// of a row) both spread over the banks
__device__ __forceinline__ int xs_slot_off(int row, int ch) { return row * 128 + ((ch ^ (row & 7)) << 4); }

// S = pieces; NR = rounds of heads (2 when H > 8).  blockDim.x = 64 * min(H, 8).
template <int S, int NR>
__global__ __launch_bounds__(64 * XS_MAXW) void cross_attn_token_scores_kernel(const p16* __restrict__ q, const p16* __restrict__ kbank,
                                                                               float* __restrict__ acc, int Q, int H, int Sk,
                                                                               long q_pstride, long bank_pstride,
                                                                               const uint32_t* __restrict__ key_bits, int first) {
  constexpr int NT = XS_NT;
  constexpr int STAGE = S * XA_TILE;  // a (step, head)'s K tile of every piece; XS_STAGES of them per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int W = H < XS_MAXW ? H : XS_MAXW;
  const int nth = W * 64;
  const int b = blockIdx.y, row0 = blockIdx.x * XS_ROWS;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int inner = H * 64;
  const int nsteps = Sk >> 5;
  char* const stage = smem + wave * (XS_STAGES * STAGE);
  char* const slots = smem + W * (XS_STAGES * STAGE);
  const bool has1 = NR == 2 && wave + XS_MAXW < H;  // this wave owns a head in round 1 (wave-uniform)

  // The user's key bits: lane holds the words of steps lane + 64 j.  One ballot per j says which steps have a valid key.
  uint32_t kw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int st = lane + 64 * j;
    kw[j] = st < nsteps ? key_bits[(size_t)b * XS_STRIDE + st] : 0u;
  }
  unsigned long long v[8];
  int total = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = xs_uniform64(__ballot(kw[j] != 0u));
    total += __builtin_popcountll(v[j]);
  }
  if (total == 0) {  // no valid key at all: every step, uniform over exactly Sk keys
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rem = nsteps - 64 * j;
      v[j] = rem >= 64 ? ~0ull : (rem > 0 ? ((1ull << rem) - 1ull) : 0ull);
    }
    total = nsteps;
  }
  // the walk over the valid steps in key order (scalar state: the word being consumed, its index, the steps left)
  int wi = 0, left = 0;
  unsigned long long bits = 0ull;
  auto rewind = [&]() {
    wi = 0;
    left = total;
    bits = v[0];
  };
  auto next = [&]() -> int {
    if (left <= 0) return nsteps;
    while (bits == 0ull && wi < 7) bits = xs_sel8(v, ++wi);
    if (bits == 0ull) {  // (cannot happen: `left` counts set bits)
      left = 0;
      return nsteps;
    }
    const int s = 64 * wi + __builtin_ctzll(bits);
    bits &= bits - 1ull;
    --left;
    return s;
  };
  // the word of key bits of a step (wave-uniform)
  auto step_word = [&](int step) -> uint32_t {
    uint32_t w = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t wj = (uint32_t)__builtin_amdgcn_readlane((int)kw[j], step & 63);
      w = (step >> 6) == j ? wj : w;
    }
    return w;
  };

  // query fragments of this wave's heads (lane: row 16 nt + c, dims 32 kd + 8 g ..+7 of the head; zeros past Q)
  const char* kb[NR];
  p16x8 qf[NR][S][NT][2];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const bool mine = r == 0 || has1;
    const int h = mine ? wave + XS_MAXW * r : wave;  // (a wave without a head in round 1 never fetches with kb[1])
    kb[r] = reinterpret_cast<const char*>(kbank + ((size_t)b * H + h) * Sk * 64);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int i = row0 + 16 * nt + c;
#pragma unroll
      for (int pc = 0; pc < S; ++pc)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd)
          qf[r][pc][nt][kd] =
              i < Q ? ld_global_b128(q + pc * q_pstride + ((size_t)b * Q + i) * inner + h * 64 + 32 * kd + 8 * g) : zero_bf16x8();
    }
  }

  // this thread's outputs: the 16-B chunks tid + k * nth of the 32 x 32 tile (row = chunk / 8), nullptr past Q or past the tile
  constexpr int NK = XS_CHUNKS / 64;  // chunks per thread at one wave
  float* orow[NK];
  int ooff[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) {
    const int idx = tid + k * nth;
    const int row = idx >> 3, ch = idx & 7;
    const bool on = idx < XS_CHUNKS && row0 + row < Q;
    orow[k] = on ? acc + ((size_t)b * Q + row0 + row) * Sk + 4 * ch : nullptr;
    ooff[k] = on ? xs_slot_off(row, ch) : 0;
  }

  // the skipped steps' outputs of a first launch: zeros
  if (first) {
    for (int s = 0; s < nsteps; ++s) {
      if ((xs_sel8(v, s >> 6) >> (s & 63)) & 1ull) continue;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (orow[k]) *reinterpret_cast<f32x4*>(orow[k] + (size_t)s * 32) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }

  // per-lane byte offsets of this lane's 16 B in each of the 4 DMA instructions of a (step, piece)
  uint32_t koff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 8 * i + (lane >> 3);  // key row of the tile; the lane lands at position lane & 7 and fetches chunk pos ^ ksw
    koff[i] = (uint32_t)(kr * 128 + (((lane & 7) ^ ksw(kr)) << 4));
  }
  const uint32_t stage0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * (XS_STAGES * STAGE);
  // stage sg (wave-uniform, 0 or 1) of this wave
  auto issue_k = [&](int sg, const char* kbh, int step) { xa_issue_k<S, XA_TILE>(stage0 + sg * STAGE, kbh, bank_pstride, step, koff); };
  p16x8 kf[S][2][2];
  auto read_k = [&](int sg) { xa_read_k<S, XA_TILE>(stage + sg * STAGE, c, g, kf); };

  // ordinary loads (query fragments, key bits) are retired here: the waits of the sweeps see DMA instructions, the loads of the old
  // values and stores only
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int pc = 0; pc < S; ++pc)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd) asm volatile("" : "+v"(qf[r][pc][nt][kd]));

  // Two stages per wave, so two tiles fly at once.  A wave with two heads keeps head r's tile of the current step in stage r and
  // re-fills a stage with the NEXT step's tile of the same head as soon as its fragments are in registers; a wave with one head
  // alternates the stages step by step and re-fills with the step after the next.
  //
  // sweep 1: (max, sum of exp) per row of every head of this wave, online.  Only DMA instructions are in flight here, so the waits
  // are counted: all but the youngest tile's 4 S instructions, or all when no younger tile was issued.
  float m[NR][NT], l[NR][NT], inv[NR][NT];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      m[r][nt] = GRAM_FMIN;
      l[r][nt] = 0.f;
    }
  auto land = [&](bool younger) {  // the oldest tile in flight has landed
    if (younger) wait_vm<4 * S>();
    else wait_vm<0>();
  };
  auto online = [&](auto rc, uint32_t kbits) {
    constexpr int r = decltype(rc)::value;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      f32x4 s[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) s[t] = xa_scores(kf, qf[r], nt, t, kbits);
      float alpha;
      const float mn = xa_row_max(s, m[r][nt], alpha);
      float ps = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) ps += __expf(s[t][j] - mn);
      l[r][nt] = xa_l_update(l[r][nt], alpha, ps);
    }
  };
  {
    rewind();
    int cur = next(), nxt = next(), p = 0;
    if (cur < nsteps) {
      issue_k(0, kb[0], cur);
      if (has1) issue_k(1, kb[NR - 1], cur);
      else if (nxt < nsteps) issue_k(1, kb[0], nxt);
    }
    while (cur < nsteps) {
      const int nn = next();  // the step after the next
      const uint32_t kbits = step_word(cur) >> (8 * g);
      if (has1) {
        land(true);  // (younger: this step's tile of the second head)
        read_k(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the fragments are in registers before their tiles are re-filled
        if (nxt < nsteps) issue_k(0, kb[0], nxt);
        online(std::integral_constant<int, 0>{}, kbits);
        land(nxt < nsteps);
        read_k(1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (nxt < nsteps) issue_k(1, kb[NR - 1], nxt);
        online(std::integral_constant<int, NR - 1>{}, kbits);
      } else {
        land(nxt < nsteps);
        read_k(p);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (nn < nsteps) issue_k(p, kb[0], nn);
        online(std::integral_constant<int, 0>{}, kbits);
        p ^= 1;
      }
      cur = nxt;
      nxt = nn;
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float lt = l[r][nt];
      lt += __shfl_xor(lt, 16, 64);
      lt += __shfl_xor(lt, 32, 64);
      inv[r][nt] = 1.f / lt;
    }

  // sweep 2: the waves walk the valid steps together; per (step, round) the same scores again, normalised, through the exchange
  // slots into the reducers' registers.  Every wave runs every barrier: the walk is the user's, the same in all of them.
  // The stages as in sweep 1.  The counter also holds the step's loads and stores here, so the one wait per step is vmcnt(0), at the
  // step's top: every tile issued a step ago has landed (a wave with two heads: both of this step's).
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (sweep 1's last fragments are in registers)
  rewind();
  int cur = next(), nxt = next(), p = 0;
  if (cur < nsteps) {
    issue_k(0, kb[0], cur);
    if (has1) issue_k(1, kb[NR - 1], cur);
    else if (nxt < nsteps) issue_k(1, kb[0], nxt);
  }
  while (cur < nsteps) {
    const int nn = next();  // the step after the next
    const uint32_t kbits = step_word(cur) >> (8 * g);
    f32x4 red[NK], old[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) red[k] = old[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (r == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this step's K tiles have landed (and the last step's stores)
        read_k(has1 ? 0 : p);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the fragments are in registers before their tiles are re-filled
        if (has1) {
          if (nxt < nsteps) issue_k(0, kb[0], nxt);
        } else {
          if (nn < nsteps) issue_k(p, kb[0], nn);
          p ^= 1;
        }
      } else if (has1) {
        read_k(1);  // (landed at the step's top)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (nxt < nsteps) issue_k(1, kb[NR - 1], nxt);
      }
      if (r == NR - 1 && !first) {  // the old values fly during the arithmetic
#pragma unroll
        for (int k = 0; k < NK; ++k)
          if (orow[k]) old[k] = *reinterpret_cast<const f32x4*>(orow[k] + (size_t)cur * 32);
      }
      if (r == 0 || has1) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const f32x4 s = xa_scores(kf, qf[r], nt, t, kbits);
            f32x4 p;
#pragma unroll
            for (int j = 0; j < 4; ++j) p[j] = __expf(s[j] - m[r][nt]) * inv[r][nt];
            *reinterpret_cast<f32x4*>(slots + wave * XS_SLOT + xs_slot_off(16 * nt + c, 2 * g + t)) = p;
          }
      }
      gram_sync();  // the round's slots are written
      const int cnt = H - XS_MAXW * r < XS_MAXW ? H - XS_MAXW * r : XS_MAXW;
#pragma unroll
      for (int k = 0; k < NK; ++k)
        if (orow[k])
          for (int hh = 0; hh < cnt; ++hh) red[k] += *reinterpret_cast<const f32x4*>(slots + hh * XS_SLOT + ooff[k]);
      if (r == NR - 1) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
          if (orow[k]) {
            if (!first) red[k] += old[k];
            *reinterpret_cast<f32x4*>(orow[k] + (size_t)cur * 32) = red[k];
          }
      }
      gram_sync();  // the slots are free again
    }
    cur = nxt;
    nxt = nn;
  }
}

inline bool xs_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

template <int S, int NR>
int xs_launch(const void* q, const void* k_layer, float* acc, int B, int Q, int H, int Sk, long q_ps, long bank_ps,
              const uint32_t* key_bits, int first, unsigned tiles, hipStream_t st) {
  const int W = H < XS_MAXW ? H : XS_MAXW;
  const int smem = W * (XS_STAGES * S * XA_TILE + XS_SLOT);
  static_assert(XS_MAXW * (XS_STAGES * GRAM_MAX_PIECES * XA_TILE + XS_SLOT) <= 160 * 1024, "the stages and the slots do not fit the LDS");
  static bool attr_set = false;
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_token_scores_kernel<S, NR>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             XS_MAXW * (XS_STAGES * S * XA_TILE + XS_SLOT));
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  hipLaunchKernelGGL((cross_attn_token_scores_kernel<S, NR>), dim3(tiles, B), dim3(64 * W), smem, st, (const p16*)q, (const p16*)k_layer,
                     acc, Q, H, Sk, q_ps, bank_ps, key_bits, first);
  GRAM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int gram_cross_attn_token_scores_split(const void* q, const void* k_layer, float* acc, int B, int Q, int H, int S, int pieces,
                                                  int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, int first,
                                                  void* stream) {
  if (!q || !k_layer || !acc || !key_bits || B < 1 || B > 65535 || Q < 1 || H < 1 || H > XS_MAX_HEADS || S < 32 || (S & 31) ||
      S > GRAM_MAX_LONG_FUSED_LEN || pieces < 1 || pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && (q_pstride < (int64_t)B * Q * H * 64 || bank_pstride < (int64_t)H * S * 64 || (q_pstride & 7) || (bank_pstride & 7)))
    return GRAM_E_ARG;
  if (xs_misaligned(q) || xs_misaligned(k_layer) || xs_misaligned(acc) || xs_misaligned(key_bits)) return GRAM_E_ARG;
  const int64_t tiles = ((int64_t)Q + XS_ROWS - 1) / XS_ROWS;
  if (tiles > 65535) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  // K twice per row tile, every piece; acc written (and read back unless first)
  gram_prof::Scope prof(GRAM_K_CROSS_ATTN, st,
                        4.0 * B * H * S * 64 * pieces * (double)tiles + 4.0 * B * Q * S * (first ? 1 : 2));
  const long qp = (long)q_pstride, bp = (long)bank_pstride;
  const unsigned nt = (unsigned)tiles;
  const int ff = first ? 1 : 0;
  if (pieces == 2)
    return H > XS_MAXW ? xs_launch<2, 2>(q, k_layer, acc, B, Q, H, S, qp, bp, key_bits, ff, nt, st)
                       : xs_launch<2, 1>(q, k_layer, acc, B, Q, H, S, qp, bp, key_bits, ff, nt, st);
  return H > XS_MAXW ? xs_launch<1, 2>(q, k_layer, acc, B, Q, H, S, qp, bp, key_bits, ff, nt, st)
                     : xs_launch<1, 1>(q, k_layer, acc, B, Q, H, S, qp, bp, key_bits, ff, nt, st);
}
