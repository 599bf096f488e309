// step_dev.h -- the pieces of the search step that more than one file's kernels are made of: the step's operands and per-user tables,
// the candidate key, the bitonic top-P selection and the advance of sequences / ancestor table / per-row state.  beam.hip (beam and
// group beam search) and sbs.hip (stochastic beam search) include this one definition, so a selection is the same function, and
// the same bits, in both.
#pragma once

#include "common.h"
#include "trie_dev.h"

namespace {

// the step's operands (the kernels' parameters, handed on by reference)
struct StepArgs {
  const gram_beam_state_t& st;
  const gram_trie_t& tr;
  const float* __restrict__ logits;
  const float* __restrict__ lse;
  int V, cur_len, rows_per_user;
  const p16* __restrict__ hd;
  const p16* __restrict__ emb;
  int d;
  const int32_t* __restrict__ rowpos;
  int pieces;
  const float* __restrict__ emb32;
  const float* __restrict__ pre;
  int pre_stride;
  const gram_user_items_t* ui;  // per-user item filter (the FILT instantiations only; nullptr otherwise)
  float lam = 0.f;              // diversity penalty (the group step only)
  // per-item score biases (the BIAS instantiations only): the potentials f32 [rows][n_nodes], the stride between a
  // user's rows (0: one row shared by all users) and the K beams' own potentials in LDS (step_setup<true> fills them)
  const float* __restrict__ phi = nullptr;
  long long phi_stride = 0;
  const float* phi_par = nullptr;
  const gram_user_mask_t* um = nullptr;  // per-user item mask (the kFilterMask instantiations only; nullptr otherwise)
};

// The biased step's operand, the LAST element of a step kernel's trailing pack (behind the item filter, if any): the unbiased
// instantiations carry none of it.
struct StepBias {
  const float* phi;
  long long stride;
};
template <typename... UI>
constexpr bool biased() {
  static_assert(StepPack<UI...>::value, "a step kernel's trailing pack (trie_dev.h)");
  return (false || ... || std::is_same_v<UI, StepBias>);
}
__device__ __forceinline__ const gram_user_items_t* items_ptr(const StepBias&) { return nullptr; }
__device__ __forceinline__ const gram_user_items_t* items_ptr(const gram_user_items_t& u, const StepBias&) { return &u; }
__device__ __forceinline__ StepBias bias_of() { return {nullptr, 0}; }
__device__ __forceinline__ StepBias bias_of(const gram_user_items_t&) { return {nullptr, 0}; }
__device__ __forceinline__ StepBias bias_of(const gram_user_mask_t&) { return {nullptr, 0}; }
__device__ __forceinline__ StepBias bias_of(const StepBias& s) { return s; }
__device__ __forceinline__ StepBias bias_of(const gram_user_items_t&, const StepBias& s) { return s; }

// The edge term of a biased step: lp = logit - lse of the candidate that moves beam k of user b along `edge`, to
// which the difference of the potentials of the edge's two ends is added.  fp32, one rounding per operation (no contraction), as
// diversity() in beam.hip writes its term; the caller adds the beam score.
__device__ __forceinline__ float edge_bias(const StepArgs& a, int b, int k, int edge, float lp) {
  const float pc = a.phi[(size_t)b * a.phi_stride + a.tr.child_node[edge]];
  return __fadd_rn(lp, __fsub_rn(pc, a.phi_par[k]));
}

// (the per-user item filters -- filtered(), filter_kind(), items_ptr(), mask_ptr(), node_alive() -- are trie_dev.h's, shared with the
// sampling step).  FILT: kFilterNone (false), kFilterLists (true) or kFilterMask
template <int FILT>
__device__ __forceinline__ bool child_alive(const StepArgs& a, int b, int edge) {
  if constexpr (FILT == kFilterMask) return node_alive(*a.um, b, a.tr.child_node[edge]);
  else if constexpr (FILT != kFilterNone) return node_alive(*a.ui, b, a.tr.child_node[edge]);
  else return true;
}

// the step's small per-user tables (static LDS, ~3 KB)
struct StepShared {
  int pre[GRAM_MAX_BEAMS + 1];
  int C, NC, isdone;
  float sel_score[GRAM_MAX_BEAMS];
  int sel_tok[GRAM_MAX_BEAMS], sel_par[GRAM_MAX_BEAMS], sel_node[GRAM_MAX_BEAMS];
  int edge[2 * GRAM_MAX_BEAMS];
  int off[GRAM_MAX_BEAMS], cnt[GRAM_MAX_BEAMS], lr[GRAM_MAX_BEAMS];
};

__device__ __forceinline__ unsigned long long cand_key(float sc, int k, int V, int tok) {
  return ((unsigned long long)f2ord(sc) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)(k * V + tok));
}

// Only the best 2K candidates are looked at (topk(2K) in beam_search), in descending order: a bitonic TOP-P
// selection, P = the power of two >= 2K.  Sort every P-block (directions alternating, as in a full bitonic sort
// stopped at stage P), then halve the array round by round: a descending block followed by an ascending one is a
// bitonic sequence, so the elementwise maxima of the pair are a bitonic block that holds the pair's P largest keys;
// re-sort it (log2 P merge stages) and go on until one block is left.  ~3x fewer compare-exchanges than sorting
// all NC keys; keys are unique (flat index in the low word), so the result is the full sort's prefix: keys[0, min(NC, P)) descending.
// NC: a power of two, 64 <= NC <= MAXN.  Ends behind a barrier.
template <int NTHR, int MAXN>
__device__ __forceinline__ void top_p_select(unsigned long long* keys, int NC, int P, int tid) {
  const int top = NC < P ? NC : P;
  auto stage = [&](int n, int kk, int j) {
    for (int i = tid; i < n; i += NTHR) {
      const int ixj = i ^ j;
      if (ixj > i) {
        const unsigned long long a = keys[i], c = keys[ixj];
        const bool desc = (i & kk) == 0;
        if (desc ? (a < c) : (a > c)) {
          keys[i] = c;
          keys[ixj] = a;
        }
      }
    }
    gram_sync();
  };
  for (int kk = 2; kk <= top; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) stage(NC, kk, j);
  for (int n = NC; n > P; n >>= 1) {
    // blocks (2q, 2q+1) -> block q of the half-size array; every thread reads its pairs before anyone writes
    const int half = n >> 1;
    constexpr int NMX = MAXN / 2 / NTHR;  // half / NTHR <= MAXN / 2 / NTHR; statically indexed: stays in registers
    unsigned long long mx[NMX];
#pragma unroll
    for (int c = 0; c < NMX; ++c) {
      const int o = tid + c * NTHR;
      if (o < half) {
        const int q = o / P, i = o - q * P;
        const unsigned long long a = keys[(2 * q) * P + i], b2 = keys[(2 * q + 1) * P + i];
        mx[c] = a > b2 ? a : b2;
      }
    }
    gram_sync();
#pragma unroll
    for (int c = 0; c < NMX; ++c) {
      const int o = tid + c * NTHR;
      if (o < half) keys[o] = mx[c];
    }
    gram_sync();
    for (int j = P >> 1; j > 0; j >>= 1) stage(half, P, j);  // bitonic blocks -> sorted, directions alternating again
  }
}

// advance sequences / ancestor table / per-row state of all K rows from sel_* (read old -> LDS -> write)
template <int NTHR>
__device__ __forceinline__ void step_advance(const StepArgs& a, const StepShared& sh, int* new_seq, int* new_anc, int b, int tid) {
  const gram_beam_state_t& st = a.st;
  const int K = st.K, T = st.Tmax, R = st.B * K, cur_len = a.cur_len;
  const int row0 = b * K;
  const int t = cur_len - 1;  // decode step whose K/V were just written
  for (int idx = tid; idx < K * T; idx += NTHR) {
    const int j = idx / T, p = idx - j * T;
    int v = 0;
    if (p < cur_len) v = st.seq[(size_t)(row0 + sh.sel_par[j]) * T + p];
    else if (p == cur_len) v = sh.sel_tok[j];
    new_seq[idx] = v;
  }
  for (int idx = tid; idx < T * K; idx += NTHR) {
    const int p = idx / K, j = idx - p * K;
    int v;
    if (p < t) v = st.anc[(size_t)p * R + row0 + sh.sel_par[j]];
    else if (p == t) v = a.rows_per_user == 1 ? b : row0 + sh.sel_par[j];  // compact step: slot t holds one row per user
    else v = row0 + j;
    new_anc[idx] = v;
  }
  gram_sync();
  for (int idx = tid; idx < K * T; idx += NTHR) st.seq[(size_t)row0 * T + idx] = new_seq[idx];
  for (int idx = tid; idx < T * K; idx += NTHR) {
    const int p = idx / K, j = idx - p * K;
    st.anc[(size_t)p * R + row0 + j] = new_anc[idx];
  }
  if (tid < K) {
    st.beam_scores[row0 + tid] = sh.sel_score[tid];
    st.tokens[row0 + tid] = sh.sel_tok[tid];
    st.node[row0 + tid] = sh.sel_node[tid];
  }
}

}  // namespace
