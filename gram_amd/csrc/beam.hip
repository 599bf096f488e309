// beam.hip -- Trie-constrained beam search state machine on the device.
//
// Replaces, per decode step and per user (reference call site gram.py:93-99, kwargs
// single_runner_gram.py:641-651; third-party transformers==4.26.0 semantics, restated in
// oracle/gram_oracle.py::beam_search):
//   log_softmax                      -> logits[tok] - lse[row]            (lse from rowops.hip)
//   PrefixConstrainedLogitsProcessor -> children of the beam's Trie node (flat CSR in HBM);
//                                       the per-beam Python callback of generation_trie.py:89-95
//                                       (one D2H sync per beam per step) disappears
//   + beam_scores, topk(2K) over K*V -> bitonic sort in LDS of the <= K*max_fanout finite
//                                       candidates (64-bit keys: orderable score | ~flat index,
//                                       so ties resolve to the lower flat index) + -inf fillers;
//                                       more candidates than the LDS holds stream through a fixed key
//                                       array, the best so far carried along (beam_step_chunked_kernel)
//   BeamSearchScorer.process         -> one thread walks the 2K ranked candidates
//   input_ids gather / _reorder_cache-> sequences and the self-attention ancestor table are
//                                       advanced in place; K/V caches are never moved
// One workgroup per user; users are independent, so this shards trivially.
#include <stdlib.h>

#include "common.h"
#include "prof.h"
#include "sparse_dot.h"
#include "step_dev.h"
#include "trie_dev.h"

namespace {

__device__ double norm_len(int len, float lp) {
  if (lp == 1.0f) return (double)len;
  if (lp == 0.0f) return 1.0;
  return pow((double)len, (double)lp);
}

// BeamHypotheses.add (list semantics: append, drop the minimum, later elements shift down)
__device__ void hyp_add(const gram_beam_state_t& st, int b, const int32_t* toks, int len, float sum_logprobs) {
  const int K = st.K, T = st.Tmax;
  double* hs = st.hyp_score + (size_t)b * (K + 1);
  int32_t* hl = st.hyp_len + (size_t)b * (K + 1);
  int32_t* ht = st.hyp_tok + (size_t)b * (K + 1) * T;
  int n = st.n_hyps[b];
  const double score = (double)sum_logprobs / norm_len(len, st.length_penalty);
  // a NaN would lose every comparison below (never kept once the heap is full, evicted first otherwise) and vanish silently; +inf cannot
  // be a sum of log-probabilities: both mean an activation left the range of the 16-bit pieces upstream (GRAM_E_NONFINITE)
  if (!(score < 1.0e300)) st.error[0] = 4;
  if (n < K || score > st.worst[b]) {
    hs[n] = score;
    hl[n] = len;
    for (int i = 0; i < len; ++i) ht[(size_t)n * T + i] = toks[i];
    ++n;
    if (n > K) {
      // sorted([(s, idx)]): minimum score, ties -> lowest index; worst = second smallest
      int imin = 0;
      for (int i = 1; i < n; ++i)
        if (hs[i] < hs[imin]) imin = i;
      double second = 1e300;
      bool have = false;
      for (int i = 0; i < n; ++i) {
        if (i == imin) continue;
        if (!have || hs[i] < second) { second = hs[i]; have = true; }
      }
      for (int i = imin; i + 1 < n; ++i) {
        hs[i] = hs[i + 1];
        hl[i] = hl[i + 1];
        for (int p = 0; p < T; ++p) ht[(size_t)i * T + p] = ht[(size_t)(i + 1) * T + p];
      }
      --n;
      st.worst[b] = second;
    } else {
      st.worst[b] = score < st.worst[b] ? score : st.worst[b];
    }
    st.n_hyps[b] = n;
  }
}

// gs: beams per group (K for the plain search: one group).  The first beam of every group starts at 0, the others at -1e9
__global__ void beam_init_kernel(gram_beam_state_t st, gram_trie_t tr, int start, int gs) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int R = st.B * st.K;
  if (r == 0) st.error[0] = 0;
  if (r < st.B) {
    st.done[r] = 0;
    st.n_hyps[r] = 0;
    st.worst[r] = 1e9;
  }
  if (r >= R) return;
  st.tokens[r] = start;
  st.beam_scores[r] = ((r % st.K) % gs) == 0 ? 0.f : -1e9f;
  for (int p = 0; p < st.Tmax; ++p) {
    st.seq[(size_t)r * st.Tmax + p] = p == 0 ? start : 0;
    st.anc[(size_t)p * R + r] = r;
  }
  const int e = find_child(tr, 0, start);
  st.node[r] = e < 0 ? -1 : tr.child_node[e];
}

// ---- the search step, in pieces shared by its two kernels: beam_step_kernel (every candidate of a user in LDS at once) and
// beam_step_chunked_kernel (candidates streamed through a fixed key array).  Both build the same keys with the same arithmetic, run
// the same top-P selection and finish with the same code, so they return the same bits wherever both can run.  (Their operands and
// tables, the candidate key, the selection and the advance are step_dev.h's, shared with the stochastic beam search of sbs.hip.)

// The Hamming diversity term of a group step: lp = logit - lse of a candidate with token tok, sel_tok[0, nprev) the
// tokens the earlier groups of this user chose in this step.  fp32, one rounding per operation (no contraction into an FMA): the
// bits of HF's `scores -= diversity_penalty * bincount`; nothing is subtracted where that would subtract 0.
__device__ __forceinline__ float diversity(const StepArgs& a, const StepShared& sh, int nprev, int tok, float lp) {
  int c = 0;
  for (int i = 0; i < nprev; ++i) c += sh.sel_tok[i] == tok ? 1 : 0;
  return (a.lam == 0.f || c == 0) ? lp : __fsub_rn(lp, __fmul_rn(a.lam, (float)c));
}

// per beam: first child edge, child count, hidden-state row; then the prefix sums of the counts: candidate ci of the user is child
// ci - pre[k] of beam k, pre[k] <= ci < pre[k + 1].  nc_max > 0: more candidates than that is error 2 (the one-shot kernel's key array)
// BIAS: the potential of every beam's own node goes to par[k] (0 for a beam that left the Trie: it has no candidates)
template <bool BIAS = false>
__device__ __forceinline__ void step_setup(const StepArgs& a, StepShared& sh, int b, int tid, int nc_max, float* par = nullptr) {
  const gram_beam_state_t& st = a.st;
  const gram_trie_t& tr = a.tr;
  const int K = st.K, row0 = b * K;
  // K threads at once (one thread walking the K beams was K dependent node -> offsets round trips, ~20 us of a 100-us step at K = 20)
  if (tid < K) {
    const int nd = st.node[row0 + tid];
    const int done = st.done[b];
    int o0 = 0, cnt = 0;
    if (!done && nd >= 0) {
      o0 = tr.child_off[nd];
      cnt = tr.child_off[nd + 1] - o0;
    }
    sh.off[tid] = o0;
    sh.cnt[tid] = cnt;
    sh.lr[tid] = a.rowpos ? a.rowpos[row0 + tid] : row0 + tid;  // live-row step: hidden/lse are indexed by compact row
    if constexpr (BIAS) par[tid] = nd >= 0 ? a.phi[(size_t)b * a.phi_stride + nd] : 0.f;
    if (tid == 0) sh.isdone = done;
  }
  gram_sync();
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < K; ++k) {
      sh.pre[k] = acc;
      acc += sh.cnt[k];
    }
    sh.pre[K] = acc;
    sh.C = acc;
    int nc = 64;
    while (nc < acc && nc < (1 << 30)) nc <<= 1;
    sh.NC = nc;
    if (nc_max > 0 && acc > nc_max) { st.error[0] = 2; sh.C = 0; sh.NC = 64; sh.pre[K] = 0; }
  }
  gram_sync();
}

// SPARSE mode: the lm_head GEMM stored only the softmax partials (lse); the logits of the allowed tokens are recomputed here as
// h[row] . E[tok] (bf16 operands, fp32 accumulate; 8 lanes per candidate, 16-byte loads).  The [rows][V] logits tensor (5 GB per step
// at B = 2048) is never written.  Candidates [c0, c0 + n) of the user's list go to kw[0, n) as keys; shared0 (step 0: all K beams sit
// on the same node and the same row): children [c0, c0 + n) of that node, their logits go to s_log[0, n) and shared0_keys makes the
// K keys of each.  The caller puts a barrier behind it.
// FILT: a candidate whose child node is not alive for the user gets the zero key ("nothing", below every real key) and no dot product;
// the shared step-0 row computes every child's logit and leaves the test to shared0_keys.
// GRP (the group step): the diversity term over the nprev tokens chosen so far goes between the log-probability and the beam score.
// BIAS (the biased step): the edge term (edge_bias, step_dev.h) goes there instead.
template <int NTHR, int FILT, bool GRP = false, bool BIAS = false>
__device__ __forceinline__ void sparse_window(const StepArgs& a, const StepShared& sh, unsigned long long* kw, float* s_log, int b, int tid,
                                              int c0, int n, bool shared0, int nprev = 0) {
  const gram_beam_state_t& st = a.st;
  const gram_trie_t& tr = a.tr;
  const int row0 = b * st.K, V = a.V;
  const int sub = tid & 7, grp = tid >> 3;
  // (beam, token) of every candidate first, all threads at once, parked in the candidate's key slot: the dot products below then
  // start from LDS instead of a node -> edge -> token chain of global loads per batch
  for (int i = tid; i < n; i += NTHR) {
    const int ci = c0 + i;
    int k = 0;
    if (!shared0)
      while (sh.pre[k + 1] <= ci) ++k;
    const int tok = tr.child_tok[sh.off[k] + (ci - sh.pre[k])];
    kw[i] = ((unsigned long long)(uint32_t)k << 32) | (unsigned long long)(uint32_t)tok;
    if constexpr (FILT != kFilterNone)
      if (!shared0 && !child_alive<FILT>(a, b, sh.off[k] + (ci - sh.pre[k]))) kw[i] |= 1ull << 63;  // (k <= 64: the bit is free)
  }
  gram_sync();
  auto dot = [&](bool act, int lr, int tok, int ci) -> float {
    if (a.pre) return act ? a.pre[(size_t)b * a.pre_stride + ci] : 0.f;  // (computed by sparse_logits_kernel: the same function, the same bits)
    return sparse_dot(act, lr, tok, sub, a.hd, a.emb, a.emb32, a.d, a.pieces);
  };
  // two candidates per 8-lane group and trip (NTHR / 4 per workgroup): their loads are independent and overlap
  constexpr int NG = NTHR / 8;
  for (int base = 0; base < n; base += 2 * NG) {
    int i2[2], k2[2], tok2[2], lr2[2];
    bool act2[2], dead2[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      i2[w] = base + NG * w + grp;
      act2[w] = i2[w] < n;
      unsigned long long kt = act2[w] ? kw[i2[w]] : 0ull;
      dead2[w] = false;
      if constexpr (FILT != kFilterNone) {
        dead2[w] = (kt >> 63) != 0;
        kt &= ~(1ull << 63);
      }
      k2[w] = (int)(kt >> 32);
      tok2[w] = (int)(kt & 0xffffffffull);
      lr2[w] = shared0 ? b : sh.lr[k2[w]];
    }
    float acc2[2];
#pragma unroll
    for (int w = 0; w < 2; ++w) acc2[w] = dot(act2[w] && !dead2[w], lr2[w], tok2[w], c0 + i2[w]);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
      if (act2[w] && sub == 0) {
        if (shared0) {
          s_log[i2[w]] = acc2[w];
        } else {
          float sc;
          if constexpr (GRP) sc = diversity(a, sh, nprev, tok2[w], acc2[w] - a.lse[lr2[w]]) + st.beam_scores[row0 + k2[w]];
          else if constexpr (BIAS)
            sc = dead2[w] ? 0.f
                          : __fadd_rn(edge_bias(a, b, k2[w], sh.off[k2[w]] + (c0 + i2[w] - sh.pre[k2[w]]), acc2[w] - a.lse[lr2[w]]),
                                      st.beam_scores[row0 + k2[w]]);
          else sc = (acc2[w] - a.lse[lr2[w]]) + st.beam_scores[row0 + k2[w]];
          kw[i2[w]] = dead2[w] ? 0ull : cand_key(sc, k2[w], V, tok2[w]);
        }
      }
    }
  }
}

// step 0's shared row: the keys of beams [k0, k0 + kg) x children [j0, j0 + nj) of the shared node, from the nj logits that
// sparse_window left in s_log: kw[(k - k0) * nj + (j - j0)].  (k0 = j0 = 0, kg = K, nj = the node's fan-out: the user's whole list
// in its flat-index order)
template <int NTHR, int FILT, bool GRP = false, bool BIAS = false>
__device__ __forceinline__ void shared0_keys(const StepArgs& a, const StepShared& sh, unsigned long long* kw, const float* s_log, int b,
                                             int tid, int j0, int nj, int k0, int kg, int nprev = 0) {
  const gram_beam_state_t& st = a.st;
  const gram_trie_t& tr = a.tr;
  const int row0 = b * st.K;
  const int cnt0 = sh.pre[1];
  const int off0 = cnt0 > 0 ? tr.child_off[st.node[row0]] : 0;
  for (int i = tid; i < kg * nj; i += NTHR) {
    const int kk = i / nj, jj = i - kk * nj;
    const int k = k0 + kk;
    const int tok = tr.child_tok[off0 + j0 + jj];
    float sc;
    if constexpr (GRP) sc = diversity(a, sh, nprev, tok, s_log[jj] - a.lse[b]) + st.beam_scores[row0 + k];
    else if constexpr (BIAS) sc = __fadd_rn(edge_bias(a, b, k, off0 + j0 + jj, s_log[jj] - a.lse[b]), st.beam_scores[row0 + k]);
    else sc = (s_log[jj] - a.lse[b]) + st.beam_scores[row0 + k];
    kw[i] = child_alive<FILT>(a, b, off0 + j0 + jj) ? cand_key(sc, k, a.V, tok) : 0ull;
  }
}

// DENSE mode, gather: log_softmax at the allowed tokens + running beam score.  Candidates [c0, c0 + n) -> kw[0, n); kw[n, npad) = 0
template <int NTHR, int FILT, bool GRP = false, bool BIAS = false>
__device__ __forceinline__ void dense_window(const StepArgs& a, const StepShared& sh, unsigned long long* kw, int b, int tid, int c0, int n,
                                             int npad, int nprev = 0) {
  const gram_beam_state_t& st = a.st;
  const gram_trie_t& tr = a.tr;
  const int row0 = b * st.K, V = a.V;
  for (int i = tid; i < npad; i += NTHR) {
    unsigned long long key = 0ull;
    if (i < n) {
      const int ci = c0 + i;
      int k = 0;
      while (sh.pre[k + 1] <= ci) ++k;
      const int r = row0 + k;
      const int e = tr.child_off[st.node[r]] + (ci - sh.pre[k]);
      const int tok = tr.child_tok[e];
      // rows_per_user == 1: the K beams of a user share one logits row (step 0: identical beams)
      const int lr = a.rows_per_user == 1 ? b : r;
      float sc;
      if constexpr (GRP) sc = diversity(a, sh, nprev, tok, a.logits[(size_t)lr * V + tok] - a.lse[lr]) + st.beam_scores[r];
      else if constexpr (BIAS) sc = __fadd_rn(edge_bias(a, b, k, e, a.logits[(size_t)lr * V + tok] - a.lse[lr]), st.beam_scores[r]);
      else sc = (a.logits[(size_t)lr * V + tok] - a.lse[lr]) + st.beam_scores[r];
      key = child_alive<FILT>(a, b, e) ? cand_key(sc, k, V, tok) : 0ull;
    }
    kw[i] = key;
  }
}

// Non-finite arithmetic is flagged HERE, at its source (GRAM_E_NONFINITE), not at the returned scores: a NaN candidate sorts above
// +inf (positive NaN) or below -inf (negative NaN) and would be picked first or never, a row whose normaliser is +inf / NaN turns
// all its candidates into -inf / NaN -- either way the search would go on and return an ordinary-looking ranking without them.
// -inf candidates are legitimate (HF's -inf refills of finished beams).  Every candidate's key passes through here before the
// selection can drop it.  FILT: the zero key of a dead candidate is no score (a real key's low word is never 0) and is passed over.
template <int NTHR, int FILT>
__device__ __forceinline__ void flag_nonfinite_keys(const StepArgs& a, const unsigned long long* kw, int n, int tid) {
  for (int i = tid; i < n; i += NTHR) {
    if constexpr (FILT != kFilterNone)
      if (kw[i] == 0ull) continue;
    const uint32_t o = (uint32_t)(kw[i] >> 32);
    if (o >= 0xff800000u || o < 0x007fffffu) a.st.error[0] = 4;  // f2ord(+inf) = 0xff800000, f2ord(-inf) = 0x007fffff
  }
}
__device__ __forceinline__ void flag_nonfinite_lse(const StepArgs& a, const StepShared& sh, int b, int tid) {
  if (tid < a.st.K && sh.cnt[tid] > 0) {
    const int lr = a.rows_per_user == 1 ? b : sh.lr[tid];
    if (lr >= 0 && !(fabsf(a.lse[lr]) < 3.0e38f)) a.st.error[0] = 4;
  }
}

// Everything behind the selection: keys[0, min(C, 2K)) hold the user's best candidates in descending order (C = sh.C of them in
// all).  BeamSearchScorer.process on one thread, then the sequences / ancestor table / per-row state are advanced through
// new_seq [K][Tmax] / new_anc [Tmax][K] (LDS).  FILT: the zero keys of dead candidates sort last, so the ranking ends at the first
// one, and a filler token is any token that is not an ALIVE child of beam 0's node.
//
// It comes in two halves.  step_rank is the scorer for beams [k0, k0 + kn) of the user -- all K of the plain search, one group of a
// group search: keys[0, min(C, 2 kn)) are THEIR best candidates (C of them in all), their slots of sel_* are filled,
// "beam 0" of the filler rule is beam k0, EOS candidates go to the user's one heap of capacity K and the done test runs against it.
// step_advance then moves all K rows at once.
template <int NTHR, int FILT>
__device__ __forceinline__ void step_rank(const StepArgs& a, StepShared& sh, const unsigned long long* keys, int b, int tid, int k0, int kn,
                                          int C) {
  const gram_beam_state_t& st = a.st;
  const gram_trie_t& tr = a.tr;
  const int K = st.K, T = st.Tmax, V = a.V, cur_len = a.cur_len;
  const int row0 = b * K;
  const bool isdone = sh.isdone != 0;

  // the Trie edge of every ranked candidate, looked up by 2K threads at once (one binary search each; the walk below ran them one
  // after the other: up to K dependent searches of ~6 global loads each on a single thread)
  if (!isdone) {
    for (int rank = tid; rank < 2 * kn; rank += NTHR) {
      int e = -1;
      if (rank < C && (FILT == kFilterNone || keys[rank] != 0ull)) {
        const unsigned long long key = keys[rank];
        const uint32_t flat = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
        const int k = (int)(flat / (uint32_t)V), tok = (int)(flat % (uint32_t)V);
        if (tok != st.eos) e = find_child(tr, st.node[row0 + k], tok);
      }
      sh.edge[rank] = e;
    }
    gram_sync();
  }

  if (tid == 0) {
    if (isdone) {
      // BeamSearchScorer.process pads a finished user
      for (int j = k0; j < k0 + kn; ++j) {
        sh.sel_score[j] = 0.f;
        sh.sel_tok[j] = st.pad;
        sh.sel_par[j] = j;
        sh.sel_node[j] = -1;
      }
    } else {
      int j = 0;
      int ftok = 0;  // next filler token candidate (beam k0, -inf), ascending flat index
      const int node0 = st.node[row0 + k0];
      float best = -INFINITY;
      for (int rank = 0; rank < 2 * kn && j < kn; ++rank) {
        float sc;
        int k, tok;
        const bool real = rank < C && (FILT == kFilterNone || keys[rank] != 0ull);
        if (real) {
          const unsigned long long key = keys[rank];
          sc = ord2f((uint32_t)(key >> 32));
          const uint32_t flat = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
          k = (int)(flat / (uint32_t)V);
          tok = (int)(flat % (uint32_t)V);
        } else {
          if constexpr (FILT != kFilterNone) {
            for (; ftok < V; ++ftok) {
              const int fe = find_child(tr, node0, ftok);
              if (fe < 0 || !child_alive<FILT>(a, b, fe)) break;
            }
          } else {
            while (ftok < V && find_child(tr, node0, ftok) >= 0) ++ftok;
          }
          sc = -INFINITY;
          k = k0;
          tok = ftok++;
        }
        if (rank == 0) best = sc;
        if (tok == st.eos) {
          if (rank >= kn) continue;
          hyp_add(st, b, st.seq + (size_t)(row0 + k) * T, cur_len, sc);
        } else {
          const int e = real ? sh.edge[rank] : -1;
          sh.sel_score[k0 + j] = sc;
          sh.sel_tok[k0 + j] = tok;
          sh.sel_par[k0 + j] = k;
          sh.sel_node[k0 + j] = e < 0 ? -1 : tr.child_node[e];
          ++j;
        }
      }
      if (j < kn) {
        st.error[0] = 1;  // HF raises ValueError here
        for (; j < kn; ++j) { sh.sel_score[k0 + j] = -INFINITY; sh.sel_tok[k0 + j] = st.pad; sh.sel_par[k0 + j] = k0; sh.sel_node[k0 + j] = -1; }
      }
      // BeamHypotheses.is_done(best_sum_logprobs = next_scores.max(), cur_len)
      if (st.n_hyps[b] >= K) {
        const double cur = (double)best / norm_len(cur_len, st.length_penalty);
        if (st.worst[b] >= cur) st.done[b] = 1;
      }
    }
  }
  gram_sync();
}

// the plain search: one group of K beams over the user's C = sh.C candidates
template <int NTHR, int FILT>
__device__ __forceinline__ void step_finish(const StepArgs& a, StepShared& sh, const unsigned long long* keys, int* new_seq, int* new_anc,
                                            int b, int tid) {
  step_rank<NTHR, FILT>(a, sh, keys, b, tid, 0, a.st.K, sh.C);
  step_advance<NTHR>(a, sh, new_seq, new_anc, b, tid);
}

constexpr int kOneShotMaxKeys = 16384;  // K * max_fanout the one-shot kernel takes (128 KB of keys)

// ONE-SHOT form: all of a user's candidates in LDS at once (K * max_fanout <= 16 384 and the LDS sum below within the CU's 160 KB).
// NTHR threads per workgroup (= per user): 256 for batches that fill the chip with workgroups; 1 024 for small batches, where one user's
// sparse logits (a trip computes NTHR / 4 candidates' dot products, each on its 8 lanes) and sort stages are the step's latency.
// UI: the per-user item filter (the lists or the mask: filter_kind(), trie_dev.h) and / or the biased step's potentials (StepBias,
// step_dev.h: BIAS)
template <int NTHR, typename... UI>
__global__ __launch_bounds__(NTHR) void beam_step_kernel(gram_beam_state_t st, gram_trie_t tr, const float* __restrict__ logits,
                                                        const float* __restrict__ lse, int V, int cur_len, int nc_max, int rows_per_user,
                                                        const p16* __restrict__ hd, const p16* __restrict__ emb, int d,
                                                        const int32_t* __restrict__ rowpos, int pieces,
                                                        const float* __restrict__ emb32, const float* __restrict__ pre, UI... ui) {
  constexpr int FILT = filter_kind<UI...>();
  constexpr bool BIAS = biased<UI...>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [nc_max]
  float* s_log = reinterpret_cast<float*>(keys + nc_max);                   // [max_fanout, rounded up to 4] shared step-0 logits
  // [K][Tmax] + [Tmax][K]: the advanced sequences / ancestor table on their way back to HBM (sized by the call, not by the maxima)
  int* new_seq = reinterpret_cast<int*>(smem + (size_t)nc_max * 8 + ((size_t)tr.max_fanout * 4 + 15) / 16 * 16);
  int* new_anc = new_seq + st.K * st.Tmax;
  __shared__ StepShared sh;
  float* par = nullptr;  // BIAS: the potentials of the K beams' own nodes
  if constexpr (BIAS) {
    __shared__ float s_par[GRAM_MAX_BEAMS];
    par = s_par;
  }
  const StepArgs a{st, tr, logits, lse, V, cur_len, rows_per_user, hd, emb, d, rowpos, pieces, emb32, pre, nc_max, items_ptr(ui...),
                   0.f, bias_of(ui...).phi, bias_of(ui...).stride, par, mask_ptr(ui...)};

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = st.K;
  step_setup<BIAS>(a, sh, b, tid, nc_max, par);
  const int C = sh.C, NC = sh.NC;
  const bool isdone = sh.isdone != 0;

  if (!isdone && logits == nullptr) {
    for (int ci = C + tid; ci < NC; ci += NTHR) keys[ci] = 0ull;
    const bool shared0 = rows_per_user == 1;
    sparse_window<NTHR, FILT, false, BIAS>(a, sh, keys, s_log, b, tid, 0, shared0 ? sh.pre[1] : C, shared0);
    if (shared0) {
      gram_sync();
      shared0_keys<NTHR, FILT, false, BIAS>(a, sh, keys, s_log, b, tid, 0, sh.pre[1], 0, K);
    }
    gram_sync();
  }
  if (!isdone && logits != nullptr) {
    dense_window<NTHR, FILT, false, BIAS>(a, sh, keys, b, tid, 0, C, NC);
    gram_sync();
  }
  if (!isdone) {
    flag_nonfinite_keys<NTHR, FILT>(a, keys, C, tid);
    flag_nonfinite_lse(a, sh, b, tid);
    int P = 64;
    while (P < 2 * K) P <<= 1;
    top_p_select<NTHR, kOneShotMaxKeys>(keys, NC, P, tid);
  }
  step_finish<NTHR, FILT>(a, sh, keys, new_seq, new_anc, b, tid);
}
// CHUNKED form: any fan-out.  The candidates stream through a fixed key array: keys[0, P) carry the best P keys so far (descending;
// zero keys -- below every real key, whose low word is never 0 -- while fewer have been seen), keys[P, P + n) take the next n <= cap
// candidates, the same top-P selection runs over the power of two >= P + n, and so on until the list is exhausted.  The keys are
// unique and the order total, so what is carried is always the P best of everything seen: at the end keys[0, 2K) are the full
// sort's prefix, the one-shot kernel's bits.  The order in which candidates arrive is free; step 0's shared row uses that: it takes
// the shared node's children kChunkLog at a time (their logits in s_log) and makes the keys of as many beams per round as fit.
//
// LDS, independent of max_fanout:   keys   [kChunkKeys] u64     32 KB
//                                   s_log  [kChunkLog]  f32      8 KB
//                                   new_seq / new_anc   2 * K * Tmax * 4 B (3.8 KB at K = 20, Tmax = 12; 64 KB at K = 64, Tmax = 64)
//                                   static tables                ~3 KB
// 4 096 keys: at the runners' shapes (K = 20) a 256-thread workgroup takes ~47 KB, so three of them (12 wavefronts) share a CU's
// 160 KB; 8 192 keys (~83 KB) would leave one workgroup, 4 wavefronts, per CU -- and the one-shot kernel at K * fan-out > 4 096 is
// there already -- while 2 048 keys would give 6 workgroups but twice the rounds, each with its barriers and its carried block
// (P of the array: 1/32 at P = 128, kChunkKeys = 4 096).  The selection's compare-exchange count per candidate does not depend on
// the array size (log^2 P block stages + the halvings), so the array only has to be large enough to keep the rounds few.  The
// worst case, K = 64 and Tmax = 64, is 32 + 8 + 64 + 3 = 107 KB: one workgroup per CU, and it fits.
constexpr int kChunkKeys = 4096;
constexpr int kChunkLog = 2048;

// One merge of the streamed forms, plain and group: kw = keys + P holds n fresh keys (all threads behind a barrier or not: one
// follows the padding); keys[0, P) end up the best P of the carried block and the fresh ones.  GRP: the group form has always put
// a barrier between flag_nonfinite_keys and top_p_select, here and in its one-shot path, and the plain form none; unjudged.
template <int NTHR, int FILT, bool GRP, int MAXN>
__device__ __forceinline__ void merge_round(const StepArgs& a, unsigned long long* keys, unsigned long long* kw, int P, int n, int tid) {
  int na = 2 * P;  // the power of two >= P + n
  while (na < P + n) na <<= 1;
  for (int i = n + tid; i < na - P; i += NTHR) kw[i] = 0ull;
  gram_sync();
  flag_nonfinite_keys<NTHR, FILT>(a, kw, n, tid);
  if constexpr (GRP) gram_sync();
  top_p_select<NTHR, MAXN>(keys, na, P, tid);
}

// (UI: as in beam_step_kernel)
template <int NTHR, typename... UI>
__global__ __launch_bounds__(NTHR) void beam_step_chunked_kernel(gram_beam_state_t st, gram_trie_t tr, const float* __restrict__ logits,
                                                                const float* __restrict__ lse, int V, int cur_len, int cap,
                                                                int rows_per_user, const p16* __restrict__ hd,
                                                                const p16* __restrict__ emb, int d, const int32_t* __restrict__ rowpos,
                                                                int pieces, const float* __restrict__ emb32, UI... ui) {
  constexpr int FILT = filter_kind<UI...>();
  constexpr bool BIAS = biased<UI...>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [kChunkKeys]
  float* s_log = reinterpret_cast<float*>(keys + kChunkKeys);              // [kChunkLog]
  int* new_seq = reinterpret_cast<int*>(s_log + kChunkLog);                // [K][Tmax] + [Tmax][K], as in the one-shot kernel
  int* new_anc = new_seq + st.K * st.Tmax;
  __shared__ StepShared sh;
  float* par = nullptr;  // (as in the one-shot kernel)
  if constexpr (BIAS) {
    __shared__ float s_par[GRAM_MAX_BEAMS];
    par = s_par;
  }
  const StepArgs a{st, tr, logits, lse, V, cur_len, rows_per_user, hd, emb, d, rowpos, pieces, emb32, nullptr, 0, items_ptr(ui...),
                   0.f, bias_of(ui...).phi, bias_of(ui...).stride, par, mask_ptr(ui...)};

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = st.K;
  step_setup<BIAS>(a, sh, b, tid, 0, par);
  const int C = sh.C;
  const bool isdone = sh.isdone != 0;

  if (!isdone) {
    flag_nonfinite_lse(a, sh, b, tid);
    int P = 64;
    while (P < 2 * K) P <<= 1;
    if (cap > kChunkKeys - P) cap = kChunkKeys - P;  // (the launcher's job; a wrong value must not reach past the array)
    if (cap < 1) cap = 1;
    unsigned long long* kw = keys + P;
    for (int i = tid; i < P; i += NTHR) keys[i] = 0ull;  // nothing carried yet
    auto merge = [&](int n) { merge_round<NTHR, FILT, false, kChunkKeys>(a, keys, kw, P, n, tid); };
    if (logits != nullptr) {
      for (int c0 = 0; c0 < C; c0 += cap) {
        const int n = C - c0 < cap ? C - c0 : cap;
        dense_window<NTHR, FILT, false, BIAS>(a, sh, kw, b, tid, c0, n, n);
        merge(n);
      }
    } else if (rows_per_user != 1) {
      for (int c0 = 0; c0 < C; c0 += cap) {
        const int n = C - c0 < cap ? C - c0 : cap;
        sparse_window<NTHR, FILT, false, BIAS>(a, sh, kw, s_log, b, tid, c0, n, false);
        merge(n);
      }
    } else {
      const int cnt0 = sh.pre[1];
      const int njmax = cap < kChunkLog ? cap : kChunkLog;
      for (int j0 = 0; j0 < cnt0; j0 += njmax) {
        const int nj = cnt0 - j0 < njmax ? cnt0 - j0 : njmax;
        sparse_window<NTHR, FILT, false, BIAS>(a, sh, kw, s_log, b, tid, j0, nj, true);
        gram_sync();
        const int kgmax = cap / nj;  // >= 1
        for (int k0 = 0; k0 < K; k0 += kgmax) {
          const int kg = K - k0 < kgmax ? K - k0 : kgmax;
          shared0_keys<NTHR, FILT, false, BIAS>(a, sh, kw, s_log, b, tid, j0, nj, k0, kg);
          merge(kg * nj);
        }
      }
    }
  }
  step_finish<NTHR, FILT>(a, sh, keys, new_seq, new_anc, b, tid);
}
// GROUP form (HF group_beam_search + HammingDiversityLogitsProcessor): the K beams are G groups of gs = K / G, searched
// one after the other inside the step.  The workgroup of a user loops over the groups: group g's keys are built from ITS beams'
// candidates only -- a contiguous range [pre[g gs], pre[(g + 1) gs]) of the user's list, so the plain step's windows serve -- with
// the diversity term over the tokens groups 0..g-1 just chose (sel_tok[0, g gs), in LDS), then the same top-P selection (P >= 2 gs)
// and step_rank for the group's slots; a user that finishes at group g has its later groups padded in the same step.  All K rows
// advance together at the end.  Every candidate's logit is still computed once per step (step 0's shared row: once into s_log while
// it fits there), and nothing but the final state goes to HBM.
// CHUNKED = false: a group's candidates in LDS at once, keys [nkeys >= gs * max_fanout] and s_log [nlog >= max_fanout];
// CHUNKED = true: streamed through keys [kChunkKeys] (cap fresh ones per round) and s_log [kChunkLog], as beam_step_chunked_kernel.
// LDS: the plain kernels' sums with gs in K's place for the keys: one-shot 8 * nkeys + 4 * max_fanout + 8 * K * Tmax + ~3 KB
// (K = 20, G = 5, fan-out 255: 8 + 1 + 1.9 + 3 = 14 KB against the plain step's 72 KB), chunked 32 + 8 + 8 * K * Tmax / 1 024 + 3 KB.
template <int NTHR, bool CHUNKED, typename... UI>
__global__ __launch_bounds__(NTHR) void beam_group_step_kernel(gram_beam_state_t st, gram_trie_t tr, const float* __restrict__ logits,
                                                              const float* __restrict__ lse, int V, int cur_len, int nkeys, int nlog,
                                                              int cap, int rows_per_user, const p16* __restrict__ hd,
                                                              const p16* __restrict__ emb, int d, const int32_t* __restrict__ rowpos,
                                                              int pieces, const float* __restrict__ emb32, int G, float lam, UI... ui) {
  constexpr bool FILT = filtered<UI...>();
  constexpr int MAXN = CHUNKED ? kChunkKeys : kOneShotMaxKeys;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);  // [nkeys]
  float* s_log = reinterpret_cast<float*>(keys + nkeys);                   // [nlog] (a multiple of 4)
  int* new_seq = reinterpret_cast<int*>(s_log + nlog);                     // [K][Tmax] + [Tmax][K]
  int* new_anc = new_seq + st.K * st.Tmax;
  __shared__ StepShared sh;
  const StepArgs a{st, tr, logits, lse, V, cur_len, rows_per_user, hd, emb, d, rowpos, pieces, emb32, nullptr, 0, items_ptr(ui...), lam};

  const int b = blockIdx.x, tid = threadIdx.x;
  const int K = st.K, gs = K / G;
  step_setup(a, sh, b, tid, 0);
  if (!sh.isdone) flag_nonfinite_lse(a, sh, b, tid);
  int P = 64;
  while (P < 2 * gs) P <<= 1;
  if (nkeys > MAXN) nkeys = MAXN;  // (the launcher's job, as cap below)
  const bool shared0 = logits == nullptr && rows_per_user == 1;
  const int cnt0 = sh.pre[1];  // shared0: the fan-out of the one node every beam stands on
  bool have_log = false;       // shared0: s_log holds all cnt0 logits (uniform over the workgroup)

  for (int g = 0; g < G; ++g) {
    const int k0 = g * gs, nprev = k0;
    const int c0 = sh.pre[k0];
    int Cg = sh.pre[k0 + gs] - c0;
    if (!sh.isdone) {
      if constexpr (!CHUNKED) {
        if (Cg > nkeys || (shared0 && cnt0 > nlog)) {  // (a Trie wider than its max_fanout says: the plain step's error 2)
          if (tid == 0) st.error[0] = 2;
          Cg = 0;
        }
        int NC = 64;
        while (NC < Cg) NC <<= 1;
        for (int i = Cg + tid; i < NC; i += NTHR) keys[i] = 0ull;
        if (Cg > 0) {
          if (logits != nullptr) {
            dense_window<NTHR, FILT, true>(a, sh, keys, b, tid, c0, Cg, Cg, nprev);
          } else if (!shared0) {
            sparse_window<NTHR, FILT, true>(a, sh, keys, s_log, b, tid, c0, Cg, false, nprev);
          } else {
            if (!have_log) {
              sparse_window<NTHR, FILT>(a, sh, keys, s_log, b, tid, 0, cnt0, true);
              have_log = true;
              gram_sync();
            }
            shared0_keys<NTHR, FILT, true>(a, sh, keys, s_log, b, tid, 0, cnt0, k0, gs, nprev);
          }
        }
        gram_sync();
        flag_nonfinite_keys<NTHR, FILT>(a, keys, Cg, tid);
        gram_sync();  // (the group forms' barrier that beam_step_kernel does not have: merge_round's GRP, unjudged)
        top_p_select<NTHR, MAXN>(keys, NC, P, tid);
      } else {
        int cp = cap;
        if (cp > nkeys - P) cp = nkeys - P;
        if (cp < 1) cp = 1;
        unsigned long long* kw = keys + P;
        for (int i = tid; i < P; i += NTHR) keys[i] = 0ull;  // nothing carried yet
        auto merge = [&](int n) { merge_round<NTHR, FILT, true, MAXN>(a, keys, kw, P, n, tid); };
        if (logits != nullptr) {
          for (int o = 0; o < Cg; o += cp) {
            const int n = Cg - o < cp ? Cg - o : cp;
            dense_window<NTHR, FILT, true>(a, sh, kw, b, tid, c0 + o, n, n, nprev);
            merge(n);
          }
        } else if (!shared0) {
          for (int o = 0; o < Cg; o += cp) {
            const int n = Cg - o < cp ? Cg - o : cp;
            sparse_window<NTHR, FILT, true>(a, sh, kw, s_log, b, tid, c0 + o, n, false, nprev);
            merge(n);
          }
        } else {
          const int njmax = cp < nlog ? cp : nlog;
          const bool single = cnt0 <= njmax;  // every logit fits s_log: computed for the first group, kept for the others
          for (int j0 = 0; j0 < cnt0; j0 += njmax) {
            const int nj = cnt0 - j0 < njmax ? cnt0 - j0 : njmax;
            if (!(single && have_log)) {
              sparse_window<NTHR, FILT>(a, sh, kw, s_log, b, tid, j0, nj, true);
              gram_sync();
            }
            const int kgmax = cp / nj;  // >= 1
            for (int kk = 0; kk < gs; kk += kgmax) {
              const int kg = gs - kk < kgmax ? gs - kk : kgmax;
              shared0_keys<NTHR, FILT, true>(a, sh, kw, s_log, b, tid, j0, nj, k0 + kk, kg, nprev);
              merge(kg * nj);
            }
          }
          have_log = true;
        }
      }
    }
    step_rank<NTHR, FILT>(a, sh, keys, b, tid, k0, gs, Cg);
    if (tid == 0) sh.isdone = st.done[b];  // (this group may have finished the user: the later ones are padded)
    gram_sync();
  }
  step_advance<NTHR>(a, sh, new_seq, new_anc, b, tid);
}

// The sparse logits of a search step, computed by MANY workgroups (a handful of users: beam_step_kernel's one workgroup per user pulls
// up to K * fan-out fp32 lm_head rows -- 15 MB at K = 20, fan-out 255 -- through ONE CU, 70 us on average and up to 290 us of a one-user
// step).  Workgroup (chunk, user) recomputes the user's candidate list exactly as beam_step_kernel does (beams in order, each beam's
// Trie children in token order) and writes h . E[tok] of candidates [32 chunk, 32 chunk + 32) to out[user][candidate]; the search
// step then reads them instead of computing them -- sparse_dot either way: the same bits.
__global__ __launch_bounds__(256) void sparse_logits_kernel(gram_beam_state_t st, gram_trie_t tr, int nc_max, int rows_per_user,
                                                            const p16* __restrict__ hd, const p16* __restrict__ emb, int d,
                                                            const int32_t* __restrict__ rowpos, int pieces,
                                                            const float* __restrict__ emb32, float* __restrict__ out) {
  __shared__ int s_pre[GRAM_MAX_BEAMS + 1], s_off[GRAM_MAX_BEAMS], s_cnt[GRAM_MAX_BEAMS], s_lr[GRAM_MAX_BEAMS];
  const int b = blockIdx.y, tid = threadIdx.x, K = st.K, row0 = b * K;
  if (st.done[b]) return;
  if (tid < K) {
    const int nd = st.node[row0 + tid];
    int o0 = 0, cnt = 0;
    if (nd >= 0) {
      o0 = tr.child_off[nd];
      cnt = tr.child_off[nd + 1] - o0;
    }
    s_off[tid] = o0;
    s_cnt[tid] = cnt;
    s_lr[tid] = rowpos ? rowpos[row0 + tid] : row0 + tid;
  }
  gram_sync();
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < K; ++k) {
      s_pre[k] = acc;
      acc += s_cnt[k];
    }
    s_pre[K] = acc;
  }
  gram_sync();
  const bool shared0 = rows_per_user == 1;
  const int nuniq = shared0 ? s_pre[1] : (s_pre[K] <= nc_max ? s_pre[K] : 0);  // (more than nc_max: the search step flags it)
  const int ci = blockIdx.x * 32 + (tid >> 3), sub = tid & 7;
  const bool act = ci < nuniq;
  int k = 0, tok = 0;
  if (act) {
    if (!shared0)
      while (s_pre[k + 1] <= ci) ++k;
    tok = tr.child_tok[s_off[k] + (ci - s_pre[k])];
  }
  const float v = sparse_dot(act, shared0 ? b : s_lr[k], tok, sub, hd, emb, emb32, d, pieces);
  if (act && sub == 0) out[(size_t)b * nc_max + ci] = v;
}

// Live rows of the coming decode step: a beam that left the Trie (its hypothesis went to the heap at EOS and HF refilled
// the slot with a -inf candidate) or belongs to a finished user can only produce -inf candidates, so its decoder row is
// never read by beam_step_kernel.  One workgroup compacts the others (ascending, i.e. grouped by user).
__global__ __launch_bounds__(1024) void live_rows_kernel(gram_beam_state_t st, gram_trie_t tr, gram_live_rows_t out) {
  __shared__ int s_w[16], s_tot;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = st.K, B = st.B, R = B * K;
  auto scan = [&](int v) {  // inclusive block scan of a 0/1 flag; returns the inclusive prefix, s_tot = block total
    for (int o = 1; o < 64; o <<= 1) {
      const int n = __shfl_up(v, o, 64);
      if (lane >= o) v += n;
    }
    gram_sync();  // previous round's s_w / s_tot readers are done
    if (lane == 63) s_w[wave] = v;
    gram_sync();
    if (tid == 0) {
      int acc = 0;
      for (int w = 0; w < 16; ++w) {
        const int t = s_w[w];
        s_w[w] = acc;
        acc += t;
      }
      s_tot = acc;
    }
    gram_sync();
    return v + s_w[wave];
  };
  int base = 0;
  for (int c0 = 0; c0 < R; c0 += 1024) {
    const int r = c0 + tid;
    int live = 0;
    if (r < R && !st.done[r / K]) {
      const int nd = st.node[r];
      live = nd >= 0 && tr.child_off[nd + 1] > tr.child_off[nd];
    }
    const int pos = base + scan(live) - 1;
    if (live) {
      out.rows[pos] = r;
      out.tokens[pos] = st.tokens[r];
    }
    if (r < R) out.rowpos[r] = live ? pos : -1;
    base += s_tot;
  }
  gram_sync();  // rowpos written by this workgroup is visible to it
  int ubase = 0;
  for (int c0 = 0; c0 < B; c0 += 1024) {
    const int b = c0 + tid;
    int live = 0;
    if (b < B)
      for (int k = 0; k < K; ++k) live |= out.rowpos[b * K + k] >= 0;
    const int pos = ubase + scan(live) - 1;
    if (live) out.users[pos] = b;
    ubase += s_tot;
  }
  if (tid == 0) {
    out.counts[0] = base;
    out.counts[1] = ubase;
  }
}

__global__ void beam_finalize_kernel(gram_beam_state_t st, int nret, int max_length, int cur_len, int64_t* __restrict__ sequences,
                                     float* __restrict__ scores, int32_t* __restrict__ out_width) {
  const int b = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int K = st.K, T = st.Tmax;
  if (!st.done[b]) {
    for (int k = 0; k < K; ++k) {
      const int r = b * K + k;
      hyp_add(st, b, st.seq + (size_t)r * T, cur_len, st.beam_scores[r]);
    }
  }
  const int n = st.n_hyps[b];
  const double* hs = st.hyp_score + (size_t)b * (K + 1);
  const int32_t* hl = st.hyp_len + (size_t)b * (K + 1);
  const int32_t* ht = st.hyp_tok + (size_t)b * (K + 1) * T;
  unsigned long long taken = 0ull;  // K+1 <= 65 entries; n <= K <= 64 here
  int maxlen = 0;
  for (int j = 0; j < nret; ++j) {
    int64_t* dst = sequences + ((size_t)b * nret + j) * max_length;
    for (int p = 0; p < max_length; ++p) dst[p] = st.pad;
    if (j >= n) {  // sorted_hyps.pop() on an empty list: IndexError in HF
      st.error[0] = 3;
      scores[b * nret + j] = -INFINITY;
      continue;
    }
    // sorted(beams, key=score) ascending + pop(): best score, ties -> highest list index
    int best = -1;
    for (int i = 0; i < n; ++i) {
      if (taken & (1ull << i)) continue;
      if (best < 0 || hs[i] >= hs[best]) best = i;
    }
    taken |= 1ull << best;
    const int len = hl[best];
    for (int p = 0; p < len && p < max_length; ++p) dst[p] = ht[(size_t)best * T + p];
    if (len < max_length) dst[len] = st.eos;
    scores[b * nret + j] = (float)hs[best];
    // log-probabilities are <= 0: a NaN or +inf score means an activation overflowed the 16-bit pieces somewhere upstream (GRAM_E_NONFINITE)
    if (hs[best] != hs[best] || hs[best] > 1.0e30) st.error[0] = 4;
    maxlen = len > maxlen ? len : maxlen;
  }
  int w = maxlen + 1;
  if (w > max_length) w = max_length;
  atomicMax(out_width, w);
}

// HF 4.26 greedy_search step (num_beams == 1): one thread per user.  argmax of the raw logits over the
// Trie children (first maximum wins, like torch.argmax on the -inf-masked row; no children -> index 0),
// finished users emit pad.  done[b] doubles as HF's (1 - unfinished_sequences); n_hyps[b] records the
// sequence length at which the user finished (0 = still running) for the final width.
// UI (the lists or the mask: filter_kind(), trie_dev.h): the argmax runs over the children that are alive for the user (node_alive).
template <typename... UI>
__global__ void greedy_step_kernel(gram_beam_state_t st, gram_trie_t tr, const float* __restrict__ logits, int V, int cur_len, UI... ui) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  const int T = st.Tmax;
  int tok = st.pad, next_node = -1;
  if (!st.done[b]) {
    const int nd = st.node[b];
    tok = 0;  // argmax of an all -inf row
    if (nd >= 0) {
      const int lo = tr.child_off[nd], hi = tr.child_off[nd + 1];
      float best = -INFINITY;
      bool any = false;
      for (int e = lo; e < hi; ++e) {
        if constexpr (filter_kind<UI...>() == kFilterMask) {
          if (!node_alive(*mask_ptr(ui...), b, tr.child_node[e])) continue;
        } else if constexpr (filtered<UI...>()) {
          if (!node_alive(*items_ptr(ui...), b, tr.child_node[e])) continue;
        }
        const int c = tr.child_tok[e];
        const float v = logits[(size_t)b * V + c];
        // children are sorted by token: strict > keeps the first maximum; a -inf logit at a lower index than
        // an allowed -inf one cannot happen for finite model outputs, NaN is never selected over a number
        if (!any || v > best) {
          best = v;
          tok = c;
          next_node = tr.child_node[e];
          any = true;
        }
      }
    }
    if (tok == st.eos) {
      st.done[b] = 1;
      st.n_hyps[b] = cur_len + 1;
    }
  }
  st.seq[(size_t)b * T + cur_len] = tok;
  st.tokens[b] = tok;
  st.node[b] = next_node;
}
// A call's per-user item lists -> sorted distinct leaf ranks (gram_user_items_prepare).  One workgroup per user: the list's entries
// become leaf ranks (padding and out-of-range indices become INT32_MAX, above every rank), a bitonic sort in LDS puts them in
// ascending order, and every thread compacts its slice of the sorted array behind an exclusive scan of the slices' distinct counts.
// npad: the power of two >= max(M, 256); dynamic LDS npad * 4 B (16 KB at GRAM_MAX_USER_ITEMS).
__global__ __launch_bounds__(256) void user_items_prepare_kernel(const int32_t* __restrict__ item_rank, int n_items,
                                                                 const int32_t* __restrict__ items, int M, int npad,
                                                                 int32_t* __restrict__ ranks, int32_t* __restrict__ count, int stride) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int32_t* s = reinterpret_cast<int32_t*>(smem);  // [npad]
  __shared__ int s_cnt[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < npad; i += 256) {
    int32_t v = INT32_MAX;
    if (i < M) {
      const int32_t it = items[(size_t)b * M + i];
      if (it >= 0 && it < n_items) {
        const int32_t r = item_rank[it];
        if (r >= 0) v = r;
      }
    }
    s[i] = v;
  }
  gram_sync();
  for (int kk = 2; kk <= npad; kk <<= 1)
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npad; i += 256) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const int32_t x = s[i], y = s[ixj];
          if (((i & kk) == 0) ? (x > y) : (x < y)) {
            s[i] = y;
            s[ixj] = x;
          }
        }
      }
      gram_sync();
    }
  // thread tid owns sorted entries [tid * per, (tid + 1) * per): an entry is kept if it is a rank and differs from its predecessor
  const int per = npad / 256;
  auto keep = [&](int i) { return s[i] != INT32_MAX && (i == 0 || s[i] != s[i - 1]); };
  int c = 0;
  for (int i = tid * per; i < (tid + 1) * per; ++i) c += keep(i) ? 1 : 0;
  s_cnt[tid] = c;
  gram_sync();
  if (tid == 0) {
    int acc = 0;
    for (int t = 0; t < 256; ++t) {
      const int n = s_cnt[t];
      s_cnt[t] = acc;
      acc += n;
    }
    count[b] = acc < stride ? acc : stride;  // (acc <= M <= stride: the launcher checks)
  }
  gram_sync();
  int pos = s_cnt[tid];
  for (int i = tid * per; i < (tid + 1) * per; ++i)
    if (keep(i)) {
      if (pos < stride) ranks[(size_t)b * stride + pos] = s[i];
      ++pos;
    }
}

// A call's item mask -> every user's records (gram_user_mask_prepare).  One workgroup per user walks the leaf ranks
// once, kMaskPassLeaves per pass: a lane per leaf (coalesced leaf_item reads, one byte of the user's mask row each), a wave's 64-bit
// ballot is two words of the bitset, and a wave takes four ballots in a row, so that its 256 gathers are in flight together.  The
// waves' popcounts meet in LDS (double-buffered: one barrier per pass); every wave adds the earlier waves' to the total carried from
// the passes before and writes its eight records.  No atomics, and no word depends on the geometry.  The pass that holds rank
// n_leaves writes the last record (n_leaves / 32: the one a count up to hi = n_leaves reads); records from stride's surplus on are
// never touched.
constexpr int kMaskPassLeaves = 1024;
__global__ __launch_bounds__(256) void user_mask_prepare_kernel(const uint8_t* __restrict__ mask, long long mask_stride, int n_items,
                                                                const int32_t* __restrict__ leaf_item, int n_leaves,
                                                                uint32_t* __restrict__ words, long long stride,
                                                                int32_t* __restrict__ count) {
  __shared__ int s_cnt[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint8_t* __restrict__ row = mask + (size_t)b * mask_stride;
  uint2* __restrict__ rec = reinterpret_cast<uint2*>(words) + (size_t)b * stride;
  const int W = n_leaves / 32 + 1;
  int total = 0;
  for (int base = 0, pass = 0; base <= n_leaves; base += kMaskPassLeaves, ++pass) {
    const int r0 = base + wave * (kMaskPassLeaves / 4);
    unsigned long long m[4];
    int c = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + q * 64 + lane;
      bool keep = false;
      if (r < n_leaves) {
        const int it = leaf_item[r];
        if (it >= 0 && it < n_items) keep = row[it] != 0;
      }
      m[q] = __ballot(keep);
      c += __popcll(m[q]);
    }
    if (lane == 0) s_cnt[pass & 1][wave] = c;
    gram_sync();
    int before = total;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int n = s_cnt[pass & 1][w];
      if (w < wave) before += n;
      total += n;
    }
    const int w0 = r0 >> 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const uint32_t lo = (uint32_t)m[q], hi = (uint32_t)(m[q] >> 32);
      if (lane == 2 * q && w0 + lane < W) rec[w0 + lane] = make_uint2(lo, (uint32_t)before);
      if (lane == 2 * q + 1 && w0 + lane < W) rec[w0 + lane] = make_uint2(hi, (uint32_t)(before + __popc(lo)));
      before += __popcll(m[q]);
    }
  }
  if (tid == 0) count[b] = total;
}

__global__ void greedy_finalize_kernel(gram_beam_state_t st, int max_length, int64_t* __restrict__ sequences,
                                       int32_t* __restrict__ out_width) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= st.B) return;
  const int T = st.Tmax;
  for (int p = 0; p < max_length; ++p) sequences[(size_t)b * max_length + p] = st.seq[(size_t)b * T + p];
  // HF stops as soon as every row is finished: width = the longest finished length (max_length if any row never finished)
  const int len = st.n_hyps[b] > 0 ? st.n_hyps[b] : max_length;
  atomicMax(out_width, len);
}

// Item index of every returned sequence: a hypothesis of a Trie-constrained search is a root-to-leaf path, so walking the CSR
// from the root along the sequence's tokens (start token first) ends on a leaf, and node_item[leaf] is the candidate it spells.
// -1: the row is not a candidate (the -inf filler beams HF pads a user with when fewer than nret hypotheses finished).
__global__ void trie_item_index_kernel(gram_trie_t tr, const int32_t* __restrict__ node_item, const int64_t* __restrict__ sequences,
                                       int rows, int T, int pad, int32_t* __restrict__ out_item) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const int64_t* seq = sequences + (size_t)r * T;
  int node = 0, p = 0;
  for (; p < T; ++p) {
    if (tr.child_off[node + 1] == tr.child_off[node]) break;  // a leaf: the candidate is complete
    const int64_t tok = seq[p];
    const int e = (tok < 0 || tok > 0x7fffffff) ? -1 : find_child(tr, node, (int)tok);
    if (e < 0) { node = -1; break; }
    node = tr.child_node[e];
  }
  int item = -1;
  if (node > 0 && tr.child_off[node + 1] == tr.child_off[node]) {
    item = node_item[node];
    for (; p < T; ++p)  // what follows a candidate is padding, or the row is some other sequence that merely starts like one
      if (seq[p] != pad) item = -1;
  }
  out_item[r] = item;
}

// ---- the forest of the tail pass (gram_forest_t, gram_hip.h).  A beam is live exactly as in live_rows_kernel.
__device__ __forceinline__ bool tail_live(const gram_beam_state_t& st, const gram_trie_t& tr, int b, int row) {
  if (st.done[b]) return false;
  const int nd = st.node[row];
  return nd >= 0 && nd < tr.n_nodes && tr.child_off[nd + 1] > tr.child_off[nd];
}

// Rows and entries per user from the per-node subtree sizes, their exclusive prefix sums and the totals: one workgroup, as
// live_rows_kernel.  A user's count saturates just above the capacity, so that no sum leaves 64 bits' easy range.
__global__ __launch_bounds__(1024) void tail_count_kernel(gram_beam_state_t st, gram_trie_t tr, gram_trie_tail_t tl, gram_forest_t f) {
  __shared__ long long s_w[16], s_tot;
  __shared__ int s_mx[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = st.K, B = st.B;
  auto scan = [&](long long v) {  // inclusive block scan; s_tot = block total
    for (int o = 1; o < 64; o <<= 1) {
      const long long n = __shfl_up(v, o, 64);
      if (lane >= o) v += n;
    }
    gram_sync();  // previous round's s_w / s_tot readers are done
    if (lane == 63) s_w[wave] = v;
    gram_sync();
    if (tid == 0) {
      long long acc = 0;
      for (int w = 0; w < 16; ++w) {
        const long long t = s_w[w];
        s_w[w] = acc;
        acc += t;
      }
      s_tot = acc;
    }
    gram_sync();
    return v + s_w[wave];
  };
  const long long sat = (long long)f.cap_rows + 1;
  long long rbase = 0, ebase = 0;
  int mx = 0;
  for (int c0 = 0; c0 < B; c0 += 1024) {
    const int b = c0 + tid;
    long long n = 0;
    if (b < B) {
      for (int k = 0; k < K; ++k)
        if (tail_live(st, tr, b, b * K + k)) {
          const int s = tl.sub_rows[st.node[b * K + k]];
          n += s > 0 ? s : 0;
        }
      n = n > sat ? sat : n;
    }
    const long long e = (n + GRAM_TAIL_ENTRY_ROWS - 1) / GRAM_TAIL_ENTRY_ROWS;
    const long long ri = scan(n);
    const long long r0 = rbase + ri - n;
    rbase += s_tot;
    const long long ei = scan(e);
    const long long e0 = ebase + ei - e;
    ebase += s_tot;
    if (b < B) {
      f.user_off[b] = (int)(r0 > INT32_MAX ? INT32_MAX : r0);
      f.ent_off[b] = (int)(e0 > INT32_MAX ? INT32_MAX : e0);
      mx = n > mx ? (int)n : mx;
    }
  }
  mx = (int)wave_max((float)mx);  // (counts are far below 2^24: exact)
  if (lane == 0) s_mx[wave] = mx;
  gram_sync();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) mx = s_mx[w] > mx ? s_mx[w] : mx;
    f.user_off[B] = (int)(rbase > INT32_MAX ? INT32_MAX : rbase);
    f.ent_off[B] = (int)(ebase > INT32_MAX ? INT32_MAX : ebase);
    f.counts[0] = f.user_off[B];
    f.counts[1] = f.ent_off[B];
    f.counts[2] = mx;
    f.counts[3] = 0;
    for (int l = 0; l < 2 * GRAM_TAIL_MAX_STEPS; ++l) f.counts[4 + l] = 0;  // (tail_fill_kernel adds the (group, level) rows up)
  }
}

// The rows of one user per thread, breadth first: the forest's rows are their own queue.  Nothing is written for a forest over
// capacity.  A subtree table that disagrees with the Trie is error 3; the rows it promised and the walk did not find are made
// harmless copies of a start row, so that nothing downstream reads outside its tables.
__global__ __launch_bounds__(64) void tail_fill_kernel(gram_beam_state_t st, gram_trie_t tr, gram_forest_t f, int t) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= st.B) return;
  if (f.counts[0] > f.cap_rows || f.counts[1] > f.cap_entries) return;
  const int K = st.K, base = f.user_off[b], cnt = f.user_off[b + 1] - base;
  auto put = [&](int i, int tok, int pos, int parent, int root, int node) {
    f.tokens[i] = tok;
    f.pos[i] = pos;
    f.parent[i] = parent;
    f.root[i] = root;
    f.node[i] = node;
  };
  int n = 0;
  for (int k = 0; k < K && n < cnt; ++k)
    if (tail_live(st, tr, b, b * K + k)) {
      put(base + n, st.tokens[b * K + k], t, -1, b * K + k, st.node[b * K + k]);
      ++n;
    }
  for (int head = 0; head < n && n < cnt; ++head) {
    const int row = base + head, nd = f.node[row];
    const int e1 = tr.child_off[nd + 1];
    for (int e = tr.child_off[nd]; e < e1 && n < cnt; ++e) {
      const int c = tr.child_node[e];
      if (c >= 0 && c < tr.n_nodes && tr.child_off[c + 1] > tr.child_off[c]) {
        put(base + n, tr.child_tok[e], f.pos[row] + 1, row, f.root[row], c);
        ++n;
      }
    }
  }
  if (n < cnt) {
    st.error[0] = 3;
    for (; n < cnt; ++n) put(base + n, st.pad, t, -1, b * K, -1);
  }
  // slots: the user's rows of a level (contiguous: the rows are depth-major) take the next cnt slots of that level in the user's
  // group (even / odd users: a level's slots are cache rows, B * K per position, and a forest level may hold more rows than that)
  const int grp = b & 1;
  for (int i = 0; i < cnt;) {
    const int l = f.pos[base + i] - t;
    int j = i + 1;
    while (j < cnt && f.pos[base + j] - t == l) ++j;
    const bool ok = l >= 0 && l < f.n_levels;
    const int s0 = ok ? atomicAdd(&f.counts[4 + grp * GRAM_TAIL_MAX_STEPS + l], j - i) : 0;
    const size_t tab = ((size_t)grp * f.n_levels + (ok ? l : 0)) * f.cap_rows;
    for (int k = i; k < j; ++k) {
      const int sl = s0 + (k - i);
      f.slot[base + k] = ok && sl < f.cap_rows ? sl : -1;
      if (ok && sl < f.cap_rows) {
        f.lvl_rows[tab + sl] = base + k;
        f.lvl_tokens[tab + sl] = f.tokens[base + k];
      }
    }
    i = j;
  }
  const int e0 = f.ent_off[b], ne = f.ent_off[b + 1] - e0;
  for (int e = 0; e < ne; ++e) {
    f.ent_users[e0 + e] = b;
    for (int s = 0; s < GRAM_TAIL_ENTRY_ROWS; ++s) {
      const int i = e * GRAM_TAIL_ENTRY_ROWS + s;
      f.ent_rows[(size_t)(e0 + e) * GRAM_TAIL_ENTRY_ROWS + s] = i < cnt ? base + i : -1;
    }
  }
}

// The ancestor table of every level (gram_forest_t.lvl_anc), one thread per forest row: column = the row's slot; below t the
// beam's column of the search's table, from t on the slots of the row's ancestors.  R = cache rows per position = B * K.
__global__ __launch_bounds__(256) void tail_anc_kernel(gram_beam_state_t st, gram_forest_t f, int t) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = f.counts[0], R = st.B * st.K;
  if (n > f.cap_rows || f.counts[1] > f.cap_entries || i >= n) return;
  const int l = f.pos[i] - t, s = f.slot[i];
  if (l < 0 || l >= f.n_levels || s < 0 || s >= R) return;
  int root = f.root[i];
  root = root < 0 ? 0 : (root >= R ? R - 1 : root);
  const int grp = (root / st.K) & 1;  // (the row's user)
  int32_t* tab = f.lvl_anc + ((size_t)grp * f.n_levels + l) * st.Tmax * R;
  for (int j = 0; j < t; ++j) tab[(size_t)j * R + s] = st.anc[(size_t)j * R + root];
  int a = f.parent[i];
  for (int u = 0; u < GRAM_TAIL_MAX_STEPS && a >= 0 && a < n; ++u) {
    const int pa = f.pos[a], sa = f.slot[a];
    if (pa >= t && pa < st.Tmax && sa >= 0 && sa < R) tab[(size_t)pa * R + s] = sa;
    a = f.parent[a];
  }
}

// dst row rows[i] = src row i (gram_scatter_rows): 16 bytes per thread
__global__ __launch_bounds__(256) void scatter_rows_kernel(const uint4* __restrict__ src, const int32_t* __restrict__ rows,
                                                           uint4* __restrict__ dst, int n, int row16, int dst_rows) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)n * row16) return;
  const int r = (int)(g / row16), c = (int)(g % row16);
  const int d = rows[r];
  if (d >= 0 && d < dst_rows) dst[(size_t)d * row16 + c] = src[g];
}

// forest row of every beam for the coming search step (a user's rows are few: a linear scan)
__global__ __launch_bounds__(256) void tail_rowpos_kernel(gram_beam_state_t st, gram_trie_t tr, gram_forest_t f) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= st.B * st.K) return;
  const int b = r / st.K;
  int pos = -1;
  if (tail_live(st, tr, b, r)) {
    const int nd = st.node[r], i1 = f.user_off[b + 1];
    for (int i = f.user_off[b]; i < i1; ++i)
      if (f.node[i] == nd) {
        pos = i;
        break;
      }
    if (pos < 0) {  // impossible: every live beam descends from a forest root
      st.error[0] = 3;
      pos = 0;
    }
  }
  f.rowpos[r] = pos;
}

}  // namespace

static int check_state(const gram_beam_state_t* st) {
  if (!st || st->B < 1 || st->K < 1 || st->K > GRAM_MAX_BEAMS || st->Tmax < 2 || st->Tmax > GRAM_MAX_DEC_LEN) return GRAM_E_ARG;
  return 0;
}

extern "C" int gram_beam_init(const gram_beam_state_t* st, const gram_trie_t* tr, int start_token, void* stream) {
  if (int e = check_state(st)) return e;
  if (!tr) return GRAM_E_ARG;
  const int R = st->B * st->K;
  hipLaunchKernelGGL(beam_init_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, *st, *tr, start_token, st->K);
  GRAM_CHECK_LAUNCH();
  return 0;
}

// gram_debug_set_beam_chunked / gram_debug_set_beam_chunk_capacity (gram_hip.h): which form of the search step runs, and a test hook
static int g_beam_chunked = -1;  // -1 / 0: by shape; 1: always the chunked kernel
static int g_beam_chunk_cap = 0;  // 0: what the key array holds; n: at most n fresh candidates per round
extern "C" int gram_debug_set_beam_chunked(int mode) {
  if (mode < -1 || mode > 1) return GRAM_E_ARG;
  g_beam_chunked = mode;
  return 0;
}
extern "C" int gram_debug_set_beam_chunk_capacity(int candidates) {
  if (candidates < 0) return GRAM_E_ARG;
  g_beam_chunk_cap = candidates;
  return 0;
}

// One search step, one workgroup per user: the 1 024-thread instantiation of a form when `wide`, its 256-thread one otherwise.  Both
// are allowed `smem` bytes of dynamic LDS first; the high-water mark is the pair's own (a static of this template's instantiation).
template <auto kStep256, auto kStep1024, typename... Args>
static int launch_step_pair(bool wide, int B, size_t smem, hipStream_t stream, const Args&... args) {
  static size_t attr_bytes = 0;
  if (smem > attr_bytes) {
    for (const void* f : {reinterpret_cast<const void*>(kStep256), reinterpret_cast<const void*>(kStep1024)})
      if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); e != hipSuccess) return (int)e;
    attr_bytes = smem;
  }
  if (wide) hipLaunchKernelGGL(kStep1024, dim3(B), dim3(1024), smem, stream, args...);
  else hipLaunchKernelGGL(kStep256, dim3(B), dim3(256), smem, stream, args...);
  GRAM_CHECK_LAUNCH();
  return 0;
}

// One call of the search step, as its entry points hand it to the launcher.
struct StepCall {
  const gram_beam_state_t* st = nullptr;
  const gram_trie_t* tr = nullptr;
  const float *logits = nullptr, *lse = nullptr;  // logits: the dense step's [rows][V]; nullptr: sparse, hd . emb / emb32 at the allowed tokens
  int V = 0, cur_len = 0, rows_per_user = 0;
  void* stream = nullptr;
  const void *hd = nullptr, *emb = nullptr;
  const float* emb32 = nullptr;
  int d = 0, pieces = 1, num_groups = 0;  // num_groups 0: the plain step; G >= 1: the group step (beam_group_step_kernel; lists only)
  const int32_t* rowpos = nullptr;
  // the step's form, i.e. the kernels' trailing pack: per-user lists, potentials (phi == nullptr: none), per-user masks (alone)
  const gram_user_items_t* items = nullptr;
  StepBias bias{nullptr, 0};
  const gram_user_mask_t* mask = nullptr;
  float diversity_penalty = 0.f;
};
static StepCall dense_call(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, const float* lse, int V, int cur_len,
                           int rows_per_user, void* stream) {
  return {st, tr, logits, lse, V, cur_len, rows_per_user, stream};  // (the struct's first fields, in its order)
}
// the lm_head operand: pieces == 1 reads lm_head_bf16, two pieces (or no lm_head_bf16) lm_head_f32
static StepCall sparse_call(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden, const void* lm_head_bf16,
                            const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user,
                            const int32_t* rowpos, int pieces, void* stream) {
  StepCall c = dense_call(st, tr, nullptr, lse, V, cur_len, rows_per_user, stream);
  const bool use32 = pieces > 1 || !lm_head_bf16;
  c.hd = hidden, c.emb = use32 ? nullptr : lm_head_bf16, c.emb32 = use32 ? lm_head_f32 : nullptr, c.d = d, c.rowpos = rowpos, c.pieces = pieces;
  return c;
}

// the (K, G, lambda) of a group search: G groups of K / G beams, a finite penalty >= 0
static int check_groups(int K, int num_groups, float diversity_penalty) {
  const bool ok = num_groups >= 1 && num_groups <= K && K % num_groups == 0 && diversity_penalty >= 0.f && diversity_penalty < INFINITY;
  return ok ? 0 : GRAM_E_ARG;
}

// The search step, plain or group.  Which form runs is decided by kb, the beams per selection (K, or K / G for a group step): a
// selection's kb * max_fanout candidates in LDS at once, or streamed.  Where the two steps differ today, a branch says so.
static int launch_search_step(const StepCall& c) {
  const gram_beam_state_t* st = c.st;
  const gram_trie_t* tr = c.tr;
  const bool group = c.num_groups != 0;
  hipStream_t stream = (hipStream_t)c.stream;
  if (int e = check_state(st)) return e;
  if (group && check_groups(st->K, c.num_groups, c.diversity_penalty)) return GRAM_E_ARG;
  if (group && c.items && check_items(c.items)) return GRAM_E_ARG;  // (the plain step's entry points judge their lists themselves)
  if (!tr || !c.lse || c.cur_len < 1 || c.cur_len >= st->Tmax || c.V < 2 || (c.rows_per_user != 1 && c.rows_per_user != st->K)) return GRAM_E_ARG;
  if (group && c.rowpos && c.rows_per_user != st->K) return GRAM_E_ARG;  // (the plain step's entry points judge it, or do not, themselves)
  if (!c.logits && (!c.hd || (!c.emb && !c.emb32) || c.d < 64 || (c.d & 63))) return GRAM_E_ARG;
  // (the plain step alone judges d for two pieces on a dense call too -- which no entry point makes today: dense calls have one piece)
  if (c.pieces < 1 || c.pieces > GRAM_MAX_PIECES || (c.pieces > 1 && (!c.emb32 || (!group && (c.d & 63))))) return GRAM_E_ARG;
  if (tr->max_fanout < 0) return GRAM_E_ARG;
  const int kb = group ? st->K / c.num_groups : st->K;
  const long long need = (long long)kb * tr->max_fanout;
  int nc = 64;
  while (nc < need && nc < kOneShotMaxKeys) nc <<= 1;
  const int nlog_one = (tr->max_fanout + 3) / 4 * 4;
  const size_t seq_bytes = (size_t)2 * st->K * st->Tmax * 4;
  const size_t smem_one = (size_t)nc * 8 + (size_t)nlog_one * 4 + seq_bytes;
  // one-shot: every candidate of a selection in LDS at once (+ ~3 KB of static arrays: the CU's 160 KB); everything else streams
  const bool chunked = g_beam_chunked == 1 || need > kOneShotMaxKeys || smem_one > 152 * 1024;
  // 32-bit scalar state of the kernels: the flat index k * V + tok < K * V, and the candidate count and its prefix sums <= K * V
  // (a node has at most V children).  The group step refuses always, the plain step only where it streams.
  if ((group || chunked) && ((long long)st->K * c.V > INT32_MAX || tr->max_fanout > c.V)) return GRAM_E_ARG;
  gram_prof::Scope prof(GRAM_K_BEAM, stream, 0.0);
  // few users: one workgroup per user leaves the chip empty and the step is that workgroup's latency -> 1 024 threads per user
  // (same per-candidate arithmetic, same total order of the keys: identical results; GRAM_BEAM_WIDE_MAXB: A/B hook, 0 = never)
  static const int wide_max_b = getenv("GRAM_BEAM_WIDE_MAXB") ? atoi(getenv("GRAM_BEAM_WIDE_MAXB")) : 128;
  const bool wide = st->B <= wide_max_b;
  int P = 64;  // (P and cap: the streamed forms and the group kernel only)
  while (P < 2 * kb) P <<= 1;
  int cap = kChunkKeys - P;
  if (g_beam_chunk_cap > 0 && g_beam_chunk_cap < cap) cap = g_beam_chunk_cap;
  const size_t smem = chunked ? (size_t)kChunkKeys * 8 + (size_t)kChunkLog * 4 + seq_bytes : smem_one;  // chunked: <= 40 KB + 64 KB
  const p16 *hd = (const p16*)c.hd, *emb = (const p16*)c.emb;
  if (group) {
    // (the small-batch sparse_logits_kernel is not used: the group step computes its logits itself at every batch size)
    const int nkeys = chunked ? kChunkKeys : nc, nlog = chunked ? kChunkLog : nlog_one;
    auto launch = [&](auto form, auto... ui) {
      constexpr bool CH = decltype(form)::value;
      return launch_step_pair<beam_group_step_kernel<256, CH, decltype(ui)...>, beam_group_step_kernel<1024, CH, decltype(ui)...>>(
          wide, st->B, smem, stream, *st, *tr, c.logits, c.lse, c.V, c.cur_len, nkeys, nlog, cap, c.rows_per_user, hd, emb, c.d, c.rowpos,
          c.pieces, c.emb32, c.num_groups, c.diversity_penalty, ui...);
    };
    if (chunked) return c.items ? launch(std::true_type{}, *c.items) : launch(std::true_type{});
    return c.items ? launch(std::false_type{}, *c.items) : launch(std::false_type{});
  }
  auto with_form = [&](auto launch) {
    if (c.mask) return launch(*c.mask);
    if (c.bias.phi) return c.items ? launch(*c.items, c.bias) : launch(c.bias);
    return c.items ? launch(*c.items) : launch();
  };
  if (chunked)
    return with_form([&](auto... ui) {
      return launch_step_pair<beam_step_chunked_kernel<256, decltype(ui)...>, beam_step_chunked_kernel<1024, decltype(ui)...>>(
          wide, st->B, smem, stream, *st, *tr, c.logits, c.lse, c.V, c.cur_len, cap, c.rows_per_user, hd, emb, c.d, c.rowpos, c.pieces,
          c.emb32, ui...);
    });
  // the plain one-shot step alone, for a handful of users: the sparse logits by their own kernel over many CUs (sparse_logits_kernel),
  // the search step reads them (gram_beam_state_t.cand_logits: caller-provided scratch; GRAM_BEAM_PRE_MAXB: A/B hook, 0 = never)
  static const int pre_max_b = getenv("GRAM_BEAM_PRE_MAXB") ? atoi(getenv("GRAM_BEAM_PRE_MAXB")) : 16;
  const float* pre = nullptr;
  if (!c.logits && st->cand_logits && st->B <= pre_max_b && st->B <= st->cand_logits_users && (long long)nc <= st->cand_logits_stride) {
    hipLaunchKernelGGL(sparse_logits_kernel, dim3((int)((need + 31) / 32), st->B), dim3(256), 0, stream, *st, *tr, nc, c.rows_per_user,
                       hd, emb, c.d, c.rowpos, c.pieces, c.emb32, st->cand_logits);
    GRAM_CHECK_LAUNCH();
    pre = st->cand_logits;
  }
  return with_form([&](auto... ui) {
    return launch_step_pair<beam_step_kernel<256, decltype(ui)...>, beam_step_kernel<1024, decltype(ui)...>>(
        wide, st->B, smem, stream, *st, *tr, c.logits, c.lse, c.V, c.cur_len, nc, c.rows_per_user, hd, emb, c.d, c.rowpos, c.pieces, c.emb32, pre,
        ui...);
  });
}

// the potentials of a biased step: present, and one row for all users or a row of at least n_nodes entries per user; then its lists, if any
static int check_bias(const gram_trie_t* tr, const float* phi, int64_t phi_stride, const gram_user_items_t* items) {
  if (!tr || !phi || (phi_stride != 0 && phi_stride < tr->n_nodes)) return GRAM_E_ARG;
  return items ? check_items(items) : 0;
}

extern "C" int gram_beam_step_bias(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, const float* lse, int V,
                                   int cur_len, int rows_per_user, const float* phi, int64_t phi_stride,
                                   const gram_user_items_t* items, void* stream) {
  if (int e = check_bias(tr, phi, phi_stride, items)) return e;
  if (!logits) return GRAM_E_ARG;
  StepCall c = dense_call(st, tr, logits, lse, V, cur_len, rows_per_user, stream);
  c.items = items, c.bias = {phi, (long long)phi_stride};
  return launch_search_step(c);
}

extern "C" int gram_beam_step_bias_sparse(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                          const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                                          int rows_per_user, const int32_t* rowpos, int pieces, const float* phi, int64_t phi_stride,
                                          const gram_user_items_t* items, void* stream) {
  if (int e = check_bias(tr, phi, phi_stride, items)) return e;
  if (!hidden_bf16 || !st || (rowpos && rows_per_user != st->K)) return GRAM_E_ARG;
  StepCall c = sparse_call(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, stream);
  c.items = items, c.bias = {phi, (long long)phi_stride};
  return launch_search_step(c);
}

extern "C" int gram_beam_init_groups(const gram_beam_state_t* st, const gram_trie_t* tr, int start_token, int num_groups, void* stream) {
  if (int e = check_state(st)) return e;
  if (!tr || num_groups < 1 || num_groups > st->K || st->K % num_groups != 0) return GRAM_E_ARG;
  const int R = st->B * st->K;
  hipLaunchKernelGGL(beam_init_kernel, dim3((R + 255) / 256), dim3(256), 0, (hipStream_t)stream, *st, *tr, start_token,
                     st->K / num_groups);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_beam_step_groups(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, const float* lse, int V,
                                     int cur_len, int rows_per_user, int num_groups, float diversity_penalty, void* stream) {
  if (int e = check_state(st)) return e;
  if (int e = check_groups(st->K, num_groups, diversity_penalty)) return e;
  if (!logits) return GRAM_E_ARG;
  StepCall c = dense_call(st, tr, logits, lse, V, cur_len, rows_per_user, stream);
  c.num_groups = num_groups, c.diversity_penalty = diversity_penalty;
  return launch_search_step(c);
}

extern "C" int gram_beam_step_groups_sparse(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                            const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V,
                                            int cur_len, int rows_per_user, const int32_t* rowpos, int pieces, int num_groups,
                                            float diversity_penalty, const gram_user_items_t* items, void* stream) {
  if (int e = check_state(st)) return e;
  if (int e = check_groups(st->K, num_groups, diversity_penalty)) return e;
  if (!hidden_bf16) return GRAM_E_ARG;
  StepCall c = sparse_call(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, stream);
  c.items = items, c.num_groups = num_groups, c.diversity_penalty = diversity_penalty;
  return launch_search_step(c);
}

extern "C" int gram_beam_step(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, const float* lse, int V,
                              int cur_len, int rows_per_user, void* stream) {
  if (!logits) return GRAM_E_ARG;
  return launch_search_step(dense_call(st, tr, logits, lse, V, cur_len, rows_per_user, stream));
}

extern "C" int gram_beam_step_sparse(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                     const void* lm_head_bf16, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                     void* stream) {
  return launch_search_step(sparse_call(st, tr, hidden_bf16, lm_head_bf16, nullptr, d, lse, V, cur_len, rows_per_user, nullptr, 1, stream));
}

extern "C" int gram_beam_step_sparse_live(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                          const void* lm_head_bf16, int d, const float* lse, int V, int cur_len,
                                          const int32_t* rowpos, void* stream) {
  if (!rowpos || !st) return GRAM_E_ARG;
  return launch_search_step(sparse_call(st, tr, hidden_bf16, lm_head_bf16, nullptr, d, lse, V, cur_len, st->K, rowpos, 1, stream));
}

extern "C" int gram_beam_step_sparse_split(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                           const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                           const int32_t* rowpos, int pieces, void* stream) {
  if (!lm_head_f32) return GRAM_E_ARG;
  return launch_search_step(sparse_call(st, tr, hidden_bf16, nullptr, lm_head_f32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, stream));
}

extern "C" int gram_beam_step_sparse_items(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                           const void* lm_head_bf16, int d, const float* lse, int V, int cur_len, int rows_per_user,
                                           const int32_t* rowpos, const gram_user_items_t* items, void* stream) {
  if (int e = check_items(items)) return e;
  if (!st || (rowpos && rows_per_user != st->K)) return GRAM_E_ARG;
  StepCall c = sparse_call(st, tr, hidden_bf16, lm_head_bf16, nullptr, d, lse, V, cur_len, rows_per_user, rowpos, 1, stream);
  c.items = items;
  return launch_search_step(c);
}

extern "C" int gram_beam_step_sparse_split_items(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                                 const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                                                 int rows_per_user, const int32_t* rowpos, int pieces, const gram_user_items_t* items,
                                                 void* stream) {
  if (int e = check_items(items)) return e;
  if (!lm_head_f32 || !st || (rowpos && rows_per_user != st->K)) return GRAM_E_ARG;
  StepCall c = sparse_call(st, tr, hidden_bf16, nullptr, lm_head_f32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, stream);
  c.items = items;
  return launch_search_step(c);
}

extern "C" int gram_user_items_prepare(const int32_t* item_rank, int n_items, const int32_t* items, int B, int M, int32_t* ranks,
                                       int32_t* count, int stride, void* stream) {
  if (!item_rank || !items || !ranks || !count || n_items < 1 || B < 1 || M < 1 || stride < M || stride > GRAM_MAX_USER_ITEMS)
    return GRAM_E_ARG;
  int npad = 256;
  while (npad < M) npad <<= 1;
  hipLaunchKernelGGL(user_items_prepare_kernel, dim3(B), dim3(256), (size_t)npad * 4, (hipStream_t)stream, item_rank, n_items, items, M,
                     npad, ranks, count, stride);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t gram_user_mask_words(int n_leaves) { return n_leaves < 1 ? GRAM_E_ARG : (int64_t)n_leaves / 32 + 1; }

extern "C" int gram_user_mask_prepare(const uint8_t* mask, int64_t mask_stride, int B, int n_items, const int32_t* leaf_item, int n_leaves,
                                      uint32_t* words, int64_t stride, int32_t* count, void* stream) {
  if (!mask || !leaf_item || !words || !count || B < 1 || n_items < 1 || mask_stride < n_items || n_leaves < 1 || n_leaves > (1 << 24) ||
      stride < gram_user_mask_words(n_leaves) || (reinterpret_cast<uintptr_t>(words) & 7))
    return GRAM_E_ARG;
  hipLaunchKernelGGL(user_mask_prepare_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, mask, (long long)mask_stride, n_items, leaf_item,
                     n_leaves, words, (long long)stride, count);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_beam_step_sparse_mask(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16,
                                          const void* lm_head_bf16, const float* lm_head_f32, int d, const float* lse, int V, int cur_len,
                                          int rows_per_user, const int32_t* rowpos, int pieces, const gram_user_mask_t* mask,
                                          void* stream) {
  if (int e = check_mask(mask)) return e;
  if (!hidden_bf16 || !st || (rowpos && rows_per_user != st->K)) return GRAM_E_ARG;
  StepCall c = sparse_call(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, rowpos, pieces, stream);
  c.mask = mask;
  return launch_search_step(c);
}

extern "C" int gram_live_rows(const gram_beam_state_t* st, const gram_trie_t* tr, const gram_live_rows_t* out, void* stream) {
  if (int e = check_state(st)) return e;
  if (!tr || !out || !out->rows || !out->rowpos || !out->users || !out->tokens || !out->counts) return GRAM_E_ARG;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(live_rows_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *st, *tr, *out);
  GRAM_CHECK_LAUNCH();
  return 0;
}

static bool forest_ok(const gram_forest_t* f) {
  return f && f->tokens && f->pos && f->parent && f->root && f->node && f->user_off && f->ent_off && f->ent_users && f->ent_rows &&
         f->rowpos && f->counts && f->slot && f->lvl_rows && f->lvl_tokens && f->lvl_anc && f->cap_rows >= 1 && f->cap_entries >= 1 &&
         f->n_levels >= 1 && f->n_levels <= GRAM_TAIL_MAX_STEPS;
}

extern "C" int gram_tail_forest(const gram_beam_state_t* st, const gram_trie_t* tr, const gram_trie_tail_t* tail,
                                const gram_forest_t* forest, int t, void* stream) {
  if (int e = check_state(st)) return e;
  if (!tr || !tail || !tail->sub_rows || !forest_ok(forest) || t < 0 || t >= st->Tmax) return GRAM_E_ARG;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(tail_count_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, *st, *tr, *tail, *forest);
  GRAM_CHECK_LAUNCH();
  hipLaunchKernelGGL(tail_fill_kernel, dim3((st->B + 63) / 64), dim3(64), 0, (hipStream_t)stream, *st, *tr, *forest, t);
  GRAM_CHECK_LAUNCH();
  hipLaunchKernelGGL(tail_anc_kernel, dim3((forest->cap_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, *st, *forest, t);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_scatter_rows(const void* src, const int32_t* rows, void* dst, int n, int row_bytes, int dst_rows, void* stream) {
  if (!src || !rows || !dst || n < 1 || row_bytes < 16 || (row_bytes & 15) || dst_rows < 1 ||
      ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15))
    return GRAM_E_ARG;
  const int row16 = row_bytes / 16;
  const long total = (long)n * row16;
  gram_prof::Scope prof(GRAM_K_ROWOPS, (hipStream_t)stream, 2.0 * n * row_bytes);
  hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const uint4*)src, rows,
                     (uint4*)dst, n, row16, dst_rows);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_tail_rowpos(const gram_beam_state_t* st, const gram_trie_t* tr, const gram_forest_t* forest, void* stream) {
  if (int e = check_state(st)) return e;
  if (!tr || !forest_ok(forest)) return GRAM_E_ARG;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(tail_rowpos_kernel, dim3((st->B * st->K + 255) / 256), dim3(256), 0, (hipStream_t)stream, *st, *tr, *forest);
  GRAM_CHECK_LAUNCH();
  return 0;
}

// what the greedy entry points share: the state checks and the launch.  ui: nothing, the lists or the mask (checked by the caller)
template <typename... UI>
static int launch_greedy_step(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, int V, int cur_len, void* stream,
                              const UI&... ui) {
  if (int e = check_state(st)) return e;
  if (!tr || st->K != 1 || cur_len < 1 || cur_len >= st->Tmax || V < 2) return GRAM_E_ARG;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(greedy_step_kernel<UI...>, dim3((st->B + 127) / 128), dim3(128), 0, (hipStream_t)stream, *st, *tr, logits, V, cur_len,
                     ui...);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_greedy_step(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, int V, int cur_len,
                               void* stream) {
  return launch_greedy_step(st, tr, logits, V, cur_len, stream);
}

extern "C" int gram_greedy_step_items(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, int V, int cur_len,
                                      const gram_user_items_t* items, void* stream) {
  if (int e = check_items(items)) return e;
  return launch_greedy_step(st, tr, logits, V, cur_len, stream, *items);
}

extern "C" int gram_greedy_step_mask(const gram_beam_state_t* st, const gram_trie_t* tr, const float* logits, int V, int cur_len,
                                     const gram_user_mask_t* mask, void* stream) {
  if (int e = check_mask(mask)) return e;
  return launch_greedy_step(st, tr, logits, V, cur_len, stream, *mask);
}

extern "C" int gram_greedy_finalize(const gram_beam_state_t* st, int max_length, int64_t* sequences, int32_t* out_width,
                                    void* stream) {
  if (int e = check_state(st)) return e;
  if (st->K != 1 || max_length != st->Tmax) return GRAM_E_ARG;
  hipError_t e = hipMemsetAsync(out_width, 0, sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(greedy_finalize_kernel, dim3((st->B + 127) / 128), dim3(128), 0, (hipStream_t)stream, *st, max_length, sequences,
                     out_width);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_beam_finalize(const gram_beam_state_t* st, int nret, int max_length, int64_t* sequences, float* scores,
                                  int32_t* out_width, void* stream) {
  if (int e = check_state(st)) return e;
  if (nret < 1 || nret > st->K || max_length != st->Tmax) return GRAM_E_ARG;
  hipError_t e = hipMemsetAsync(out_width, 0, sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(st->B), dim3(64), 0, (hipStream_t)stream, *st, nret, max_length, max_length,
                     sequences, scores, out_width);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_trie_item_index(const gram_trie_t* tr, const int32_t* node_item, const int64_t* sequences, int rows, int T,
                                    int32_t* out_item, void* stream) {
  if (!tr || !tr->child_off || !node_item || !sequences || !out_item || rows < 0 || T < 1 || tr->n_nodes < 1) return GRAM_E_ARG;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(trie_item_index_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, *tr, node_item, sequences, rows,
                     T, /*pad=*/0, out_item);
  GRAM_CHECK_LAUNCH();
  return 0;
}
