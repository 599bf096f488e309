// sbs.hip -- sampling WITHOUT replacement on the Trie: stochastic beam search (Kool, van Hoof, Welling, ICML 2019) on the device
// (gram_hip.h, "Sampling without replacement").  A beam search over Gumbel-perturbed log-probabilities that are
// conditioned top-down: the R rows of a user end as the R items with the largest perturbed log-probability, which is a sample
// without replacement (Plackett-Luce order) from the Trie-renormalised distribution of gram_sample with top_k and top_p off.
//   the distribution    -> y = z / temperature on the RAW logits z = h . E[tok] (sparse_dot: the search step's bits), softmax over the
//                          row's (alive) children
//   the uniforms        -> Philox4x32-10 keyed by the seed, counter = (path of the row, token, position): a function of
//                          (seed, user key, token prefix) only -- not of the node numbering, the batch, R or the row's slot
//   the selection       -> the beam search's: 64-bit keys (orderable G | ~flat index) streamed through a fixed key array, top_p_select
//   the reordering      -> step_advance (sequences, ancestor table, node) + the four extra per-row words gathered alongside
// One workgroup of 256 threads per USER.  A user's candidates (the alive children of its live rows, in row order, token order inside a
// row) are 8 B each -- f32 y, later the perturbed score, and the i32 token: up to kSbsCap = 4 096 of them live in LDS (32 KB), beyond
// that the same two arrays lie in st.cand_logits: the same code over another pointer, hence the same bits.  The keys stream through
// kSbsKeys = 2 048 words (16 KB) whatever the fan-out.  With new_seq / new_anc (1.9 KB at R = 20, Tmax = 12; 32 KB at the maxima) and
// ~6 KB of static tables that is ~56 KB at the runners' shapes: two workgroups (8 wavefronts) per CU, and a batch of 256 users is
// one workgroup per CU anyway; the worst case (86 KB) still fits a CU's 160 KB.
//
// REDUCTION ORDERS (fp32 throughout), all over a row's alive children numbered j = 0 .. n-1 in token order:
//   max y, max G~   : exact, any order
//   sum exp(y - max): lane l of ONE wave adds j = l, l + 64, l + 128, ... in ascending order, then the wave's butterfly (xor 32, 16,
//                     8, 4, 2, 1: every lane ends with the same bits).
// Nothing depends on which wave serves a row, on R, on the batch or on where the candidates lie.
#include "common.h"
#include "prof.h"
#include "sparse_dot.h"
#include "step_dev.h"
#include "trie_dev.h"

namespace {

constexpr int kSbsThreads = 256;
constexpr int kSbsWaves = kSbsThreads / WAVE;
constexpr int kSbsCap = 4096;
constexpr int kSbsKeys = 2048;

struct Philox {
  uint32_t w[4];
};
// Philox4x32-10 (Salmon et al., SC 2011)
__device__ __forceinline__ Philox philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox{{c0, c1, c2, c3}};
}
// -log(-log u), u = ((w >> 8) + 0.5) 2^-24 in (0, 1).  m + 0.5 is exact in fp32 below 2^23; above, 1 - u = (2^24 - m - 0.5) 2^-24 is,
// and -log u = -log1p(-(1 - u)): u itself would round to 1 at the top of the range.
__device__ __forceinline__ float gumbel_of(uint32_t w) {
  const uint32_t m = w >> 8;
  const float nl = m < (1u << 23) ? -logf(((float)m + 0.5f) * 0x1p-24f) : -log1pf(-(((float)((1u << 24) - m) - 0.5f) * 0x1p-24f));
  return -logf(nl);
}
// the three formulas that more than one place evaluates: one definition each, so the same bits
__device__ __forceinline__ float scaled_logit(float z, float temperature) { return z / temperature; }
__device__ __forceinline__ float child_phi(float phi, float y, float lse_k) { return phi + (y - lse_k); }
// a child's G from its parent's G (T), its own perturbed score gt and the maximum Z over the parent's children
__device__ __forceinline__ float condition(float T, float gt, float Z) {
  if (gt == Z) return T;
  const float v = (T - gt) + log1pf(-expf(gt - Z));
  return (T - fmaxf(0.f, v)) - log1pf(expf(-fabsf(v)));
}

// the rows' own words (static LDS, ~3 KB)
struct SbsShared {
  float G[GRAM_MAX_BEAMS], phi[GRAM_MAX_BEAMS], model[GRAM_MAX_BEAMS], lse_row[GRAM_MAX_BEAMS], lse_k[GRAM_MAX_BEAMS], Z[GRAM_MAX_BEAMS];
  uint32_t path_lo[GRAM_MAX_BEAMS], path_hi[GRAM_MAX_BEAMS];
  int fin[GRAM_MAX_BEAMS], live[GRAM_MAX_BEAMS], node[GRAM_MAX_BEAMS];
  float sel_z[GRAM_MAX_BEAMS];
  int sel_kind[GRAM_MAX_BEAMS];  // 0 dead, 1 a finished row carried, 2 a child
};

__global__ void sbs_init_kernel(gram_beam_state_t st, uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ user_keys,
                                float* __restrict__ phi, float* __restrict__ model, unsigned long long* __restrict__ path) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= st.B * st.K) return;
  st.hyp_len[r] = 0;
  if (r % st.K != 0) {  // only row 0 of a user is live at the root
    st.beam_scores[r] = -INFINITY;
    phi[r] = -INFINITY;
    model[r] = -INFINITY;
    path[r] = 0ull;
    return;
  }
  const unsigned long long uk = (unsigned long long)user_keys[r / st.K];
  const Philox w = philox4x32_10((uint32_t)uk, (uint32_t)(uk >> 32), 0u, 0u, seed_lo, seed_hi);
  st.beam_scores[r] = gumbel_of(w.w[2]);
  phi[r] = 0.f;
  model[r] = 0.f;
  path[r] = ((unsigned long long)w.w[1] << 32) | w.w[0];
}

// UI: the per-user item filter (filtered(), trie_dev.h).  cap: candidates the dynamic LDS holds.
template <typename... UI>
__global__ __launch_bounds__(kSbsThreads) void sbs_step_kernel(gram_beam_state_t st, gram_trie_t tr, const p16* __restrict__ hd,
                                                               const p16* __restrict__ emb, const float* __restrict__ emb32, int d,
                                                               const float* __restrict__ lse, int V, int cur_len, int rows_per_user,
                                                               int pieces, float temperature, uint32_t seed_lo, uint32_t seed_hi,
                                                               float* __restrict__ phi, float* __restrict__ model,
                                                               unsigned long long* __restrict__ path, int cap, UI... ui) {
  constexpr bool FILT = filtered<UI...>();
  constexpr int NTHR = kSbsThreads;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned long long* const keys = reinterpret_cast<unsigned long long*>(smem);  // [kSbsKeys]
  float* const cy_lds = reinterpret_cast<float*>(keys + kSbsKeys);               // [cap, a multiple of 4]  y, then the perturbed score
  int* const ct_lds = reinterpret_cast<int*>(cy_lds + cap);                      // [cap]                   token
  int* const new_seq = ct_lds + cap;                                             // [K][Tmax] + [Tmax][K] (step_advance)
  int* const new_anc = new_seq + st.K * st.Tmax;
  __shared__ StepShared sh;
  __shared__ SbsShared ss;
  const StepArgs a{st, tr, nullptr, lse, V, cur_len, rows_per_user, hd, emb, d, nullptr, pieces, emb32, nullptr, 0, items_ptr(ui...)};

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int K = st.K, row0 = b * K;

  // ---- the rows' state; a live row's children [off, off + F)
  if (tid < K) {
    const int row = row0 + tid;
    const int fin = st.hyp_len[row];
    const float G = st.beam_scores[row];
    const int nd = st.node[row];
    if (!(G < 3.0e38f)) st.error[0] = 4;  // (NaN or +inf: no perturbed score)
    const bool carried = fin > 0 && G > -INFINITY && G < 3.0e38f;
    const bool live = fin == 0 && G > -INFINITY && G < 3.0e38f && nd >= 0 && nd < tr.n_nodes;
    int o0 = 0, F = 0;
    if (live) {
      o0 = tr.child_off[nd];
      F = tr.child_off[nd + 1] - o0;
      if (F < 0 || F > V) F = 0;  // (a Trie that disagrees with itself)
    }
    const int lr = rows_per_user == 1 ? b : row;  // compact step: hidden and lse hold one row per user
    const float lr_lse = live ? lse[lr] : 0.f;
    if (live && !(fabsf(lr_lse) < 3.0e38f)) st.error[0] = 4;
    sh.off[tid] = o0;
    sh.edge[tid] = F;  // (children, alive or not; sh.cnt = the alive ones)
    sh.lr[tid] = lr;
    ss.G[tid] = G;
    ss.phi[tid] = phi[row];
    ss.model[tid] = model[row];
    ss.lse_row[tid] = lr_lse;
    const unsigned long long p = path[row];
    ss.path_lo[tid] = (uint32_t)p;
    ss.path_hi[tid] = (uint32_t)(p >> 32);
    ss.fin[tid] = carried ? fin : 0;
    ss.live[tid] = live ? 1 : 0;
    ss.node[tid] = nd;
  }
  gram_sync();

  // ---- alive children per row (one wave per row, 64 children per ballot), then the rows' places in the user's candidate list
  for (int k = wave; k < K; k += kSbsWaves) {
    const int F = sh.edge[k];
    int n = F;
    if constexpr (FILT) {
      n = 0;
      for (int i0 = 0; i0 < F; i0 += 64) {
        const bool alive = i0 + lane < F && child_alive<true>(a, b, sh.off[k] + i0 + lane);
        n += __popcll(__ballot(alive));
      }
    }
    if (lane == 0) sh.cnt[k] = n;
  }
  gram_sync();
  float* cy = cy_lds;
  int* ct = ct_lds;
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < K; ++k) {
      sh.pre[k] = acc;
      acc += sh.cnt[k];
    }
    long long room = cap;
    if (acc > cap) room = (st.cand_logits && (long long)row0 + K <= st.cand_logits_users) ? (long long)K * st.cand_logits_stride / 2 : 0;
    if (acc > room) {  // nowhere to put them (the launcher checks the worst case: a wrong state must not write outside)
      st.error[0] = 2;
      for (int k = 0; k <= K; ++k) sh.pre[k] = 0;
      for (int k = 0; k < K; ++k) sh.cnt[k] = 0;
      acc = 0;
    }
    sh.pre[K] = acc;
    sh.C = acc;
  }
  gram_sync();
  const int C = sh.C;
  if (C > cap) {
    const size_t half = (size_t)K * st.cand_logits_stride / 2;
    cy = st.cand_logits + (size_t)row0 * st.cand_logits_stride;
    ct = reinterpret_cast<int*>(cy + half);
  }

  // ---- the candidates' tokens, compacted to the alive numbering (the same wave per row, the same ballots)
  for (int k = wave; k < K; k += kSbsWaves) {
    const int F = sh.edge[k], p0 = sh.pre[k];
    if (sh.cnt[k] == 0) continue;
    int base = 0;
    for (int i0 = 0; i0 < F; i0 += 64) {
      const int i = i0 + lane;
      const bool alive = i < F && child_alive<FILT>(a, b, sh.off[k] + i);
      const unsigned long long m = __ballot(alive);
      if (alive) ct[p0 + base + __popcll(m & ((1ull << lane) - 1ull))] = tr.child_tok[sh.off[k] + i];
      base += __popcll(m);
    }
  }
  gram_sync();

  // ---- y = z / temperature of every candidate: 8 lanes each, two candidates per group and trip (as the search step's sparse_window)
  {
    const int sub = tid & 7, grp = tid >> 3;
    constexpr int NG = NTHR / 8;
    for (int base = 0; base < C; base += 2 * NG) {
      int i2[2], tok2[2], lr2[2];
      bool act2[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        i2[w] = base + NG * w + grp;
        act2[w] = i2[w] < C;
        int k = 0;
        if (act2[w])
          while (sh.pre[k + 1] <= i2[w]) ++k;
        tok2[w] = act2[w] ? ct[i2[w]] : 0;
        lr2[w] = sh.lr[k];
      }
      float z2[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) z2[w] = sparse_dot(act2[w], lr2[w], tok2[w], sub, hd, emb, emb32, d, pieces);
#pragma unroll
      for (int w = 0; w < 2; ++w)
        if (act2[w] && sub == 0) cy[i2[w]] = scaled_logit(z2[w], temperature);
    }
  }
  gram_sync();

  // ---- per row, one wave: lse_k over its children, then every child's perturbed score G~ (in y's place) and their maximum Z
  for (int k = wave; k < K; k += kSbsWaves) {
    const int n = sh.cnt[k], p0 = sh.pre[k];
    if (n == 0) continue;
    float mx = -INFINITY;
    bool nonfinite = false;
    for (int j = lane; j < n; j += 64) {
      const float y = cy[p0 + j];
      nonfinite |= !(fabsf(y) < 3.0e38f);
      mx = fmaxf(mx, y);
    }
    if (nonfinite) st.error[0] = 4;
    mx = wave_max(mx);
    float s = 0.f;
    for (int j = lane; j < n; j += 64) s += expf(cy[p0 + j] - mx);
    s = wave_sum(s);
    const float lse_k = mx + logf(s);
    const float ph = ss.phi[k];
    const uint32_t plo = ss.path_lo[k], phi_ = ss.path_hi[k];
    float zm = -INFINITY;
    for (int j = lane; j < n; j += 64) {
      const Philox w = philox4x32_10(plo, phi_, (uint32_t)ct[p0 + j], (uint32_t)cur_len, seed_lo, seed_hi);
      const float gt = child_phi(ph, cy[p0 + j], lse_k) + gumbel_of(w.w[2]);
      cy[p0 + j] = gt;
      zm = fmaxf(zm, gt);
    }
    zm = wave_max(zm);
    if (lane == 0) {
      ss.lse_k[k] = lse_k;
      ss.Z[k] = zm;
    }
  }
  gram_sync();

  // ---- the keys, streamed: keys[0, P) carry the best P so far, keys[P, P + n) take the next candidates (beam_step_chunked_kernel's
  // scheme).  The list: the C children, then one slot per row, which holds the row itself where it is finished.
  int P = 64;
  while (P < K) P <<= 1;
  {
    const int fresh = kSbsKeys - P;
    unsigned long long* const kw = keys + P;
    for (int i = tid; i < P; i += NTHR) keys[i] = 0ull;
    const int total = C + K;
    for (int c0 = 0; c0 < total; c0 += fresh) {
      const int n = total - c0 < fresh ? total - c0 : fresh;
      int na = 2 * P;  // the power of two >= P + n
      while (na < P + n) na <<= 1;
      for (int i = tid; i < na - P; i += NTHR) {
        unsigned long long key = 0ull;
        const int ci = c0 + i;
        if (i < n && ci < C) {
          int k = 0;
          while (sh.pre[k + 1] <= ci) ++k;
          const float g = condition(ss.G[k], cy[ci], ss.Z[k]);
          if (!(g < 3.0e38f)) st.error[0] = 4;
          key = cand_key(g, k, V, ct[ci]);
        } else if (i < n && ss.fin[ci - C] > 0) {
          key = cand_key(ss.G[ci - C], ci - C, V, st.pad);
        }
        kw[i] = key;
      }
      gram_sync();
      top_p_select<NTHR, kSbsKeys>(keys, na, P, tid);
    }
  }

  // ---- the R best, in descending order of G: what each new row is
  if (tid < K) {
    const unsigned long long key = keys[tid];
    float sc = -INFINITY;
    int tok = st.pad, par = tid, node = -1, kind = 0;
    if (key != 0ull) {
      sc = ord2f((uint32_t)(key >> 32));
      const uint32_t flat = 0xffffffffu - (uint32_t)(key & 0xffffffffull);
      par = (int)(flat / (uint32_t)V);
      par = par < K ? par : K - 1;
      if (ss.fin[par] > 0) {
        kind = 1;
      } else {
        kind = 2;
        tok = (int)(flat % (uint32_t)V);
        const int e = find_child(tr, ss.node[par], tok);
        node = (e < 0 || tok == st.eos) ? -1 : tr.child_node[e];
      }
    }
    sh.sel_score[tid] = sc;
    sh.sel_tok[tid] = tok;
    sh.sel_par[tid] = par;
    sh.sel_node[tid] = node;
    ss.sel_kind[tid] = kind;
  }
  gram_sync();
  // a chosen child's raw logit once more (the same function, the same bits): 8 lanes each
  for (int base = 0; base < K; base += NTHR / 8) {
    const int j = base + (tid >> 3);
    const bool act = j < K && ss.sel_kind[j] == 2;
    const float z = sparse_dot(act, act ? sh.lr[sh.sel_par[j]] : 0, act ? sh.sel_tok[j] : 0, tid & 7, hd, emb, emb32, d, pieces);
    if (act && (tid & 7) == 0) ss.sel_z[j] = z;
  }
  gram_sync();
  // the four extra words move with the selection (old values from LDS, so nothing is read after it was overwritten)
  if (tid < K) {
    const int row = row0 + tid, par = sh.sel_par[tid], kind = ss.sel_kind[tid];
    float nphi = -INFINITY, nmodel = -INFINITY;
    unsigned long long npath = 0ull;
    int nfin = 0;
    if (kind == 1) {
      nphi = ss.phi[par];
      nmodel = ss.model[par];
      npath = ((unsigned long long)ss.path_hi[par] << 32) | ss.path_lo[par];
      nfin = ss.fin[par];
    } else if (kind == 2) {
      const int tok = sh.sel_tok[tid];
      const float z = ss.sel_z[tid];
      nphi = child_phi(ss.phi[par], scaled_logit(z, temperature), ss.lse_k[par]);
      nmodel = ss.model[par] + (z - ss.lse_row[par]);
      const Philox w = philox4x32_10(ss.path_lo[par], ss.path_hi[par], (uint32_t)tok, (uint32_t)cur_len, seed_lo, seed_hi);
      npath = ((unsigned long long)w.w[1] << 32) | w.w[0];
      nfin = tok == st.eos ? cur_len + 1 : 0;
    }
    phi[row] = nphi;
    model[row] = nmodel;
    path[row] = npath;
    st.hyp_len[row] = nfin;
  }
  step_advance<NTHR>(a, sh, new_seq, new_anc, b, tid);
}

// dead rows (G = -inf) come back as the start token followed by padding, with -inf in all three
__global__ void sbs_finalize_kernel(gram_beam_state_t st, int max_length, const float* __restrict__ phi, const float* __restrict__ model,
                                    int64_t* __restrict__ sequences, float* __restrict__ seq_logprobs,
                                    float* __restrict__ sample_logprobs, float* __restrict__ perturbed, int32_t* __restrict__ out_width) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= st.B * st.K) return;
  const int T = st.Tmax;
  const float G = st.beam_scores[r];
  const bool dead = !(G > -INFINITY);
  for (int p = 0; p < max_length; ++p) sequences[(size_t)r * max_length + p] = (dead && p > 0) ? st.pad : st.seq[(size_t)r * T + p];
  const float lm = dead ? -INFINITY : model[r], ls = dead ? -INFINITY : phi[r];
  // a NaN or +inf anywhere, or -inf on a row that is not dead, means an activation overflowed upstream
  if (G != G || G > 3.0e38f || (!dead && (!(fabsf(lm) < 3.0e38f) || !(fabsf(ls) < 3.0e38f)))) st.error[0] = 4;
  seq_logprobs[r] = lm;
  sample_logprobs[r] = ls;
  perturbed[r] = dead ? -INFINITY : G;
  const int len = dead ? 1 : (st.hyp_len[r] > 0 ? st.hyp_len[r] : max_length);
  atomicMax(out_width, len < max_length ? len : max_length);
}

int check_sbs_state(const gram_beam_state_t* st) {
  if (!st || st->B < 1 || st->K < 1 || st->K > GRAM_MAX_BEAMS || st->Tmax < 2 || st->Tmax > GRAM_MAX_DEC_LEN ||
      (long long)st->B * st->K > INT32_MAX / GRAM_MAX_DEC_LEN)
    return GRAM_E_ARG;
  if (!st->tokens || !st->node || !st->seq || !st->anc || !st->hyp_len || !st->error || !st->beam_scores) return GRAM_E_ARG;
  return 0;
}

int g_sbs_cap = 0;  // gram_debug_set_sbs_capacity: 0 = kSbsCap

// ui: nothing, or the lists (checked by the caller)
template <typename... UI>
int launch_sbs_step(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden, const void* lm16, const float* lm32, int d,
                    const float* lse, int V, int cur_len, int rows_per_user, int pieces, float temperature, uint64_t seed, float* phi,
                    float* model, uint64_t* path, void* stream, const UI&... ui) {
  if (int e = check_sbs_state(st)) return e;
  if (!tr || !tr->child_off || !tr->child_tok || !tr->child_node || !hidden || (!lm16 && !lm32) || !lse || !phi || !model || !path ||
      cur_len < 1 || cur_len >= st->Tmax || V < 2 || (rows_per_user != 1 && rows_per_user != st->K))
    return GRAM_E_ARG;
  if (d < 64 || (d & 63) || pieces < 1 || pieces > GRAM_MAX_PIECES || (pieces > 1 && !lm32)) return GRAM_E_ARG;
  if (!(temperature > 0.f) || !(temperature < 3.0e38f)) return GRAM_E_ARG;
  if (tr->max_fanout < 0 || tr->max_fanout > V || tr->n_nodes < 1 || (long long)st->K * V > 0xffffffffll) return GRAM_E_ARG;
  const int K = st->K, cap = gram_sbs_capacity();
  const long long worst = (long long)K * tr->max_fanout;  // candidates of one user
  if (worst > cap && (!st->cand_logits || st->cand_logits_users < st->B * K || st->cand_logits_stride < 2 * tr->max_fanout ||
                      (reinterpret_cast<uintptr_t>(st->cand_logits) & 3)))
    return GRAM_E_ARG;
  const int n_lds = (int)(((worst < cap ? (worst > 0 ? worst : 1) : cap) + 3) / 4 * 4);
  const size_t smem = (size_t)kSbsKeys * 8 + (size_t)n_lds * 8 + (size_t)2 * K * st->Tmax * 4;
  if (smem > 150 * 1024) return GRAM_E_ARG;
  static size_t attr_bytes = 48 * 1024;  // (of this instantiation)
  if (smem > attr_bytes) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sbs_step_kernel<UI...>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        e != hipSuccess)
      return (int)e;
    attr_bytes = smem;
  }
  // one piece with a 16-bit lm_head: the search step's one-piece operands; otherwise the fp32 table (sparse_dot)
  const float* const emb32 = (pieces > 1 || !lm16) ? lm32 : nullptr;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(sbs_step_kernel<UI...>, dim3(st->B), dim3(kSbsThreads), smem, (hipStream_t)stream, *st, *tr, (const p16*)hidden,
                     (const p16*)lm16, emb32, d, lse, V, cur_len, rows_per_user, pieces, temperature, (uint32_t)seed,
                     (uint32_t)(seed >> 32), phi, model, reinterpret_cast<unsigned long long*>(path), n_lds, ui...);
  GRAM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int gram_sbs_capacity(void) { return g_sbs_cap > 0 ? g_sbs_cap : kSbsCap; }
extern "C" int gram_debug_set_sbs_capacity(int candidates) {
  if (candidates < 0) return GRAM_E_ARG;
  g_sbs_cap = candidates > kSbsCap ? kSbsCap : candidates;
  return 0;
}

extern "C" int gram_sbs_init(const gram_beam_state_t* st, const gram_trie_t* tr, int start_token, uint64_t seed, const int64_t* user_keys,
                             float* sample_logprob, float* model_logprob, uint64_t* path, void* stream) {
  if (int e = check_sbs_state(st)) return e;
  if (!tr || !user_keys || !sample_logprob || !model_logprob || !path) return GRAM_E_ARG;
  if (int e = gram_beam_init(st, tr, start_token, stream)) return e;
  const int rows = st->B * st->K;
  hipLaunchKernelGGL(sbs_init_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, *st, (uint32_t)seed,
                     (uint32_t)(seed >> 32), user_keys, sample_logprob, model_logprob, reinterpret_cast<unsigned long long*>(path));
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int gram_sbs_step(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16, const void* lm_head_bf16,
                             const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                             float temperature, uint64_t seed, float* sample_logprob, float* model_logprob, uint64_t* path,
                             void* stream) {
  return launch_sbs_step(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, pieces, temperature, seed,
                         sample_logprob, model_logprob, path, stream);
}

extern "C" int gram_sbs_step_items(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16, const void* lm_head_bf16,
                                   const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                                   float temperature, uint64_t seed, float* sample_logprob, float* model_logprob, uint64_t* path,
                                   const gram_user_items_t* items, void* stream) {
  if (int e = check_items(items)) return e;
  return launch_sbs_step(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, pieces, temperature, seed,
                         sample_logprob, model_logprob, path, stream, *items);
}

extern "C" int gram_sbs_finalize(const gram_beam_state_t* st, int max_length, const float* model_logprob, const float* sample_logprob,
                                 int64_t* sequences, float* seq_logprobs, float* sample_logprobs, float* perturbed_scores,
                                 int32_t* out_width, void* stream) {
  if (int e = check_sbs_state(st)) return e;
  if (max_length != st->Tmax || !model_logprob || !sample_logprob || !sequences || !seq_logprobs || !sample_logprobs ||
      !perturbed_scores || !out_width)
    return GRAM_E_ARG;
  hipError_t e = hipMemsetAsync(out_width, 0, sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const int rows = st->B * st->K;
  hipLaunchKernelGGL(sbs_finalize_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, *st, max_length, sample_logprob,
                     model_logprob, sequences, seq_logprobs, sample_logprobs, perturbed_scores, out_width);
  GRAM_CHECK_LAUNCH();
  return 0;
}
