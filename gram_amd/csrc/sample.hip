// sample.hip -- Trie-constrained sampling on the device: HF 4.26 `sample` (generate with do_sample=True, num_beams == 1) restated
// for a Trie (gram_hip.h, "Trie-constrained sampling").
//   PrefixConstrainedLogitsProcessor -> the children of the row's Trie node (with the lists: the alive ones), in token order
//   TemperatureLogitsWarper          -> y = z / temperature on the RAW logits z = h . E[tok] (sparse_dot: the search step's bits)
//   TopKLogitsWarper                 -> y >= the k'-th largest y, found by bisection over the order-preserving integer image
//   TopPLogitsWarper                 -> the ascending cumulative softmax mass, as a second bisection over the same image
//   torch.multinomial                -> inverse-CDF draw from the caller's uniform: first kept child whose running sum exceeds u * W
// One workgroup of 256 threads per ROW (a sample of a user).  Nothing is reordered: a row keeps its cache row, its ancestors and its
// slot, so the step writes its own row's token, node, sequence position and accumulators and nothing else.
//
// A row's candidates are f32 y values, 4 B each: up to kSampleCap = 8 192 of them live in LDS (32 KB + < 1 KB of static tables, so
// four workgroups -- 16 wavefronts -- share a CU's 160 KB; 16 384 would still leave two, but a node with more than 8 192 children is
// a flat catalogue, where the array is written once and swept ~70 times from the L2 just as well).  Beyond the capacity the same
// array lies in st.cand_logits [row][stride]: the same code over another pointer, hence the same bits.
// With the lists (FILT) the alive children are numbered 0 .. n-1 through a bit mask + per-word prefix counts in LDS (8 B per 32
// children); everything behind that numbering sees exactly what the unfiltered kernel sees on Trie(A_b).
#include "common.h"
#include "prof.h"
#include "sparse_dot.h"
#include "trie_dev.h"

namespace {

constexpr int kSampleThreads = 256;
constexpr int kSampleWaves = kSampleThreads / WAVE;
constexpr int kSampleCap = 8192;

// Workgroup reductions and scans in ONE fixed order: lanes by the wave's butterfly (every lane ends with the same bits), then the
// four waves in order.  Each call uses the other half of its 2 x 4 staging words than the call before it, so one barrier per call
// is enough: a wave can be at most one call ahead of the slowest reader.
struct SampleShared {
  float f[2][kSampleWaves];
  int i[2][kSampleWaves];
};

__device__ __forceinline__ float block_sum(SampleShared& sh, int& par, float v, int tid) {
  v = wave_sum(v);
  if ((tid & 63) == 0) sh.f[par][tid >> 6] = v;
  gram_sync();
  const float r = ((sh.f[par][0] + sh.f[par][1]) + sh.f[par][2]) + sh.f[par][3];
  par ^= 1;
  return r;
}
__device__ __forceinline__ float block_max(SampleShared& sh, int& par, float v, int tid) {
  v = wave_max(v);
  if ((tid & 63) == 0) sh.f[par][tid >> 6] = v;
  gram_sync();
  const float r = fmaxf(fmaxf(sh.f[par][0], sh.f[par][1]), fmaxf(sh.f[par][2], sh.f[par][3]));
  par ^= 1;
  return r;
}
__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_imin(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int n = __shfl_xor(v, o, 64);
    v = n < v ? n : v;
  }
  return v;
}
__device__ __forceinline__ int block_isum(SampleShared& sh, int& par, int v, int tid) {
  v = wave_isum(v);
  if ((tid & 63) == 0) sh.i[par][tid >> 6] = v;
  gram_sync();
  const int r = sh.i[par][0] + sh.i[par][1] + sh.i[par][2] + sh.i[par][3];
  par ^= 1;
  return r;
}
__device__ __forceinline__ int block_imin(SampleShared& sh, int& par, int v, int tid) {
  v = wave_imin(v);
  if ((tid & 63) == 0) sh.i[par][tid >> 6] = v;
  gram_sync();
  int r = sh.i[par][0];
#pragma unroll
  for (int w = 1; w < kSampleWaves; ++w) r = sh.i[par][w] < r ? sh.i[par][w] : r;
  par ^= 1;
  return r;
}
// inclusive scan over the workgroup's 256 values in thread order; total = their sum
__device__ __forceinline__ float block_scan(SampleShared& sh, int& par, float v, int tid, float& total) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) sh.f[par][wave] = v;
  gram_sync();
  float off = 0.f, acc = 0.f;
#pragma unroll
  for (int w = 0; w < kSampleWaves; ++w) {
    if (w == wave) off = acc;
    acc += sh.f[par][w];
  }
  total = acc;
  par ^= 1;
  return off + v;
}
__device__ __forceinline__ int block_iscan(SampleShared& sh, int& par, int v, int tid, int& total) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  if (lane == 63) sh.i[par][wave] = v;
  gram_sync();
  int off = 0, acc = 0;
#pragma unroll
  for (int w = 0; w < kSampleWaves; ++w) {
    if (w == wave) off = acc;
    acc += sh.i[par][w];
  }
  total = acc;
  par ^= 1;
  return off + v;
}

// UI: the per-user item filter (filtered(), trie_dev.h).  cap: candidates the dynamic LDS holds; mask_words: words of the alive mask
// (FILT; even, >= the words of max_fanout children).
template <typename... UI>
__global__ __launch_bounds__(kSampleThreads) void sample_step_kernel(gram_beam_state_t st, gram_trie_t tr, const p16* __restrict__ hd,
                                                                     const p16* __restrict__ emb, const float* __restrict__ emb32,
                                                                     int d, const float* __restrict__ lse, int V, int cur_len,
                                                                     int rows_per_user, int pieces, gram_sample_params_t prm,
                                                                     const float* __restrict__ u, int u_stride,
                                                                     float* __restrict__ acc_sample, float* __restrict__ acc_model,
                                                                     int cap, int mask_words, UI... ui) {
  constexpr bool FILT = filtered<UI...>();
  constexpr int NTHR = kSampleThreads;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const cand_lds = reinterpret_cast<float*>(smem);                                 // [cap, rounded up to 4]
  uint32_t* const amask = reinterpret_cast<uint32_t*>(smem + ((size_t)cap * 4 + 15) / 16 * 16);  // [mask_words]  FILT only
  int* const apre = reinterpret_cast<int*>(amask + mask_words);                           // [mask_words]  alive children before a word
  __shared__ SampleShared sh;
  int par = 0;

  const int row = blockIdx.x, tid = threadIdx.x;
  const int K = st.K, T = st.Tmax, b = row / K;
  const int lr = rows_per_user == 1 ? b : row;  // compact step: hidden and lse hold one row per user
  if (tid == 0 && rows_per_user == 1) st.anc[(size_t)(cur_len - 1) * st.B * K + row] = b;  // (slot cur_len - 1 holds one row per user)

  auto emit = [&](int tok, int node, int fin) {  // thread 0
    st.seq[(size_t)row * T + cur_len] = tok;
    st.tokens[row] = tok;
    st.node[row] = node;
    if (fin > 0) st.hyp_len[row] = fin;
  };
  if (st.hyp_len[row] > 0) {  // finished: pad, and the accumulators stay
    if (tid == 0) emit(st.pad, -1, 0);
    return;
  }
  const int nd = st.node[row];
  int off0 = 0, F = 0;
  if (nd >= 0 && nd < tr.n_nodes) {
    off0 = tr.child_off[nd];
    F = tr.child_off[nd + 1] - off0;
  }
  if (F > V) F = 0;  // (a Trie that disagrees with itself: flagged below)

  // ---- the row's children, numbered 0 .. n-1 in token order
  int n = F;
  if constexpr (FILT) {
    const gram_user_items_t& it = *items_ptr(ui...);
    const int nw = (F + 31) >> 5;
    if (nw > mask_words) {
      n = 0;  // (the launcher sized the mask by max_fanout: a wider node is a wrong Trie)
    } else {
      for (int i0 = 0; i0 < F; i0 += NTHR) {  // (a wave tests 64 consecutive children: two mask words per ballot)
        const int i = i0 + tid;
        const bool alive = i < F && node_alive(it, b, tr.child_node[off0 + i]);
        const unsigned long long m = __ballot(alive);
        if ((tid & 63) == 0) {
          const int w0 = (i0 + tid) >> 5;
          if (w0 < nw) amask[w0] = (uint32_t)m;
          if (w0 + 1 < nw) amask[w0 + 1] = (uint32_t)(m >> 32);
        }
      }
      gram_sync();
      int base = 0;
      for (int w0 = 0; w0 < nw; w0 += NTHR) {
        const int w = w0 + tid;
        const int c = w < nw ? __popc(amask[w]) : 0;
        int total;
        const int incl = block_iscan(sh, par, c, tid, total);
        if (w < nw) apre[w] = base + incl - c;
        base += total;
      }
      n = base;
      gram_sync();
    }
  }
  // child index (0 .. F-1) of candidate j
  auto child_of = [&](int j) -> int {
    if constexpr (FILT) {
      int lo = 0, hi = ((F + 31) >> 5) - 1;  // the last word w with apre[w] <= j
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (apre[mid] <= j) lo = mid; else hi = mid - 1;
      }
      uint32_t m = amask[lo];
      for (int k = j - apre[lo]; k > 0; --k) m &= m - 1;
      const int c = (lo << 5) + __ffs((int)m) - 1;
      return c < 0 ? 0 : (c >= F ? F - 1 : c);  // (in range whatever the mask holds)
    } else {
      return j;
    }
  };

  float* cand = cand_lds;
  bool bad = n < 1;
  if (n > cap) {
    if (st.cand_logits && (long long)n <= st.cand_logits_stride && row < st.cand_logits_users) cand = st.cand_logits + (size_t)row * st.cand_logits_stride;
    else bad = true;
  }
  if (bad) {  // no child to draw: HF raises here
    if (tid == 0) {
      st.error[0] = n < 1 ? 1 : 2;
      emit(st.pad, -1, cur_len + 1);
    }
    return;
  }

  // ---- y_i = z_i / temperature: 8 lanes per candidate, two candidates per group and trip (as the search step's sparse_window)
  {
    const int sub = tid & 7, grp = tid >> 3;
    constexpr int NG = NTHR / 8;
    for (int base = 0; base < n; base += 2 * NG) {
      int i2[2], tok2[2];
      bool act2[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) {
        i2[w] = base + NG * w + grp;
        act2[w] = i2[w] < n;
        tok2[w] = act2[w] ? tr.child_tok[off0 + child_of(i2[w])] : 0;
      }
      float z2[2];
#pragma unroll
      for (int w = 0; w < 2; ++w) z2[w] = sparse_dot(act2[w], lr, tok2[w], sub, hd, emb, emb32, d, pieces);
#pragma unroll
      for (int w = 0; w < 2; ++w)
        if (act2[w] && sub == 0) cand[i2[w]] = z2[w] / prm.temperature;
    }
  }
  gram_sync();

  // ---- maximum, and the non-finite check at its source (GRAM_E_NONFINITE)
  float mx = -INFINITY;
  bool nonfinite = false;
  for (int i = tid; i < n; i += NTHR) {
    const float y = cand[i];
    nonfinite |= !(fabsf(y) < 3.0e38f);
    mx = fmaxf(mx, y);
  }
  const float lse_row = lse[lr];
  if (tid == 0) nonfinite |= !(fabsf(lse_row) < 3.0e38f);
  if (nonfinite) st.error[0] = 4;
  const float ymax = block_max(sh, par, mx, tid);
  const uint32_t omax = f2ord(ymax);

  // ---- top_k: the largest o with #{ord(y) >= o} >= k'
  uint32_t thr = 0u;
  if (prm.top_k > 0) {
    const int kk = prm.top_k < n ? prm.top_k : n;
    if (kk < n) {
      uint32_t lo = 0u, hi = omax;
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1) + ((hi - lo) & 1u);
        int c = 0;
        for (int i = tid; i < n; i += NTHR) c += f2ord(cand[i]) >= mid ? 1 : 0;
        if (block_isum(sh, par, c, tid) >= kk) lo = mid; else hi = mid - 1u;
      }
      thr = lo;
    }
  }

  // the weight of candidate i among those at or above `from` and at or below `upto` (ordinals), thread-strided partial sums
  auto mass = [&](uint32_t from, uint32_t upto) -> float {
    float s = 0.f;
    for (int i = tid; i < n; i += NTHR) {
      const float y = cand[i];
      const uint32_t o = f2ord(y);
      if (o >= from && o <= upto) s += expf(y - ymax);
    }
    return block_sum(sh, par, s, tid);
  };

  // ---- top_p over what top_k kept: the smallest o with S(o) = sum_{ord(y) <= o} w > (1 - top_p) * S(max); the maximum always stays.
  // (a fixed-order fp32 sum of non-negative terms is monotone in every term, so S is monotone in o and the bisection is exact)
  if (prm.top_p < 1.0f) {
    const float Wk = mass(thr, omax);
    const float c = (1.0f - prm.top_p) * Wk;
    uint32_t lo = thr, hi = omax;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (mass(thr, mid) > c) hi = mid; else lo = mid + 1u;
    }
    thr = lo;
  }

  // ---- W and the draw: running sums in chunks of 256 candidates (an inclusive scan each, the chunks' totals carried in order)
  auto weight = [&](int i) -> float {
    if (i >= n) return 0.f;
    const float y = cand[i];
    return f2ord(y) >= thr ? expf(y - ymax) : 0.f;
  };
  float W = 0.f;
  int last = -1;  // (of this thread's kept candidates)
  for (int i0 = 0; i0 < n; i0 += NTHR) {
    const float w = weight(i0 + tid);
    if (i0 + tid < n && f2ord(cand[i0 + tid]) >= thr) last = i0 + tid;
    float total;
    (void)block_scan(sh, par, w, tid, total);
    W += total;
  }
  float uu = u[(size_t)row * u_stride];
  uu = fminf(fmaxf(uu, 0.f), 0x1.fffffep-1f);  // (NaN -> 0)
  const float target = uu * W;
  int pick = INT32_MAX;
  float base = 0.f;
  for (int i0 = 0; i0 < n && pick == INT32_MAX; i0 += NTHR) {
    const int i = i0 + tid;
    const float w = weight(i);
    float total;
    const float run = base + block_scan(sh, par, w, tid, total);
    const bool hit = i < n && f2ord(cand[i]) >= thr && run > target;
    pick = block_imin(sh, par, hit ? i : INT32_MAX, tid);
    base += total;
  }
  if (pick == INT32_MAX) pick = -block_imin(sh, par, -last, tid);  // rounding left none: the last kept candidate
  pick = pick < 0 ? 0 : (pick >= n ? n - 1 : pick);                // (NaN logits -- flagged above -- must not index outside the row)

  // ---- the drawn child: its raw logit once more (the same function, the same bits), the accumulators, the row's state
  const int e = off0 + child_of(pick);
  const int tok = tr.child_tok[e];
  const float z = sparse_dot(tid < 8, lr, tok, tid & 7, hd, emb, emb32, d, pieces);
  if (tid == 0) {
    acc_sample[row] += (cand[pick] - ymax) - logf(W);
    acc_model[row] += z - lse_row;
    emit(tok, tr.child_node[e], tok == st.eos ? cur_len + 1 : 0);
  }
}

__global__ void sample_finalize_kernel(gram_beam_state_t st, int max_length, const float* __restrict__ acc_model,
                                       const float* __restrict__ acc_sample, int64_t* __restrict__ sequences,
                                       float* __restrict__ seq_logprobs, float* __restrict__ sample_logprobs,
                                       int32_t* __restrict__ out_width) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= st.B * st.K) return;
  const int T = st.Tmax;
  for (int p = 0; p < max_length; ++p) sequences[(size_t)r * max_length + p] = st.seq[(size_t)r * T + p];
  const float lm = acc_model[r], ls = acc_sample[r];
  // log-probabilities are <= 0 and finite (a draw has positive weight): anything else means an activation overflowed upstream
  if (!(fabsf(lm) < 3.0e38f) || !(fabsf(ls) < 3.0e38f)) st.error[0] = 4;
  seq_logprobs[r] = lm;
  sample_logprobs[r] = ls;
  // HF stops as soon as every row is finished: width = the longest finished length (max_length if any row never finished)
  const int len = st.hyp_len[r] > 0 ? st.hyp_len[r] : max_length;
  atomicMax(out_width, len < max_length ? len : max_length);
}

int check_sample_state(const gram_beam_state_t* st) {
  if (!st || st->B < 1 || st->K < 1 || st->K > GRAM_MAX_BEAMS || st->Tmax < 2 || st->Tmax > GRAM_MAX_DEC_LEN ||
      (long long)st->B * st->K > INT32_MAX / GRAM_MAX_DEC_LEN)
    return GRAM_E_ARG;
  if (!st->tokens || !st->node || !st->seq || !st->anc || !st->hyp_len || !st->error) return GRAM_E_ARG;
  return 0;
}

int g_sample_cap = 0;  // gram_debug_set_sample_capacity: 0 = kSampleCap

// ui: nothing, or the lists (checked by the caller)
template <typename... UI>
int launch_sample_step(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden, const void* lm16, const float* lm32, int d,
                       const float* lse, int V, int cur_len, int rows_per_user, int pieces, const gram_sample_params_t* prm,
                       const float* u, int u_stride, float* acc_sample, float* acc_model, void* stream, const UI&... ui) {
  if (int e = check_sample_state(st)) return e;
  if (!tr || !tr->child_off || !tr->child_tok || !tr->child_node || !hidden || (!lm16 && !lm32) || !lse || !prm || !u || !acc_sample ||
      !acc_model || cur_len < 1 || cur_len >= st->Tmax || V < 2 || (rows_per_user != 1 && rows_per_user != st->K) || u_stride < 1)
    return GRAM_E_ARG;
  if (d < 64 || (d & 63) || pieces < 1 || pieces > GRAM_MAX_PIECES || (pieces > 1 && !lm32)) return GRAM_E_ARG;
  if (!(prm->temperature > 0.f) || !(prm->temperature < 3.0e38f) || prm->top_k < 0 || !(prm->top_p > 0.f) || !(prm->top_p <= 1.f))
    return GRAM_E_ARG;
  if (tr->max_fanout < 0 || tr->max_fanout > V || tr->n_nodes < 1) return GRAM_E_ARG;
  const int rows = st->B * st->K;
  const int cap = gram_sample_capacity();
  if (tr->max_fanout > cap && (!st->cand_logits || st->cand_logits_users < rows || st->cand_logits_stride < tr->max_fanout)) return GRAM_E_ARG;
  const int n_lds = tr->max_fanout < cap ? (tr->max_fanout > 0 ? tr->max_fanout : 1) : cap;
  const int words = filtered<UI...>() ? (tr->max_fanout + 63) / 64 * 2 + 2 : 0;
  const size_t smem = ((size_t)n_lds * 4 + 15) / 16 * 16 + (size_t)words * 8;
  if (smem > 150 * 1024) return GRAM_E_ARG;
  static size_t attr_bytes = 48 * 1024;  // (of this instantiation)
  if (smem > attr_bytes) {
    if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sample_step_kernel<UI...>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        e != hipSuccess)
      return (int)e;
    attr_bytes = smem;
  }
  // one piece with a 16-bit lm_head: the search step's one-piece operands; otherwise the fp32 table (sparse_dot)
  const float* const emb32 = (pieces > 1 || !lm16) ? lm32 : nullptr;
  gram_prof::Scope prof(GRAM_K_BEAM, (hipStream_t)stream, 0.0);
  hipLaunchKernelGGL(sample_step_kernel<UI...>, dim3(rows), dim3(kSampleThreads), smem, (hipStream_t)stream, *st, *tr, (const p16*)hidden,
                     (const p16*)lm16, emb32, d, lse, V, cur_len, rows_per_user, pieces, *prm, u, u_stride, acc_sample, acc_model, n_lds, words,
                     ui...);
  GRAM_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int gram_sample_capacity(void) { return g_sample_cap > 0 ? g_sample_cap : kSampleCap; }
extern "C" int gram_debug_set_sample_capacity(int candidates) {
  if (candidates < 0) return GRAM_E_ARG;
  g_sample_cap = candidates > kSampleCap ? kSampleCap : candidates;
  return 0;
}

extern "C" int gram_sample_step(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16, const void* lm_head_bf16,
                                const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                                const gram_sample_params_t* params, const float* u, int u_stride, float* sample_logprob,
                                float* model_logprob, void* stream) {
  return launch_sample_step(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, pieces, params, u, u_stride,
                            sample_logprob, model_logprob, stream);
}

extern "C" int gram_sample_step_items(const gram_beam_state_t* st, const gram_trie_t* tr, const void* hidden_bf16, const void* lm_head_bf16,
                                      const float* lm_head_f32, int d, const float* lse, int V, int cur_len, int rows_per_user, int pieces,
                                      const gram_sample_params_t* params, const float* u, int u_stride, float* sample_logprob,
                                      float* model_logprob, const gram_user_items_t* items, void* stream) {
  if (int e = check_items(items)) return e;
  return launch_sample_step(st, tr, hidden_bf16, lm_head_bf16, lm_head_f32, d, lse, V, cur_len, rows_per_user, pieces, params, u, u_stride,
                            sample_logprob, model_logprob, stream, *items);
}

extern "C" int gram_sample_finalize(const gram_beam_state_t* st, int max_length, const float* model_logprob, const float* sample_logprob,
                                    int64_t* sequences, float* seq_logprobs, float* sample_logprobs, int32_t* out_width, void* stream) {
  if (int e = check_sample_state(st)) return e;
  if (max_length != st->Tmax || !model_logprob || !sample_logprob || !sequences || !seq_logprobs || !sample_logprobs || !out_width)
    return GRAM_E_ARG;
  hipError_t e = hipMemsetAsync(out_width, 0, sizeof(int32_t), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const int rows = st->B * st->K;
  hipLaunchKernelGGL(sample_finalize_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream, *st, max_length, model_logprob,
                     sample_logprob, sequences, seq_logprobs, sample_logprobs, out_width);
  GRAM_CHECK_LAUNCH();
  return 0;
}
