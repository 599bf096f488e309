// xattn_long.hip -- the decode cross-attention over fused contexts of up to GRAM_MAX_LONG_FUSED_LEN = 16 384 keys
// (gram_model_set_max_fused_len; dec_attn.hip's cross_attn_kernel holds a user's key bits in two words per lane: <= 4096 keys).
//
// Split-key: a user's VALID 32-key steps, counted in key order, are cut into segments of 128; one workgroup of two waves per
// (head, user, segment) runs the 32-key step of xattn_tile.h (xa_step_qk, xa_step_pv) over its segment -- cross_attn_kernel's K / V^T
// tiles by LDS-DMA, its half-stage refill, its three-product MFMA order, wave w owning the steps of ordinal parity w -- and merges the two
// waves' partial softmaxes (m, l, O[64]) UNNORMALISED.  A user whose valid steps fit one segment is normalised and stored by that
// workgroup; otherwise the segment leaves its partial in fp32 scratch and cross_attn_long_merge_kernel folds a row's partials in
// ascending segment order, normalises, splits into pieces and stores.  No atomics; every sum has one fixed order.
//
// What a row's bits depend on: the query row and the user's valid steps IN ORDER (each with its word of key bits) -- the segment of a
// step, the wave that takes it and the fold are functions of the step's ordinal among the user's valid steps alone.  They do not
// depend on B or the user's place in the batch, on K (every beam-tile count runs two waves), on the live-row form, or on where the
// masked steps between the valid ones lie (the batch's L and N, trailing masked passages, keys moving across a multiple of 4096).
// A user without any valid key keeps every step: the uniform row over exactly S keys (the reference's softmax over all-finfo.min
// scores), which by definition depends on S.  Fully masked steps are never fetched; in a partly masked step of a user that has
// valid keys the masked keys' V^T columns are zeroed in registers, so that whatever the bank holds there -- NaN included --
// contributes exactly nothing (their scores are replaced by finfo.min before the softmax already).
#include "common.h"
#include "prof.h"
#include "xattn_tile.h"

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int XL_SEG_STEPS = 128;                      // valid steps per segment (4096 keys)
constexpr int XL_WORDS = GRAM_KEY_BITS_LONG_WORDS;     // step words of a key_bits row
constexpr int XL_STRIDE = GRAM_KEY_BITS_LONG_STRIDE;   // words between rows; word XL_WORDS = the user's number of valid steps
constexpr int XL_PART = 68;                            // floats of one partial: O[64], m, l, two of padding (16-B rows)

// The fold of two unnormalised partial softmaxes, spelled out once for the two-wave merge and the segment merge (hipcc decides fma
// contraction per call site): weights, then a * wa + b * wb for l and every element of O; the normalisation at the very end.
__device__ __forceinline__ void xl_fold_w(float ma, float mb, float& M, float& wa, float& wb) {
  M = fmaxf(fmaxf(GRAM_FMIN, ma), mb);
  wa = __expf(ma - M);
  wb = __expf(mb - M);
}
__device__ __forceinline__ float xl_fold(float a, float b, float wa, float wb) { return __builtin_fmaf(b, wb, a * wa); }
__device__ __forceinline__ f32x4 xl_fold4(f32x4 a, f32x4 b, float wa, float wb) {
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = xl_fold(a[e], b[e], wa, wb);
  return r;
}
__device__ __forceinline__ f32x4 xl_norm(f32x4 o, float l) {
  const float inv = 1.f / l;
  f32x4 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) r[e] = o[e] * inv;
  return r;
}
__device__ __forceinline__ unsigned long long uniform64(unsigned long long v) {
  return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
         ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
}
// a[i] of eight wave-uniform values by a wave-uniform index, without a dynamically indexed array (0 past the end)
__device__ __forceinline__ unsigned long long sel8(const unsigned long long (&a)[8], int i) {
  unsigned long long r = 0ull;
#pragma unroll
  for (int j = 0; j < 8; ++j) r = i == j ? a[j] : r;
  return r;
}

// NT = 16-beam tiles; LIVE: live-row step (gram_live_rows_t); S = bf16 pieces.  Grid (H, users, segments), two waves.
template <int NT, bool LIVE, int S>
__global__ __launch_bounds__(128) void cross_attn_long_kernel(
    const p16* __restrict__ q, const p16* __restrict__ kbank, const p16* __restrict__ vtbank, p16* __restrict__ out, int K, int H,
    int Sk, const int32_t* __restrict__ users, const int32_t* __restrict__ rowpos, long q_pstride, long bank_pstride,
    const uint32_t* __restrict__ key_bits, float* __restrict__ scratch) {
  constexpr int NW = 2;
  constexpr int NB = NT * 16;        // padded beams
  constexpr int PSTR = 2 * XA_TILE;  // piece stride inside the stage: K tile | V^T tile
  constexpr int STAGE = S * PSTR;    // per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* sm_m = reinterpret_cast<float*>(smem);  // [NW][NB]     (the merge buffers alias the stages)
  float* sm_l = sm_m + NW * NB;                  // [NW][NB]
  float* sm_o = sm_l + NW * NB;                  // [NW][NB][64]

  const int h = blockIdx.x, y = blockIdx.y, z = blockIdx.z, nseg = gridDim.z;
  const int b = LIVE ? users[y] : y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int inner = H * 64;
  const int nsteps = Sk >> 5;

  // The user's key bits: lane holds the words of steps lane + 64 j.  One ballot per j says which steps have a valid key.
  uint32_t kw[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int st = lane + 64 * j;
    kw[j] = st < nsteps ? key_bits[(size_t)b * XL_STRIDE + st] : 0u;
  }
  unsigned long long v[8];
  int total = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    v[j] = uniform64(__ballot(kw[j] != 0u));
    total += __builtin_popcountll(v[j]);
  }
  const bool any = total != 0;
  if (!any) {  // no valid key at all: every step, uniform over exactly Sk keys
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int rem = nsteps - 64 * j;
      v[j] = rem >= 64 ? ~0ull : (rem > 0 ? ((1ull << rem) - 1ull) : 0ull);
    }
    total = nsteps;
  }
  const int nseg_user = (total + XL_SEG_STEPS - 1) / XL_SEG_STEPS;
  if (z >= nseg_user) return;  // (the whole workgroup: nothing of this user falls into this segment)
  const bool direct = nseg_user == 1;

  const char* kb = reinterpret_cast<const char*>(kbank + ((size_t)b * H + h) * Sk * 64);
  const char* vt = reinterpret_cast<const char*>(vtbank + ((size_t)b * H + h) * 64 * Sk);

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
  // query fragments (lane: beam 16 nt + c, dims 32 kd + 8 g ..+7 of the head; zeros for a beam that has no row)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int qrow = xa_row<LIVE>(b, K, 16 * nt + c, rowpos);
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd)
        qf[pc][nt][kd] = qrow >= 0 ? ld_global_b128(q + pc * q_pstride + (size_t)qrow * inner + h * 64 + 32 * kd + 8 * g) : zero_bf16x8();
  }

  // The segment's steps: the valid steps of ordinals [128 z, 128 z + 128), dealt to the waves by ordinal parity.  Scalar state: the
  // word of valid-step bits being consumed, what is left of it, and the steps left in the segment.
  int wi = 0, left = total - XL_SEG_STEPS * z, ord = 0;
  left = left < XL_SEG_STEPS ? left : XL_SEG_STEPS;
  unsigned long long bits = v[0];
  for (int skip = XL_SEG_STEPS * z; skip > 0;) {
    const int pc = __builtin_popcountll(bits);
    if (pc <= skip && wi < 7) {
      skip -= pc;
      bits = sel8(v, ++wi);
    } else {
      bits &= bits - 1ull;
      --skip;
    }
  }
  auto next = [&]() -> int {
    while (left > 0) {
      while (bits == 0ull && wi < 7) bits = sel8(v, ++wi);
      if (bits == 0ull) break;  // (cannot happen: `left` counts set bits)
      const int s = 64 * wi + __builtin_ctzll(bits);
      bits &= bits - 1ull;
      --left;
      const bool mine = ord == wave;
      ord ^= 1;
      if (mine) return s;
    }
    return nsteps;
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

  // per-lane byte offsets of this lane's 16 B in each of the 4 + 4 DMA instructions of a (step, piece)
  uint32_t koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kr = 8 * i + (lane >> 3);  // key row of the tile; the lane lands at position lane & 7 and fetches chunk pos ^ ksw
    koff[i] = (uint32_t)(kr * 128 + (((lane & 7) ^ ksw(kr)) << 4));
    const int d = 16 * i + (lane >> 2);  // V^T row; position lane & 3
    voff[i] = (uint32_t)(d * 64 + (((lane & 3) ^ vsw(d)) << 4));
  }
  const uint32_t stage0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem + wave * STAGE;
  auto issue_k = [&](int step) {
    const uint32_t dst = stage0;
#pragma unroll
    for (int pc = 0; pc < S; ++pc) {
      const char* kbase = kb + (size_t)pc * bank_pstride * 2 + (size_t)step * (32 * 128);
#pragma unroll
      for (int i = 0; i < 4; ++i) dma16_nt(dst + pc * PSTR + i * 1024, koff[i], kbase);
    }
  };
  auto issue_v = [&](int step) {
    const uint32_t dst = stage0;
#pragma unroll
    for (int pc = 0; pc < S; ++pc) {
      const char* vbase = vt + (size_t)pc * bank_pstride * 2 + (size_t)step * 4096;
#pragma unroll
      for (int i = 0; i < 4; ++i) dma16(dst + pc * PSTR + XA_TILE + i * 1024, voff[i], vbase);
    }
  };
  const int krow = 8 * (c >> 2) + (c & 3);  // + 4t: key row of S^T tile t this lane feeds
  p16x8 kf[S][2][2], vf[S][4];
  auto read_k = [&]() {
    const char* stg = smem + wave * STAGE;
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int kd = 0; kd < 2; ++kd) {
          const int r = krow + 4 * t;
          kf[pc][t][kd] = *reinterpret_cast<const p16x8*>(stg + pc * PSTR + r * 128 + (((g + 4 * kd) ^ ksw(r)) << 4));
        }
  };
  auto read_v = [&]() {
    const char* stg = smem + wave * STAGE;
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int d = 16 * mt + c;
        vf[pc][mt] = *reinterpret_cast<const p16x8*>(stg + pc * PSTR + XA_TILE + d * 64 + ((g ^ vsw(d)) << 4));
      }
  };
  // a partly masked step: this lane's V^T fragments hold keys 8 g ..+7 of every row -- the masked ones become +0
  auto mask_v = [&](uint32_t kword) {
    const uint32_t k8 = kword >> (8 * g);
    uint32_t vm[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vm[i] = (((k8 >> (2 * i)) & 1u) ? 0xffffu : 0u) | (((k8 >> (2 * i + 1)) & 1u) ? 0xffff0000u : 0u);
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        u32x4 u = __builtin_bit_cast(u32x4, vf[pc][mt]);
#pragma unroll
        for (int i = 0; i < 4; ++i) u[i] &= vm[i];
        vf[pc][mt] = __builtin_bit_cast(p16x8, u);
      }
  };
  p16x8 pf[S][NT];  // exp(S^T - max) of the step, as pieces: the B operand of O^T += V^T P^T
  // the shared 32-key step on this kernel's registers (through lambdas: see cross_attn_kernel, dec_attn.hip)
  auto step_qk = [&](uint32_t kword) { xa_step_qk<NT>(kword, g, kf, qf, pf, m, l, o); };
  auto step_pv = [&]() { xa_step_pv<NT>(vf, pf, o); };

  // ordinary loads (the key bits, the query fragments) are retired so that the counted waits below see DMA instructions only
  wait_vm<0>();
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int pc = 0; pc < S; ++pc)
#pragma unroll
      for (int kd = 0; kd < 2; ++kd) asm volatile("" : "+v"(qf[pc][nt][kd]));
  // one stage per wave, consumed and re-filled in halves, as in cross_attn_kernel; the arithmetic of a step is xattn_tile.h's.  (The DMA,
  // the fragment reads and the query load stay spelled out: through the shared functions this kernel did not time inside the parent's spread.)
  int cur = next();
  if (cur < nsteps) {
    issue_k(cur);
    issue_v(cur);
  }
  while (cur < nsteps) {
    const int nxt = next();
    const uint32_t kword = step_word(cur);
    wait_vm<4 * S>();  // all but the newest half-stage (this step's V^T tiles): its K tiles have landed
    read_k();
    if (nxt < nsteps) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the K fragments are in registers before their tiles are re-filled
      issue_k(nxt);
    }
    step_qk(kword);
    if (nxt < nsteps) wait_vm<4 * S>();  // (newest: the next step's K tiles)
    else wait_vm<0>();
    read_v();
    if (nxt < nsteps) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      issue_v(nxt);
    }
    if (any && kword != 0xffffffffu) mask_v(kword);
    step_pv();
    cur = nxt;
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
    float M, w0, w1;
    xl_fold_w(sm_m[beam], sm_m[NB + beam], M, w0, w1);
    const float ls = xl_fold(sm_l[beam], sm_l[NB + beam], w0, w1);
    const f32x4 ov = xl_fold4(*reinterpret_cast<const f32x4*>(sm_o + ((size_t)beam) * 64 + d4),
                              *reinterpret_cast<const f32x4*>(sm_o + ((size_t)(NB + beam)) * 64 + d4), w0, w1);
    if (direct) {
      int orow = b * K + beam;
      if constexpr (LIVE) orow = rowpos[orow];
      if (orow >= 0) xa_store<S>(out, orow, inner, h * 64 + d4, xl_norm(ov, ls));
    } else {
      // the partial of (slot y * K + beam, head, segment): slots are the launch's own (user, beam) pairs, live or not
      float* p = scratch + ((((size_t)y * K + beam) * H + h) * nseg + z) * XL_PART;
      *reinterpret_cast<f32x4*>(p + d4) = ov;
      if (d4 == 0) {
        p[64] = M;
        p[65] = ls;
      }
    }
  }
}

// folds the partials of the users whose valid steps span more than one segment, in ascending segment order
template <bool LIVE, int S>
__global__ __launch_bounds__(256) void cross_attn_long_merge_kernel(const float* __restrict__ scratch, p16* __restrict__ out, int K, int H,
                                                                    int Sk, const int32_t* __restrict__ users,
                                                                    const int32_t* __restrict__ rowpos,
                                                                    const uint32_t* __restrict__ key_bits, int nseg) {
  const int h = blockIdx.x, y = blockIdx.y;
  const int b = LIVE ? users[y] : y;
  const int cnt = (int)key_bits[(size_t)b * XL_STRIDE + XL_WORDS];
  const int total = cnt ? cnt : (Sk >> 5);
  int nseg_user = (total + XL_SEG_STEPS - 1) / XL_SEG_STEPS;
  nseg_user = nseg_user < nseg ? nseg_user : nseg;
  if (nseg_user <= 1) return;  // stored by its one segment
  const int inner = H * 64;
  for (int idx = threadIdx.x; idx < K * 16; idx += 256) {
    const int beam = idx >> 4, d4 = (idx & 15) * 4;
    int orow = b * K + beam;
    if constexpr (LIVE) orow = rowpos[orow];
    if (orow < 0) continue;
    const float* p = scratch + ((((size_t)y * K + beam) * H + h) * nseg) * XL_PART;
    float mm = p[64], ll = p[65];
    f32x4 ov = *reinterpret_cast<const f32x4*>(p + d4);
    for (int zz = 1; zz < nseg_user; ++zz) {
      const float* pz = p + (size_t)zz * XL_PART;
      float M, wa, wb;
      xl_fold_w(mm, pz[64], M, wa, wb);
      ll = xl_fold(ll, pz[65], wa, wb);
      ov = xl_fold4(ov, *reinterpret_cast<const f32x4*>(pz + d4), wa, wb);
      mm = M;
    }
    xa_store<S>(out, orow, inner, h * 64 + d4, xl_norm(ov, ll));
  }
}

// key_bits[b]: XL_WORDS step words (bit j of word st = mask[b][32 st + j] != 0, zero from S / 32 on), then the number of nonzero
// words, then zeros up to XL_STRIDE
__global__ __launch_bounds__(512) void mask_key_bits_long_kernel(const uint8_t* __restrict__ mask, uint32_t* __restrict__ bits, int Sk) {
  const int b = blockIdx.x, st = threadIdx.x;
  uint32_t w = 0;
  if (st < (Sk >> 5)) w = xa_pack32(mask + (size_t)b * Sk + 32 * st);
  bits[(size_t)b * XL_STRIDE + st] = w;
  const int cnt = __syncthreads_count(w != 0u);
  if (st < XL_STRIDE - XL_WORDS) bits[(size_t)b * XL_STRIDE + XL_WORDS + st] = st == 0 ? (uint32_t)cnt : 0u;
}

struct XlLaunch {
  const void *q, *k, *vt;
  void* out;
  int B, K, H, Sk;
  const int32_t *users, *rowpos;
  long q_ps, bank_ps;
  const uint32_t* key_bits;
  float* scratch;
  hipStream_t st;
};

inline int xl_segments(int S) { return (S + 32 * XL_SEG_STEPS - 1) / (32 * XL_SEG_STEPS); }

// Two waves at every beam-tile count (dec_attn.hip runs one above two tiles): a row's bits must not depend on K.
template <int NT, int S>
int launch_long(const XlLaunch& a) {
  constexpr int NB = NT * 16;
  constexpr int stages = 2 * S * 2 * XA_TILE, merge = (2 * 2 * NB + 2 * NB * 64) * 4;
  constexpr int smem = stages > merge ? stages : merge;
  static_assert(smem <= 160 * 1024, "the stages do not fit the LDS");
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_long_kernel<NT, false, S>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e == hipSuccess)
      e = hipFuncSetAttribute(reinterpret_cast<const void*>(cross_attn_long_kernel<NT, true, S>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return (int)e;
    attr_set = true;
  }
  const dim3 grid(a.H, a.B, xl_segments(a.Sk));
  if (a.users)
    hipLaunchKernelGGL((cross_attn_long_kernel<NT, true, S>), grid, dim3(128), smem, a.st, (const p16*)a.q, (const p16*)a.k,
                       (const p16*)a.vt, (p16*)a.out, a.K, a.H, a.Sk, a.users, a.rowpos, a.q_ps, a.bank_ps, a.key_bits, a.scratch);
  else
    hipLaunchKernelGGL((cross_attn_long_kernel<NT, false, S>), grid, dim3(128), smem, a.st, (const p16*)a.q, (const p16*)a.k,
                       (const p16*)a.vt, (p16*)a.out, a.K, a.H, a.Sk, a.users, a.rowpos, a.q_ps, a.bank_ps, a.key_bits, a.scratch);
  GRAM_CHECK_LAUNCH();
  return 0;
}

template <int S>
int launch_long_nt(const XlLaunch& a) {
  int e;
  switch ((a.K + 15) / 16) {
    case 1: e = launch_long<1, S>(a); break;
    case 2: e = launch_long<2, S>(a); break;
    case 3: e = launch_long<3, S>(a); break;
    default: e = launch_long<4, S>(a); break;
  }
  const int nseg = xl_segments(a.Sk);
  if (e || nseg == 1) return e;  // (one segment: every user was stored by it)
  if (a.users)
    hipLaunchKernelGGL((cross_attn_long_merge_kernel<true, S>), dim3(a.H, a.B), dim3(256), 0, a.st, a.scratch, (p16*)a.out, a.K, a.H, a.Sk,
                       a.users, a.rowpos, a.key_bits, nseg);
  else
    hipLaunchKernelGGL((cross_attn_long_merge_kernel<false, S>), dim3(a.H, a.B), dim3(256), 0, a.st, a.scratch, (p16*)a.out, a.K, a.H, a.Sk,
                       a.users, a.rowpos, a.key_bits, nseg);
  GRAM_CHECK_LAUNCH();
  return 0;
}

inline bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int gram_mask_key_bits_long(const uint8_t* mask, uint32_t* key_bits, int B, int S, void* stream) {
  if (!mask || !key_bits || B < 1 || S < 32 || (S & 31) || S > GRAM_MAX_LONG_FUSED_LEN || misaligned(mask, 16) || misaligned(key_bits, 4))
    return GRAM_E_ARG;
  hipLaunchKernelGGL(mask_key_bits_long_kernel, dim3(B), dim3(XL_WORDS), 0, (hipStream_t)stream, mask, key_bits, S);
  GRAM_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t gram_cross_attn_long_scratch_bytes(int rows, int H, int S) {
  if (rows < 1 || H < 1 || S < 32 || (S & 31) || S > GRAM_MAX_LONG_FUSED_LEN) return GRAM_E_ARG;
  const int nseg = xl_segments(S);
  return nseg == 1 ? 0 : (int64_t)rows * H * nseg * XL_PART * (int64_t)sizeof(float);
}

namespace {
// every refusal of the long cross-attention, before any launch (rows_q: the rows q holds, 0 = not known: a live-row call)
int xl_check(const void* q, const void* k_layer, const void* vt_layer, const void* out, int B, int K, int H, int S, const int32_t* users,
             const int32_t* rowpos, int pieces, int64_t q_pstride, int64_t bank_pstride, const uint32_t* key_bits, const float* scratch,
             int64_t rows_q) {
  if (!q || !k_layer || !vt_layer || !out || !key_bits || B < 1 || K < 1 || K > GRAM_MAX_BEAMS || H < 1 || S < 32 || (S & 31) ||
      S > GRAM_MAX_LONG_FUSED_LEN || pieces < 1 || pieces > GRAM_MAX_PIECES || (users == nullptr) != (rowpos == nullptr))
    return GRAM_E_ARG;
  if (S > GRAM_MAX_FUSED_LEN && !scratch) return GRAM_E_ARG;
  if (pieces > 1 && (q_pstride < (rows_q ? rows_q * H * 64 : 1) || bank_pstride < (int64_t)H * S * 64)) return GRAM_E_ARG;
  if (misaligned(q, 16) || misaligned(k_layer, 16) || misaligned(vt_layer, 16) || misaligned(out, 8) || misaligned(key_bits, 4) ||
      misaligned(scratch, 16) || (pieces > 1 && (q_pstride & 7)))
    return GRAM_E_ARG;
  return 0;
}
}  // namespace

extern "C" int gram_cross_attn_long_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out, int B,
                                          int K, int H, int S, const int32_t* users, const int32_t* rowpos, int pieces, int64_t q_pstride,
                                          int64_t bank_pstride, const uint32_t* key_bits, float* scratch, void* stream) {
  (void)mask;  // (the key bits are the kernel's whole view of the mask)
  // (the live-row form's q holds the step's compact rows, whose number this call does not know)
  const int bad = xl_check(q, k_layer, vt_layer, out, B, K, H, S, users, rowpos, pieces, q_pstride, bank_pstride, key_bits, scratch,
                           users ? 0 : (int64_t)B * K);
  if (bad) return bad;
  hipStream_t st = (hipStream_t)stream;
  gram_prof::Scope prof(GRAM_K_CROSS_ATTN, st, 4.0 * B * H * S * 64 * pieces);  // K + V^T, bf16, every piece
  const XlLaunch a{q, k_layer, vt_layer, out, B, K, H, S, users, rowpos, (long)q_pstride, (long)bank_pstride, key_bits, scratch, st};
  return pieces == 2 ? launch_long_nt<2>(a) : launch_long_nt<1>(a);
}

extern "C" int gram_cross_attn_rows_long_split(const void* q, const void* k_layer, const void* vt_layer, const uint8_t* mask, void* out,
                                               int B, int Q, int H, int S, int pieces, int64_t q_pstride, int64_t bank_pstride,
                                               const uint32_t* key_bits, float* scratch, int32_t* rowmap, void* stream) {
  if (Q < 1) return GRAM_E_ARG;
  if (Q <= GRAM_MAX_BEAMS)  // one call: rows b * Q + i are the kernel's own (user, beam) rows
    return gram_cross_attn_long_split(q, k_layer, vt_layer, mask, out, B, Q, H, S, nullptr, nullptr, pieces, q_pstride, bank_pstride, key_bits,
                                      scratch, stream);
  if (!rowmap || (int64_t)B * Q > INT32_MAX) return GRAM_E_ARG;
  int32_t* users = rowmap;
  int32_t* full = users + B;
  int32_t* tail = full + (size_t)B * GRAM_MAX_BEAMS;
  const int bad = xl_check(q, k_layer, vt_layer, out, B, GRAM_MAX_BEAMS, H, S, users, full, pieces, q_pstride, bank_pstride, key_bits, scratch,
                           (int64_t)B * Q);
  if (bad) return bad;
  const int e0 = gram_tf_rowmap(rowmap, B, Q, stream);
  if (e0) return e0;
  const size_t inner = (size_t)H * 64;
  for (int r0 = 0; r0 < Q; r0 += GRAM_MAX_BEAMS) {
    const int kc = Q - r0 < GRAM_MAX_BEAMS ? Q - r0 : GRAM_MAX_BEAMS;
    // q planar: row r0 of every piece is r0 * inner elements in (the pieces stay q_pstride apart); out: [rows][pieces * inner]
    const int e = gram_cross_attn_long_split((const p16*)q + r0 * inner, k_layer, vt_layer, mask, (p16*)out + r0 * inner * pieces, B, kc, H, S,
                                             users, kc == GRAM_MAX_BEAMS ? full : tail, pieces, q_pstride, bank_pstride, key_bits, scratch,
                                             stream);
    if (e) return e;
  }
  return 0;
}
