// forest_attn.hip -- the decoder self-attention of the tail pass (generate.hip, tail_pass): every row of the forest in ONE launch per
// layer (gram_dec_self_attn_forest_split).
//
// dec_self_attn_forest_kernel: forest row i stands at position p = pos[i] >= t0 of the beam root[i].  It attends, in position order,
//   positions j < t0        the search's cache rows (j, anc[j][root[i]]) -- what the decode steps before the pass wrote;
//   positions t0 <= j < p   the k and v columns of the q|k|v row of its ancestor at position j, found by walking parent[] from i:
//                           the pass's QKV GEMM (or the token table of layer 0) holds q|k|v of ALL forest rows before this launch;
//   position p              its own k and v,
// and writes row i of `out`.  Nothing goes through the cache, so there are no levels to run one after the other, no gather by slot
// and no scatter: the level-by-level train of the step-wise kernel (dec_attn.hip) that this replaces wrote every row's k and v to
// cache rows only later levels of the same pass read.  The arithmetic of a row is self_attn_row.h's -- the one text the step-wise
// kernel calls too -- over the same pieces in the same order, so a forest row gets the bits the level train gives it.
// One workgroup per row, 16 * H threads (a row's loads are whole lines), no LDS, no barrier.  Every index that decides where a
// workgroup goes is the same for all its threads: the compiler keeps the tables' loads and the walk on the scalar unit.
#include <stdlib.h>

#include "common.h"
#include "prof.h"
#include "self_attn_row.h"

namespace {

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// qkv_rows != NULL: qkv is a per-token table and forest row r reads its row qkv_rows[r] (layer 0: the forest's tokens).
// xcd_chunk > 0: workgroup w serves row (w % 8) * xcd_chunk + w / 8 -- workgroups are dealt round-robin to the 8 XCDs, so each XCD
// gets a contiguous eighth of the rows and a row's ancestors, a few rows before it, went through the L2 it asks.
template <int S>
__global__ __launch_bounds__(256) void dec_self_attn_forest_kernel(
    const p16* __restrict__ qkv, const int32_t* __restrict__ qkv_rows, const p16* __restrict__ kcache, const p16* __restrict__ vcache,
    const int32_t* __restrict__ anc, const int32_t* __restrict__ pos, const int32_t* __restrict__ parent,
    const int32_t* __restrict__ root, const float* __restrict__ bias, p16* __restrict__ out, int n_rows, int R, int H, int t0, int Tmax,
    int nlev, long qkv_ps, long cache_ps, int xcd_chunk) {
  constexpr int U = 2, ML = GRAM_TAIL_MAX_STEPS;
  static_assert(ML % U == 0, "the in-pass ancestors are taken in whole batches");
  const int w = blockIdx.x, tid = threadIdx.x;  // tid: 16 threads per head, 4 dims each
  const int i = xcd_chunk > 0 ? (w & 7) * xcd_chunk + (w >> 3) : w;
  if (i >= n_rows) return;
  const int p = pos[i], l = p - t0;  // l: the row's level = its in-pass ancestors
  if (l < 0 || l >= nlev || p >= Tmax) return;  // (a row below the call's last level is not this launch's: tail_pass)
  const int inner = H * 64, h = tid >> 4;
  const int rt = clampi(root[i], 0, R - 1);  // (as tail_anc_kernel clamps it)
  auto src = [&](int r) { return qkv + (size_t)(qkv_rows ? qkv_rows[r] : r) * 3 * inner + 4 * tid; };
  const float* const bias_h = bias + h * GRAM_MAX_DEC_LEN;

  // the row's own q | k | v
  const p16* const row = src(i);
  p16x4 q4[S], k4[S], v4[S];
#pragma unroll
  for (int pc = 0; pc < S; ++pc) {
    q4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps);
    k4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps + inner);
    v4[pc] = *reinterpret_cast<const p16x4*>(row + pc * qkv_ps + 2 * inner);
  }
  // Cached positions in batches of U, as in dec_self_attn_kernel: the U ancestor indices go out together, then the 2 * S * U row
  // loads they address -- two round trips per batch, not two per position.  U = 2 where that kernel has 8, and a batch of cached
  // positions and a batch of in-pass ancestors in flight together (below): what this kernel is short of is workgroups in flight
  // per CU, not loads in flight per workgroup.  Measured on the bench, self-attention per step (profiles/forest_attn_bench_ab.txt):
  // U = 8: 46.5 ms (165 registers in the two-piece form, three waves per SIMD), 4: 36.2 (100), 4 with the loads of absent levels
  // skipped: 34.2, and held to 96 registers: 32.7, 2: 30.8 (68 registers, seven waves), 1: 30.6.
  auto cache_issue = [&](int j0, p16x4(&kk)[U][S], p16x4(&vv)[U][S]) {
    int a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) a[u] = anc[(size_t)min(j0 + u, t0 - 1) * R + rt];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const size_t off = ((size_t)min(j0 + u, t0 - 1) * R + clampi(a[u], 0, R - 1)) * inner + 4 * tid;
#pragma unroll
      for (int pc = 0; pc < S; ++pc) {
        kk[u][pc] = *reinterpret_cast<const p16x4*>(kcache + pc * cache_ps + off);
        vv[u][pc] = *reinterpret_cast<const p16x4*>(vcache + pc * cache_ps + off);
      }
    }
  };
  // the in-pass ancestors rows[0 .. U - 1] at the levels e0 .. e0 + U - 1; nothing is requested for a level the row does not have
  auto pass_issue = [&](int e0, const int(&rows)[U], p16x4(&kk)[U][S], p16x4(&vv)[U][S]) {
    const p16* ar[U];
#pragma unroll
    for (int u = 0; u < U; ++u) ar[u] = src(rows[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e0 + u < l) {
#pragma unroll
        for (int pc = 0; pc < S; ++pc) {
          kk[u][pc] = *reinterpret_cast<const p16x4*>(ar[u] + pc * qkv_ps + inner);
          vv[u][pc] = *reinterpret_cast<const p16x4*>(ar[u] + pc * qkv_ps + 2 * inner);
        }
      }
    }
  };

  float qf[4], m = -INFINITY, lsum = 0.f, acc[4] = {0.f, 0.f, 0.f, 0.f};
  // positions j0 .. j0 + U - 1 below `end`, in order
  auto eat = [&](int j0, int end, const p16x4(&kk)[U][S], const p16x4(&vv)[U][S]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (j0 + u < end) {
        float kj[4], vj[4];
        sa_sum<S>(kk[u], kj);
        sa_sum<S>(vv[u], vj);
        sa_step(qf, kj, vj, bias_h[p - (j0 + u)], m, lsum, acc);
      }
    }
  };

  // The first batch of cached positions is requested before the walk, the first batch of in-pass ancestors right behind it: the
  // walk is a chain of dependent table loads, and the cache rows fly meanwhile.
  p16x4 ck[U][S], cv[U][S];
  if (t0 > 0) cache_issue(0, ck, cv);
  // asc[e] = the row's ancestor at level e < l: parent[] walked from i, one hop per level (a forest row walks ML parents at most);
  // every index is clamped into the forest, so a corrupt table is never followed out of the q|k|v buffer
  int asc[ML];
#pragma unroll
  for (int e = 0; e < ML; ++e) asc[e] = i;
  {
    int cur = i;
#pragma unroll
    for (int e = ML - 1; e >= 0; --e) {
      if (e < l) {
        cur = clampi(parent[cur], 0, n_rows - 1);
        asc[e] = cur;
      }
    }
  }
  p16x4 pk[U][S], pv[U][S];
  {
    int rows[U];
#pragma unroll
    for (int u = 0; u < U; ++u) rows[u] = asc[u];
    if (l > 0) pass_issue(0, rows, pk, pv);
  }

  sa_sum<S>(q4, qf);
  if (t0 > 0) eat(0, t0, ck, cv);
  for (int j0 = U; j0 < t0; j0 += U) {
    cache_issue(j0, ck, cv);
    eat(j0, t0, ck, cv);
  }
  if (l > 0) eat(t0, p, pk, pv);
#pragma unroll
  for (int e0 = U; e0 < ML; e0 += U) {
    if (e0 < l) {
      int rows[U];
#pragma unroll
      for (int u = 0; u < U; ++u) rows[u] = asc[e0 + u];
      pass_issue(e0, rows, pk, pv);
      eat(t0 + e0, p, pk, pv);
    }
  }
  float kn[4], vn[4];
  sa_sum<S>(k4, kn);
  sa_sum<S>(v4, vn);
  sa_step(qf, kn, vn, bias_h[0], m, lsum, acc);
  sa_store<S>(out + (size_t)i * inner * S, 4 * tid, lsum, acc);
}

}  // namespace

extern "C" int gram_dec_self_attn_forest_split(const void* qkv, const int32_t* qkv_rows, const void* kcache, const void* vcache,
                                               const int32_t* anc, const int32_t* pos, const int32_t* parent, const int32_t* root,
                                               const float* bias, void* out, int n_rows, int R, int H, int t0, int Tmax, int nlev,
                                               int pieces, int64_t qkv_pstride, int64_t cache_pstride, void* stream) {
  if (!qkv || !kcache || !vcache || !anc || !pos || !parent || !root || !bias || !out || n_rows < 1 || n_rows > INT32_MAX / 4 ||
      R < 1 || H < 1 || H > 16 || t0 < 0 || t0 >= Tmax || Tmax > GRAM_MAX_DEC_LEN || nlev < 1 || nlev > GRAM_TAIL_MAX_STEPS ||
      pieces < 1 || pieces > GRAM_MAX_PIECES)
    return GRAM_E_ARG;
  if (pieces > 1 && (qkv_pstride < 1 || cache_pstride < (int64_t)Tmax * R * H * 64)) return GRAM_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  // the row's own q|k|v and its output; the cached positions and the ancestors come from the cache hierarchy for most rows
  gram_prof::Scope prof(GRAM_K_DEC_SELF_ATTN, st, 2.0 * 4 * n_rows * H * 64 * pieces);
  // GRAM_FOREST_ROW_ORDER=0: workgroup w serves row w (an A/B hook; the default gives every XCD a contiguous eighth of the rows)
  static const bool by_xcd = [] {
    const char* e = getenv("GRAM_FOREST_ROW_ORDER");
    return !(e && e[0] == '0');
  }();
  const int chunk = by_xcd ? (n_rows + 7) / 8 : 0;
  const dim3 grid(by_xcd ? 8 * chunk : n_rows), block(H * 16);
  if (pieces == 2)
    hipLaunchKernelGGL(dec_self_attn_forest_kernel<2>, grid, block, 0, st, (const p16*)qkv, qkv_rows, (const p16*)kcache,
                       (const p16*)vcache, anc, pos, parent, root, bias, (p16*)out, n_rows, R, H, t0, Tmax, nlev, (long)qkv_pstride,
                       (long)cache_pstride, chunk);
  else
    hipLaunchKernelGGL(dec_self_attn_forest_kernel<1>, grid, block, 0, st, (const p16*)qkv, qkv_rows, (const p16*)kcache,
                       (const p16*)vcache, anc, pos, parent, root, bias, (p16*)out, n_rows, R, H, t0, Tmax, nlev, (long)qkv_pstride,
                       (long)cache_pstride, chunk);
  GRAM_CHECK_LAUNCH();
  return 0;
}
