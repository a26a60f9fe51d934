// Cosine nearest neighbours over the static-vectors table (spaCy's
// Vectors.most_similar, the operation under Vocab.prune_vectors): for every
// query the n best table rows by cosine similarity, without ever writing the
// [nQ, V] similarity matrix.  `table` [V, nMp] and `queries` [nQ, nMp] are in
// the padded bf16 layout of Vectors.device_table (nMp = roundup(nM, 32) <=
// 320, pad columns zero).  Over the bf16 values as given:
//   inv(x)      = 1 / sqrt(sum x_k^2) in fp32, 0 when the sum is exactly 0
//   score[i, r] = dot(q_i, t_r) * inv(t_r) * inv(q_i), clipped to [-1, 1]
// and the result is sorted by (score descending, row ascending), a total
// order, so it does not depend on how the work is split.
//
// vecsim_rowinv_kernel: inv(t_r) -> fp32 [V], 16 lanes per row, fixed order.
//
// vecsim_topn_kernel<KC, N>, KC = nMp / 32 (compile time: the query
// fragments and the K loop are fully unrolled, nothing is indexed at run
// time), N = 1 or 8 results per query (1 < n < 8 runs N = 8, the launcher
// slices):
// * grid = query tiles x V-splits.  A workgroup is 8 waves and owns 256
//   queries; wave w owns queries [32 w, +32) of the tile and keeps their
//   MFMA B fragments in registers for the whole kernel (2 KC fragments of 8
//   bf16: 80 VGPRs at nMp = 320), loaded once with 16-byte loads; a query >=
//   nQ is a zero fragment.  A wave whose 32 queries are all >= nQ stages
//   table tiles with the others but issues no MFMA and no selection;
// * the table is streamed through LDS in tiles of 64 rows, [64][nMp + 8]
//   bf16 (the +8 pad: row stride 4 mod 16 dwords, ds_read_b128 conflict
//   free, see srx_mwe.hip.h), double buffered with a register prefetch, one
//   barrier per tile; inv(t_r) of the tile's rows is staged with it.  Rows
//   >= V are staged as zeros and read no memory;
// * v_mfma_f32_32x32x16_bf16 with the table rows on M and the queries on N:
//   a lane's 16 accumulator registers are the scores of 16 table rows for
//   the one query lane & 31, rows (rr & 3) + 8 (rr >> 2) + 4 (lane >> 5) of
//   the 32-row half tile.  The two half tiles are independent accumulator
//   chains;
// * selection runs on s = acc * inv(t_r) (inv(q_i) > 0 is constant within a
//   query and is applied when the scores are written).  The running top-N
//   of a lane lives in 2 N registers, sorted; a lane meets its rows in
//   ascending order, so a candidate enters only when it is strictly greater
//   and ties keep the lower row.  The insertion is N unrolled
//   compare/selects.  For N = 8 a tile is first tested as a whole (max of
//   the 16 scores against the lane's 8th best) and then per candidate, and
//   the insertion is skipped wave-wide when no lane qualifies.  In a tail
//   tile rows >= V are set to -inf and can never be selected;
// * at the end lane l < 32 takes the list of lane l + 32 (same query, the
//   other rows) and merges it under the (score, row) order;
// * one split: lanes < 32 write rows and clip(s * inv(q_i)) directly.
//   Several splits: every split writes its N (s, row) pairs to a workspace
//   and vecsim_merge_kernel (one wave per query: a lane takes every 64th
//   split in split order, then a butterfly over the lanes) merges them
//   under the same total order, then applies inv(q_i) and the clip with the
//   same two instructions.  Splits are ranges of whole tiles, so a
//   (query, row) score is the same instruction sequence whatever the split:
//   results are bit-identical across split counts and runs.  No atomics.
// An unfilled slot is (-inf, INT_MAX); n <= V guarantees none is returned.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950): see docs/KERNELS.md, "Vectors.most_similar".
#pragma once
#include "srx_common.hip.h"
#include "srx_mwe.hip.h"

#define SRX_VECSIM_WAVES 8
#define SRX_VECSIM_THREADS (SRX_VECSIM_WAVES * SRX_WAVE)
#define SRX_VECSIM_QT (SRX_VECSIM_WAVES * 32)  // queries per workgroup
#define SRX_VECSIM_TR 64                       // table rows per tile
#define SRX_VECSIM_NOROW 0x7fffffff

__host__ __device__ constexpr int vecsim_ap(int KC) { return 32 * KC + 8; }
__host__ __device__ constexpr int vecsim_lds_bytes(int KC) {
  return 2 * SRX_VECSIM_TR * vecsim_ap(KC) * 2 + 2 * SRX_VECSIM_TR * 4;
}

__device__ __forceinline__ float vs_sumsq8(const srx_u32x4_t& v, float acc) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const float x = bf2f((bf16_t)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu));
    acc += x * x;
  }
  return acc;
}

__device__ __forceinline__ float vs_inv_norm(float ss) {
  return ss == 0.f ? 0.f : 1.f / sqrtf(ss);
}

__device__ __forceinline__ float vs_final_score(float s, float invq) {
  return fminf(fmaxf(s * invq, -1.f), 1.f);
}

// 16 lanes per table row; every lane sums its pieces in ascending order,
// then an xor butterfly over the 16 lanes
__global__ __launch_bounds__(256) void vecsim_rowinv_kernel(
    const bf16_t* __restrict__ table, float* __restrict__ inv, int V, int nMp) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long r = gid / 16;  // uniform over the 16 lanes of a group
  const int l = (int)(gid % 16);
  const int Q = nMp / 8;
  float ss = 0.f;
  if (r < V)
    for (int q = l; q < Q; q += 16)
      ss = vs_sumsq8(*(const srx_u32x4_t*)(table + r * nMp + q * 8), ss);
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) ss += __shfl_xor(ss, off, SRX_WAVE);
  if (r < V && l == 0) inv[r] = vs_inv_norm(ss);
}

// sorted insert of (v, row) under the total order (score desc, row asc).
// STRICT: the candidate's row is known to be above every row in the list,
// so it enters only when strictly greater.
template <int N, bool STRICT>
__device__ __forceinline__ void vs_insert(float (&s)[N], int (&r)[N], float v,
                                          int row) {
  bool carry = false;  // once the candidate is placed, the rest shifts down
#pragma unroll
  for (int j = 0; j < N; j++) {
    const bool better =
        STRICT ? v > s[j] : (v > s[j] || (v == s[j] && row < r[j]));
    const bool sw = carry || better;
    const float ts = s[j];
    const int tr = r[j];
    s[j] = sw ? v : ts;
    r[j] = sw ? row : tr;
    v = sw ? ts : v;
    row = sw ? tr : row;
    carry = sw;
  }
}

// the 16 scores of one 32-row half tile into the lane's list.  row0 is the
// lane's first row, r0 + 32 h + 4 (lane >> 5)
template <int N>
__device__ __forceinline__ void vs_select(float (&s)[N], int (&r)[N],
                                          const srx_f32x16& acc,
                                          const float* __restrict__ invt,
                                          int row0, int V, bool tail) {
  float v[16];
#pragma unroll
  for (int rr = 0; rr < 16; rr++) {
    const int i = (rr & 3) + 8 * (rr >> 2);
    v[rr] = acc[rr] * invt[i];
    if (tail && row0 + i >= V) v[rr] = -INFINITY;
  }
  if (N > 1) {
    float m = v[0];
#pragma unroll
    for (int rr = 1; rr < 16; rr++) m = fmaxf(m, v[rr]);
    if (!__any(m > s[N - 1])) return;
  }
#pragma unroll
  for (int rr = 0; rr < 16; rr++) {
    const int i = (rr & 3) + 8 * (rr >> 2);
    if (N == 1) {
      const bool b = v[rr] > s[0];
      s[0] = b ? v[rr] : s[0];
      r[0] = b ? row0 + i : r[0];
    } else if (__any(v[rr] > s[N - 1])) {
      vs_insert<N, true>(s, r, v[rr], row0 + i);
    }
  }
}

template <int KC, int N>
__global__ __launch_bounds__(SRX_VECSIM_THREADS) void vecsim_topn_kernel(
    const bf16_t* __restrict__ queries,  // [nQ, 32 KC]
    const bf16_t* __restrict__ table,    // [V, 32 KC]
    const float* __restrict__ invt,      // [V]
    int* __restrict__ out_rows,          // [nQ, n]            (one split)
    float* __restrict__ out_scores,      // [nQ, n]            (one split)
    float* __restrict__ ws_s,            // [splits, nQ, N]    (several)
    int* __restrict__ ws_r,              // [splits, nQ, N]
    float* __restrict__ ws_invq,         // [nQ]
    long nQ, int V, int n, int ntiles) {
  constexpr int nMp = 32 * KC, AP = vecsim_ap(KC), TR = SRX_VECSIM_TR;
  constexpr int NT = SRX_VECSIM_THREADS;
  constexpr int Q = nMp / 8;                // 16-byte pieces per row
  constexpr int PIECES = TR * Q;            // per tile
  constexpr int PF = (PIECES + NT - 1) / NT;
  constexpr int KS = 2 * KC;                // MFMA K steps
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsT = lds;                                // [2][TR][AP]
  float* ldsI = (float*)(lds + 2 * TR * AP);         // [2][TR]

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int half = lane >> 5;
  const int splits = gridDim.y, split = blockIdx.y;
  const int tb = (int)((long)ntiles * split / splits);
  const int te = (int)((long)ntiles * (split + 1) / splits);
  const long qw0 = (long)blockIdx.x * SRX_VECSIM_QT + 32 * wave;
  const long qi = qw0 + (lane & 31);
  const bool wave_live = qw0 < nQ;  // uniform over the wave

  // query fragments, loop invariant; inv(q) from the same registers
  srx_bf16x8 qf[KS];
  float ssq = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ks++) {
    srx_u32x4_t u = {0u, 0u, 0u, 0u};
    if (qi < nQ) u = *(const srx_u32x4_t*)(queries + qi * nMp + 16 * ks + 8 * half);
    ssq = vs_sumsq8(u, ssq);
    qf[ks] = __builtin_bit_cast(srx_bf16x8, u);
  }
  ssq += __shfl_xor(ssq, 32, SRX_WAVE);
  const float invq = vs_inv_norm(ssq);

  float s[N];
  int r[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    s[j] = -INFINITY;
    r[j] = SRX_VECSIM_NOROW;
  }

  // this thread's pieces of a table tile, and (tid < TR) one inv(t)
  srx_u32x4_t pf[PF];
  float pfi = 0.f;
  auto fetch = [&](int t) {
    const long r0 = (long)t * TR;
#pragma unroll
    for (int u = 0; u < PF; u++) {
      const int id = u * NT + tid;
      const int i = id / Q, q = id - i * Q;
      pf[u] = srx_u32x4_t{0u, 0u, 0u, 0u};
      if (id < PIECES && r0 + i < V)
        pf[u] = *(const srx_u32x4_t*)(table + (r0 + i) * nMp + q * 8);
    }
    pfi = (tid < TR && r0 + tid < V) ? invt[r0 + tid] : 0.f;
  };
  auto stage = [&](int b) {
#pragma unroll
    for (int u = 0; u < PF; u++) {
      const int id = u * NT + tid;
      const int i = id / Q, q = id - i * Q;
      if (id < PIECES) *(srx_u32x4_t*)(ldsT + (b * TR + i) * AP + q * 8) = pf[u];
    }
    if (tid < TR) ldsI[b * TR + tid] = pfi;
  };

  fetch(tb);
  stage(0);
  __syncthreads();

  for (int t = tb; t < te; t++) {
    const int b = (t - tb) & 1;
    if (t + 1 < te) fetch(t + 1);
    if (wave_live) {
      srx_f32x16 acc0, acc1;
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        acc0[rr] = 0.f;
        acc1[rr] = 0.f;
      }
      const bf16_t* arow = ldsT + (b * TR + (lane & 31)) * AP + 8 * half;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const srx_bf16x8 a0 = *(const srx_bf16x8*)(arow + 16 * ks);
        const srx_bf16x8 a1 = *(const srx_bf16x8*)(arow + 32 * AP + 16 * ks);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, qf[ks], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, qf[ks], acc1, 0, 0, 0);
      }
      const int r0 = t * TR;
      const bool tail = r0 + TR > V;
      const float* it = ldsI + b * TR + 4 * half;
      vs_select<N>(s, r, acc0, it, r0 + 4 * half, V, tail);
      vs_select<N>(s, r, acc1, it + 32, r0 + 32 + 4 * half, V, tail);
    }
    if (t + 1 < te) stage(b ^ 1);
    __syncthreads();
  }
  if (!wave_live) return;

  // lane l < 32 merges the list of lane l + 32: same query, the other rows
#pragma unroll
  for (int j = 0; j < N; j++) {
    const float os = __shfl_xor(s[j], 32, SRX_WAVE);
    const int orow = __shfl_xor(r[j], 32, SRX_WAVE);
    if (half == 0) vs_insert<N, false>(s, r, os, orow);
  }
  if (half != 0 || qi >= nQ) return;
  if (splits == 1) {
#pragma unroll
    for (int j = 0; j < N; j++)
      if (j < n) {
        out_rows[qi * n + j] = r[j];
        out_scores[qi * n + j] = vs_final_score(s[j], invq);
      }
  } else {
    const long o = ((long)split * nQ + qi) * N;
#pragma unroll
    for (int j = 0; j < N; j++) {
      ws_s[o + j] = s[j];
      ws_r[o + j] = r[j];
    }
    if (split == 0) ws_invq[qi] = invq;
  }
}

// one wave per query: lane l merges the partial lists of splits l, l + 64,
// ... in split order, then an xor butterfly merges the 64 lanes' lists.  The
// (score, row) order is total and the rows of different splits are
// distinct, so the top N of the union is the same whatever the grouping.
template <int N>
__global__ __launch_bounds__(256) void vecsim_merge_kernel(
    const float* __restrict__ ws_s, const int* __restrict__ ws_r,
    const float* __restrict__ ws_invq, int* __restrict__ out_rows,
    float* __restrict__ out_scores, long nQ, int splits, int n) {
  const int lane = threadIdx.x % SRX_WAVE;
  const long qi = (long)blockIdx.x * (blockDim.x / SRX_WAVE) + threadIdx.x / SRX_WAVE;
  if (qi >= nQ) return;  // uniform over the wave
  float s[N];
  int r[N];
#pragma unroll
  for (int j = 0; j < N; j++) {
    s[j] = -INFINITY;
    r[j] = SRX_VECSIM_NOROW;
  }
  for (int sp = lane; sp < splits; sp += SRX_WAVE) {
    const long o = ((long)sp * nQ + qi) * N;
#pragma unroll
    for (int j = 0; j < N; j++) vs_insert<N, false>(s, r, ws_s[o + j], ws_r[o + j]);
  }
#pragma unroll 1
  for (int off = SRX_WAVE / 2; off > 0; off >>= 1) {
    float os[N];
    int orow[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
      os[j] = __shfl_xor(s[j], off, SRX_WAVE);
      orow[j] = __shfl_xor(r[j], off, SRX_WAVE);
    }
#pragma unroll
    for (int j = 0; j < N; j++) vs_insert<N, false>(s, r, os[j], orow[j]);
  }
  if (lane != 0) return;
  const float invq = ws_invq[qi];
#pragma unroll
  for (int j = 0; j < N; j++)
    if (j < n) {
      out_rows[qi * n + j] = r[j];
      out_scores[qi * n + j] = vs_final_score(s[j], invq);
    }
}
