// Attention pooling: Thinc's ParametricAttention followed by reduce_sum, the
// pooling of spacy.TextCatEnsemble.v2 and spacy.TextCatParametricAttention.v1.
// For doc d = rows [a, e) of X [T, W], query q [W] and keys K [T, W] (K = X
// when there are none):
//   s_t = K_t . q      a = softmax of s over the doc's rows      P_d = sum_t a_t X_t
// An empty doc gives a zero row and no gradient.  Backward, with g_t = X_t .
// dP_d, c_d = sum_t a_t g_t = P_d . dP_d and ds_t = a_t (g_t - c_d):
//   without K: dX_t = a_t dP_d + ds_t q                dq = sum_t ds_t X_t
//   with K:    dX_t = a_t dP_d       dK_t = ds_t q     dq = sum_t ds_t K_t
// The op is GEMV-shaped (two dot products and two axpys per row) and memory
// bound, so there is no matrix-instruction work here.
//
// Row layout (the span-pool convention, srx_spanpool.hip.h): a row is Q = W /
// V pieces of 16 bytes (V = 8 bf16 or 4 fp32 columns).  A sub-wave of SW = 8
// / 16 / 32 / 64 lanes owns a row, a wave works on G = 64 / SW rows side by
// side (row group g takes rows r0 + g, r0 + g + G, ...: neighbouring groups
// read neighbouring rows), a lane owns the NP = ceil(Q / SW) <= 3 pieces ql,
// ql + SW, ...  q lives in registers as fp32 for the lane's pieces; in the
// backward so do dP_d and, for c_d, the saved fp32 P_d.  Dot products are
// butterfly sums over the sub-wave (every lane of it gets the same bits).  A
// trip loads U = 4 (NP = 1) or 2 rows per group before the first is used, so
// 2 .. 6 (with K 4 .. 12) 16-byte loads are in flight per lane.
//
// Work split: a unit is (doc, chunk of at most CH = 64 rows), so a 5000-row
// doc is 79 units on as many waves.  Every doc has max(1, ceil(len / CH))
// units; the host takes the cumsum of that on the device (unit_offsets [D +
// 1], no sync) and launches over the shape-derived bound D + T / CH; a wave
// finds its unit's doc by binary search.  Units are dealt out in fixed blocks
// of 64: workgroup trip b takes units [64 b, 64 b + 64), wave w of it the
// units 64 b + 4 i + w, and the blocks are grid-strided.  The forward appends
// one pseudo-unit per pad row [D, Dpad) of P, which stores zeros.
//
// attention_pool_fwd_kernel<T, SW, NP, HASK>: flash-style online softmax, one
// pass over the unit's rows.  Each row group keeps a running maximum m, a
// running sum l and fp32 acc (the lane's pieces), rescaled once per trip when
// m moves.  The G groups merge at the end of the unit by a butterfly over the
// lane bits above SW (a fixed order); group 0 stores.  A doc of at most CH
// rows is finished there: P_d = acc / l rounded once, the unrounded fp32 P_d
// and lse_d = m + log l for the backward.  A longer doc's units store (m, l,
// acc) in fp32 to a workspace of at most 2 T / CH slots (slot 2 (unit_offsets
// [d] - d) + chunk) and attention_pool_merge_kernel, a wave per such doc,
// combines them in chunk order.  Floor: T W sizeof(T) (twice that with K)
// read, D W (sizeof(T) + 4) written.
//
// attention_pool_bwd_kernel<T, SW, NP, HASK>: one pass.  c_d = P32_d . dP_d
// up front, then per row: recompute s_t, a_t = exp(s_t - lse_d), g_t, ds_t,
// and store dX_t (and dK_t) once with one rounding.  No [T]- or [T, W]-sized
// intermediate goes through HBM in either direction.  Offsets are clamped to
// [0, T] (an end to [start, T]) in the kernels; rows of X before the first
// and after the last doc get a zero gradient from the first and the last
// unit.  Floor: T W sizeof(T) read and written (twice that with K).
//
// dq: per-lane fp32 partials over the wave's units of the block, a butterfly
// over the row groups, the four waves' rows through LDS (4 x 768 floats, the
// only LDS of the pooling kernels) summed in wave order into dq_part [block,
// W]; attention_pool_dq_kernel sums the blocks in 16 fixed interleaved
// slices per column and the slices in order.  The grouping follows the unit
// numbers alone, so the result does not depend on the grid.
//
// No atomics anywhere: every output is bit-identical from run to run and
// independent of the grid size, so SRX_DETERMINISTIC needs no variant.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0 and scratch 0 in all; 256 threads; LDS 12288 bytes in the
// backward, 1024 in attention_pool_dq_kernel, 0 elsewhere; the range is over
// SW and HASK):
//                                   NP  VGPR       SGPR    waves / SIMD
//   attention_pool_fwd_kernel<bf16_t>  1   84 ..  94  74 .. 80   5
//                                      2   90 .. 101  76 .. 86   4 .. 5
//                                      3  122 .. 136  78 .. 90   3 .. 4
//   attention_pool_bwd_kernel<bf16_t>  1  111 .. 117  80 .. 94   4
//                                      2  139 .. 143  81 .. 96   3
//                                      3  181 .. 186  89 .. 98   2
//   attention_pool_fwd_kernel<float>   1   58 ..  90  72 .. 78   5 .. 8
//                                      2   62 ..  80  74 .. 84   6 .. 8
//                                      3   77 .. 104  76 .. 88   4 .. 6
//   attention_pool_bwd_kernel<float>   1   74 ..  94  78 .. 90   5 .. 6
//                                      2   82 ..  96  79 .. 94   5
//                                      3  102 .. 118  87 .. 96   4
//   attention_pool_merge_kernel<*>         31         56 .. 58   8
//   attention_pool_dq_kernel               14         18         8
// (the default sub-wave gives NP = 1 up to W = 512 bf16 / 256 fp32, NP = 2
// at W = 768 bf16 and NP = 3 at W = 768 fp32)
#pragma once
#include "srx_spanpool.hip.h"  // SpanPiece: a 16-byte piece <-> V floats

#define SRX_ATTNPOOL_THREADS 256
#define SRX_ATTNPOOL_CHUNK 64   // CH: rows per unit
#define SRX_ATTNPOOL_UNITS 64   // units per workgroup trip, 16 per wave
#define SRX_ATTNPOOL_MAXW 768

template <int SW>
__device__ __forceinline__ float ap_sub_sum(float v) {
#pragma unroll
  for (int off = SW / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SRX_WAVE);
  return v;
}

// V fp32 values <-> 16-byte accesses of an fp32 row
template <int V>
__device__ __forceinline__ void ap_ld_f32(const float* __restrict__ p, float* v) {
#pragma unroll
  for (int k = 0; k < V; k += 4) {
    const float4 x = *(const float4*)(p + k);
    v[k] = x.x; v[k + 1] = x.y; v[k + 2] = x.z; v[k + 3] = x.w;
  }
}

template <int V>
__device__ __forceinline__ void ap_st_f32(float* __restrict__ p, const float* v) {
#pragma unroll
  for (int k = 0; k < V; k += 4)
    *(float4*)(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
}

// the unit's doc: the largest d in [0, D) with unit_offsets[d] <= u (every
// doc has at least one unit, so unit_offsets is strictly increasing)
__device__ __forceinline__ int ap_find_doc(const int* __restrict__ uo, int D, int u) {
  int lo = 0, hi = D - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (uo[mid] <= u) lo = mid; else hi = mid - 1;
  }
  return lo;
}

struct ApUnit {
  int d, chunk, n_chunks;
  int a, e;    // the doc's rows, clamped
  int r0, r1;  // the unit's rows
};

__device__ __forceinline__ ApUnit ap_unit(const int* __restrict__ offsets,
                                          const int* __restrict__ uo, int D, int Tn,
                                          int u) {
  ApUnit t;
  t.d = ap_find_doc(uo, D, u);
  t.chunk = u - uo[t.d];
  t.n_chunks = uo[t.d + 1] - uo[t.d];
  t.a = min(max(offsets[t.d], 0), Tn);
  t.e = min(max(offsets[t.d + 1], t.a), Tn);
  t.r0 = (int)min((long)t.a + (long)t.chunk * SRX_ATTNPOOL_CHUNK, (long)t.e);
  t.r1 = (int)min((long)t.r0 + SRX_ATTNPOOL_CHUNK, (long)t.e);
  return t;
}

template <typename T, int SW, int NP, bool HASK>
__global__ __launch_bounds__(SRX_ATTNPOOL_THREADS) void attention_pool_fwd_kernel(
    const T* __restrict__ X,          // [Tn, W]
    const T* __restrict__ K,          // [Tn, W] (HASK)
    const int* __restrict__ offsets,  // [D + 1]
    const int* __restrict__ uo,       // [D + 1] unit offsets
    const float* __restrict__ q,      // [W]
    T* __restrict__ P,                // [Dpad, W]
    float* __restrict__ P32,          // [D, W]
    float* __restrict__ lse,          // [D]
    float* __restrict__ ws_ml,        // [slots, 2]
    float* __restrict__ ws_acc,       // [slots, W]
    int D, int Dpad, int Tn, int W, int bound, int n_slots) {
  using Pc = SpanPiece<T>;
  constexpr int V = Pc::V;
  constexpr int G = SRX_WAVE / SW;
  constexpr int U = NP == 1 ? 4 : 2;
  constexpr int WPB = SRX_ATTNPOOL_THREADS / SRX_WAVE;
  const int lane = threadIdx.x % SRX_WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / SRX_WAVE);
  const int g = lane / SW, ql = lane % SW;
  const int Q = W / V;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};
  const float ninf = -__builtin_inff();

  bool has[NP];
  float qr[NP][V];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    has[p] = ql + p * SW < Q;
#pragma unroll
    for (int i = 0; i < V; i++) qr[p][i] = 0.f;
    if (has[p]) ap_ld_f32<V>(q + (ql + p * SW) * V, qr[p]);
  }

  const int n_units = bound + (Dpad - D);
  const int n_real = D > 0 ? uo[D] : 0;
  const int n_blocks = (n_units + SRX_ATTNPOOL_UNITS - 1) / SRX_ATTNPOOL_UNITS;
  for (int ub = blockIdx.x; ub < n_blocks; ub += gridDim.x) {
    for (int it = 0; it < SRX_ATTNPOOL_UNITS / WPB; it++) {
      const int u = ub * SRX_ATTNPOOL_UNITS + it * WPB + wave;
      if (u >= n_units) break;
      if (u >= bound) {  // a pad row of P
        if (g == 0) {
          T* __restrict__ row = P + (long)(D + (u - bound)) * W;
#pragma unroll
          for (int p = 0; p < NP; p++)
            if (has[p]) *(srx_u32x4_t*)(row + (ql + p * SW) * V) = zero;
        }
        continue;
      }
      if (u >= n_real) continue;
      const ApUnit t = ap_unit(offsets, uo, D, Tn, u);

      float m = ninf, l = 0.f;
      float acc[NP][V];
#pragma unroll
      for (int p = 0; p < NP; p++)
#pragma unroll
        for (int i = 0; i < V; i++) acc[p][i] = 0.f;

      for (int base = t.r0; base < t.r1; base += G * U) {
        srx_u32x4_t x[U][NP], kk[U][NP];
        bool ok[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
          const int r = base + j * G + g;
          ok[j] = r < t.r1;
#pragma unroll
          for (int p = 0; p < NP; p++) {
            const long at = (long)r * W + (ql + p * SW) * V;
            x[j][p] = kk[j][p] = zero;
            if (ok[j] && has[p]) {
              x[j][p] = *(const srx_u32x4_t*)(X + at);
              if (HASK) kk[j][p] = *(const srx_u32x4_t*)(K + at);
            }
          }
        }
        float s[U];
        float mn = m;
#pragma unroll
        for (int j = 0; j < U; j++) {
          float dot = 0.f;
#pragma unroll
          for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < V; i++)
              dot += Pc::get(HASK ? kk[j][p] : x[j][p], i) * qr[p][i];
          dot = ap_sub_sum<SW>(dot);  // every lane takes part
          s[j] = ok[j] ? dot : ninf;
          mn = fmaxf(mn, s[j]);
        }
        if (mn > ninf) {  // this group has seen a row
          const float sc = expf(m - mn);  // m = -inf: 0
          l *= sc;
#pragma unroll
          for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < V; i++) acc[p][i] *= sc;
#pragma unroll
          for (int j = 0; j < U; j++) {
            const float w = ok[j] ? expf(s[j] - mn) : 0.f;
            l += w;
#pragma unroll
            for (int p = 0; p < NP; p++)
#pragma unroll
              for (int i = 0; i < V; i++) acc[p][i] += w * Pc::get(x[j][p], i);
          }
          m = mn;
        }
      }

      // merge the row groups: lane bits SW, 2 SW, ..., 32
#pragma unroll
      for (int off = SW; off < SRX_WAVE; off <<= 1) {
        const float mo = __shfl_xor(m, off, SRX_WAVE);
        const float lo = __shfl_xor(l, off, SRX_WAVE);
        const float mn = fmaxf(m, mo);
        const float sa = m > ninf ? expf(m - mn) : 0.f;
        const float sb = mo > ninf ? expf(mo - mn) : 0.f;
        l = l * sa + lo * sb;
#pragma unroll
        for (int p = 0; p < NP; p++)
#pragma unroll
          for (int i = 0; i < V; i++) {
            const float ao = __shfl_xor(acc[p][i], off, SRX_WAVE);
            acc[p][i] = acc[p][i] * sa + ao * sb;
          }
        m = mn;
      }

      if (g != 0) continue;
      if (t.n_chunks == 1) {
        const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
        for (int p = 0; p < NP; p++) {
          if (!has[p]) continue;
          const long at = (long)t.d * W + (ql + p * SW) * V;
          float o[V];
#pragma unroll
          for (int i = 0; i < V; i++) o[i] = acc[p][i] * inv;
          ap_st_f32<V>(P32 + at, o);
          *(srx_u32x4_t*)(P + at) = Pc::pack_round(o);
        }
        if (ql == 0) lse[t.d] = l > 0.f ? m + logf(l) : 0.f;
      } else {
        const long slot = 2L * (uo[t.d] - t.d) + t.chunk;
        if (slot >= n_slots) continue;  // offsets that are not ascending
#pragma unroll
        for (int p = 0; p < NP; p++)
          if (has[p]) ap_st_f32<V>(ws_acc + slot * W + (ql + p * SW) * V, acc[p]);
        if (ql == 0) {
          ws_ml[2 * slot] = m;
          ws_ml[2 * slot + 1] = l;
        }
      }
    }
  }
}

// a wave per doc of more than one unit: the chunks' (m, l, acc) in chunk order
template <typename T>
__global__ __launch_bounds__(SRX_ATTNPOOL_THREADS) void attention_pool_merge_kernel(
    const int* __restrict__ uo, const float* __restrict__ ws_ml,
    const float* __restrict__ ws_acc, T* __restrict__ P, float* __restrict__ P32,
    float* __restrict__ lse, int D, int W, int n_slots) {
  const int lane = threadIdx.x % SRX_WAVE;
  const int wpb = blockDim.x / SRX_WAVE;
  for (int d = blockIdx.x * wpb + threadIdx.x / SRX_WAVE; d < D; d += gridDim.x * wpb) {
    const int n = uo[d + 1] - uo[d];
    const long slot = 2L * (uo[d] - d);
    if (n <= 1 || slot + n > n_slots) continue;
    float M = -__builtin_inff();
    for (int c = 0; c < n; c++) M = fmaxf(M, ws_ml[2 * (slot + c)]);
    float L = 0.f;
    for (int c = 0; c < n; c++)
      L += ws_ml[2 * (slot + c) + 1] * expf(ws_ml[2 * (slot + c)] - M);
    const float inv = L > 0.f ? 1.f / L : 0.f;
    for (int col = lane; col < W; col += SRX_WAVE) {
      float s = 0.f;
      for (int c = 0; c < n; c++)
        s += ws_acc[(slot + c) * W + col] * expf(ws_ml[2 * (slot + c)] - M);
      s *= inv;
      P32[(long)d * W + col] = s;
      Elem<T>::st(P + (long)d * W + col, s);
    }
    if (lane == 0) lse[d] = L > 0.f ? M + logf(L) : 0.f;
  }
}

template <typename T, int SW, int NP, bool HASK>
__global__ __launch_bounds__(SRX_ATTNPOOL_THREADS) void attention_pool_bwd_kernel(
    const T* __restrict__ X,          // [Tn, W]
    const T* __restrict__ K,          // [Tn, W] (HASK)
    const int* __restrict__ offsets,  // [D + 1]
    const int* __restrict__ uo,       // [D + 1]
    const float* __restrict__ q,      // [W]
    const T* __restrict__ dP,         // [>= D, W]
    const float* __restrict__ P32,    // [D, W]
    const float* __restrict__ lse,    // [D]
    T* __restrict__ dX,               // [Tn, W]
    T* __restrict__ dK,               // [Tn, W] (HASK)
    float* __restrict__ dq_part,      // [n_blocks, W]
    int D, int Tn, int W, int bound) {
  using Pc = SpanPiece<T>;
  constexpr int V = Pc::V;
  constexpr int G = SRX_WAVE / SW;
  constexpr int U = NP == 1 ? 4 : 2;
  constexpr int WPB = SRX_ATTNPOOL_THREADS / SRX_WAVE;
  __shared__ float red[WPB][SRX_ATTNPOOL_MAXW];
  const int lane = threadIdx.x % SRX_WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / SRX_WAVE);
  const int g = lane / SW, ql = lane % SW;
  const int Q = W / V;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};

  bool has[NP];
  float qr[NP][V];
#pragma unroll
  for (int p = 0; p < NP; p++) {
    has[p] = ql + p * SW < Q;
#pragma unroll
    for (int i = 0; i < V; i++) qr[p][i] = 0.f;
    if (has[p]) ap_ld_f32<V>(q + (ql + p * SW) * V, qr[p]);
  }

  const int n_real = uo[D];
  const int n_blocks = (bound + SRX_ATTNPOOL_UNITS - 1) / SRX_ATTNPOOL_UNITS;
  for (int ub = blockIdx.x; ub < n_blocks; ub += gridDim.x) {
    float dqp[NP][V];
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
      for (int i = 0; i < V; i++) dqp[p][i] = 0.f;

    for (int it = 0; it < SRX_ATTNPOOL_UNITS / WPB; it++) {
      const int u = ub * SRX_ATTNPOOL_UNITS + it * WPB + wave;
      if (u >= n_real) break;
      const ApUnit t = ap_unit(offsets, uo, D, Tn, u);

      // rows that belong to no doc: before the first, after the last
      if (t.chunk == 0 && t.d == 0)
        for (int r = g; r < t.a; r += G)
#pragma unroll
          for (int p = 0; p < NP; p++)
            if (has[p]) {
              const long at = (long)r * W + (ql + p * SW) * V;
              *(srx_u32x4_t*)(dX + at) = zero;
              if (HASK) *(srx_u32x4_t*)(dK + at) = zero;
            }
      if (t.chunk == t.n_chunks - 1 && t.d == D - 1)
        for (int r = t.e + g; r < Tn; r += G)
#pragma unroll
          for (int p = 0; p < NP; p++)
            if (has[p]) {
              const long at = (long)r * W + (ql + p * SW) * V;
              *(srx_u32x4_t*)(dX + at) = zero;
              if (HASK) *(srx_u32x4_t*)(dK + at) = zero;
            }
      if (t.r0 >= t.r1) continue;

      float dpr[NP][V];
      float cd = 0.f;
#pragma unroll
      for (int p = 0; p < NP; p++) {
#pragma unroll
        for (int i = 0; i < V; i++) dpr[p][i] = 0.f;
        if (has[p]) {
          const long at = (long)t.d * W + (ql + p * SW) * V;
          const srx_u32x4_t raw = *(const srx_u32x4_t*)(dP + at);
          float p32[V];
          ap_ld_f32<V>(P32 + at, p32);
#pragma unroll
          for (int i = 0; i < V; i++) {
            dpr[p][i] = Pc::get(raw, i);
            cd += p32[i] * dpr[p][i];
          }
        }
      }
      cd = ap_sub_sum<SW>(cd);
      const float lsed = lse[t.d];

      for (int base = t.r0; base < t.r1; base += G * U) {
        srx_u32x4_t x[U][NP], kk[U][NP];
        bool ok[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
          const int r = base + j * G + g;
          ok[j] = r < t.r1;
#pragma unroll
          for (int p = 0; p < NP; p++) {
            const long at = (long)r * W + (ql + p * SW) * V;
            x[j][p] = kk[j][p] = zero;
            if (ok[j] && has[p]) {
              x[j][p] = *(const srx_u32x4_t*)(X + at);
              if (HASK) kk[j][p] = *(const srx_u32x4_t*)(K + at);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
          float dot = 0.f, gt = 0.f;
#pragma unroll
          for (int p = 0; p < NP; p++)
#pragma unroll
            for (int i = 0; i < V; i++) {
              dot += Pc::get(HASK ? kk[j][p] : x[j][p], i) * qr[p][i];
              gt += Pc::get(x[j][p], i) * dpr[p][i];
            }
          dot = ap_sub_sum<SW>(dot);
          gt = ap_sub_sum<SW>(gt);
          const float at_ = ok[j] ? expf(dot - lsed) : 0.f;
          const float ds = at_ * (gt - cd);
          const int r = base + j * G + g;
#pragma unroll
          for (int p = 0; p < NP; p++) {
            float ox[V], ok_[V];
#pragma unroll
            for (int i = 0; i < V; i++) {
              dqp[p][i] += ds * Pc::get(HASK ? kk[j][p] : x[j][p], i);
              ok_[i] = ds * qr[p][i];
              ox[i] = HASK ? at_ * dpr[p][i] : at_ * dpr[p][i] + ok_[i];
            }
            if (ok[j] && has[p]) {
              const long at = (long)r * W + (ql + p * SW) * V;
              *(srx_u32x4_t*)(dX + at) = Pc::pack_round(ox);
              if (HASK) *(srx_u32x4_t*)(dK + at) = Pc::pack_round(ok_);
            }
          }
        }
      }
    }

    // the block's dq row: row groups by butterfly, waves through LDS in order
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
      for (int i = 0; i < V; i++) {
        float v = dqp[p][i];
#pragma unroll
        for (int off = SW; off < SRX_WAVE; off <<= 1) v += __shfl_xor(v, off, SRX_WAVE);
        if (g == 0 && has[p]) red[wave][(ql + p * SW) * V + i] = v;
      }
    __syncthreads();
    for (int col = threadIdx.x; col < W; col += SRX_ATTNPOOL_THREADS)
      dq_part[(long)ub * W + col] =
          ((red[0][col] + red[1][col]) + red[2][col]) + red[3][col];
    __syncthreads();
  }
}

// dq [W] from dq_part [n_blocks, W]: a workgroup per 16 columns, 16 slices
// of interleaved blocks per column, the slices summed in order
__global__ __launch_bounds__(SRX_ATTNPOOL_THREADS) void attention_pool_dq_kernel(
    const float* __restrict__ dq_part, float* __restrict__ dq, int n_blocks, int W) {
  __shared__ float red[16][16];
  const int c = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + c;
  float s = 0.f;
  if (col < W)
    for (int b = sl; b < n_blocks; b += 16) s += dq_part[(long)b * W + col];
  red[sl][c] = s;
  __syncthreads();
  if (sl == 0 && col < W) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) t += red[k][c];
    dq[col] = t;
  }
}
