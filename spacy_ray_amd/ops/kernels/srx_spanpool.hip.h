// Span pooling for the span categorizer: spaCy's mean_max_reducer input.
// For span s = [a, e) over the token matrix X [T, W], L = e - a:
//   R[s]        = X[e-1] | X[a] | mean_t X[t] | max_t X[t]      ([4 W])
//   which[s, c] = t - a of the FIRST token attaining the maximum in column c
// (section order last, first, mean, max as in spaCy).  L == 0 gives an
// all-zero row, all-zero `which` and no gradient.  `which` is a byte, so the
// host sends only span sets with L <= 255 here.  Non-finite inputs are out
// of scope (a NaN never replaces the running maximum).
//
// A row is Q = W / V pieces of 16 bytes (V = 8 bf16 or 4 fp32 columns).  SW
// = 8 / 16 / 32 / 64 lanes (the power of two >= Q, at most 64) form the
// sub-wave of one row, a wave works on 64 / SW rows side by side, a lane
// owns pieces ql, ql + SW, ... (W = 768 bf16: two passes).  Row groups are
// grid-strided over all waves.
//
// span_pool_fwd_kernel<T, SW>: a sub-wave per span.
// * the next group's (start, end) is fetched while this one is pooled;
//   both are clamped to [0, T] (end to [start, T]) in the kernel, so memory
//   safety does not depend on the host;
// * the span's token rows are walked with four independent 16-byte loads
//   in flight per lane.  Per column: an fp32 sum in token order, a running
//   maximum and its offset (a later token replaces it only when strictly
//   greater).  The first and last sections are copies of the loaded
//   pieces, the max section is the winning input value itself;
// * mean = the fp32 sum, one IEEE division by float(L), one round to
//   nearest even;
// * four 16-byte stores into the row's sections and one 8-byte (fp32:
//   4-byte) store of the `which` piece; rows [S, Spad) of R are written as
//   zeros (the mixer kernels want a row count that is a multiple of 64).
// The kernel is write-bound: per span it writes 4 W sizeof(T) + W bytes
// (W = 96 bf16: 864) against W sizeof(T) bytes read per token (192), and
// the rows that neighbouring n-gram spans share hit in cache.  So the token
// rows are not staged in LDS.  Floor: S (4 W sizeof(T) + W) + T W sizeof(T).
//
// span_pool_bwd_kernel<T, SW>: gather form, a sub-wave per TOKEN row t.
// * walks the token's entries in the token -> span CSR (tok_offsets [T+1],
//   tok_spans [nnz], ascending span id per token) and accumulates in fp32,
//   in that fixed order and per entry in this order:
//     + dMean[s] / float(L_s)
//     + dLast[s]   if t == e - 1     (loaded only then)
//     + dFirst[s]  if t == a         (loaded only then)
//     + dMax[s, c] if which[s, c] == t - a
// * two entries are processed per trip, their span ids, bounds and pieces
//   loaded before the first is used;
// * one rounding, one 16-byte store; a token that no span covers stores
//   zeros, so every dX row is written and the host need not clear it.
// No atomics: bit-identical from run to run and independent of the grid,
// so SRX_DETERMINISTIC needs no variant.  CSR offsets are clamped to
// [0, nnz], an entry with a span id outside [0, S) or a span that does not
// contain t adds nothing.  Floor: S 4 W sizeof(T) + S W + T W sizeof(T).
//
// Neither kernel uses LDS, scratch or atomics.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0, scratch 0 and LDS 0 in all sixteen; 256 threads; the four
// SW variants of a row are equal; 5 waves / SIMD):
//   span_pool_fwd_kernel<bf16_t, *>   94 VGPR 66 SGPR
//   span_pool_bwd_kernel<bf16_t, *>   96 VGPR 64 SGPR
//   span_pool_fwd_kernel<float, *>    90 VGPR 70 SGPR
//   span_pool_bwd_kernel<float, *>    84 VGPR 64 SGPR
#pragma once
#include "srx_common.hip.h"

#define SRX_SPANPOOL_THREADS 256
// scalar fp32 VALU only: the sums below are eight independent chains per
// lane, which the compiler would otherwise pair into packed fp32 adds
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define SRX_SPANPOOL_FN __attribute__((target("no-packed-fp32-ops")))
#else
#define SRX_SPANPOOL_FN
#endif

typedef __attribute__((__vector_size__(8))) uint32_t srx_sp_u32x2_t;

// one 16-byte piece <-> V floats; the raw bits travel with it so that
// copies (first / last / max) never go through a conversion
template <typename T>
struct SpanPiece;

template <>
struct SpanPiece<bf16_t> {
  static constexpr int V = 8;
  static __device__ __forceinline__ float get(const srx_u32x4_t& p, int i) {
    return __uint_as_float((i & 1) ? (p[i >> 1] & 0xffff0000u) : (p[i >> 1] << 16));
  }
  // v holds values that are exactly representable (copies of inputs)
  static __device__ __forceinline__ srx_u32x4_t pack_exact(const float* v) {
    srx_u32x4_t p;
#pragma unroll
    for (int k = 0; k < 4; k++)
      p[k] = (__float_as_uint(v[2 * k]) >> 16) |
             (__float_as_uint(v[2 * k + 1]) & 0xffff0000u);
    return p;
  }
  static __device__ __forceinline__ srx_u32x4_t pack_round(const float* v) {
    srx_u32x4_t p;
#pragma unroll
    for (int k = 0; k < 4; k++)
      p[k] = (uint32_t)f2bf(v[2 * k]) | ((uint32_t)f2bf(v[2 * k + 1]) << 16);
    return p;
  }
  static __device__ __forceinline__ void st_which(uint8_t* p, const int* w) {
    srx_sp_u32x2_t o;
    o[0] = (uint32_t)w[0] | ((uint32_t)w[1] << 8) | ((uint32_t)w[2] << 16) |
           ((uint32_t)w[3] << 24);
    o[1] = (uint32_t)w[4] | ((uint32_t)w[5] << 8) | ((uint32_t)w[6] << 16) |
           ((uint32_t)w[7] << 24);
    *(srx_sp_u32x2_t*)p = o;
  }
  static __device__ __forceinline__ void ld_which(const uint8_t* p, int* w) {
    const srx_sp_u32x2_t o = *(const srx_sp_u32x2_t*)p;
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = (int)((o[i >> 2] >> (8 * (i & 3))) & 0xffu);
  }
};

template <>
struct SpanPiece<float> {
  static constexpr int V = 4;
  static __device__ __forceinline__ float get(const srx_u32x4_t& p, int i) {
    return __uint_as_float(p[i]);
  }
  static __device__ __forceinline__ srx_u32x4_t pack_exact(const float* v) {
    srx_u32x4_t p;
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = __float_as_uint(v[k]);
    return p;
  }
  static __device__ __forceinline__ srx_u32x4_t pack_round(const float* v) {
    return pack_exact(v);
  }
  static __device__ __forceinline__ void st_which(uint8_t* p, const int* w) {
    *(uint32_t*)p = (uint32_t)w[0] | ((uint32_t)w[1] << 8) |
                    ((uint32_t)w[2] << 16) | ((uint32_t)w[3] << 24);
  }
  static __device__ __forceinline__ void ld_which(const uint8_t* p, int* w) {
    const uint32_t o = *(const uint32_t*)p;
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (int)((o >> (8 * i)) & 0xffu);
  }
};

template <typename T, int SW>
__global__ __launch_bounds__(SRX_SPANPOOL_THREADS) SRX_SPANPOOL_FN void
span_pool_fwd_kernel(
    const T* __restrict__ X,          // [Tn, W]
    const int* __restrict__ starts,   // [S]
    const int* __restrict__ ends,     // [S]
    T* __restrict__ R,                // [Spad, 4 W]
    uint8_t* __restrict__ which,      // [S, W]
    int S, int Spad, int Tn, int W) {
  using P = SpanPiece<T>;
  constexpr int V = P::V;
  constexpr int G = SRX_WAVE / SW;  // spans per wave
  const int lane = threadIdx.x % SRX_WAVE;
  const int g = lane / SW, ql = lane % SW;
  const int Q = W / V;
  const long wpb = blockDim.x / SRX_WAVE;
  const long stride = (long)gridDim.x * wpb * G;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};

  long s = ((long)blockIdx.x * wpb + threadIdx.x / SRX_WAVE) * G + g;
  int a_next = s < S ? starts[s] : 0;
  int e_next = s < S ? ends[s] : 0;
  for (; s < Spad; s += stride) {
    const long sn = s + stride;
    int a = a_next, e = e_next;
    a_next = sn < S ? starts[sn] : 0;
    e_next = sn < S ? ends[sn] : 0;
    a = min(max(a, 0), Tn);
    e = min(max(e, a), Tn);
    if (s >= S) e = a;  // pad row: zeros
    T* __restrict__ row = R + s * 4L * W;

    for (int q = ql; q < Q; q += SW) {
      const T* __restrict__ col = X + q * V;
      float sum[V], mx[V];
      int wh[V];
      srx_u32x4_t first = zero, last = zero;
#pragma unroll
      for (int i = 0; i < V; i++) {
        sum[i] = 0.f;
        mx[i] = 0.f;
        wh[i] = 0;
      }
      for (int t = a; t < e; t += 4) {
        srx_u32x4_t v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          v[j] = zero;
          if (t + j < e) v[j] = *(const srx_u32x4_t*)(col + (long)(t + j) * W);
        }
        if (t == a) first = v[0];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          if (t + j < e) {
            last = v[j];
            const int off = t + j - a;
#pragma unroll
            for (int i = 0; i < V; i++) {
              const float x = P::get(v[j], i);
              sum[i] += x;
              if (off == 0 || x > mx[i]) {
                mx[i] = x;
                wh[i] = off;
              }
            }
          }
        }
      }
      if (e > a) {
        const float d = (float)(e - a);
#pragma unroll
        for (int i = 0; i < V; i++) sum[i] = sum[i] / d;
      }
      *(srx_u32x4_t*)(row + q * V) = last;
      *(srx_u32x4_t*)(row + W + q * V) = first;
      *(srx_u32x4_t*)(row + 2 * W + q * V) = P::pack_round(sum);
      *(srx_u32x4_t*)(row + 3 * W + q * V) = P::pack_exact(mx);
      if (s < S) P::st_which(which + s * (long)W + q * V, wh);
    }
  }
}

template <typename T, int SW>
__global__ __launch_bounds__(SRX_SPANPOOL_THREADS) SRX_SPANPOOL_FN void
span_pool_bwd_kernel(
    const T* __restrict__ dR,             // [>= S, 4 W]
    const uint8_t* __restrict__ which,    // [S, W]
    const int* __restrict__ starts,       // [S]
    const int* __restrict__ ends,         // [S]
    const int* __restrict__ tok_offsets,  // [Tn + 1]
    const int* __restrict__ tok_spans,    // [nnz]
    T* __restrict__ dX,                   // [Tn, W]
    int S, int Tn, int W, int nnz) {
  using P = SpanPiece<T>;
  constexpr int V = P::V;
  constexpr int G = SRX_WAVE / SW;  // token rows per wave
  constexpr int U = 2;              // entries per trip
  const int lane = threadIdx.x % SRX_WAVE;
  const int g = lane / SW, ql = lane % SW;
  const int Q = W / V;
  const long wpb = blockDim.x / SRX_WAVE;
  const long stride = (long)gridDim.x * wpb * G;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};

  for (long t = ((long)blockIdx.x * wpb + threadIdx.x / SRX_WAVE) * G + g; t < Tn;
       t += stride) {
    int beg = tok_offsets[t], end = tok_offsets[t + 1];
    beg = min(max(beg, 0), nnz);
    end = min(max(end, beg), nnz);
    for (int q = ql; q < Q; q += SW) {
      float acc[V];
#pragma unroll
      for (int i = 0; i < V; i++) acc[i] = 0.f;
      for (int k = beg; k < end; k += U) {
        int a[U], e[U];
        bool ok[U];
        const T* src[U];
        srx_u32x4_t dmean[U], dmax[U], dlast[U], dfirst[U];
        int wh[U][V];
#pragma unroll
        for (int j = 0; j < U; j++) {
          const int sp = k + j < end ? tok_spans[k + j] : -1;
          ok[j] = sp >= 0 && sp < S;
          a[j] = e[j] = 0;
          if (ok[j]) {
            a[j] = min(max(starts[sp], 0), Tn);
            e[j] = min(max(ends[sp], a[j]), Tn);
          }
          ok[j] = ok[j] && t >= a[j] && t < e[j];
          src[j] = dR + (long)(ok[j] ? sp : 0) * 4L * W + q * V;
          dmean[j] = dmax[j] = dlast[j] = dfirst[j] = zero;
#pragma unroll
          for (int i = 0; i < V; i++) wh[j][i] = -1;
          if (ok[j]) {
            dmean[j] = *(const srx_u32x4_t*)(src[j] + 2 * W);
            dmax[j] = *(const srx_u32x4_t*)(src[j] + 3 * W);
            P::ld_which(which + (long)sp * W + q * V, wh[j]);
            if (t == e[j] - 1) dlast[j] = *(const srx_u32x4_t*)(src[j]);
            if (t == a[j]) dfirst[j] = *(const srx_u32x4_t*)(src[j] + W);
          }
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
          if (ok[j]) {
            const float d = (float)(e[j] - a[j]);
            const int off = (int)t - a[j];
            const bool is_last = t == e[j] - 1, is_first = t == a[j];
#pragma unroll
            for (int i = 0; i < V; i++) {
              acc[i] += P::get(dmean[j], i) / d;
              if (is_last) acc[i] += P::get(dlast[j], i);
              if (is_first) acc[i] += P::get(dfirst[j], i);
              if (wh[j][i] == off) acc[i] += P::get(dmax[j], i);
            }
          }
        }
      }
      *(srx_u32x4_t*)(dX + t * (long)W + q * V) = P::pack_round(acc);
    }
  }
}
