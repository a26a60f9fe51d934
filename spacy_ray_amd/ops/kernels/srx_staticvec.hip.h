// Static word vectors (spaCy's StaticVectors layer), fused:
//   forward   Y[t, col_off : col_off + NO] = table[rows[t]] @ W^T
//   backward  dW = dY^T @ table[rows]        (dY = strided column view of dX)
// without ever writing the [T, nM] gather.  rows[t] < 0 is out of vocabulary:
// a zero output row in the forward, no contribution in the backward.  The
// table is the padded bf16 device copy of vocab.Vectors: [V, nMp], nMp =
// roundup(nM, 32), pad columns zero, so every row is 16-byte aligned and the
// K padding needs no masking on the A side.
//
// Forward (static_vectors_fwd_kernel<NO>), NO = 96 or 128, the MWE forward's
// tile shape (srx_mwe.hip.h):
// * one 128-token tile per workgroup, 2 * NO/32 waves; wave (mh, w) owns
//   rows [64 mh, +64) and output columns [32 w, +32);
// * the tile's row ids go to LDS first, then the A image [128][nMp + 8] is
//   gathered with 16-byte loads (4 in flight per thread); an OOV row, a row
//   id >= V or a token >= T is staged as zeros and touches no global memory;
// * B = W [NO, nM] is streamed in 32-wide K chunks, k-contiguous, double
//   buffered in LDS with a register prefetch (one barrier per chunk); the
//   nM..nMp tail is zero-filled on the way in.  W rows are only 16-byte
//   aligned when nM % 8 == 0, otherwise the chunk is read element-wise (W is
//   <= 80 KB and cache resident);
// * +8 bf16 pad on every LDS row: strides are 4 mod 16 dwords, conflict-free
//   for ds_read_b128 (see srx_mwe.hip.h);
// * epilogue: fp32 accumulators -> bf16 tile in LDS -> 16-byte row stores
//   into the column block (2-byte stores when ldY / col_off / the base
//   pointer are not 16-byte aligned).  Rows >= T and columns outside the
//   block are never written.
// A whole-K image of both operands would need 168 KB at nM = 300, NO = 128;
// with the B stream it is 102.5 KB (one workgroup per CU), 45 KB at nM = 96.
//
// Backward (static_vectors_bwd_dw_kernel<NO>): the reduction runs over
// tokens, so both MFMA operands are needed token-contiguous.  They are
// staged transposed: a thread loads the 16-byte pieces of two neighbouring
// tokens and writes 8 packed dwords, lanes along the token axis (no bank
// conflicts, half the LDS writes of a 2-byte transpose).  Images are
// [NO][128 + 8] and [nMp][128 + 8].  Wave (mt, nh) keeps the [32, 160] slab
// o in [32 mt, +32), k in [160 nh, +160) of dW in 5 accumulator tiles (80
// VGPRs) across a grid-strided loop over token tiles, then writes it once
// to a [G, NO, nMp] fp32 workspace; static_vectors_reduce_kernel sums over G
// in a fixed order.  No atomics: bit-identical from run to run.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0 and scratch 0 in all five; the LDS is dynamic, so the
// report shows 0 and the figures below are the launcher's, for nMp = 320):
//   static_vectors_fwd_kernel<96>      70 VGPR 47 SGPR  LDS  99,840 B  1 workgroup (6 waves) / CU
//   static_vectors_fwd_kernel<128>     70 VGPR 47 SGPR  LDS 104,960 B  1 workgroup (8 waves) / CU
//   static_vectors_bwd_dw_kernel<96>  136 VGPR 58 SGPR  LDS 113,664 B  1 workgroup (6 waves) / CU
//   static_vectors_bwd_dw_kernel<128> 136 VGPR 58 SGPR  LDS 122,368 B  1 workgroup (8 waves) / CU
//   static_vectors_reduce_kernel        8 VGPR 16 SGPR  LDS       0 B
#pragma once
#include "srx_common.hip.h"
#include "srx_mwe.hip.h"

template <int NO_>
struct SvCfg {
  static constexpr int NO = NO_;
  static constexpr int NW = NO / 32;        // 32-col output tile positions
  static constexpr int MT = 128;            // tokens per tile
  static constexpr int NT = 64 * 2 * NW;    // threads = 4 NO
  static constexpr int KC = 32;             // K chunk of the W stream
  static constexpr int BP = KC + 8;         // padded W chunk row (bf16)
  static constexpr int B_ELEMS = 2 * NO * BP;
  static constexpr int YP = NO + 8;         // epilogue tile row (bf16)
  static constexpr int TP = MT + 8;         // transposed image row (bf16)
  static constexpr int MAXK = 320;          // largest supported nMp
  static constexpr int NJ = MAXK / 64;      // backward: n-tiles per wave
  static_assert(NO * (KC / 8) == NT, "one 16-byte W piece per thread");
  static_assert((MT * (NO / 8)) % NT == 0, "Y tile must split evenly");
};

__device__ __forceinline__ bf16_t sv_half(const srx_u32x4_t& v, int e) {
  return (bf16_t)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
}

// this thread's 8 k-elements of W chunk c (row tid / 4, piece tid % 4)
template <class C>
__device__ __forceinline__ srx_u32x4_t sv_b_fetch(const bf16_t* __restrict__ Wm,
                                                  int c, int tid, int nM,
                                                  bool w_vec) {
  const int j = tid / (C::KC / 8), q = tid % (C::KC / 8);
  const int k0 = c * C::KC + q * 8;
  const bf16_t* src = Wm + (long)j * nM + k0;
  if (w_vec && k0 + 8 <= nM) return *(const srx_u32x4_t*)src;
  srx_u32x4_t v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint32_t h = (k0 + e < nM) ? (uint32_t)src[e] : 0u;
    v[e >> 1] |= h << (16 * (e & 1));
  }
  return v;
}

template <class C>
__device__ __forceinline__ void sv_b_store(bf16_t* ldsBbuf, int tid,
                                           const srx_u32x4_t& pf) {
  const int j = tid / (C::KC / 8), q = tid % (C::KC / 8);
  *(srx_u32x4_t*)(ldsBbuf + j * C::BP + q * 8) = pf;
}

// row ids of the tile -> LDS; everything that must not be gathered is -1
__device__ __forceinline__ void sv_stage_rows(const int* __restrict__ rows,
                                              long T, long t0, int V, int tid,
                                              int* ldsR) {
  if (tid < 128) {
    const long t = t0 + tid;
    int r = -1;
    if (t < T) {
      r = rows[t];
      if (r >= V) r = -1;
    }
    ldsR[tid] = r;
  }
}

// ---------------------------------------------------------------- forward
template <int NO>
__global__ __launch_bounds__(4 * NO) void static_vectors_fwd_kernel(
    const bf16_t* __restrict__ table,  // [V, nMp], pad columns zero
    const int* __restrict__ rows,      // [T], < 0 = OOV
    const bf16_t* __restrict__ Wm,     // [NO, nM] row-major
    bf16_t* __restrict__ Y,            // row stride ldY
    long ldY, int col_off, long T, int V, int nM, int nMp, int w_vec,
    int y_vec) {
  using C = SvCfg<NO>;
  constexpr int MT = C::MT, NT = C::NT, NW = C::NW;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  const int AP = nMp + 8;
  bf16_t* ldsA = lds;                      // gathered image [MT][AP]
  bf16_t* ldsB = lds + MT * AP;            // W chunks x2
  int* ldsR = (int*)(ldsB + C::B_ELEMS);   // row ids [MT]
  bf16_t* ldsY = lds;                      // epilogue tile [MT][YP]

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;
  const long t0 = (long)blockIdx.x * MT;

  sv_stage_rows(rows, T, t0, V, tid, ldsR);
  srx_u32x4_t pf = sv_b_fetch<C>(Wm, 0, tid, nM, w_vec);
  __syncthreads();

  // gather: 4 independent 16-byte loads in flight per thread
  const int Q = nMp / 8;
  const int total = MT * Q;
  for (int base = 0; base < total; base += 4 * NT) {
    srx_u32x4_t v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int id = base + u * NT + tid;
      v[u] = srx_u32x4_t{0u, 0u, 0u, 0u};
      if (id < total) {
        const int i = id / Q, q = id - i * Q;
        const int r = ldsR[i];
        if (r >= 0) v[u] = *(const srx_u32x4_t*)(table + (long)r * nMp + q * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int id = base + u * NT + tid;
      if (id < total) {
        const int i = id / Q, q = id - i * Q;
        *(srx_u32x4_t*)(ldsA + i * AP + q * 8) = v[u];
      }
    }
  }
  sv_b_store<C>(ldsB, tid, pf);
  __syncthreads();

  srx_f32x16 acc[2];
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) acc[mi][rr] = 0.f;

  const int NC = nMp / C::KC;
  const bf16_t* arow = ldsA + (64 * mh + (lane & 31)) * AP + 8 * (lane >> 5);
  for (int c = 0; c < NC; c++) {
    if (c + 1 < NC) pf = sv_b_fetch<C>(Wm, c + 1, tid, nM, w_vec);
    const bf16_t* bbase = ldsB + (c & 1) * (NO * C::BP) +
                          (32 * w + (lane & 31)) * C::BP + 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < C::KC / 16; ks++) {
      const srx_bf16x8 a0 = *(const srx_bf16x8*)(arow + c * C::KC + ks * 16);
      const srx_bf16x8 a1 =
          *(const srx_bf16x8*)(arow + 32 * AP + c * C::KC + ks * 16);
      const srx_bf16x8 bfrag = *(const srx_bf16x8*)(bbase + ks * 16);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, bfrag, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, bfrag, acc[1], 0, 0, 0);
    }
    if (c + 1 < NC) sv_b_store<C>(ldsB + ((c + 1) & 1) * (NO * C::BP), tid, pf);
    __syncthreads();
  }

  // accumulators -> bf16 tile (the images are free after the last barrier)
  const int col = 32 * w + (lane & 31);
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 64 * mh + 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      ldsY[r * C::YP + col] = f2bf(acc[mi][rr]);
    }
  __syncthreads();

  for (int id = tid; id < MT * (NO / 8); id += NT) {
    const int r = id / (NO / 8), q = id % (NO / 8);
    if (t0 + r >= T) continue;
    const srx_u32x4_t v = *(const srx_u32x4_t*)(ldsY + r * C::YP + q * 8);
    bf16_t* dst = Y + (t0 + r) * ldY + col_off + q * 8;
    if (y_vec) {
      *(srx_u32x4_t*)dst = v;
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) dst[e] = sv_half(v, e);
    }
  }
}

// --------------------------------------------------------------- backward
// two neighbouring tokens' 16-byte pieces -> 8 packed dwords of a
// token-contiguous image (element e of token 2 tp and of 2 tp + 1)
__device__ __forceinline__ void sv_store_tr(bf16_t* img, int TP, int q, int tp,
                                            const srx_u32x4_t& v0,
                                            const srx_u32x4_t& v1) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint32_t lo = sv_half(v0, e), hi = sv_half(v1, e);
    *(uint32_t*)(img + (q * 8 + e) * TP + 2 * tp) = lo | (hi << 16);
  }
}

__device__ __forceinline__ srx_u32x4_t sv_load8(const bf16_t* __restrict__ p,
                                                bool vec) {
  if (vec) return *(const srx_u32x4_t*)p;
  srx_u32x4_t v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int e = 0; e < 8; e++) v[e >> 1] |= (uint32_t)p[e] << (16 * (e & 1));
  return v;
}

template <int NO>
__global__ __launch_bounds__(4 * NO) void static_vectors_bwd_dw_kernel(
    const bf16_t* __restrict__ table,  // [V, nMp]
    const int* __restrict__ rows,      // [T]
    const bf16_t* __restrict__ dX,     // row stride ldX; dY = columns col_off..
    long ldX, int col_off,
    float* __restrict__ ws,            // [gridDim.x, NO, nMp]
    long T, int V, int nMp, int ntiles, int x_vec) {
  using C = SvCfg<NO>;
  constexpr int MT = C::MT, NT = C::NT, NW = C::NW, TP = C::TP, NJ = C::NJ;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsAt = lds;                    // dY^T    [NO][TP]
  bf16_t* ldsBt = lds + NO * TP;          // table^T [nMp][TP]
  int* ldsR = (int*)(ldsBt + nMp * TP);   // row ids [MT]

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mt = wave % NW, nh = wave / NW;

  srx_f32x16 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; j++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) acc[j][rr] = 0.f;

  const int Q = nMp / 8;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = (long)tile * MT;
    sv_stage_rows(rows, T, t0, V, tid, ldsR);
    __syncthreads();

    // dY^T: 64 token pairs x NO/8 pieces = 2 per thread.  An OOV token's dY
    // is staged as zero too, so a non-finite gradient there cannot leak.
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int id = u * NT + tid;
      const int tp = id % 64, q = id / 64;
      const bf16_t* src = dX + (t0 + 2 * tp) * ldX + col_off + q * 8;
      const srx_u32x4_t v0 = ldsR[2 * tp] >= 0 ? sv_load8(src, x_vec) : zero;
      const srx_u32x4_t v1 =
          ldsR[2 * tp + 1] >= 0 ? sv_load8(src + ldX, x_vec) : zero;
      sv_store_tr(ldsAt, TP, q, tp, v0, v1);
    }
    // table^T: 64 token pairs x nMp/8 pieces, two pairs in flight
    const int total = 64 * Q;
    for (int base = 0; base < total; base += 2 * NT) {
      srx_u32x4_t v0[2], v1[2];
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int id = base + u * NT + tid;
        v0[u] = zero;
        v1[u] = zero;
        if (id < total) {
          const int tp = id % 64, q = id / 64;
          const int r0 = ldsR[2 * tp], r1 = ldsR[2 * tp + 1];
          if (r0 >= 0) v0[u] = *(const srx_u32x4_t*)(table + (long)r0 * nMp + q * 8);
          if (r1 >= 0) v1[u] = *(const srx_u32x4_t*)(table + (long)r1 * nMp + q * 8);
        }
      }
#pragma unroll
      for (int u = 0; u < 2; u++) {
        const int id = base + u * NT + tid;
        if (id < total) sv_store_tr(ldsBt, TP, id / 64, id % 64, v0[u], v1[u]);
      }
    }
    __syncthreads();

    const bf16_t* abase = ldsAt + (32 * mt + (lane & 31)) * TP + 8 * (lane >> 5);
    const bf16_t* bbase = ldsBt + (lane & 31) * TP + 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < MT / 16; ks++) {
      const srx_bf16x8 afrag = *(const srx_bf16x8*)(abase + ks * 16);
#pragma unroll
      for (int j = 0; j < NJ; j++) {
        const int n0 = 32 * (NJ * nh + j);
        if (n0 < nMp) {
          const srx_bf16x8 bfrag = *(const srx_bf16x8*)(bbase + n0 * TP + ks * 16);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, acc[j],
                                                          0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  float* out = ws + (long)blockIdx.x * NO * nMp;
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    const int n0 = 32 * (NJ * nh + j);
    if (n0 < nMp) {
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int o = 32 * mt + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
        out[(long)o * nMp + n0 + (lane & 31)] = acc[j][rr];
      }
    }
  }
}

// dW[o, k] = sum over g, in order, of ws[g, o, k]; drops the K padding
__global__ void static_vectors_reduce_kernel(const float* __restrict__ ws,
                                             float* __restrict__ dW, int G,
                                             int NO, int nM, int nMp) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= NO * nM) return;
  const int o = idx / nM, k = idx - o * nM;
  float s = 0.f;
  for (int g = 0; g < G; g++) s += ws[((long)g * NO + o) * nMp + k];
  dW[idx] = s;
}
