// Floret vectors: one bf16 vector per distinct word of a batch, the mean of
// the table rows its character n-grams hash to (vocab/vectors.py, floret
// mode).  The host ships the words as a CSR (offsets [U + 1], idx [nnz]):
//   out[u, :] = ( sum_{e in [offsets[u], offsets[u+1])} table[idx[e], :] ) / n_u
// `table` is the padded bf16 device copy of vocab.Vectors ([R, nMp], pad
// columns zero), `out` [U, nMp] has the same layout, so the static-vectors
// kernels (srx_staticvec.hip.h) read it as their table with rows = the
// batch's token -> word map.
//
// floret_words_mean_kernel<SW>:
// * one wave64 per word, words grid-strided over all waves (word lengths
//   are skewed, a fixed slab per workgroup would wait for its longest);
// * a lane owns one 16-byte piece (8 columns) of the row.  SW = 8 / 16 / 32
//   / 64 is the number of lanes one row needs (the power of two >= nMp / 8,
//   64 when nMp > 512, where the pieces are walked in passes of 64); the
//   wave runs S = 64 / SW entry streams side by side, stream s takes
//   entries s, s + S, s + 2 S, ... of the word;
// * the word's indices are read once, 64 at a time, one per lane, and
//   broadcast with a wave shuffle; four independent 16-byte row loads are
//   in flight per lane;
// * fp32 accumulation in entry order inside a stream, the S streams are
//   combined by an xor butterfly (SW, 2 SW, ...: every lane adds the same
//   pairs, so all lanes hold the same bits), then one IEEE fp32 division by
//   float(n_u), one round-to-nearest-even to bf16 and a 16-byte store.
// The order of the additions depends only on the word's own slice and on SW
// (a property of the table), never on U, the word's position or the grid:
// the same word gives the same bits in every batch.  No atomics, no LDS.
//
// Memory safety does not depend on the host: the slice is clamped to
// [0, nnz) (n_u is the clamped length), an entry < 0 or >= R adds +0.0
// without touching memory, rows >= U are never written.  n_u == 0 writes a
// zero row.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0, scratch 0 and LDS 0 in all four; 256 threads):
//   floret_words_mean_kernel<8>    56 VGPR 49 SGPR  8 waves / SIMD
//   floret_words_mean_kernel<16>   54 VGPR 49 SGPR  8 waves / SIMD
//   floret_words_mean_kernel<32>   52 VGPR 49 SGPR  8 waves / SIMD
//   floret_words_mean_kernel<64>   62 VGPR 46 SGPR  8 waves / SIMD
#pragma once
#include "srx_common.hip.h"

#define SRX_FLORET_THREADS 256

template <int SW>
__global__ __launch_bounds__(SRX_FLORET_THREADS) void floret_words_mean_kernel(
    const bf16_t* __restrict__ table,  // [R, nMp], pad columns zero
    const int* __restrict__ offsets,   // [U + 1]
    const int* __restrict__ idx,       // [nnz]
    bf16_t* __restrict__ out,          // [>= U, nMp]
    int U, int R, int nMp, int nnz) {
  constexpr int S = SRX_WAVE / SW;  // entry streams per wave
  const int lane = threadIdx.x % SRX_WAVE;
  const int s = lane / SW, ql = lane % SW;
  const int Q = nMp / 8;
  const int wpb = blockDim.x / SRX_WAVE;
  const int nwaves = gridDim.x * wpb;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};

  for (int u = blockIdx.x * wpb + threadIdx.x / SRX_WAVE; u < U; u += nwaves) {
    int beg = offsets[u], end = offsets[u + 1];
    beg = min(max(beg, 0), nnz);
    end = min(max(end, beg), nnz);
    const int n = end - beg;
    for (int q0 = 0; q0 < Q; q0 += SW) {  // one pass unless nMp > 512
      const int q = q0 + ql;
      const bool live = q < Q;
      const bf16_t* col = table + q * 8;
      float acc[8];
#pragma unroll
      for (int i = 0; i < 8; i++) acc[i] = 0.f;

      for (int c = beg; c < end; c += SRX_WAVE) {
        const int e = c + lane;
        const int mine = e < end ? idx[e] : -1;
        const int cn = min(end - c, SRX_WAVE);
        // 64 / S is a multiple of 4, so (k + j) * S + s stays below 64
        for (int k = 0; k * S < cn; k += 4) {
          srx_u32x4_t v[4];
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const int r = __shfl(mine, (k + j) * S + s, SRX_WAVE);
            v[j] = zero;
            if (live && r >= 0 && r < R)
              v[j] = *(const srx_u32x4_t*)(col + (long)r * nMp);
          }
#pragma unroll
          for (int j = 0; j < 4; j++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
              acc[2 * i] += bf2f((bf16_t)(v[j][i] & 0xffffu));
              acc[2 * i + 1] += bf2f((bf16_t)(v[j][i] >> 16));
            }
        }
      }
#pragma unroll
      for (int off = SW; off < SRX_WAVE; off <<= 1)
#pragma unroll
        for (int i = 0; i < 8; i++) acc[i] += __shfl_xor(acc[i], off, SRX_WAVE);

      if (live && s == 0) {
        srx_u32x4_t o = zero;
        if (n > 0) {
          const float d = (float)n;
#pragma unroll
          for (int i = 0; i < 4; i++)
            o[i] = (uint32_t)f2bf(acc[2 * i] / d) |
                   ((uint32_t)f2bf(acc[2 * i + 1] / d) << 16);
        }
        *(srx_u32x4_t*)(out + (long)u * nMp + q * 8) = o;
      }
    }
  }
}
