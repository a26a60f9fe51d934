// Pretraining against static vectors (spaCy's PretrainVectors objective):
// distance between each predicted row and a row gathered from the vectors
// table, and its gradient, in one launch.  Per row i, p = pred[i, :nM], y =
// table[rows[i], :nM]:
//   cosine  loss_i = 1 - c,  c = p.y / (|p| |y|)
//           dp     = -scale (y / (|p| |y|) - c p / |p|^2)
//   L2      loss_i = sum (p - y)^2,   dp = scale (p - y)
//           (thinc's L2Distance: the gradient carries no factor 2)
// A row is skipped (loss 0, dPred row exactly zero) when rows[i] < 0, when
// rows[i] >= V, and for the cosine also when |y|^2 == 0 or |p|^2 == 0 (as
// fp32 sums of squares: every element zero, or so small that the sum
// underflows).  A skipped row's prediction is never used, so a non-finite
// value there reaches no output.  `table` is the padded bf16 device copy of
// vocab.Vectors or a floret batch's temporary table ([V, nMp], rows 16-byte
// aligned, srx_staticvec.hip.h); its pad columns are masked, not trusted.
//
// vectors_loss_kernel<SW, PV>:
// * a row is Q = nMp / 8 <= 40 pieces of 8 columns; a lane owns one piece
//   (8 p, 8 y in registers).  SW = 8 / 16 / 32 / 64 lanes form the sub-wave
//   of one row (the power of two >= Q), a wave works on S = 64 / SW rows
//   side by side; groups of S rows are grid-strided over all waves, the
//   next group's row id is fetched while this one is computed;
// * table side: one 16-byte load per lane, issued only for a row id in
//   [0, V), so a skipped row touches no table memory;
// * prediction side: row i starts at pred + i ldP, 16-byte aligned only
//   when the base and 2 ldP are.  PV = 8 / 4 / 2 / 1 is the number of bf16
//   per load and store (16 / 8 / 4 / 2 bytes), the widest the host found
//   that divides both base pointers, both row strides and nM; a piece is
//   moved as 8 / PV accesses, each entirely below column nM or not issued.
//   nM = 300 runs at PV = 4, nM = 50 at PV = 2, nM % 8 == 0 at PV = 8;
// * fp32 throughout; p.p, y.y and p.y (L2: sum (p - y)^2) are xor
//   butterflies over the SW lanes of the sub-wave, every lane ends with
//   the same bits; each gradient element is rounded to bf16 once;
// * lane 0 of the sub-wave writes loss_i (fp32; the host sums the N values
//   with one torch.sum).  No atomics, no LDS: bit-identical from run to
//   run, and a row's bits do not depend on N or on its position.
// Rows >= N and columns >= nM are neither read nor written.
//
// Floor: N (2 nM 2 + nMp 2) bytes (p in, dp out, y in).
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0, scratch 0 and LDS 0 in all sixteen; 256 threads; VGPR /
// SGPR; 8 waves / SIMD, 7 in the PV = 1 column):
//   SW \ PV     8         4         2         1
//    8       62 / 68   60 / 63   56 / 63   70 / 63
//   16       62 / 68   60 / 63   56 / 63   70 / 63
//   32       60 / 68   58 / 63   54 / 63   68 / 63
//   64       56 / 67   56 / 65   52 / 65   66 / 65
#pragma once
#include "srx_common.hip.h"

#define SRX_VECLOSS_THREADS 256

typedef __attribute__((__vector_size__(8))) uint32_t srx_u32x2_t;

// columns [col0, col0 + 8) of one prediction row -> 4 packed dwords; a
// PV-element access is issued only when it lies below column nM
template <int PV>
__device__ __forceinline__ srx_u32x4_t vl_load8(const bf16_t* __restrict__ row,
                                                int col0, int nM) {
  srx_u32x4_t v = {0u, 0u, 0u, 0u};
  if (PV == 8) {
    if (col0 < nM) v = *(const srx_u32x4_t*)(row + col0);
  } else if (PV == 4) {
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (col0 + 4 * j < nM) {
        const srx_u32x2_t t = *(const srx_u32x2_t*)(row + col0 + 4 * j);
        v[2 * j] = t[0];
        v[2 * j + 1] = t[1];
      }
  } else if (PV == 2) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (col0 + 2 * j < nM) v[j] = *(const uint32_t*)(row + col0 + 2 * j);
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++)
      if (col0 + e < nM) v[e >> 1] |= (uint32_t)row[col0 + e] << (16 * (e & 1));
  }
  return v;
}

template <int PV>
__device__ __forceinline__ void vl_store8(bf16_t* __restrict__ row, int col0,
                                          int nM, const srx_u32x4_t& v) {
  if (PV == 8) {
    if (col0 < nM) *(srx_u32x4_t*)(row + col0) = v;
  } else if (PV == 4) {
#pragma unroll
    for (int j = 0; j < 2; j++)
      if (col0 + 4 * j < nM) {
        const srx_u32x2_t t = {v[2 * j], v[2 * j + 1]};
        *(srx_u32x2_t*)(row + col0 + 4 * j) = t;
      }
  } else if (PV == 2) {
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (col0 + 2 * j < nM) *(uint32_t*)(row + col0 + 2 * j) = v[j];
  } else {
#pragma unroll
    for (int e = 0; e < 8; e++)
      if (col0 + e < nM)
        row[col0 + e] = (bf16_t)((v[e >> 1] >> (16 * (e & 1))) & 0xffffu);
  }
}

// sum over the SW lanes of a sub-wave; all of them get the same bits
template <int SW>
__device__ __forceinline__ float vl_reduce(float v) {
#pragma unroll
  for (int off = SW / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, SRX_WAVE);
  return v;
}

template <int SW, int PV>
__global__ __launch_bounds__(SRX_VECLOSS_THREADS) void vectors_loss_kernel(
    const bf16_t* __restrict__ pred,   // row stride ldP, columns [0, nM)
    const bf16_t* __restrict__ table,  // [V, nMp]
    const int* __restrict__ rows,      // [N]
    float* __restrict__ row_loss,      // [>= N]
    bf16_t* __restrict__ dpred,        // row stride ldD, columns [0, nM)
    long ldP, long ldD, long N, int V, int nM, int nMp, int l2, float scale) {
  constexpr int S = SRX_WAVE / SW;  // rows per wave
  const int lane = threadIdx.x % SRX_WAVE;
  const int s = lane / SW, ql = lane % SW;
  const int Q = nMp / 8;
  const int col0 = ql * 8;
  const bool live = ql < Q;
  const long wpb = blockDim.x / SRX_WAVE;
  const long stride = (long)gridDim.x * wpb * S;
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};

  long i = ((long)blockIdx.x * wpb + threadIdx.x / SRX_WAVE) * S + s;
  // loop bound on the group's first row: the trip count is the same for
  // all 64 lanes, the shuffles below always see a full wave
  int r_next = i < N ? rows[i] : -1;
  for (; i - s < N; i += stride) {
    const int r = r_next;
    const long in = i + stride;
    r_next = in < N ? rows[in] : -1;
    const bool inrow = i < N;
    const bool valid = inrow && r >= 0 && r < V;

    srx_u32x4_t pv = zero, yv = zero;
    if (valid && live) {
      pv = vl_load8<PV>(pred + i * ldP, col0, nM);
      yv = *(const srx_u32x4_t*)(table + (long)r * nMp + col0);
    }
    float p[8], y[8];
#pragma unroll
    for (int e = 0; e < 8; e++) {
      p[e] = bf2f((bf16_t)((pv[e >> 1] >> (16 * (e & 1))) & 0xffffu));
      const float t = bf2f((bf16_t)((yv[e >> 1] >> (16 * (e & 1))) & 0xffffu));
      y[e] = col0 + e < nM ? t : 0.f;  // table pad columns
    }

    float loss = 0.f, ca = 0.f, cb = 0.f;  // cosine: dp = ca y + cb p
    bool skip = !valid;
    if (l2) {
      float dd = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const float d = p[e] - y[e];
        dd += d * d;
      }
      loss = vl_reduce<SW>(dd);
    } else {
      float pp = 0.f, yy = 0.f, py = 0.f;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        pp += p[e] * p[e];
        yy += y[e] * y[e];
        py += p[e] * y[e];
      }
      pp = vl_reduce<SW>(pp);
      yy = vl_reduce<SW>(yy);
      py = vl_reduce<SW>(py);
      skip = skip || yy == 0.f || pp == 0.f;
      if (!skip) {
        const float inv = 1.f / (sqrtf(pp) * sqrtf(yy));
        const float c = py * inv;
        loss = 1.f - c;
        ca = -scale * inv;
        cb = scale * c / pp;
      }
    }

    srx_u32x4_t o = zero;
    if (!skip) {
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; e++)
        g[e] = l2 ? scale * (p[e] - y[e]) : ca * y[e] + cb * p[e];
#pragma unroll
      for (int k = 0; k < 4; k++)
        o[k] = (uint32_t)f2bf(g[2 * k]) | ((uint32_t)f2bf(g[2 * k + 1]) << 16);
    }
    if (inrow && live) vl_store8<PV>(dpred + i * ldD, col0, nM, o);
    if (inrow && ql == 0) row_loss[i] = skip ? 0.f : loss;
  }
}
