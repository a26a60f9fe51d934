// MaxoutWindowEncoder weight gradient without dPre, seq2col or a library
// GEMM (mwe_bwd_dw_kernel<W>, W = 96):
//   dW[p W + c, s W + j] = sum_t [which[t,c] == p] dM[t,c] X[t - 1 + s, j]
// with section s = 0 dropped at a doc start / t = 0 and s = 2 at a doc end /
// t = T-1, exactly where seq2col_fwd_kernel writes zeros.  It reads dM
// [T, W] (the compact output of mwe_bwd_fused_kernel), `which`, X and the
// boundary bytes: 480 B per token instead of the 2.3 KB per token of the
// dPre [T, 3W] / X3 [T, 3W] round trip it replaces.
//
// Structure (gfx950):
// * persistent grid, at most one workgroup per CU, grid-strided over
//   128-token tiles; 12 waves (768 threads).  The 288 x 288 fp32 result
//   stays in registers across all of a workgroup's tiles: 18 x 18 tiles of
//   v_mfma_f32_16x16x32_bf16, 27 per wave (108 VGPRs).  Wave (ct, jh) owns
//   rows {p W + 16 ct + [0, 16)} for all three pieces p and columns
//   {s W + 16 (3 jh + jj) + [0, 16)} for all three sections s, jj < 3;
// * the reduction runs over tokens, so both operands are staged
//   token-contiguous (transposed), two neighbouring tokens packed per dword
//   as static_vectors_bwd_dw_kernel does: wave q stages the 8 columns
//   [8 q, 8 q + 8), lane l the tokens 2 l and 2 l + 1 of the tile;
// * five [W][128] bf16 images: dM^T, the one-hot code 1 << which^T, and
//   X^T once per section, shifted by s - 1 tokens with the (token, section)
//   boundary mask already applied, so a B fragment is one aligned
//   ds_read_b128 and the inner loop has no per-token masking.  The shifted
//   pairs come from the neighbouring lanes (the tile's two halo tokens
//   t0 - 1 and t0 + 128 are loaded by lanes 0 and 63);
// * the piece expansion happens in registers: a wave reads one dM fragment
//   and one code fragment per 32 tokens and ANDs three masked A fragments
//   out of them, never in memory;
// * the images are interleaved by row (row r of all five, then row r + 1:
//   every LDS address of a thread is one register plus a 16-bit immediate).
//   Image rows are 128 + 8 bf16, so 16 consecutive rows of one image start
//   on 16 distinct 4-bank slots, and rows 4..11 of every 16 swap each even
//   16-byte chunk with its odd neighbour.  A 16x16x32 fragment read has lane
//   = row and lane >> 4 = chunk, and ds_read_b128 serves lanes {0-3, 12-15,
//   20-27} together: rows 0-3 and 12-15 at chunk c with rows 4-11 at chunk
//   c + 1.  With the swap all 16 read the same chunk position, so they stay
//   on 16 distinct slots; with the padding alone two of them collide;
// * the next tile's global loads (26 VGPRs) are issued before the current
//   tile's MFMAs and written to LDS after them: two barriers per tile;
// * each workgroup writes one fp32 partial [3W, 3W]; mwe_dw_reduce_kernel
//   adds the partials in workgroup order in fp64 and rounds to bf16 once.
//   No atomics: bit-identical from run to run in every mode.
//
// W = 128 (384 x 384 accumulators) does not fit one workgroup this way and
// stays on the seq2col + chunked-GEMM path (docs/KERNELS.md).
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0 and scratch 0 in both; the LDS is dynamic):
//   mwe_bwd_dw_kernel<96>  168 VGPR 50 SGPR  LDS 130,560 B  1 workgroup (12 waves) / CU
//   mwe_dw_reduce_kernel    16 VGPR 19 SGPR  LDS       0 B
// Measured at T = 1M (MI355X): 0.26 ms with the reduction, against 0.19 +
// 0.42 ms for seq2col_fwd + the chunked GEMM; see profiles/README.md.
#pragma once
#include "srx_common.hip.h"
#include "srx_mwe.hip.h"
#include "srx_staticvec.hip.h"

typedef __attribute__((__vector_size__(4 * sizeof(float)))) float srx_f32x4;

template <int W_>
struct MweDwCfg {
  static constexpr int W = W_;
  static constexpr int MT = 128;               // tokens per tile
  static constexpr int NWAVE = W / 8;          // one 8-column piece per wave
  static constexpr int NT = 64 * NWAVE;        // 768 threads at W = 96
  static constexpr int CT = W / 16;            // 16-row tiles per piece
  static constexpr int JH = NWAVE / CT;        // column groups (2)
  static constexpr int NJ = CT / JH;           // 16-col tiles per section per wave
  static constexpr int TP = MT + 8;            // image row (bf16)
  static constexpr int NIMG = 5;               // dM, code, X section 0 / 1 / 2
  static constexpr int RP = NIMG * TP;         // row pitch: images interleaved
  static constexpr int LDS_BYTES = W * RP * 2;
  static_assert(W == 96, "mwe_bwd_dw_kernel: 288 x 288 accumulators, 12 waves");
  static_assert(NWAVE == CT * JH && CT == NJ * JH, "wave decomposition");
};

// the next tile's operands, in registers
struct MweDwPrefetch {
  srx_u32x4_t da, db;  // dM, tokens 2l and 2l + 1
  srx_u32x4_t xa, xb;  // X
  srx_u32x4_t xh;      // X halo: lane 0 token t0 - 1, lane 63 token t0 + 128
  uint2 wa, wb;        // which
  uint32_t bnd;        // is_start (bits 0, 1) and is_end (bits 2, 3) of the pair
};

template <int W>
__device__ __forceinline__ void mwe_dw_fetch(
    const bf16_t* __restrict__ dM, const uint8_t* __restrict__ which,
    const bf16_t* __restrict__ X, const uint8_t* __restrict__ is_start,
    const uint8_t* __restrict__ is_end, long T, long t0, int q, int lane,
    MweDwPrefetch& pf) {
  const srx_u32x4_t zero = {0u, 0u, 0u, 0u};
  const long ta = t0 + 2 * lane;  // T is even: ta < T implies ta + 1 < T
  pf.da = pf.db = pf.xa = pf.xb = pf.xh = zero;
  pf.wa = pf.wb = make_uint2(0u, 0u);
  pf.bnd = 0u;
  if (ta < T) {
    const long o = ta * W + q * 8;
    pf.da = *(const srx_u32x4_t*)(dM + o);
    pf.db = *(const srx_u32x4_t*)(dM + o + W);
    pf.xa = *(const srx_u32x4_t*)(X + o);
    pf.xb = *(const srx_u32x4_t*)(X + o + W);
    pf.wa = *(const uint2*)(which + o);
    pf.wb = *(const uint2*)(which + o + W);
    pf.bnd = (is_start[ta] ? 1u : 0u) | (is_start[ta + 1] ? 2u : 0u) |
             (is_end[ta] ? 4u : 0u) | (is_end[ta + 1] ? 8u : 0u);
  }
  if (lane == 0 && t0 > 0)
    pf.xh = *(const srx_u32x4_t*)(X + (t0 - 1) * W + q * 8);
  if (lane == 63 && t0 + 128 < T)
    pf.xh = *(const srx_u32x4_t*)(X + (t0 + 128) * W + q * 8);
}

__device__ __forceinline__ srx_u32x4_t mwe_dw_shfl_up1(const srx_u32x4_t& v) {
  srx_u32x4_t r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = __shfl_up(v[k], 1, SRX_WAVE);
  return r;
}

__device__ __forceinline__ srx_u32x4_t mwe_dw_shfl_down1(const srx_u32x4_t& v) {
  srx_u32x4_t r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = __shfl_down(v[k], 1, SRX_WAVE);
  return r;
}

// Dword of (image m, row, token pair l): row * 340 + m * 68 + (l ^ 4 key(row)),
// key = 1 for rows 4..11 of every 16 (the chunk swap of the file comment).
// A staging thread's rows are q 8 + e: key = (e >= 4) != (q odd), so its
// eight dwords are two lane terms (l0 for e < 4, l0 ^ 4 above) plus
// compile-time offsets.
__device__ __forceinline__ int mwe_dw_dword(int m, int q, int e, int l0) {
  return (q * 8 + e) * 340 + m * 68 + (e < 4 ? l0 : (l0 ^ 4));
}

// element e of v0 (token 2l) and of v1 (token 2l + 1), ANDed with `mask`
__device__ __forceinline__ void mwe_dw_store_tr(bf16_t* lds, int m, int q, int l0,
                                                const srx_u32x4_t& v0,
                                                const srx_u32x4_t& v1,
                                                uint32_t mask) {
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint32_t lo = sv_half(v0, e), hi = sv_half(v1, e);
    ((uint32_t*)lds)[mwe_dw_dword(m, q, e, l0)] = (lo | (hi << 16)) & mask;
  }
}

template <int W>
__device__ __forceinline__ void mwe_dw_stage(const MweDwPrefetch& pf, int q,
                                             int lane, bf16_t* lds) {
  static_assert(MweDwCfg<W>::RP == 2 * 340, "mwe_dw_dword");
  const int l0 = lane ^ ((q & 1) << 2);
  mwe_dw_store_tr(lds, 0, q, l0, pf.da, pf.db, 0xffffffffu);
  // one-hot piece code per element
#pragma unroll
  for (int e = 0; e < 8; e++) {
    const uint32_t ba = ((e < 4 ? pf.wa.x : pf.wa.y) >> (8 * (e & 3))) & 0xffu;
    const uint32_t bb = ((e < 4 ? pf.wb.x : pf.wb.y) >> (8 * (e & 3))) & 0xffu;
    ((uint32_t*)lds)[mwe_dw_dword(1, q, e, l0)] = (1u << ba) | ((1u << bb) << 16);
  }
  // X: section s holds X[t - 1 + s] at token t, zero where seq2col drops it.
  // t = 0 and t = T - 1 need no test: the neighbour is staged as zero.
  srx_u32x4_t prevb = mwe_dw_shfl_up1(pf.xb);
  srx_u32x4_t nexta = mwe_dw_shfl_down1(pf.xa);
  if (lane == 0) prevb = pf.xh;
  if (lane == 63) nexta = pf.xh;
  const uint32_t m0 = ((pf.bnd & 1u) ? 0u : 0x0000ffffu) |
                      ((pf.bnd & 2u) ? 0u : 0xffff0000u);
  const uint32_t m2 = ((pf.bnd & 4u) ? 0u : 0x0000ffffu) |
                      ((pf.bnd & 8u) ? 0u : 0xffff0000u);
  mwe_dw_store_tr(lds, 2, q, l0, prevb, pf.xa, m0);
  mwe_dw_store_tr(lds, 3, q, l0, pf.xa, pf.xb, 0xffffffffu);
  mwe_dw_store_tr(lds, 4, q, l0, pf.xb, nexta, m2);
}

template <int W>
__global__ __launch_bounds__(8 * W) void mwe_bwd_dw_kernel(
    const bf16_t* __restrict__ dM,        // [T, W]
    const uint8_t* __restrict__ which,    // [T, W]
    const bf16_t* __restrict__ X,         // [T, W]
    const uint8_t* __restrict__ is_start, // [T]
    const uint8_t* __restrict__ is_end,   // [T]
    float* __restrict__ ws,               // [gridDim.x, 3W, 3W]
    long T, int ntiles) {
  using C = MweDwCfg<W>;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = __builtin_amdgcn_readfirstlane(tid / SRX_WAVE);  // scalar
  const int ct = wave % C::CT, jh = wave / C::CT;
  const int r = lane & 15, g = lane >> 4;

  srx_f32x4 acc[3][C::NJ][3];  // [piece][column tile][section]
#pragma unroll
  for (int p = 0; p < 3; p++)
#pragma unroll
    for (int jj = 0; jj < C::NJ; jj++)
#pragma unroll
      for (int s = 0; s < 3; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) acc[p][jj][s][k] = 0.f;

  // fragment addresses at k-step 0: this lane's row and (swapped) chunk
  const int coff = (8 * g) ^ (((r + 4) & 8) ? 8 : 0);
  const bf16_t* arow = lds + (16 * ct + r) * C::RP + coff;
  const bf16_t* crow = arow + C::TP;
  const bf16_t* xrow = lds + (16 * C::NJ * jh + r) * C::RP + 2 * C::TP + coff;

  MweDwPrefetch pf;
  int tile = blockIdx.x;
  if (tile < ntiles)
    mwe_dw_fetch<W>(dM, which, X, is_start, is_end, T, (long)tile * C::MT, wave,
                    lane, pf);
  for (; tile < ntiles; tile += gridDim.x) {
    mwe_dw_stage<W>(pf, wave, lane, lds);
    __syncthreads();
    const int next = tile + gridDim.x;
    if (next < ntiles)
      mwe_dw_fetch<W>(dM, which, X, is_start, is_end, T, (long)next * C::MT, wave,
                      lane, pf);

#pragma unroll 1
    for (int ks = 0; ks < C::MT / 32; ks++) {
      const int off = 32 * ks;
      const srx_u32x4_t dmf = *(const srx_u32x4_t*)(arow + off);
      const srx_u32x4_t cdf = *(const srx_u32x4_t*)(crow + off);
      srx_bf16x8 afrag[3];
#pragma unroll
      for (int p = 0; p < 3; p++) {
        srx_u32x4_t a;
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t m = (cdf[k] >> p) & 0x00010001u;
          a[k] = dmf[k] & ((m << 16) - m);  // 0xffff per selected half
        }
        afrag[p] = (srx_bf16x8)a;
      }
#pragma unroll
      for (int jj = 0; jj < C::NJ; jj++) {
#pragma unroll
        for (int s = 0; s < 3; s++) {
          const srx_bf16x8 bfrag =
              *(const srx_bf16x8*)(xrow + s * C::TP + jj * 16 * C::RP + off);
#pragma unroll
          for (int p = 0; p < 3; p++)
            acc[p][jj][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                afrag[p], bfrag, acc[p][jj][s], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  // C/D layout of 16x16x32: column = lane & 15, row = 4 (lane >> 4) + k.
  // The lane id is read again here (mbcnt) so that no index register has to
  // stay live across the tile loop, where there is none to spare.
  const int el = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  const int er = el & 15, eg = el >> 4;
  float* out = ws + (long)blockIdx.x * (3 * W) * (3 * W);
#pragma unroll
  for (int p = 0; p < 3; p++)
#pragma unroll
    for (int jj = 0; jj < C::NJ; jj++)
#pragma unroll
      for (int s = 0; s < 3; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int row = p * W + 16 * ct + 4 * eg + k;
          const int col = s * W + 16 * (C::NJ * jh + jj) + er;
          out[(long)row * (3 * W) + col] = acc[p][jj][s][k];
        }
}

// dW[i] = bf16(sum over g, in order, of ws[g, i]); fp64 accumulation
__global__ void mwe_dw_reduce_kernel(const float* __restrict__ ws,
                                     bf16_t* __restrict__ dW, int G, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
#pragma unroll 8
  for (int gi = 0; gi < G; gi++) s += (double)ws[(long)gi * n + i];
  dW[i] = f2bf((float)s);
}
