// Fused MultiHashEmbed mixer:
//   Y = dropmask * LayerNorm(maxout_{P=3}(E @ Wm^T + bias)),  E [T, NS*W]
// in ONE kernel launch, and the matching backward (stage 1 + dE) in one
// launch.  This is the MaxoutWindowEncoder block of srx_mwe.hip.h without
// the window and the residual: NS plain K sections instead of 3 shifted
// and masked ones, so it shares that file's tile machinery (mwe_b_fetch /
// mwe_b_store / mwe_chunk_mfma), its forward epilogue (mwe_fwd_epilogue)
// and its stage-1 prologue (mwe_stage1_tile / mwe_colsums_*).
//
// Forward, mixer_fwd_kernel<W, NS>: 128 rows per workgroup, 2 * W/32 waves,
// wave (mh, w) owns rows [64 mh, +64) and within-piece columns [32 w, +32)
// of all 3 pieces.  Every E element is used exactly once, so A is not
// staged as a whole-tile image: it is streamed in the same 32-wide K chunks
// as B ([128][32] next to [3W][32]), both double-buffered in LDS with a
// register prefetch, one barrier per chunk.  The stream buffers are 66 KB
// at W = 96; the epilogue tiles (Y, mask / Mout, which) reuse them.
//
// Backward, mixer_bwd_fused_kernel<W, NS>: the stage-1 rows of the tile
// (dropmask x LayerNorm backward x maxout scatter, no halo) go straight
// into the LDS A image [128][3W] and leave once as dPre for the dW GEMM;
// then, per section s < NS,
//   dE[:, sW:(s+1)W] = dPre_tile @ Wm[:, sW:(s+1)W]
// with B = rows [sW, (s+1)W) of Wm^T streamed in K chunks.  Each section
// has its own accumulators and leaves through a bf16 LDS tile with 16-byte
// row-contiguous stores.  dg / db / dbias: one fp32 row per tile, folded by
// mwe_colsum_kernel — no atomics, bit-reproducible.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950) and measurements: docs/KERNELS.md.
#pragma once
#include "srx_mwe.hip.h"

template <int W_, int NS_, bool BWD_>
struct MixCfg {
  static constexpr int W = W_;
  static constexpr int NS = NS_;
  static constexpr bool BWD = BWD_;
  static constexpr int NW = W / 32;
  static constexpr int MT = 128;
  static constexpr int NT = 64 * 2 * NW;
  static constexpr int KA = BWD ? 3 * W : W;   // K per section
  // backward at W = 128: a 96-wide chunk would put the A image, two B
  // chunks and the output tile past the 160 KB of LDS
  static constexpr int KC = BWD ? (W == 96 ? 96 : 32) : 32;
  static constexpr int BP = KC + 8;
  static constexpr int NBR = BWD ? W : 3 * W;  // B rows per chunk
  static constexpr int LDB = BWD ? 3 * W : NS * W;  // B row stride in memory
  static constexpr int NP = BWD ? 1 : 3;
  static constexpr int CPS = KA / KC;
  static constexpr int NC = NS * CPS;
  static constexpr int PF = NBR * (KC / 8) / NT;
  static constexpr int B_ELEMS = 2 * NBR * BP;
  // forward: streamed A chunk [MT][KC], same padded row as B
  static constexpr int A_CHUNK = MT * BP;
  static constexpr int APF = (MT * (KC / 8) + NT - 1) / NT;
  // backward: A image [MT][3W], no halo
  static constexpr int AP = 3 * W + 8;
  static constexpr int A_ELEMS = MT * AP;
  static constexpr int OP = W + 8;             // bf16 output tile row
  static_assert(KA % KC == 0, "K chunking");
  static_assert(PF * NT == NBR * (KC / 8), "B chunk must split evenly");
};

template <int W, int NS>
struct MixFwdLds {
  using C = MixCfg<W, NS, false>;
  static constexpr int WP = W + 8, WHP = W + 16;
  static constexpr int STREAM = (2 * C::A_CHUNK + C::B_ELEMS) * 2;  // bytes
  static constexpr int EPI = 2 * C::MT * WP * 2 + C::MT * WHP;
  static constexpr int TILES = ((STREAM > EPI ? STREAM : EPI) + 15) / 16 * 16;
  static constexpr int BYTES = TILES + (2 * C::NW * C::MT + 2 * C::MT) * 4;
};

// global -> registers / registers -> LDS: this thread's pieces of A chunk c
template <class C>
__device__ __forceinline__ void mixer_a_fetch(const bf16_t* __restrict__ E, int c,
                                              long T, long t0, int tid,
                                              srx_u32x4_t (&pa)[C::APF]) {
#pragma unroll
  for (int i = 0; i < C::APF; i++) {
    const int id = i * C::NT + tid;
    const int r = id / (C::KC / 8), q = id % (C::KC / 8);
    pa[i] = srx_u32x4_t{0u, 0u, 0u, 0u};
    if (r < C::MT && t0 + r < T)
      pa[i] = *(const srx_u32x4_t*)(E + (t0 + r) * (long)(C::NS * C::W) +
                                    c * C::KC + q * 8);
  }
}

template <class C>
__device__ __forceinline__ void mixer_a_store(bf16_t* ldsAbuf, int tid,
                                              const srx_u32x4_t (&pa)[C::APF]) {
#pragma unroll
  for (int i = 0; i < C::APF; i++) {
    const int id = i * C::NT + tid;
    const int r = id / (C::KC / 8), q = id % (C::KC / 8);
    if (r < C::MT) *(srx_u32x4_t*)(ldsAbuf + r * C::BP + q * 8) = pa[i];
  }
}

// -------------------------------------------------------------- forward
template <int W, int NS>
__global__ __launch_bounds__(4 * W) void mixer_fwd_kernel(
    const bf16_t* __restrict__ E,      // [T, NS*W]
    const bf16_t* __restrict__ Wm,     // [3W (out, pieces-major), NS*W (in)]
    const bf16_t* __restrict__ bias,   // [3W]
    const bf16_t* __restrict__ g,      // [W]
    const bf16_t* __restrict__ b,      // [W]
    const bf16_t* __restrict__ dropmask,  // [T, W] 0 or 1/keep, or nullptr
    bf16_t* __restrict__ Y,            // [T, W]
    bf16_t* __restrict__ Mout,         // [T, W] maxout output (for bwd)
    uint8_t* __restrict__ which,       // [T, W]
    float* __restrict__ mu_out,        // [T]
    float* __restrict__ rstd_out,      // [T]
    long T, float eps) {
  using C = MixCfg<W, NS, false>;
  using L = MixFwdLds<W, NS>;
  constexpr int NW = C::NW, MT = C::MT;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;                               // A chunks x2
  bf16_t* ldsB = lds + 2 * C::A_CHUNK;              // B chunks x2
  bf16_t* ldsY = lds;                               // epilogue: Y
  bf16_t* ldsM = lds + MT * L::WP;                  // epilogue: mask, then Mout
  uint8_t* ldsWh = (uint8_t*)(lds + 2 * MT * L::WP);  // epilogue: which
  float* ldsP = (float*)((char*)lds + L::TILES);    // LN partials [2][NW][MT]
  float* ldsS = ldsP + 2 * NW * MT;                 // mu, rstd [2][MT]

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;
  const long t0 = (long)blockIdx.x * MT;

  srx_u32x4_t pf[C::PF], pa[C::APF];
  mwe_b_fetch<C>(Wm, 0, tid, pf);
  mixer_a_fetch<C>(E, 0, T, t0, tid, pa);

  srx_f32x16 acc[3][2];  // [piece][m-tile]
#pragma unroll
  for (int p = 0; p < 3; p++)
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int rr = 0; rr < 16; rr++) acc[p][mi][rr] = 0.f;

  mwe_b_store<C>(ldsB, tid, pf);
  mixer_a_store<C>(ldsA, tid, pa);
  __syncthreads();

  for (int c = 0; c < C::NC; c++) {
    if (c + 1 < C::NC) {
      mwe_b_fetch<C>(Wm, c + 1, tid, pf);
      mixer_a_fetch<C>(E, c + 1, T, t0, tid, pa);
    }
    const bf16_t* abase = ldsA + (c & 1) * C::A_CHUNK +
                          (64 * mh + (lane & 31)) * C::BP + 8 * (lane >> 5);
    const bf16_t* bbase = ldsB + (c & 1) * (C::NBR * C::BP) +
                          (32 * w + (lane & 31)) * C::BP + 8 * (lane >> 5);
    mwe_chunk_mfma<C, C::BP>(abase, bbase, false, false, acc);
    if (c + 1 < C::NC) {
      mwe_b_store<C>(ldsB + ((c + 1) & 1) * (C::NBR * C::BP), tid, pf);
      mixer_a_store<C>(ldsA + ((c + 1) & 1) * C::A_CHUNK, tid, pa);
    }
    __syncthreads();
  }

  mwe_fwd_epilogue<W, false>(acc, bias, g, b, dropmask, ldsY, ldsM, ldsWh, ldsP,
                             ldsS, Y, Mout, which, mu_out, rstd_out, T, t0, eps);
}

// ------------------------------------------------- backward: stage 1 + dE
template <int W, int NS>
__global__ __launch_bounds__(4 * W) void mixer_bwd_fused_kernel(
    const bf16_t* __restrict__ dY,        // [T, W]
    const bf16_t* __restrict__ dropmask,  // [T, W] or nullptr
    const bf16_t* __restrict__ Mout,      // [T, W]
    const bf16_t* __restrict__ g,         // [W]
    const float* __restrict__ mu,         // [T]
    const float* __restrict__ rstd,       // [T]
    const uint8_t* __restrict__ which,    // [T, W]
    const bf16_t* __restrict__ WT,        // [NS*W, 3W] = Wm^T, row-major
    bf16_t* __restrict__ dPre,            // [T, 3W]
    bf16_t* __restrict__ dE,              // [T, NS*W]
    float* __restrict__ partials,         // [gridDim.x, 5W]
    long T) {
  using C = MixCfg<W, NS, true>;
  constexpr int NW = C::NW, MT = C::MT, NT = C::NT, AP = C::AP, OP = C::OP;
  constexpr int Q = W / 8;
  constexpr int NWAVE = NT / SRX_WAVE;
  static_assert(NWAVE * 5 * W * 4 <= C::B_ELEMS * 2, "column-sum partials");
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;                      // stage-1 rows [MT][3W]
  bf16_t* ldsB = lds + C::A_ELEMS;         // B chunks x2
  bf16_t* ldsO = ldsB + C::B_ELEMS;        // one section's dE tile [MT][W]
  float* ldsC = (float*)ldsB;  // epilogue: column sums [NWAVE][5W] over B

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;
  const long t0 = (long)blockIdx.x * MT;

  srx_u32x4_t pf[C::PF];
  mwe_b_fetch<C>(WT, 0, tid, pf);

  float dg_loc[8], db_loc[8], dbias_loc[3][8];
  mwe_stage1_tile<W, NT, AP, 0>(dY, dropmask, Mout, g, mu, rstd, which, T, t0,
                                tid, ldsA, dg_loc, db_loc, dbias_loc);
  mwe_b_store<C>(ldsB, tid, pf);
  __syncthreads();

  // ---- dPre out, once, for the dW GEMM
  for (int id = tid; id < MT * (3 * Q); id += NT) {
    const int r = id / (3 * Q), c = id % (3 * Q);
    if (t0 + r < T)
      *(srx_u32x4_t*)(dPre + (t0 + r) * (3 * W) + c * 8) =
          *(const srx_u32x4_t*)(ldsA + r * AP + c * 8);
  }

  const int col = 32 * w + (lane & 31);
  const bf16_t* arow = ldsA + (64 * mh + (lane & 31)) * AP + 8 * (lane >> 5);
#pragma nounroll
  for (int s = 0; s < NS; s++) {
    srx_f32x16 acc[1][2];
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int rr = 0; rr < 16; rr++) acc[0][mi][rr] = 0.f;
#pragma nounroll
    for (int kc = 0; kc < C::CPS; kc++) {
      const int c = s * C::CPS + kc;
      if (c + 1 < C::NC) mwe_b_fetch<C>(WT, c + 1, tid, pf);
      const bf16_t* bbase = ldsB + (c & 1) * (C::NBR * C::BP) +
                            (32 * w + (lane & 31)) * C::BP + 8 * (lane >> 5);
      mwe_chunk_mfma<C, AP>(arow + kc * C::KC, bbase, false, false, acc);
      if (c + 1 < C::NC)
        mwe_b_store<C>(ldsB + ((c + 1) & 1) * (C::NBR * C::BP), tid, pf);
      __syncthreads();
    }
    // this section's [MT][W] block of dE, through LDS.  The tile is read
    // below and next written after the next section's CPS >= 3 barriers.
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int r = 64 * mh + 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
        ldsO[r * OP + col] = f2bf(acc[0][mi][rr]);
      }
    __syncthreads();
    for (int id = tid; id < MT * Q; id += NT) {
      const int r = id / Q, qq = id % Q;
      if (t0 + r < T)
        *(srx_u32x4_t*)(dE + (t0 + r) * (long)(NS * W) + s * W + qq * 8) =
            *(const srx_u32x4_t*)(ldsO + r * OP + qq * 8);
    }
  }

  // ---- column sums (the B region is free after the last chunk's barrier)
  mwe_colsums_park<W>(dg_loc, db_loc, dbias_loc, ldsC, tid);
  __syncthreads();
  mwe_colsums_out<W, NT>(ldsC, partials + (long)blockIdx.x * (5 * W), tid);
}
