// Fused MaxoutWindowEncoder layer (SURVEY.md §2.5 `mwe_layer`):
//   Y = X + LayerNorm(maxout_{P=3}(seq2col_{win=1}(X) @ Wt^T + bias))
// in ONE kernel launch, and the matching backward dX
//   dX[t] = dY[t] + sum_s m_s(t) * dPre[t+1-s] @ weight[:, sW:(s+1)W]
// also in one launch — hand-written MFMA (v_mfma_f32_32x32x16_bf16) with
// LDS-tiled operands.  Both are the same "3 shifted sections" GEMM and
// share the tile machinery below (MweCfg / mwe_tile_gemm).
//
// Tile machinery (gfx950), W = 96 or 128:
// * one 128-row M tile per workgroup, 2 * W/32 waves (384 / 512 threads):
//   wave (mh, w) owns rows [64 mh, 64 mh + 64) and the 32-col tile position
//   w.  In the forward that is within-piece position w of ALL 3 pieces
//   (global n-tile p*(W/32)+w): the P=3 maxout is an in-register
//   elementwise max over the wave's own 3 accumulators;
// * the A operand (X, or dPre with K = 3W) is staged ONCE as a halo image,
//   rows t0-1 .. t0+128, by all threads with 16-byte coalesced accesses.
//   Section s reads it at row offset s (forward) or 2-s (backward).  The
//   doc-boundary zeroing is per (row, section), so it is applied to the A
//   fragment in registers (a v_cndmask on 4 VGPRs), never to the image;
// * the B operand is streamed in K chunks ([3W][32] forward, [W][96]
//   backward; rows are k-contiguous so a lane's 8 k-elements are one
//   ds_read_b128), double-buffered in LDS with a register prefetch: the
//   global loads of chunk c+1 are issued before the MFMAs of chunk c and
//   written to the other buffer after them — one barrier per chunk, 12
//   MFMAs per wave between barriers.  The weight is staged once per 128
//   rows (was once per 64);
// * +8 bf16 row pad on every image: strides of 20 / 52 / 68 / 148 / 196
//   dwords put 16 consecutive rows on 16 distinct 4-bank slots, which is
//   conflict-free for ds_read_b128's 16-lane groups.
//
// Forward epilogue: maxout in fp32 on the accumulators; LayerNorm row sums
// by a halving butterfly (lanes swap half of their 16 row values per step:
// 16 shuffles per quantity instead of 80), partials combined through LDS,
// mu / rstd computed once per row.  The dropmask tile is staged into the
// (now free) B region with 16-byte loads; the residual comes from the
// staged X image; Y overwrites the X image, Mout the mask tile, `which`
// its own tile, and all three leave with 16-byte row-contiguous stores.
//
// The training backward is mwe_bwd_fused_kernel: stage 1 (dropmask x
// LayerNorm backward x maxout scatter) computed per tile straight into the
// dX GEMM's A image, so the [T, 3W] dPre is written once (for the dW GEMM)
// and never read back; column sums without atomics.  See its own comment.
// mwe_bwd_stage1_kernel and mwe_bwd_dx_kernel stay as the two-kernel form
// (tests, tools/kbench.py).
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0 and scratch 0 in all of them):
//   mwe_layer_fwd_kernel<96>   147 VGPR  LDS  77,216 B  2 workgroups (12 waves) / CU
//   mwe_layer_fwd_kernel<128>  149 VGPR  LDS 101,920 B  1 workgroup  ( 8 waves) / CU
//   mwe_bwd_dx_kernel<96>      118 VGPR  LDS 116,896 B  1 workgroup  ( 6 waves) / CU
//   mwe_bwd_dx_kernel<128>     126 VGPR  LDS 155,168 B  1 workgroup  ( 8 waves) / CU
//   mwe_bwd_fused_kernel<96>   189 VGPR  LDS 116,896 B  1 workgroup  ( 6 waves) / CU
//   mwe_bwd_fused_kernel<96, COMPACT>  204 VGPR, same LDS and occupancy
//   mwe_bwd_fused_kernel<128>  164 VGPR  LDS 155,168 B  1 workgroup  ( 8 waves) / CU
// Measured at T=1M, W=96 (MI355X): forward 1.32 -> 0.54 ms, dX 0.77
// (GEMM + seq2col_bwd) -> 0.47 ms, stage 1 + dX 1.02 + 0.48 -> 0.80 ms
// fused; see profiles/README.md.
//
// Saved for the backward: maxout output M, argmax, mu, rstd (backward =
// mwe_bwd_fused + recomputed seq2col + dW GEMM).
#pragma once
#include "srx_common.hip.h"

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short srx_bf16x8;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float srx_f32x16;

// ---------------------------------------------------- shared tile machinery
template <int W_, bool BWD_>
struct MweCfg {
  static constexpr int W = W_;
  static constexpr bool BWD = BWD_;
  static constexpr int NW = W / 32;            // 32-col tile positions
  static constexpr int MT = 128;               // rows per workgroup
  static constexpr int NT = 64 * 2 * NW;       // threads = 4 W
  static constexpr int KA = BWD ? 3 * W : W;   // A row length = K per section
  static constexpr int AP = KA + 8;            // padded A image row (bf16)
  static constexpr int KC = BWD ? 96 : 32;     // K chunk of the B stream
  static constexpr int BP = KC + 8;            // padded B chunk row (bf16)
  static constexpr int NBR = BWD ? W : 3 * W;  // B rows per chunk
  static constexpr int LDB = 3 * W;            // B row stride in memory
  static constexpr int NP = BWD ? 1 : 3;       // accumulator tiles per wave / 2
  static constexpr int CPS = KA / KC;          // chunks per section
  static constexpr int NC = 3 * CPS;
  static constexpr int PF = NBR * (KC / 8) / NT;  // 16-byte pieces per thread
  static constexpr int A_ROWS = MT + 2;
  static constexpr int A_ELEMS = A_ROWS * AP;
  static constexpr int B_ELEMS = 2 * NBR * BP;
  static constexpr int A_ITERS = (A_ROWS * (KA / 8) + NT - 1) / NT;
  static_assert(KA % KC == 0, "K chunking");
  static_assert(PF * NT == NBR * (KC / 8), "B chunk must split evenly");
};

// global -> registers: this thread's pieces of B chunk c
template <class C>
__device__ __forceinline__ void mwe_b_fetch(const bf16_t* __restrict__ Bm, int c,
                                            int tid, srx_u32x4_t (&pf)[C::PF]) {
  const int s = c / C::CPS, kc = c % C::CPS;
  const int rowbase = C::BWD ? s * C::W : 0;
  const int coloff = (C::BWD ? 0 : s * C::W) + kc * C::KC;
#pragma unroll
  for (int i = 0; i < C::PF; i++) {
    const int id = i * C::NT + tid;
    const int j = id / (C::KC / 8), q = id % (C::KC / 8);
    pf[i] = *(const srx_u32x4_t*)(Bm + (long)(rowbase + j) * C::LDB +
                                  coloff + q * 8);
  }
}

template <class C>
__device__ __forceinline__ void mwe_b_store(bf16_t* ldsBbuf, int tid,
                                            const srx_u32x4_t (&pf)[C::PF]) {
#pragma unroll
  for (int i = 0; i < C::PF; i++) {
    const int id = i * C::NT + tid;
    const int j = id / (C::KC / 8), q = id % (C::KC / 8);
    *(srx_u32x4_t*)(ldsBbuf + j * C::BP + q * 8) = pf[i];
  }
}

// The tile GEMM, in four separable steps (mwe_tile_gemm below runs them in
// order; mwe_bwd_fused_kernel builds the A image itself):
//   acc[p][mi] = sum over the 3 sections of mask_s(row) * A[row + shift_s]
// times B_s, for this wave's rows [64 mh + 32 mi, +32) and B rows
// 32 (p NW + w) + [0, 32).  A is [T, KA]; image row i holds A[t0 - 1 + i]
// (zero outside [0, T)).  Section s of the forward multiplies A[t - 1 + s]
// by Bm[:, sW + k] and is dropped for s=0 at a doc start / t=0 and for s=2
// at a doc end / t=T-1; section s of the backward multiplies A[t + 1 - s]
// by Bm[sW + n, k] and is dropped for s=0 when t+1 starts a doc / is T and
// for s=2 when t-1 ends a doc / t=0 (the masks of seq2col_bwd_kernel).

// A halo image from global memory: all loads first, then all LDS writes
template <class C>
__device__ __forceinline__ void mwe_stage_a(const bf16_t* __restrict__ A, long T,
                                            long t0, int tid, bf16_t* ldsA) {
  srx_u32x4_t v[C::A_ITERS];
#pragma unroll
  for (int it = 0; it < C::A_ITERS; it++) {
    const int id = it * C::NT + tid;
    const int i = id / (C::KA / 8), q = id % (C::KA / 8);
    const long t = t0 - 1 + i;
    v[it] = srx_u32x4_t{0u, 0u, 0u, 0u};
    if (i < C::A_ROWS && t >= 0 && t < T)
      v[it] = *(const srx_u32x4_t*)(A + t * C::KA + q * 8);
  }
#pragma unroll
  for (int it = 0; it < C::A_ITERS; it++) {
    const int id = it * C::NT + tid;
    const int i = id / (C::KA / 8), q = id % (C::KA / 8);
    if (i < C::A_ROWS) *(srx_u32x4_t*)(ldsA + i * C::AP + q * 8) = v[it];
  }
}

// per-lane section masks of its two A rows: bit s set = section s is zero
template <class C>
__device__ __forceinline__ void mwe_section_masks(
    const uint8_t* __restrict__ is_start, const uint8_t* __restrict__ is_end,
    long T, long t0, int mh, int lane, int (&zmask)[2]) {
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
    const long t = t0 + 64 * mh + 32 * mi + (lane & 31);
    int z = 7;
    if (t < T) {
      bool z0, z2;
      if (C::BWD) {
        z0 = (t + 1 >= T) || is_start[t + 1];
        z2 = (t == 0) || is_end[t - 1];
      } else {
        z0 = (t == 0) || is_start[t];
        z2 = (t == T - 1) || is_end[t];
      }
      z = (z0 ? 1 : 0) | (z2 ? 4 : 0);
    }
    zmask[mi] = z;
  }
}

// The MFMAs of one B chunk.  `abase` / `bbase` are this lane's fragment
// addresses at k = 0 of the chunk; the A rows have pitch APITCH.  zr0 / zr1
// zero the lane's two A rows (a dropped section).
template <class C, int APITCH>
__device__ __forceinline__ void mwe_chunk_mfma(const bf16_t* abase,
                                               const bf16_t* bbase, bool zr0,
                                               bool zr1,
                                               srx_f32x16 (&acc)[C::NP][2]) {
#pragma unroll
  for (int ks = 0; ks < C::KC / 16; ks++) {
    // A fragment (32x32x16 bf16): lane holds A[row (lane&31)]
    // [k + 8*(lane>>5) + e], e=0..7 — one ds_read_b128
    srx_bf16x8 afrag[2];
    afrag[0] = *(const srx_bf16x8*)(abase + ks * 16);
    afrag[1] = *(const srx_bf16x8*)(abase + 32 * APITCH + ks * 16);
    const srx_bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    if (zr0) afrag[0] = zero;
    if (zr1) afrag[1] = zero;
#pragma unroll
    for (int p = 0; p < C::NP; p++) {
      srx_bf16x8 bfrag =
          *(const srx_bf16x8*)(bbase + p * (32 * C::NW) * C::BP + ks * 16);
#pragma unroll
      for (int mi = 0; mi < 2; mi++)
        acc[p][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            afrag[mi], bfrag, acc[p][mi], 0, 0, 0);
    }
  }
}

// The K-chunk loop.  On entry the A image and B chunk 0 (buffer 0) are in
// LDS and a barrier has been passed; `pf` is scratch for the B prefetch.
// Ends with a barrier: both LDS regions are free afterwards.
template <class C>
__device__ __forceinline__ void mwe_chunk_loop(
    const bf16_t* __restrict__ Bm, const bf16_t* ldsA, bf16_t* ldsB,
    const int (&zmask)[2], srx_u32x4_t (&pf)[C::PF],
    srx_f32x16 (&acc)[C::NP][2]) {
  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / C::NW, w = wave % C::NW;

#pragma unroll
  for (int p = 0; p < C::NP; p++)
#pragma unroll
    for (int mi = 0; mi < 2; mi++)
#pragma unroll
      for (int rr = 0; rr < 16; rr++) acc[p][mi][rr] = 0.f;

  for (int c = 0; c < C::NC; c++) {
    if (c + 1 < C::NC) mwe_b_fetch<C>(Bm, c + 1, tid, pf);
    const int s = c / C::CPS, kc = c % C::CPS;
    const bf16_t* bbuf = ldsB + (c & 1) * (C::NBR * C::BP);
    const int arow = 64 * mh + (lane & 31) + (C::BWD ? 2 - s : s);
    const bf16_t* abase = ldsA + arow * C::AP + kc * C::KC + 8 * (lane >> 5);
    const bf16_t* bbase = bbuf + (32 * w + (lane & 31)) * C::BP + 8 * (lane >> 5);
    const bool zr0 = (zmask[0] >> s) & 1, zr1 = (zmask[1] >> s) & 1;
    mwe_chunk_mfma<C, C::AP>(abase, bbase, zr0, zr1, acc);
    if (c + 1 < C::NC)
      mwe_b_store<C>(ldsB + ((c + 1) & 1) * (C::NBR * C::BP), tid, pf);
    __syncthreads();
  }
}

// A from global memory: B chunk 0 prefetch, A image, masks, chunk loop.
template <class C>
__device__ __forceinline__ void mwe_tile_gemm(
    const bf16_t* __restrict__ A, const bf16_t* __restrict__ Bm,
    const uint8_t* __restrict__ is_start, const uint8_t* __restrict__ is_end,
    long T, long t0, bf16_t* ldsA, bf16_t* ldsB,
    srx_f32x16 (&acc)[C::NP][2]) {
  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int mh = (tid / SRX_WAVE) / C::NW;

  srx_u32x4_t pf[C::PF];
  mwe_b_fetch<C>(Bm, 0, tid, pf);
  mwe_stage_a<C>(A, T, t0, tid, ldsA);
  int zmask[2];
  mwe_section_masks<C>(is_start, is_end, T, t0, mh, lane, zmask);
  mwe_b_store<C>(ldsB, tid, pf);
  __syncthreads();
  mwe_chunk_loop<C>(Bm, ldsA, ldsB, zmask, pf, acc);
}

// One halving step of the row-sum butterfly: the lane keeps the half of
// its N values selected by bit `BIT` of its id, sends the other half to
// lane ^ (1 << BIT) and adds what it receives.  After steps 16, 8, 4, 2 on
// bits 0..3, v[0] is the sum over 16 lanes of the value with index
// 8 b0 + 4 b1 + 2 b2 + b3 (b_i = bit i of the lane id).
template <int N, int BIT>
__device__ __forceinline__ void mwe_fold(float (&v)[16], int lane) {
  const bool hi = (lane >> BIT) & 1;
#pragma unroll
  for (int i = 0; i < N / 2; i++) {
    const float keep = hi ? v[i + N / 2] : v[i];
    const float send = hi ? v[i] : v[i + N / 2];
    v[i] = keep + __shfl_xor(send, 1 << BIT, SRX_WAVE);
  }
}

__device__ __forceinline__ float mwe_row_sums(float (&v)[16], int lane) {
  mwe_fold<16, 0>(v, lane);
  mwe_fold<8, 1>(v, lane);
  mwe_fold<4, 2>(v, lane);
  mwe_fold<2, 3>(v, lane);
  return v[0] + __shfl_xor(v[0], 16, SRX_WAVE);
}

// -------------------------------------------------------------- forward
// The forward epilogue of a 128-row tile, from the wave's accumulators
// acc[piece][m-tile] (see the file comment).  All LDS tiles must be free on
// entry (a barrier passed): ldsY [MT][W+8] receives Y — with RESID it holds
// the residual on entry —, ldsM [MT][W+8] the mask and then Mout, ldsWh
// [MT][W+16] bytes `which`; ldsP [2][NW][MT] and ldsS [2][MT] are fp32.
template <int W, bool RESID>
__device__ __forceinline__ void mwe_fwd_epilogue(
    srx_f32x16 (&acc)[3][2], const bf16_t* __restrict__ bias,
    const bf16_t* __restrict__ g, const bf16_t* __restrict__ b,
    const bf16_t* __restrict__ dropmask, bf16_t* ldsY, bf16_t* ldsM,
    uint8_t* ldsWh, float* ldsP, float* ldsS, bf16_t* __restrict__ Y,
    bf16_t* __restrict__ Mout, uint8_t* __restrict__ which,
    float* __restrict__ mu_out, float* __restrict__ rstd_out, long T, long t0,
    float eps) {
  constexpr int WP = W + 8, NW = W / 32, MT = 128, NT = 4 * W;
  constexpr int WHP = W + 16;
  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;

  // dropmask tile -> LDS (16-byte loads)
  if (dropmask) {
    for (int id = tid; id < MT * (W / 8); id += NT) {
      const int r = id / (W / 8), q = id % (W / 8);
      if (t0 + r < T)
        *(srx_u32x4_t*)(ldsM + r * WP + q * 8) =
            *(const srx_u32x4_t*)(dropmask + (t0 + r) * W + q * 8);
    }
  }

  // +bias, maxout over pieces (fp32, first index wins ties)
  const int col = 32 * w + (lane & 31);  // within-piece column
  float bias_p[3];
#pragma unroll
  for (int p = 0; p < 3; p++) bias_p[p] = bf2f(bias[p * W + col]);
  const float gv = bf2f(g[col]), bv = bf2f(b[col]);

  float mx[2][16];
  uint8_t arg[2][16];
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      float best = acc[0][mi][rr] + bias_p[0];
      uint8_t bp = 0;
#pragma unroll
      for (int p = 1; p < 3; p++) {
        float v = acc[p][mi][rr] + bias_p[p];
        if (v > best) { best = v; bp = (uint8_t)p; }
      }
      mx[mi][rr] = best;
      arg[mi][rr] = bp;
    }
  }

  // LayerNorm row partials over this wave's 32 columns
  const int b0 = lane & 1, b1 = (lane >> 1) & 1, b2 = (lane >> 2) & 1,
            b3 = (lane >> 3) & 1;
  const int rsel = 8 * b0 + 4 * b1 + 2 * b2 + b3;  // row index this lane ends with
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
    float v1[16], v2[16];
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      v1[rr] = mx[mi][rr];
      v2[rr] = mx[mi][rr] * mx[mi][rr];
    }
    const float s1 = mwe_row_sums(v1, lane);
    const float s2 = mwe_row_sums(v2, lane);
    if (((lane >> 4) & 1) == 0) {
      const int r = 64 * mh + 32 * mi + (rsel & 3) + 8 * (rsel >> 2) + 4 * (lane >> 5);
      ldsP[w * MT + r] = s1;
      ldsP[(NW + w) * MT + r] = s2;
    }
  }
  __syncthreads();
  if (tid < MT) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < NW; w2++) {
      s1 += ldsP[w2 * MT + tid];
      s2 += ldsP[(NW + w2) * MT + tid];
    }
    const float mu = s1 / W;
    const float var = s2 / W - mu * mu;
    const float rstd = rsqrtf(fmaxf(var, 0.f) + eps);
    ldsS[tid] = mu;
    ldsS[MT + tid] = rstd;
    if (t0 + tid < T) {
      mu_out[t0 + tid] = mu;
      rstd_out[t0 + tid] = rstd;
    }
  }
  __syncthreads();

  // normalise, mask, residual from the Y tile; results stay in LDS
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 64 * mh + 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      const float mu = ldsS[r], rstd = ldsS[MT + r];
      const float v = mx[mi][rr];
      float y = (v - mu) * rstd * gv + bv;
      if (dropmask) y *= bf2f(ldsM[r * WP + col]);
      if (RESID) y += bf2f(ldsY[r * WP + col]);
      ldsY[r * WP + col] = f2bf(y);
      ldsM[r * WP + col] = f2bf(v);
      ldsWh[r * WHP + col] = arg[mi][rr];
    }
  }
  __syncthreads();

  // 16-byte row-contiguous stores
  for (int id = tid; id < MT * (W / 8); id += NT) {
    const int r = id / (W / 8), q = id % (W / 8);
    if (t0 + r < T) {
      *(srx_u32x4_t*)(Y + (t0 + r) * W + q * 8) =
          *(const srx_u32x4_t*)(ldsY + r * WP + q * 8);
      *(srx_u32x4_t*)(Mout + (t0 + r) * W + q * 8) =
          *(const srx_u32x4_t*)(ldsM + r * WP + q * 8);
    }
  }
  for (int id = tid; id < MT * (W / 16); id += NT) {
    const int r = id / (W / 16), q = id % (W / 16);
    if (t0 + r < T)
      *(srx_u32x4_t*)(which + (t0 + r) * W + q * 16) =
          *(const srx_u32x4_t*)(ldsWh + r * WHP + q * 16);
  }
}

template <int W>
__global__ __launch_bounds__(4 * W) void mwe_layer_fwd_kernel(
    const bf16_t* __restrict__ X,      // [T, W]
    const bf16_t* __restrict__ Wt,     // [3W (out, pieces-major), 3W (in)] row-major
    const bf16_t* __restrict__ bias,   // [3W]
    const bf16_t* __restrict__ g,      // [W]
    const bf16_t* __restrict__ b,      // [W]
    const uint8_t* __restrict__ is_start,
    const uint8_t* __restrict__ is_end,
    const bf16_t* __restrict__ dropmask,  // [T, W] 0 or 1/keep, or nullptr
    bf16_t* __restrict__ Y,            // [T, W]
    bf16_t* __restrict__ Mout,         // [T, W] maxout output (for bwd)
    uint8_t* __restrict__ which,       // [T, W]
    float* __restrict__ mu_out,        // [T]
    float* __restrict__ rstd_out,      // [T]
    long T, float eps) {
  using C = MweCfg<W, false>;
  constexpr int WP = C::AP, NW = C::NW, MT = C::MT;
  constexpr int WHP = W + 16;  // `which` tile row stride (bytes)
  static_assert(MT * WP * 2 + MT * WHP <= C::B_ELEMS * 2, "epilogue tiles");
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;                               // X halo image, then Y
  bf16_t* ldsB = lds + C::A_ELEMS;                  // B chunks x2
  bf16_t* ldsM = ldsB;                              // epilogue: mask, then Mout
  uint8_t* ldsWh = (uint8_t*)(ldsB + MT * WP);      // epilogue: which
  float* ldsP = (float*)(ldsB + C::B_ELEMS);        // LN partials [2][NW][MT]
  float* ldsS = ldsP + 2 * NW * MT;                 // mu, rstd [2][MT]
  const long t0 = (long)blockIdx.x * MT;

  srx_f32x16 acc[3][2];  // [piece][m-tile]
  mwe_tile_gemm<C>(X, Wt, is_start, is_end, T, t0, ldsA, ldsB, acc);

  // Y tile = the X image's own rows: the residual is read from it
  mwe_fwd_epilogue<W, true>(acc, bias, g, b, dropmask, ldsA + WP, ldsM, ldsWh,
                            ldsP, ldsS, Y, Mout, which, mu_out, rstd_out, T, t0,
                            eps);
}

// ---------------------------------------------------------- backward dX
// dX = dY + seq2col_bwd(dPre @ weight) without materialising the [T, 3W]
// product: fp32 accumulation over all three sections, one rounding.
// WT is the launcher's transposed copy of the weight ([3W in, 3W out]),
// so that section s's B rows n = WT[sW + n, :] are k-contiguous.
template <int W>
__global__ __launch_bounds__(4 * W) void mwe_bwd_dx_kernel(
    const bf16_t* __restrict__ dPre,   // [T, 3W]
    const bf16_t* __restrict__ WT,     // [3W, 3W] = weight^T, row-major
    const uint8_t* __restrict__ is_start,
    const uint8_t* __restrict__ is_end,
    const bf16_t* __restrict__ dY,     // [T, W]
    bf16_t* __restrict__ dX,           // [T, W]
    long T) {
  using C = MweCfg<W, true>;
  constexpr int NW = C::NW, MT = C::MT, NT = C::NT;
  constexpr int OP = W + 4;  // fp32 output tile row stride
  static_assert(MT * OP * 4 <= C::A_ELEMS * 2, "output tile");
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;
  bf16_t* ldsB = lds + C::A_ELEMS;
  float* ldsO = (float*)lds;  // epilogue: fp32 [MT][OP] over the A image

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;
  const long t0 = (long)blockIdx.x * MT;

  srx_f32x16 acc[1][2];
  mwe_tile_gemm<C>(dPre, WT, is_start, is_end, T, t0, ldsA, ldsB, acc);

  const int col = 32 * w + (lane & 31);
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 64 * mh + 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      ldsO[r * OP + col] = acc[0][mi][rr];
    }
  __syncthreads();
  for (int id = tid; id < MT * (W / 8); id += NT) {
    const int r = id / (W / 8), q = id % (W / 8);
    if (t0 + r < T) {
      float v[8], d[8];
      ElemV<bf16_t, 8>::ld(dY + (t0 + r) * W + q * 8, d);
      const float4 lo = *(const float4*)(ldsO + r * OP + q * 8);
      const float4 hi = *(const float4*)(ldsO + r * OP + q * 8 + 4);
      v[0] = lo.x + d[0]; v[1] = lo.y + d[1]; v[2] = lo.z + d[2]; v[3] = lo.w + d[3];
      v[4] = hi.x + d[4]; v[5] = hi.y + d[5]; v[6] = hi.z + d[6]; v[7] = hi.w + d[7];
      ElemV<bf16_t, 8>::st(dX + (t0 + r) * W + q * 8, v);
    }
  }
}

// ------------------------------------------- fused MWE backward stage 1
// One kernel for: dL = dY * dropmask; LayerNorm backward over the saved
// maxout output (Mout, mu, rstd); maxout scatter into the pieces-major
// [T, 3W] pre-activation gradient; the 3W bias column-sum; and the LN
// dg/db column sums — replacing 3 kernels + 2 reduce passes per encoder
// block per step.  Structure follows layernorm_bwd_kernel (one wave per
// row, per-wave register accumulation for the column sums, one atomic per
// column per wave; DET => int64 fixed-point).  W <= 256.
template <typename T, bool DET = false>
__global__ void mwe_bwd_stage1_kernel(
    const T* __restrict__ dY, const T* __restrict__ dropmask,  // mask may be null
    const T* __restrict__ Mout, const T* __restrict__ g,
    const float* __restrict__ mu, const float* __restrict__ rstd,
    const uint8_t* __restrict__ which, T* __restrict__ dPre,
    void* __restrict__ dg32, void* __restrict__ db32,
    void* __restrict__ dbias32, long N, int W) {
  const int lane = threadIdx.x & (SRX_WAVE - 1);
  const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) / SRX_WAVE;
  const long nwaves = ((long)gridDim.x * blockDim.x) / SRX_WAVE;
  const int ncols = (W + SRX_WAVE - 1) / SRX_WAVE;
  float dg_loc[4], db_loc[4], dbias_loc[4 * 3];
  for (int c = 0; c < ncols; c++) { dg_loc[c] = 0.f; db_loc[c] = 0.f; }
  for (int k = 0; k < ncols * 3; k++) dbias_loc[k] = 0.f;
  for (long n = wave; n < N; n += nwaves) {
    const T* dyrow = dY + n * (long)W;
    const T* mrow = Mout + n * (long)W;
    const T* maskrow = dropmask ? dropmask + n * (long)W : nullptr;
    float m = mu[n], r = rstd[n];
    float s1 = 0.f, s2 = 0.f;
    float dl[4], xh[4];
    for (int c = 0; c < ncols; c++) {
      int w = lane + c * SRX_WAVE;
      if (w >= W) { dl[c] = 0.f; xh[c] = 0.f; continue; }
      float d = Elem<T>::ld(dyrow + w);
      if (maskrow) d *= Elem<T>::ld(maskrow + w);
      float xhat = (Elem<T>::ld(mrow + w) - m) * r;
      float dxhat = d * Elem<T>::ld(g + w);
      dl[c] = d;
      xh[c] = xhat;
      s1 += dxhat;
      s2 += dxhat * xhat;
      dg_loc[c] += d * xhat;
      db_loc[c] += d;
    }
    s1 = wave_reduce_sum(s1) / W;
    s2 = wave_reduce_sum(s2) / W;
    T* out = dPre + n * (long)(3 * W);
    const uint8_t* wrow = which + n * (long)W;
    for (int c = 0; c < ncols; c++) {
      int w = lane + c * SRX_WAVE;
      if (w >= W) continue;
      float dxhat = dl[c] * Elem<T>::ld(g + w);
      float dM = r * (dxhat - s1 - xh[c] * s2);
      int p = wrow[w];
      for (int q = 0; q < 3; q++)
        Elem<T>::st(out + q * W + w, q == p ? dM : 0.f);
      dbias_loc[c * 3 + p] += dM;
    }
  }
  for (int c = 0; c < ncols; c++) {
    int w = lane + c * SRX_WAVE;
    if (w >= W) continue;
    if (dg_loc[c] != 0.f) srx_atomic_add<DET>(dg32, w, dg_loc[c]);
    if (db_loc[c] != 0.f) srx_atomic_add<DET>(db32, w, db_loc[c]);
    for (int q = 0; q < 3; q++)
      if (dbias_loc[c * 3 + q] != 0.f)
        srx_atomic_add<DET>(dbias32, (long)q * W + w, dbias_loc[c * 3 + q]);
  }
}

// ------------------------------- fused MWE backward: stage 1 + dX, one pass
// mwe_bwd_stage1_kernel and mwe_bwd_dx_kernel in one launch: the stage-1
// result of a 128-row tile (plus its two halo rows, recomputed per tile) is
// written straight into the dX GEMM's LDS A image instead of making the
// round trip through the [T, 3W] dPre tensor in HBM.  dPre still leaves
// once (the dW GEMM reads it), with 16-byte row-contiguous stores from the
// image.
//
// Prologue mapping: 16 lanes per row, 8 columns per lane (lanes 12..15 idle
// at W = 96), NT / 16 rows per pass; every global load is 16 bytes (`which`:
// 8) and all passes' loads are issued before the first is used.  The LN row
// sums are four xor-shuffles.  The fp32 arithmetic is that of
// mwe_bwd_stage1_kernel; only the order of the row sums differs.
//
// Column sums: a thread owns the same 8 columns in every pass, so dg / db /
// dbias accumulate in 40 registers over the tile's own rows < T (never the
// halo), are folded over the wave's four row groups by shuffles, over the
// waves through the free B region, and leave as one fp32 row [5W] =
// dg | db | dbias per workgroup.  mwe_colsum_kernel adds those rows in a
// fixed order: no atomics, bit-reproducible in every mode.

// The stage-1 prologue (shared with the mixer backward, srx_mixer.hip.h):
// image row i = stage 1 of row t0 - HALO + i (zero outside [0, T)), rows of
// pitch AP, for i < 128 + 2 HALO.  The column sums of the tile's own rows
// are returned in dg_out / db_out / dbias_out for mwe_colsums_park.  (They
// accumulate in locals and are copied out at the end: accumulating through
// the references keeps the arrays out of registers — 256 VGPRs and scratch.)
// With COMPACT the tile's own rows of dM (the value scattered above, before
// the piece expansion) also leave for memory as [T, W], straight from the
// registers: the input of mwe_bwd_dw_kernel (srx_mwe_dw.hip.h).
template <int W, int NT, int AP, int HALO, bool COMPACT = false>
__device__ __forceinline__ void mwe_stage1_tile(
    const bf16_t* __restrict__ dY, const bf16_t* __restrict__ dropmask,
    const bf16_t* __restrict__ Mout, const bf16_t* __restrict__ g,
    const float* __restrict__ mu, const float* __restrict__ rstd,
    const uint8_t* __restrict__ which, long T, long t0, int tid, bf16_t* ldsA,
    float (&dg_out)[8], float (&db_out)[8], float (&dbias_out)[3][8],
    bf16_t* __restrict__ dMout = nullptr) {
  constexpr int MT = 128, A_ROWS = MT + 2 * HALO;
  constexpr int Q = W / 8;                        // 16-byte groups per row
  constexpr int RG = NT / 16;                     // rows per prologue pass
  constexpr int NPASS = (A_ROWS + RG - 1) / RG;
  const int q = tid & 15, rg = tid >> 4;
  const bool qv = q < Q;
  float gv[8];
#pragma unroll
  for (int j = 0; j < 8; j++) gv[j] = 0.f;
  if (qv) ElemV<bf16_t, 8>::ld(g + q * 8, gv);

  srx_u32x4_t rdy[NPASS], rmk[NPASS], rmo[NPASS];
  uint2 rwh[NPASS];
  float rmu[NPASS], rrs[NPASS];
#pragma unroll
  for (int ps = 0; ps < NPASS; ps++) {
    const int i = ps * RG + rg;
    const long t = t0 - HALO + i;
    rdy[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
    rmk[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
    rmo[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
    rwh[ps] = make_uint2(0u, 0u);
    rmu[ps] = 0.f;
    rrs[ps] = 0.f;
    if (qv && i < A_ROWS && t >= 0 && t < T) {
      rdy[ps] = *(const srx_u32x4_t*)(dY + t * W + q * 8);
      if (dropmask) rmk[ps] = *(const srx_u32x4_t*)(dropmask + t * W + q * 8);
      rmo[ps] = *(const srx_u32x4_t*)(Mout + t * W + q * 8);
      rwh[ps] = *(const uint2*)(which + t * W + q * 8);
      rmu[ps] = mu[t];
      rrs[ps] = rstd[t];
    }
  }

  float dg_loc[8], db_loc[8], dbias_loc[3][8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dg_loc[j] = 0.f;
    db_loc[j] = 0.f;
    dbias_loc[0][j] = dbias_loc[1][j] = dbias_loc[2][j] = 0.f;
  }

#pragma unroll
  for (int ps = 0; ps < NPASS; ps++) {
    const int i = ps * RG + rg;
    const long t = t0 - HALO + i;
    const bool live = qv && i < A_ROWS && t >= 0 && t < T;
    const bool own = live && i >= HALO && i < MT + HALO;
    const float m = rmu[ps], r = rrs[ps];
    float d[8], xh[8], dxh[8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int sh = 16 * (j & 1);
      d[j] = bf2f((bf16_t)((rdy[ps][j >> 1] >> sh) & 0xffffu));
      if (dropmask) d[j] *= bf2f((bf16_t)((rmk[ps][j >> 1] >> sh) & 0xffffu));
      xh[j] = (bf2f((bf16_t)((rmo[ps][j >> 1] >> sh) & 0xffffu)) - m) * r;
      dxh[j] = d[j] * gv[j];
      s1 += dxh[j];
      s2 += dxh[j] * xh[j];
    }
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      s1 += __shfl_xor(s1, off, SRX_WAVE);
      s2 += __shfl_xor(s2, off, SRX_WAVE);
    }
    s1 = s1 / W;
    s2 = s2 / W;
    uint32_t hb[8], wh[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float dM = r * (dxh[j] - s1 - xh[j] * s2);
      wh[j] = ((j < 4 ? rwh[ps].x : rwh[ps].y) >> (8 * (j & 3))) & 0xffu;
      hb[j] = live ? (uint32_t)f2bf(dM) : 0u;
      if (own) {
        dg_loc[j] = fmaf(d[j], xh[j], dg_loc[j]);
        db_loc[j] += d[j];
#pragma unroll
        for (int p = 0; p < 3; p++) dbias_loc[p][j] += (wh[j] == (uint32_t)p) ? dM : 0.f;
      }
    }
    if (COMPACT && own) {
      srx_u32x4_t o;
#pragma unroll
      for (int k = 0; k < 4; k++) o[k] = hb[2 * k] | (hb[2 * k + 1] << 16);
      *(srx_u32x4_t*)(dMout + t * W + q * 8) = o;
    }
    // expanded row: dM at piece `which`, exact zero in the other two
    if (qv && i < A_ROWS) {
#pragma unroll
      for (int p = 0; p < 3; p++) {
        srx_u32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; k++)
          o[k] = (wh[2 * k] == (uint32_t)p ? hb[2 * k] : 0u) |
                 ((wh[2 * k + 1] == (uint32_t)p ? hb[2 * k + 1] : 0u) << 16);
        *(srx_u32x4_t*)(ldsA + i * AP + p * W + q * 8) = o;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dg_out[j] = dg_loc[j];
    db_out[j] = db_loc[j];
#pragma unroll
    for (int p = 0; p < 3; p++) dbias_out[p][j] = dbias_loc[p][j];
  }
}

// Column sums of mwe_stage1_tile: fold the wave's 4 row groups and park one
// row [5W] = dg | db | dbias per wave in ldsC ...
template <int W>
__device__ __forceinline__ void mwe_colsums_park(float (&dg_loc)[8],
                                                 float (&db_loc)[8],
                                                 float (&dbias_loc)[3][8],
                                                 float* ldsC, int tid) {
  const int lane = tid % SRX_WAVE, wave = tid / SRX_WAVE;
  const int q = tid & 15;
  const bool qv = q < W / 8;
#pragma unroll
  for (int j = 0; j < 8; j++) {
#pragma unroll
    for (int off = 16; off < SRX_WAVE; off <<= 1) {
      dg_loc[j] += __shfl_xor(dg_loc[j], off, SRX_WAVE);
      db_loc[j] += __shfl_xor(db_loc[j], off, SRX_WAVE);
#pragma unroll
      for (int p = 0; p < 3; p++)
        dbias_loc[p][j] += __shfl_xor(dbias_loc[p][j], off, SRX_WAVE);
    }
  }
  if (lane < 16 && qv) {
    float* row = ldsC + wave * (5 * W) + q * 8;
    ElemV<float, 4>::st(row, dg_loc);
    ElemV<float, 4>::st(row + 4, dg_loc + 4);
    ElemV<float, 4>::st(row + W, db_loc);
    ElemV<float, 4>::st(row + W + 4, db_loc + 4);
#pragma unroll
    for (int p = 0; p < 3; p++) {
      ElemV<float, 4>::st(row + (2 + p) * W, dbias_loc[p]);
      ElemV<float, 4>::st(row + (2 + p) * W + 4, dbias_loc[p] + 4);
    }
  }
}

// ... and, after a barrier, add the waves' rows in order into the tile's row
template <int W, int NT>
__device__ __forceinline__ void mwe_colsums_out(const float* ldsC,
                                                float* __restrict__ out, int tid) {
  for (int c = tid; c < 5 * W; c += NT) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < NT / SRX_WAVE; wv++) s += ldsC[wv * (5 * W) + c];
    out[c] = s;
  }
}

template <int W, bool COMPACT = false>
__global__ __launch_bounds__(4 * W) void mwe_bwd_fused_kernel(
    const bf16_t* __restrict__ dY,        // [T, W]
    const bf16_t* __restrict__ dropmask,  // [T, W] or nullptr
    const bf16_t* __restrict__ Mout,      // [T, W]
    const bf16_t* __restrict__ g,         // [W]
    const float* __restrict__ mu,         // [T]
    const float* __restrict__ rstd,       // [T]
    const uint8_t* __restrict__ which,    // [T, W]
    const bf16_t* __restrict__ WT,        // [3W, 3W] = weight^T, row-major
    const uint8_t* __restrict__ is_start,
    const uint8_t* __restrict__ is_end,
    bf16_t* __restrict__ dPre,            // [T, 3W]; COMPACT: dM [T, W]
    bf16_t* __restrict__ dX,              // [T, W]
    float* __restrict__ partials,         // [gridDim.x, 5W]
    long T) {
  using C = MweCfg<W, true>;
  constexpr int NW = C::NW, MT = C::MT, NT = C::NT, AP = C::AP;
  constexpr int Q = W / 8;                        // 16-byte groups per row
  constexpr int NWAVE = NT / SRX_WAVE;
  constexpr int OP = W + 4;  // fp32 output tile row stride
  static_assert(MT * OP * 4 <= C::A_ELEMS * 2, "output tile");
  static_assert(NWAVE * 5 * W * 4 <= C::B_ELEMS * 2, "column-sum partials");
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;
  bf16_t* ldsB = lds + C::A_ELEMS;
  float* ldsO = (float*)lds;   // epilogue: fp32 [MT][OP] over the A image
  float* ldsC = (float*)ldsB;  // epilogue: column sums [NWAVE][5W] over B

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mh = wave / NW, w = wave % NW;
  const long t0 = (long)blockIdx.x * MT;

  srx_u32x4_t pf[C::PF];
  mwe_b_fetch<C>(WT, 0, tid, pf);

  float dg_loc[8], db_loc[8], dbias_loc[3][8];
  mwe_stage1_tile<W, NT, AP, 1, COMPACT>(dY, dropmask, Mout, g, mu, rstd, which,
                                         T, t0, tid, ldsA, dg_loc, db_loc,
                                         dbias_loc, dPre);

  int zmask[2];
  mwe_section_masks<C>(is_start, is_end, T, t0, mh, lane, zmask);
  mwe_b_store<C>(ldsB, tid, pf);
  __syncthreads();

  // ---- dPre out: the tile's own rows, before the epilogue reuses the image
  // (COMPACT: dM has already left from the prologue's registers)
  for (int id = tid; !COMPACT && id < MT * (3 * Q); id += NT) {
    const int r = id / (3 * Q), c = id % (3 * Q);
    if (t0 + r < T)
      *(srx_u32x4_t*)(dPre + (t0 + r) * (3 * W) + c * 8) =
          *(const srx_u32x4_t*)(ldsA + (r + 1) * AP + c * 8);
  }

  srx_f32x16 acc[1][2];
  mwe_chunk_loop<C>(WT, ldsA, ldsB, zmask, pf, acc);

  // ---- column sums, per wave, into the free B region
  mwe_colsums_park<W>(dg_loc, db_loc, dbias_loc, ldsC, tid);

  // ---- dX epilogue (as mwe_bwd_dx_kernel)
  const int col = 32 * w + (lane & 31);
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 64 * mh + 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      ldsO[r * OP + col] = acc[0][mi][rr];
    }
  __syncthreads();
  for (int id = tid; id < MT * Q; id += NT) {
    const int r = id / Q, qq = id % Q;
    if (t0 + r < T) {
      float v[8], d[8];
      ElemV<bf16_t, 8>::ld(dY + (t0 + r) * W + qq * 8, d);
      const float4 lo = *(const float4*)(ldsO + r * OP + qq * 8);
      const float4 hi = *(const float4*)(ldsO + r * OP + qq * 8 + 4);
      v[0] = lo.x + d[0]; v[1] = lo.y + d[1]; v[2] = lo.z + d[2]; v[3] = lo.w + d[3];
      v[4] = hi.x + d[4]; v[5] = hi.y + d[5]; v[6] = hi.z + d[6]; v[7] = hi.w + d[7];
      ElemV<bf16_t, 8>::st(dX + (t0 + r) * W + qq * 8, v);
    }
  }
  mwe_colsums_out<W, NT>(ldsC, partials + (long)blockIdx.x * (5 * W), tid);
}

// out[b, c] = sum over rows [b R, min((b+1) R, n)) of in[:, c], added in row
// order in fp64 and rounded to fp32 once: the fixed-order reduction of the
// per-tile column sums above (applied until one row is left).
__global__ void mwe_colsum_kernel(const float* __restrict__ in,
                                  float* __restrict__ out, long n, int R,
                                  int ncols) {
  const int c = blockIdx.y * blockDim.x + threadIdx.x;
  if (c >= ncols) return;
  const long r0 = (long)blockIdx.x * R;
  const long r1 = r0 + R < n ? r0 + R : n;
  double s = 0.0;
  for (long r = r0; r < r1; r++) s += (double)in[r * ncols + c];
  out[(long)blockIdx.x * ncols + c] = (float)s;
}
