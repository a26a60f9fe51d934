// The fused MaxoutWindowEncoder block at W = 256 (spaCy's accuracy preset):
//   Y = X + mask * LayerNorm(maxout_3(seq2col(X) @ Wt^T + bias))
// and its fused backward, for the width at which the tiles of srx_mwe.hip.h
// no longer fit: MweCfg<256, false> would need 191 KB of LDS and the
// backward's [130][776] dPre image alone 201 KB, against 160 KB.  Semantics,
// arguments and saved tensors are those of mwe_layer_fwd_kernel /
// mwe_bwd_fused_kernel; the B stream, the halo image, the section masks and
// the MFMA chunk loop are the helpers of srx_mwe.hip.h, driven by the two
// configurations below.
//
// Forward (mwe_wide_fwd_kernel): one workgroup owns 64 whole rows, i.e. all
// 768 pre-activations of each, so maxout and LayerNorm never leave registers
// and LDS.  8 waves; wave w holds column position w (32 columns) of all
// three pieces for all 64 rows: acc[3][2] srx_f32x16, the in-register
// three-piece maxout of the narrow kernel.  LDS: the X halo image [66][264]
// bf16 (34,848 B) and the double-buffered 32-deep weight chunk [768][40] x 2
// (122,880 B); every epilogue tile (mask / Mout, which, LayerNorm partials,
// row statistics) lives in the B region once the chunk loop has ended.  12
// MFMAs per wave between barriers, as in the narrow kernel.  T % 64 == 0, so
// a forward tile is never partial.
//
// Backward (mwe_wide_bwd_fused_kernel): a 128-row tile, 8 waves.  Stage 1
// (dropmask x LayerNorm backward) runs with 32 lanes per row and leaves in
// LDS only the compact dM [130][264] bf16 (68,640 B) and one tag byte
// 1 << which per element [130][272] (35,360 B) — not the [rows][3W] image.
// dPre [T, 3W] leaves for memory straight from the stage-1 registers, with
// exact zeros off the argmax piece.  The dX GEMM has K = 3W per section; its
// chunk kc covers piece p = kc / 8, columns 32 (kc % 8) .. + 32, and the A
// fragment of that piece is formed in registers: the lane's 8 dM values
// ANDed with masks made from its 8 tag bytes.  The tag bytes of four
// consecutive elements are stored in the order e0 e2 e1 e3, so that
// `tags << (15 - p)` puts the match bits of e0 / e1 on bits 15 / 31 and
// `tags << (7 - p)` those of e2 / e3; one packed 16-bit arithmetic shift
// right by 15 turns either into the two 16-bit masks of a bf16 pair: 12
// VALU instructions per fragment.  A dropped section (doc boundary) clears
// the tags, so it costs nothing more.  Wave (mq, nh) owns rows [32 mq, + 32)
// and columns [128 nh, + 128): acc[4] srx_f32x16, one A fragment per four
// MFMAs.  The transposed weight streams per section in 32-deep chunks
// [256][40] x 2 (40,960 B).  Epilogue: dX = acc + dY in fp32, one rounding,
// through a bf16 tile over the dM image; dg / db / dbias as fixed-order
// column sums (no atomics), one fp32 row [5W] per tile for mwe_colsum_kernel.
//
// Rows of 264 bf16 (132 dwords) and 40 bf16 (20 dwords) are the +8 pad of
// srx_mwe.hip.h; the tag rows of 272 bytes (68 dwords) put 16 consecutive
// rows of an 8-byte read on 16 distinct 4-bank slots.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0 and scratch 0 in both, LDS is dynamic):
//   mwe_wide_fwd_kernel<256>        159 VGPR  106 SGPR  LDS 157,728 B  1 workgroup (8 waves) / CU
//   mwe_wide_bwd_fused_kernel<256>  162 VGPR   74 SGPR  LDS 144,960 B  1 workgroup (8 waves) / CU
// (the register counts alone would allow 3 waves / SIMD; LDS sets the limit).
// Measured on an MI355X, one block, forward + backward with dW against the
// composed route: 2.18 vs 2.81 ms at T = 256K, 8.82 vs 9.36 ms at T = 1M;
// see profiles/README.md.
#pragma once
#include "srx_mwe.hip.h"

// The members mwe_b_fetch / mwe_b_store / mwe_stage_a / mwe_section_masks /
// mwe_chunk_loop read from a configuration (see MweCfg).
struct MweWideFwdCfg {
  static constexpr int W = 256;
  static constexpr bool BWD = false;
  static constexpr int NW = 8;              // 32-col tile positions = waves
  static constexpr int MT = 64;             // rows per workgroup
  static constexpr int NT = 64 * NW;        // 512 threads
  static constexpr int KA = W;
  static constexpr int AP = KA + 8;
  static constexpr int KC = 32;
  static constexpr int BP = KC + 8;
  static constexpr int NBR = 3 * W;
  static constexpr int LDB = 3 * W;
  static constexpr int NP = 3;
  static constexpr int CPS = KA / KC;
  static constexpr int NC = 3 * CPS;
  static constexpr int PF = NBR * (KC / 8) / NT;  // 6
  static constexpr int A_ROWS = MT + 2;
  static constexpr int A_ELEMS = A_ROWS * AP;
  static constexpr int B_ELEMS = 2 * NBR * BP;
  static constexpr int A_ITERS = (A_ROWS * (KA / 8) + NT - 1) / NT;
  static constexpr int WHP = W + 16;        // `which` tile row stride (bytes)
  // epilogue tiles inside the B region: Mout, which, LN partials, mu / rstd
  static constexpr int EPI_BYTES =
      MT * AP * 2 + MT * WHP + (2 * NW * MT + 2 * MT) * 4;
  static constexpr int LDS_BYTES = (A_ELEMS + B_ELEMS) * 2;
  static_assert(PF * NT == NBR * (KC / 8), "B chunk must split evenly");
  static_assert(EPI_BYTES <= B_ELEMS * 2, "epilogue tiles");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

struct MweWideBwdCfg {
  static constexpr int W = 256;
  static constexpr bool BWD = true;
  static constexpr int MT = 128;            // rows per workgroup
  static constexpr int NT = 512;            // 8 waves: 4 row x 2 column groups
  static constexpr int KA = 3 * W;          // K per section
  static constexpr int AP = W + 8;          // dM image row (bf16)
  static constexpr int TP = W + 16;         // tag image row (bytes)
  static constexpr int KC = 32;
  static constexpr int BP = KC + 8;
  static constexpr int NBR = W;
  static constexpr int LDB = 3 * W;
  static constexpr int CPS = KA / KC;       // 24 = 3 pieces x 8 column chunks
  static constexpr int NC = 3 * CPS;
  static constexpr int PF = NBR * (KC / 8) / NT;  // 2
  static constexpr int A_ROWS = MT + 2;
  static constexpr int A_ELEMS = A_ROWS * AP;
  static constexpr int T_BYTES = A_ROWS * TP;
  static constexpr int B_ELEMS = 2 * NBR * BP;
  static constexpr int LDS_BYTES = A_ELEMS * 2 + T_BYTES + B_ELEMS * 2;
  static_assert(PF * NT == NBR * (KC / 8), "B chunk must split evenly");
  static_assert((A_ELEMS * 2) % 16 == 0 && T_BYTES % 16 == 0, "alignment");
  static_assert(MT * AP * 2 <= A_ELEMS * 2, "dX tile over the dM image");
  static_assert((NT / SRX_WAVE) * 5 * W * 4 <= B_ELEMS * 2, "column sums");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

// ------------------------------------------------------------------ forward
template <int W>
__global__ __launch_bounds__(512) void mwe_wide_fwd_kernel(
    const bf16_t* __restrict__ X,      // [T, W]
    const bf16_t* __restrict__ Wt,     // [3W (out, pieces-major), 3W (in)]
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
  using C = MweWideFwdCfg;
  static_assert(W == C::W, "the wide kernels are W = 256");
  constexpr int WP = C::AP, NW = C::NW, MT = C::MT, NT = C::NT, WHP = C::WHP;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;                           // X halo image, then Y
  bf16_t* ldsB = lds + C::A_ELEMS;              // B chunks x2
  bf16_t* ldsY = ldsA + WP;                     // the image's own rows
  bf16_t* ldsM = ldsB;                          // epilogue: mask, then Mout
  uint8_t* ldsWh = (uint8_t*)(ldsM + MT * WP);  // epilogue: which
  float* ldsP = (float*)(ldsWh + MT * WHP);     // LN partials [2][NW][MT]
  float* ldsS = ldsP + 2 * NW * MT;             // mu, rstd [2][MT]
  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int w = tid / SRX_WAVE;
  const long t0 = (long)blockIdx.x * MT;

  srx_f32x16 acc[3][2];  // [piece][m-tile]
  mwe_tile_gemm<C>(X, Wt, is_start, is_end, T, t0, ldsA, ldsB, acc);

  // dropmask tile -> the free B region (16-byte loads)
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

  // LayerNorm row partials over this wave's 32 columns (mwe_row_sums)
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
      const int r = 32 * mi + (rsel & 3) + 8 * (rsel >> 2) + 4 * (lane >> 5);
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

  // normalise, mask, residual from the X image; results stay in LDS
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 32 * mi + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      const float mu = ldsS[r], rstd = ldsS[MT + r];
      const float v = mx[mi][rr];
      float y = (v - mu) * rstd * gv + bv;
      if (dropmask) y *= bf2f(ldsM[r * WP + col]);
      y += bf2f(ldsY[r * WP + col]);
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

// ----------------------------------------------------------------- backward
typedef short srx_s16x2 __attribute__((ext_vector_type(2)));

// both 16-bit halves of z replaced by 16 copies of their top bit
__device__ __forceinline__ uint32_t mwe_wide_half_masks(uint32_t z) {
  srx_s16x2 v = __builtin_bit_cast(srx_s16x2, z);
  v = v >> 15;
  return __builtin_bit_cast(uint32_t, v);
}

// The A fragment of piece p: the lane's 8 dM values where their tag byte has
// bit p, zero elsewhere.  tags.x / tags.y hold the bytes of elements
// e0 e2 e1 e3 / e4 e6 e5 e7 (see the file comment).
__device__ __forceinline__ srx_bf16x8 mwe_wide_select(srx_u32x4_t dm, uint2 tags,
                                                      int p) {
  srx_u32x4_t o;
  o[0] = dm[0] & mwe_wide_half_masks(tags.x << (15 - p));
  o[1] = dm[1] & mwe_wide_half_masks(tags.x << (7 - p));
  o[2] = dm[2] & mwe_wide_half_masks(tags.y << (15 - p));
  o[3] = dm[3] & mwe_wide_half_masks(tags.y << (7 - p));
  return __builtin_bit_cast(srx_bf16x8, o);
}

// Stage 1 of image rows [0, MT + 2): row i = row t0 - 1 + i of the batch
// (zero outside [0, T)).  32 lanes per row, 8 columns per lane, NT / 32 rows
// per pass, the passes in groups of GP whose global loads are all issued
// before the first is used.  The fp32 arithmetic is that of
// mwe_stage1_tile (srx_mwe.hip.h).  Writes dM and the tags to LDS and the
// tile's own rows of dPre to memory; returns the column sums of the own rows.
template <class C>
__device__ __forceinline__ void mwe_wide_stage1(
    const bf16_t* __restrict__ dY, const bf16_t* __restrict__ dropmask,
    const bf16_t* __restrict__ Mout, const bf16_t* __restrict__ g,
    const float* __restrict__ mu, const float* __restrict__ rstd,
    const uint8_t* __restrict__ which, long T, long t0, int tid, bf16_t* ldsA,
    uint8_t* ldsT, bf16_t* __restrict__ dPre, float (&dg_out)[8],
    float (&db_out)[8], float (&dbias_out)[3][8]) {
  constexpr int W = C::W, MT = C::MT, A_ROWS = C::A_ROWS;
  constexpr int RG = C::NT / 32;                  // rows per pass
  constexpr int GP = 3;                           // passes per group
  constexpr int NGROUP = (A_ROWS + GP * RG - 1) / (GP * RG);
  const int q = tid & 31, rg = tid >> 5;
  float gv[8];
  ElemV<bf16_t, 8>::ld(g + q * 8, gv);

  float dg_loc[8], db_loc[8], dbias_loc[3][8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dg_loc[j] = 0.f;
    db_loc[j] = 0.f;
    dbias_loc[0][j] = dbias_loc[1][j] = dbias_loc[2][j] = 0.f;
  }

#pragma unroll 1
  for (int grp = 0; grp < NGROUP; grp++) {
    srx_u32x4_t rdy[GP], rmk[GP], rmo[GP];
    uint2 rwh[GP];
    float rmu[GP], rrs[GP];
#pragma unroll
    for (int ps = 0; ps < GP; ps++) {
      const int i = (grp * GP + ps) * RG + rg;
      const long t = t0 - 1 + i;
      rdy[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
      rmk[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
      rmo[ps] = srx_u32x4_t{0u, 0u, 0u, 0u};
      rwh[ps] = make_uint2(0u, 0u);
      rmu[ps] = 0.f;
      rrs[ps] = 0.f;
      if (i < A_ROWS && t >= 0 && t < T) {
        rdy[ps] = *(const srx_u32x4_t*)(dY + t * W + q * 8);
        if (dropmask) rmk[ps] = *(const srx_u32x4_t*)(dropmask + t * W + q * 8);
        rmo[ps] = *(const srx_u32x4_t*)(Mout + t * W + q * 8);
        rwh[ps] = *(const uint2*)(which + t * W + q * 8);
        rmu[ps] = mu[t];
        rrs[ps] = rstd[t];
      }
    }
#pragma unroll
    for (int ps = 0; ps < GP; ps++) {
      const int i = (grp * GP + ps) * RG + rg;
      const long t = t0 - 1 + i;
      const bool live = i < A_ROWS && t >= 0 && t < T;
      const bool own = live && i >= 1 && i < MT + 1;
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
      for (int off = 1; off < 32; off <<= 1) {
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
          for (int p = 0; p < 3; p++)
            dbias_loc[p][j] += (wh[j] == (uint32_t)p) ? dM : 0.f;
        }
      }
      if (i < A_ROWS) {
        srx_u32x4_t o;
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = hb[2 * k] | (hb[2 * k + 1] << 16);
        *(srx_u32x4_t*)(ldsA + i * C::AP + q * 8) = o;
        // tag 1 << which (0 for a piece outside 0..2), bytes e0 e2 e1 e3
        uint32_t tg[8];
#pragma unroll
        for (int j = 0; j < 8; j++) tg[j] = (live && wh[j] < 3u) ? (1u << wh[j]) : 0u;
        *(uint2*)(ldsT + i * C::TP + q * 8) = make_uint2(
            tg[0] | (tg[2] << 8) | (tg[1] << 16) | (tg[3] << 24),
            tg[4] | (tg[6] << 8) | (tg[5] << 16) | (tg[7] << 24));
      }
      // dPre out: dM at piece `which`, exact zero in the other two
      if (own) {
#pragma unroll
        for (int p = 0; p < 3; p++) {
          srx_u32x4_t o;
#pragma unroll
          for (int k = 0; k < 4; k++)
            o[k] = (wh[2 * k] == (uint32_t)p ? hb[2 * k] : 0u) |
                   ((wh[2 * k + 1] == (uint32_t)p ? hb[2 * k + 1] : 0u) << 16);
          *(srx_u32x4_t*)(dPre + t * (3 * W) + p * W + q * 8) = o;
        }
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

template <int W>
__global__ __launch_bounds__(512) void mwe_wide_bwd_fused_kernel(
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
    bf16_t* __restrict__ dPre,            // [T, 3W]
    bf16_t* __restrict__ dX,              // [T, W]
    float* __restrict__ partials,         // [gridDim.x, 5W]
    long T) {
  using C = MweWideBwdCfg;
  static_assert(W == C::W, "the wide kernels are W = 256");
  constexpr int MT = C::MT, NT = C::NT, AP = C::AP, TP = C::TP, BP = C::BP;
  constexpr int NWAVE = NT / SRX_WAVE;
  extern __shared__ __attribute__((aligned(16))) bf16_t lds[];
  bf16_t* ldsA = lds;                                    // dM [130][AP]
  uint8_t* ldsT = (uint8_t*)(lds + C::A_ELEMS);          // tags [130][TP]
  bf16_t* ldsB = (bf16_t*)(ldsT + C::T_BYTES);           // B chunks x2
  bf16_t* ldsO = lds;          // epilogue: dX [MT][AP] over the dM image
  float* ldsC = (float*)ldsB;  // epilogue: column sums [NWAVE][5W] over B

  const int tid = threadIdx.x;
  const int lane = tid % SRX_WAVE;
  const int wave = tid / SRX_WAVE;
  const int mq = wave >> 1, nh = wave & 1;
  const long t0 = (long)blockIdx.x * MT;

  srx_u32x4_t pf[C::PF];
  mwe_b_fetch<C>(WT, 0, tid, pf);

  float dg_loc[8], db_loc[8], dbias_loc[3][8];
  mwe_wide_stage1<C>(dY, dropmask, Mout, g, mu, rstd, which, T, t0, tid, ldsA,
                     ldsT, dPre, dg_loc, db_loc, dbias_loc);

  // dropped sections of this lane's row (the masks of seq2col_bwd_kernel):
  // s = 0 when t + 1 starts a doc or is T, s = 2 when t - 1 ends a doc or
  // t = 0; a row >= T drops everything
  const int rrow = 32 * mq + (lane & 31);
  bool drop0 = true, drop2 = true, dead = true;
  {
    const long t = t0 + rrow;
    if (t < T) {
      dead = false;
      drop0 = (t + 1 >= T) || is_start[t + 1];
      drop2 = (t == 0) || is_end[t - 1];
    }
  }
  mwe_b_store<C>(ldsB, tid, pf);
  __syncthreads();

  srx_f32x16 acc[4];  // columns 128 nh + 32 n + [0, 32)
#pragma unroll
  for (int n = 0; n < 4; n++)
#pragma unroll
    for (int rr = 0; rr < 16; rr++) acc[n][rr] = 0.f;

  for (int c = 0; c < C::NC; c++) {
    if (c + 1 < C::NC) mwe_b_fetch<C>(WT, c + 1, tid, pf);
    const int s = c / C::CPS, kc = c % C::CPS;
    const int p = kc >> 3, c0 = (kc & 7) * 32;
    const bool zr = dead || (s == 0 && drop0) || (s == 2 && drop2);
    const int aoff = c0 + 8 * (lane >> 5);
    const bf16_t* abase = ldsA + (rrow + 2 - s) * AP + aoff;
    const uint8_t* tbase = ldsT + (rrow + 2 - s) * TP + aoff;
    const bf16_t* bbase = ldsB + (c & 1) * (C::NBR * BP) +
                          (128 * nh + (lane & 31)) * BP + 8 * (lane >> 5);
#pragma unroll
    for (int ks = 0; ks < C::KC / 16; ks++) {
      const srx_u32x4_t dm = *(const srx_u32x4_t*)(abase + ks * 16);
      uint2 tags = *(const uint2*)(tbase + ks * 16);
      if (zr) tags = make_uint2(0u, 0u);
      const srx_bf16x8 afrag = mwe_wide_select(dm, tags, p);
#pragma unroll
      for (int n = 0; n < 4; n++) {
        const srx_bf16x8 bfrag =
            *(const srx_bf16x8*)(bbase + n * 32 * BP + ks * 16);
        acc[n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(afrag, bfrag, acc[n],
                                                         0, 0, 0);
      }
    }
    if (c + 1 < C::NC)
      mwe_b_store<C>(ldsB + ((c + 1) & 1) * (C::NBR * BP), tid, pf);
    __syncthreads();
  }

  // ---- column sums: fold the wave's two row groups, park one row [5W] per
  // wave in the free B region
  {
    const int q = tid & 31;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      dg_loc[j] += __shfl_xor(dg_loc[j], 32, SRX_WAVE);
      db_loc[j] += __shfl_xor(db_loc[j], 32, SRX_WAVE);
#pragma unroll
      for (int p = 0; p < 3; p++)
        dbias_loc[p][j] += __shfl_xor(dbias_loc[p][j], 32, SRX_WAVE);
    }
    if (lane < 32) {
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

  // ---- dX = acc + dY in fp32, one rounding, into the bf16 tile
#pragma unroll
  for (int n = 0; n < 4; n++) {
    const int col = 128 * nh + 32 * n + (lane & 31);
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int r = 32 * mq + (rr & 3) + 8 * (rr >> 2) + 4 * (lane >> 5);
      float v = acc[n][rr];
      if (t0 + r < T) v += bf2f(dY[(t0 + r) * W + col]);
      ldsO[r * AP + col] = f2bf(v);
    }
  }
  __syncthreads();
  for (int id = tid; id < MT * (W / 8); id += NT) {
    const int r = id / (W / 8), qq = id % (W / 8);
    if (t0 + r < T)
      *(srx_u32x4_t*)(dX + (t0 + r) * W + qq * 8) =
          *(const srx_u32x4_t*)(ldsO + r * AP + qq * 8);
  }
  mwe_colsums_out<W, NT>(ldsC, partials + (long)blockIdx.x * (5 * W), tid);
}
