// CharacterEmbed (spacy.CharacterEmbed.v2): a per-position byte table
// E [nC, 256, nM]; token t, position c embeds as E[c, ids[t, c]], the nC
// pieces concatenated into [T, nC * nM].  ids are uint8 [T, nC], 255 = pad.
//
// Forward: a pure gather from a table that lives in L2 (256 KB in bf16 at
// nC = 8, nM = 64).  Backward: one 256-bin histogram of nM-wide rows per
// position with very hot bins (the pad byte and a few letters take most
// tokens), accumulated in LDS so that hot rows never meet in global memory.
#pragma once
#include "srx_common.hip.h"

#define SRX_CE_BINS 256
#define SRX_CE_THREADS 256
#define SRX_CE_UNROLL 4

// ------------------------------------------------------------- forward
// A thread moves one 16-byte piece (V elements): item = t * (nC * LPT) +
// c * LPT + p with LPT = nM / V, so consecutive lanes write consecutive
// pieces of a token's nC * nM run of X (1 KB at nC = 8, nM = 64 bf16) and
// the lanes of a token read bytes of one nC-byte group of ids (one
// transaction, shared through the cache line).  The output is the table
// row's bits.  The caller guarantees T * nC * LPT < 2^31.
template <typename T, int V>
__global__ void char_embed_fwd_kernel(const T* __restrict__ E,
                                      const uint8_t* __restrict__ ids,
                                      T* __restrict__ X, long nT, int nC, int nM,
                                      long ldX) {
  const uint32_t LPT = (uint32_t)(nM / V);
  const uint32_t LP = (uint32_t)nC * LPT;
  const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t tu = item / LP;
  if ((long)tu >= nT) return;
  const long t = tu;
  const uint32_t j = item - tu * LP;
  const uint32_t c = j / LPT;
  const uint32_t p = j - c * LPT;
  const uint32_t id = ids[t * nC + c];
  const srx_u32x4_t v =
      *(const srx_u32x4_t*)(E + ((long)(c * SRX_CE_BINS + id) * nM + p * V));
  *(srx_u32x4_t*)(X + t * ldX + (long)c * nM + p * V) = v;
}

// ------------------------------------------------------------ backward
// Grid (nC, S): workgroup (c, s) owns position c and tokens [s * per,
// min(nT, (s + 1) * per)).  It zeroes an fp32 [256, nM] accumulator in LDS
// (64 KB at nM = 64: two workgroups per CU; 128 KB at nM = 128), streams
// its tokens and writes the accumulator to part[s, c] (fp32 [S, nC, 256,
// nM]); char_embed_reduce_kernel sums the S partials in fixed order.
//
// DET = false: LPT = nM / V lanes serve a token, each owning V fixed
// columns (one 16-byte load of the dX row).  The 256 threads cover 256 /
// LPT tokens per pass and SRX_CE_UNROLL passes are loaded before the first
// is consumed; every value is added to LDS row ids[t, c] with a float add
// whose result is not returned.  Hot bins contend inside LDS only.
//
// DET = true (one wave per workgroup): tokens are taken one at a time, in
// order; lane l owns columns l and l + 64 and does a plain LDS
// read-add-write, so the sums are bit-identical from run to run.
template <typename T, int V, bool DET>
__global__ void char_embed_bwd_kernel(const T* __restrict__ dX,
                                      const uint8_t* __restrict__ ids,
                                      float* __restrict__ part, long nT, long per,
                                      int nC, int nM, long ldX) {
  extern __shared__ __attribute__((aligned(16))) float ce_acc[];
  const int c = blockIdx.x;
  const long s = blockIdx.y;
  const int tid = threadIdx.x;
  const int n_acc = SRX_CE_BINS * nM;
  for (int i = tid * 4; i < n_acc; i += blockDim.x * 4)
    *(float4*)(ce_acc + i) = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();

  const long t0 = s * per;
  const long t1 = t0 + per < nT ? t0 + per : nT;
  const T* dx = dX + (long)c * nM;
  if (DET) {
    for (long tb = t0; tb < t1; tb += SRX_CE_UNROLL) {
      float v[SRX_CE_UNROLL][2];
      int row[SRX_CE_UNROLL];
#pragma unroll
      for (int u = 0; u < SRX_CE_UNROLL; u++) {
        const long t = tb + u;
        const bool ok = t < t1;
        row[u] = ok ? (int)ids[t * nC + c] * nM : 0;
        v[u][0] = ok && tid < nM ? Elem<T>::ld(dx + t * ldX + tid) : 0.f;
        v[u][1] = ok && tid + SRX_WAVE < nM
                      ? Elem<T>::ld(dx + t * ldX + tid + SRX_WAVE) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < SRX_CE_UNROLL; u++) {
        if (tb + u < t1) {
          if (tid < nM) ce_acc[row[u] + tid] += v[u][0];
          if (tid + SRX_WAVE < nM) ce_acc[row[u] + tid + SRX_WAVE] += v[u][1];
        }
      }
    }
  } else {
    const int LPT = nM / V;
    const int tpp = SRX_CE_THREADS / LPT;  // tokens per pass
    const int sub = tid / LPT;             // this lane's token of a pass
    const int col = (tid - sub * LPT) * V;
    if (sub < tpp) {
      for (long tb = t0 + sub; tb < t1; tb += (long)tpp * SRX_CE_UNROLL) {
        float v[SRX_CE_UNROLL][V];
        int row[SRX_CE_UNROLL];
#pragma unroll
        for (int u = 0; u < SRX_CE_UNROLL; u++) {
          const long t = tb + (long)u * tpp;
          if (t < t1) {
            row[u] = (int)ids[t * nC + c] * nM + col;
            ElemV<T, V>::ld(dx + t * ldX + col, v[u]);
          } else {
            row[u] = -1;
          }
        }
#pragma unroll
        for (int u = 0; u < SRX_CE_UNROLL; u++) {
          if (row[u] >= 0) {
#pragma unroll
            for (int k = 0; k < V; k++)
              __hip_atomic_fetch_add(ce_acc + row[u] + k, v[u][k],
                                     __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
          }
        }
      }
    }
  }
  __syncthreads();
  float* out = part + (s * nC + c) * (long)n_acc;
  for (int i = tid * 4; i < n_acc; i += blockDim.x * 4)
    *(float4*)(out + i) = *(const float4*)(ce_acc + i);
}

// dE[i] = sum over s (ascending) of part[s, i], converted to the table
// dtype; a thread owns V adjacent elements, n = nC * 256 * nM.
template <typename T, int V>
__global__ void char_embed_reduce_kernel(const float* __restrict__ part,
                                         T* __restrict__ dE, long n, long S) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * V;
  if (i >= n) return;
  float acc[V];
#pragma unroll
  for (int k = 0; k < V; k++) acc[k] = 0.f;
  for (long s = 0; s < S; s++) {
#pragma unroll
    for (int k = 0; k < V; k += 4) {
      const float4 x = *(const float4*)(part + s * n + i + k);
      acc[k] += x.x; acc[k + 1] += x.y; acc[k + 2] += x.z; acc[k + 3] += x.w;
    }
  }
  ElemV<T, V>::st(dE + i, acc);
}
