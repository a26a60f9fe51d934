// SparseLinear over hashed token n-grams: the hot path of spaCy's TextCatBOW.
//
// Definition.  ids int64 [Tn] (uint64 token keys, bit-cast), offsets int32
// [D + 1], G = ngram_size <= 4, weight [L, nO] with L a power of two.  Every
// doc d, n in 1..G and position i with i + n <= len(d) is an OCCURRENCE:
//   key = murmur2_64a(ids[beg + i .. beg + i + n), 8 n bytes, seed 0)
//   h   = murmur3_hash4_u64(key, seed 0);  b0 = h[0] & (L-1), b1 = h[1] & (L-1)
//   scores[d] = bias + sum over the doc's occurrences of weight[b0] + weight[b1]
//   dWeight[r] = sum over (occurrence, bucket) ENTRIES with bucket r of dScores[doc]
// Occurrences are numbered n-major, then by position, inside a doc.
//
// The window of up to four ids is a register array that is only ever indexed
// by unrolled loop counters; which words take part is a predicate (j < n).
//
// ngram_buckets_kernel: a thread per token.  It finds its doc by binary
// search in offsets and writes the (b0, b1) of the n-grams that START at it
// to their doc-major slot (occ_offsets is the prefix sum of the docs'
// occurrence counts).  The seam between the host and device hashes and the
// input of the composed path; the fused kernels never read its output.
//
// sparse_linear_fwd_kernel<T, SW, C>: a sub-wave of SW lanes per doc, docs
// grid-strided in wave-uniform groups of 64 / SW.
// * A row is nC = nO / C chunks of C columns (C the largest power of two
//   <= 16 bytes / sizeof(T) that divides nO: one 16-byte load for nO = 8
//   bf16 or 4 fp32, 2-byte loads for an odd bf16 nO).  CL = the power of
//   two >= nC (at most 64) lanes share a row, so a sub-wave works on
//   SW / CL occurrences ("slots") side by side.  A lane = (slot, chunk q).
// * A lane takes occurrences slot, slot + slots, ... of its doc, hashes each
//   itself (the CL lanes of a row repeat the hash: lanes that would idle
//   otherwise) and loads its chunk of BOTH rows.  Two occurrences per trip:
//   four row loads in flight per lane.  fp32 accumulation, per lane in
//   occurrence order, b0 before b1.
// * After the occurrence loop the wave has reconverged; an xor butterfly over
//   the slot bits (offsets SW/2 .. CL) sums the lanes of one chunk, slot 0
//   adds the bias and stores fp32.  An empty doc stores the bias.
// * nC > 64 (odd nO above 64) makes further passes over the row.
// The summation order of a doc depends on that doc, SW and CL only, never on
// the grid or on neighbouring docs.  SW changes the order, so the launcher
// takes it as an argument (0 = choose from the mean occurrences per doc).
// No LDS, no atomics.  offsets are clamped to [0, Tn] and buckets are masked,
// so memory safety does not depend on the host.
//
// Backward, atomic-free, over ENTRIES = (occurrence, bucket):
// 1. sparse_linear_keys_kernel: a thread per token writes, for each n in
//    1..G, two int64 `(bucket << 32) | doc` into slot (t G + n - 1) 2.  An
//    n-gram that would cross the doc's end writes the sentinel (bucket field
//    0x7fffffff) instead, so the array has the fixed length 2 G Tn and no
//    count has to come back to the host.
// 2. One sort of those values (the host's library call).  Equal values are
//    interchangeable, so the order is fully determined; sentinels go last.
// 3. sparse_linear_bwd_kernel<T, VEC>: a wave per chunk of 256 sorted
//    entries, four consecutive entries per lane (one 32-byte load).  Per pass
//    of four columns a lane gathers dScores[doc] (small, L2-resident), scans
//    its four entries serially, then the wave runs a segmented Kogge-Stone
//    scan (shuffle-up by 1, 2, .. 32; the segment flags of all six steps are
//    computed once per chunk).  The last entry of a run holds its sum.  Runs
//    wholly inside the chunk are rounded once and stored to dWeight with
//    plain stores.  The first and the last run of a chunk always go, as fp32
//    partial rows with their bucket, to the carry buffer [n_chunks, 2, nO];
//    a chunk that is one single run stores its sum in slot 0 and a zero row
//    in slot 1, so the carries of one bucket are always contiguous.
// 4. sparse_linear_fixup_kernel<T>: a lane per (carry entry, column).  The
//    entry whose predecessor has another bucket is the head: it adds the
//    following carries of its bucket in chunk order (loads eight ahead) and
//    stores the rounded row.
// Each dWeight row has exactly one writer (a bucket is one run of the sorted
// array); dWeight is zeroed first, rows never hit stay zero.  A hot row with
// a run of R entries is reduced by R / 256 waves in parallel and then by one
// lane per column over 2 R / 256 carries.  Every order is fixed: bit-identical
// between runs and for every grid, so SRX_DETERMINISTIC needs no variant.
//
// Compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage,
// gfx950; AGPR 0, scratch 0 and LDS 0 in all 36 kernels; 256 threads; the
// full table is in docs/KERNELS.md):
//   ngram_buckets / sparse_linear_keys     26 VGPR  48 SGPR  8 waves / SIMD
//   sparse_linear_fwd_kernel<bf16, *, 8>   66 VGPR  86..90 SGPR  7
//   sparse_linear_fwd_kernel<*, *, <= 4>   38..43 VGPR  86..90 SGPR  8
//   sparse_linear_bwd_kernel<*, *>         54..58 VGPR  106 SGPR  7
//   sparse_linear_fixup_kernel<*>          46 VGPR  46..47 SGPR  8
#pragma once
#include "srx_common.hip.h"

#define SRX_SPL_THREADS 256
#define SRX_SPL_CHUNK 256  // sorted entries per wave in the backward
#define SRX_SPL_BAD 0x7fffffff
// scalar fp32 VALU only (independent accumulation chains per lane would
// otherwise be paired into packed fp32 adds)
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass does not know the feature
#define SRX_SPL_FN __attribute__((target("no-packed-fp32-ops")))
#else
#define SRX_SPL_FN
#endif

typedef __attribute__((__vector_size__(8))) uint32_t srx_spl_u32x2_t;

// ---- MurmurHash64A of n <= 4 little-endian 8-byte words: device twin of
// ops/csrc/murmur3.h::murmur2_64a for len = 8 n (no tail bytes) — MUST stay
// bit-identical.  w is indexed by the unrolled counter only.
__device__ __forceinline__ uint64_t murmur2_64a_words_dev(const uint64_t (&w)[4],
                                                          int n, uint64_t seed) {
  const uint64_t m = 0xc6a4a7935bd1e995ULL;
  const int r = 47;
  uint64_t h = seed ^ ((uint64_t)(8 * n) * m);
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j < n) {
      uint64_t k = w[j];
      k *= m;
      k ^= k >> r;
      k *= m;
      h ^= k;
      h *= m;
    }
  }
  h ^= h >> r;
  h *= m;
  h ^= h >> r;
  return h;
}

__device__ __forceinline__ void spl_window(const int64_t* __restrict__ ids, long t,
                                           int n, uint64_t (&w)[4]) {
#pragma unroll
  for (int j = 0; j < 4; j++) w[j] = j < n ? (uint64_t)ids[t + j] : 0ULL;
}

__device__ __forceinline__ void spl_buckets(const uint64_t (&w)[4], int n,
                                            uint32_t mask, int& b0, int& b1) {
  uint32_t h[4];
  murmur3_hash4_u64_dev(murmur2_64a_words_dev(w, n, 0ULL), 0u, h);
  b0 = (int)(h[0] & mask);
  b1 = (int)(h[1] & mask);
}

// occurrences of a doc of `len` tokens
__device__ __forceinline__ int spl_count(int len, int G) {
  int m = 0;
#pragma unroll
  for (int k = 1; k <= 4; k++)
    if (k <= G) m += max(0, len - k + 1);
  return m;
}

// occurrence o -> (n, position i); n = 0 when o is past the doc's last
__device__ __forceinline__ void spl_decode(int o, int len, int G, int& n, int& i) {
  n = 0;
  i = 0;
#pragma unroll
  for (int k = 1; k <= 4; k++) {
    const int cnt = k <= G ? max(0, len - k + 1) : 0;
    if (n == 0) {
      if (o < cnt) {
        n = k;
        i = o;
      } else {
        o -= cnt;
      }
    }
  }
}

// the doc that holds token t: the last d with offsets[d] <= t, and how many
// tokens of it start at or after t (0 when t lies in no doc)
__device__ __forceinline__ int spl_doc_of(const int* __restrict__ offsets, int D,
                                          int Tn, long t, int& remaining) {
  int lo = 0, hi = D + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((long)offsets[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const int d = lo - 1;
  remaining = 0;
  if (d >= 0 && d < D) remaining = (int)max(0L, (long)min(offsets[d + 1], Tn) - t);
  return d;
}

__global__ __launch_bounds__(SRX_SPL_THREADS) void ngram_buckets_kernel(
    const int64_t* __restrict__ ids,          // [Tn]
    const int* __restrict__ offsets,          // [D + 1]
    const int64_t* __restrict__ occ_offsets,  // [D + 1]
    int* __restrict__ out,                    // [nnz, 2]
    int D, int Tn, int G, uint32_t mask, long nnz) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < Tn; t += stride) {
    int remaining;
    const int d = spl_doc_of(offsets, D, Tn, t, remaining);
    if (remaining <= 0) continue;
    const int beg = offsets[d];
    const int len = (int)(t - beg) + remaining;
    uint64_t w[4];
    spl_window(ids, t, min(remaining, G), w);
    long slot = occ_offsets[d] + (t - beg);
#pragma unroll
    for (int n = 1; n <= 4; n++) {
      if (n <= G && n <= remaining) {
        int b0, b1;
        spl_buckets(w, n, mask, b0, b1);
        if (slot >= 0 && slot < nnz) {
          out[2 * slot] = b0;
          out[2 * slot + 1] = b1;
        }
      }
      slot += max(0, len - n + 1);
    }
  }
}

// C columns of a row <-> C floats
template <typename T, int C>
struct SplRow;

template <>
struct SplRow<bf16_t, 1> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) { v[0] = bf2f(*p); }
};
template <>
struct SplRow<bf16_t, 2> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const uint32_t u = *(const uint32_t*)p;
    v[0] = __uint_as_float(u << 16);
    v[1] = __uint_as_float(u & 0xffff0000u);
  }
};
template <>
struct SplRow<bf16_t, 4> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const srx_spl_u32x2_t u = *(const srx_spl_u32x2_t*)p;
#pragma unroll
    for (int i = 0; i < 2; i++) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
};
template <>
struct SplRow<bf16_t, 8> {
  static __device__ __forceinline__ void ld(const bf16_t* p, float* v) {
    const srx_u32x4_t u = *(const srx_u32x4_t*)p;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      v[2 * i] = __uint_as_float(u[i] << 16);
      v[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
    }
  }
};
template <>
struct SplRow<float, 1> {
  static __device__ __forceinline__ void ld(const float* p, float* v) { v[0] = *p; }
};
template <>
struct SplRow<float, 2> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float2 x = *(const float2*)p;
    v[0] = x.x; v[1] = x.y;
  }
};
template <>
struct SplRow<float, 4> {
  static __device__ __forceinline__ void ld(const float* p, float* v) {
    const float4 x = *(const float4*)p;
    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  }
};

template <typename T, int SW, int C>
__global__ __launch_bounds__(SRX_SPL_THREADS) SRX_SPL_FN void sparse_linear_fwd_kernel(
    const int64_t* __restrict__ ids,   // [Tn]
    const int* __restrict__ offsets,   // [D + 1]
    const T* __restrict__ weight,      // [L, nO]
    const float* __restrict__ bias,    // [nO]
    float* __restrict__ scores,        // [D, nO]
    int D, int Tn, int G, int nO, uint32_t mask,
    int CL) {                          // lanes per row: power of two, <= SW
  constexpr int DPW = SRX_WAVE / SW;   // docs per wave
  const int lane = threadIdx.x % SRX_WAVE;
  const int g = lane / SW, sl = lane % SW;
  const int ql = sl & (CL - 1), slot = sl / CL, slots = SW / CL;
  const int nC = nO / C;
  const long wpb = blockDim.x / SRX_WAVE;
  const long ngroups = ((long)D + DPW - 1) / DPW;

  for (long grp = (long)blockIdx.x * wpb + threadIdx.x / SRX_WAVE; grp < ngroups;
       grp += (long)gridDim.x * wpb) {
    const long d = grp * DPW + g;
    int beg = 0, end = 0;
    if (d < D) {
      beg = offsets[d];
      end = offsets[d + 1];
    }
    beg = min(max(beg, 0), Tn);
    end = min(max(end, beg), Tn);
    const int len = end - beg;
    const int M = spl_count(len, G);

    for (int q0 = 0; q0 < nC; q0 += CL) {  // one pass unless nC > 64
      const int q = q0 + ql;
      const bool colok = q < nC;
      const T* __restrict__ col = weight + q * C;
      float acc[C];
#pragma unroll
      for (int c = 0; c < C; c++) acc[c] = 0.f;

      for (int o = slot; o < M; o += 2 * slots) {
        int b[2][2];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          int n, i;
          spl_decode(o + u * slots, len, G, n, i);
          ok[u] = n > 0 && colok;
          uint64_t w[4];
          spl_window(ids, (long)beg + i, n, w);
          spl_buckets(w, n, mask, b[u][0], b[u][1]);
        }
        float v[2][2][C];
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
          for (int k = 0; k < 2; k++) {
#pragma unroll
            for (int c = 0; c < C; c++) v[u][k][c] = 0.f;
            if (ok[u]) SplRow<T, C>::ld(col + (long)b[u][k] * nO, v[u][k]);
          }
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
          for (int k = 0; k < 2; k++)
#pragma unroll
            for (int c = 0; c < C; c++) acc[c] += v[u][k][c];
      }
      // the wave has reconverged: sum the slots of each chunk
#pragma unroll
      for (int off = SW / 2; off >= 1; off >>= 1)
        if (off >= CL) {
#pragma unroll
          for (int c = 0; c < C; c++) acc[c] += __shfl_xor(acc[c], off, SRX_WAVE);
        }
      if (d < D && colok && slot == 0) {
#pragma unroll
        for (int c = 0; c < C; c++)
          scores[d * nO + q * C + c] = acc[c] + bias[q * C + c];
      }
    }
  }
}

__global__ __launch_bounds__(SRX_SPL_THREADS) void sparse_linear_keys_kernel(
    const int64_t* __restrict__ ids,  // [Tn]
    const int* __restrict__ offsets,  // [D + 1]
    int64_t* __restrict__ keys,       // [2 G Tn]
    int D, int Tn, int G, uint32_t mask) {
  const int64_t bad = (int64_t)SRX_SPL_BAD << 32;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < Tn; t += stride) {
    int remaining;
    const int d = spl_doc_of(offsets, D, Tn, t, remaining);
    uint64_t w[4];
    spl_window(ids, t, min(remaining, G), w);
#pragma unroll
    for (int n = 1; n <= 4; n++) {
      if (n <= G) {
        int64_t k0 = bad, k1 = bad;
        if (n <= remaining) {
          int b0, b1;
          spl_buckets(w, n, mask, b0, b1);
          k0 = ((int64_t)b0 << 32) | (int64_t)d;
          k1 = ((int64_t)b1 << 32) | (int64_t)d;
        }
        const long slot = (t * G + (n - 1)) * 2;
        keys[slot] = k0;
        keys[slot + 1] = k1;
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ void spl_store_row(T* __restrict__ p, const float* v, int nc,
                                              bool vec);

template <>
__device__ __forceinline__ void spl_store_row<float>(float* __restrict__ p,
                                                      const float* v, int nc,
                                                      bool vec) {
  if (vec) {  // nO % 4 == 0: the piece is 16-byte aligned
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < nc) p[c] = v[c];
  }
}

template <>
__device__ __forceinline__ void spl_store_row<bf16_t>(bf16_t* __restrict__ p,
                                                       const float* v, int nc,
                                                       bool vec) {
  if (vec) {
    srx_spl_u32x2_t o;
    o[0] = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    o[1] = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    *(srx_spl_u32x2_t*)p = o;
  } else {
#pragma unroll
    for (int c = 0; c < 4; c++)
      if (c < nc) p[c] = f2bf(v[c]);
  }
}

// VEC: nO % 4 == 0, every column pass is a whole 16-byte piece
template <typename T, bool VEC>
__global__ __launch_bounds__(SRX_SPL_THREADS) SRX_SPL_FN void sparse_linear_bwd_kernel(
    const int64_t* __restrict__ sorted,  // [N] ascending (bucket << 32) | doc
    const float* __restrict__ dS,        // [D, nO]
    T* __restrict__ dW,                  // [L, nO], zeroed
    int* __restrict__ cbucket,           // [n_chunks, 2]
    float* __restrict__ crow,            // [n_chunks, 2, nO]
    long N, long n_chunks, int D, int L, int nO) {
  const int lane = threadIdx.x % SRX_WAVE;
  const long wpb = blockDim.x / SRX_WAVE;
  const int64_t bad = (int64_t)SRX_SPL_BAD << 32;

  for (long ch = (long)blockIdx.x * wpb + threadIdx.x / SRX_WAVE; ch < n_chunks;
       ch += (long)gridDim.x * wpb) {
    const long e0 = ch * SRX_SPL_CHUNK + lane * 4;
    int b[4], doc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int64_t k = e0 + j < N ? sorted[e0 + j] : bad;
      b[j] = (int)(k >> 32);
      doc[j] = (int)(k & 0xffffffffLL);
      if (b[j] < 0 || b[j] >= L || doc[j] < 0 || doc[j] >= D) {
        b[j] = SRX_SPL_BAD;
        doc[j] = -1;
      }
    }
    int prevb = __shfl_up(b[3], 1, SRX_WAVE);
    int nextb = __shfl_down(b[0], 1, SRX_WAVE);
    if (lane == 0) prevb = -2;
    if (lane == SRX_WAVE - 1) nextb = -2;
    const int firstb = __shfl(b[0], 0, SRX_WAVE);
    const int lastb = __shfl(b[3], SRX_WAVE - 1, SRX_WAVE);
    const bool same0 = b[0] == prevb;
    bool same[4], infirst[4], tail[4];
    same[0] = same0;
    infirst[0] = true;
#pragma unroll
    for (int j = 1; j < 4; j++) {
      same[j] = b[j] == b[j - 1];
      infirst[j] = infirst[j - 1] && same[j];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) tail[j] = !same[j + 1];
    tail[3] = b[3] != nextb;
    // segment flag of the lane's last run, as each scan step sees it
    int f = (infirst[3] && same0) ? 0 : 1;
    int fstep[6];
#pragma unroll
    for (int s = 0; s < 6; s++) {
      fstep[s] = f;
      const int fo = __shfl_up(f, 1 << s, SRX_WAVE);
      if (lane >= (1 << s)) f |= fo;
    }
    if (lane == 0) {
      cbucket[2 * ch] = firstb;
      cbucket[2 * ch + 1] = lastb;
    }

    for (int c0 = 0; c0 < nO; c0 += 4) {
      const int nc = VEC ? 4 : min(4, nO - c0);
      float s[4][4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int c = 0; c < 4; c++) s[j][c] = 0.f;
        if (doc[j] >= 0) {
          const float* __restrict__ src = dS + (long)doc[j] * nO + c0;
          if (VEC) {
            const float4 x = *(const float4*)src;
            s[j][0] = x.x; s[j][1] = x.y; s[j][2] = x.z; s[j][3] = x.w;
          } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
              if (c < nc) s[j][c] = src[c];
          }
        }
      }
      // serial scan of the lane's four entries
#pragma unroll
      for (int j = 1; j < 4; j++)
        if (same[j]) {
#pragma unroll
          for (int c = 0; c < 4; c++) s[j][c] += s[j - 1][c];
        }
      // segmented scan over the lanes' last runs
      float x[4];
#pragma unroll
      for (int c = 0; c < 4; c++) x[c] = s[3][c];
#pragma unroll
      for (int st = 0; st < 6; st++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const float y = __shfl_up(x[c], 1 << st, SRX_WAVE);
          if (lane >= (1 << st) && !fstep[st]) x[c] += y;
        }
      }
      float cin[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        cin[c] = __shfl_up(x[c], 1, SRX_WAVE);
        if (!same0) cin[c] = 0.f;  // lane 0 included: prevb = -2
      }
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (tail[j]) {
          float tot[4];
#pragma unroll
          for (int c = 0; c < 4; c++) tot[c] = infirst[j] ? s[j][c] + cin[c] : s[j][c];
          if (b[j] == firstb) {
            spl_store_row<float>(crow + (2 * ch) * nO + c0, tot, nc, VEC);
            if (firstb == lastb) {
              const float z[4] = {0.f, 0.f, 0.f, 0.f};
              spl_store_row<float>(crow + (2 * ch + 1) * nO + c0, z, nc, VEC);
            }
          } else if (b[j] == lastb) {
            spl_store_row<float>(crow + (2 * ch + 1) * nO + c0, tot, nc, VEC);
          } else if (b[j] < L) {
            spl_store_row<T>(dW + (long)b[j] * nO + c0, tot, nc, VEC);
          }
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(SRX_SPL_THREADS) SRX_SPL_FN void sparse_linear_fixup_kernel(
    const int* __restrict__ cbucket,  // [NE]
    const float* __restrict__ crow,   // [NE, nO]
    T* __restrict__ dW,               // [L, nO]
    long NE, int L, int nO) {
  const long total = NE * nO;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += stride) {
    const long e = idx / nO;
    const int c = (int)(idx - e * nO);
    const int b = cbucket[e];
    if (b < 0 || b >= L) continue;
    if (e > 0 && cbucket[e - 1] == b) continue;  // not the head
    float acc = crow[e * nO + c];
    bool go = true;
    for (long k = e + 1; go; k += 8) {
      int bb[8];
      float vv[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const bool in = k + u < NE;
        bb[u] = in ? cbucket[k + u] : -1;
        vv[u] = in ? crow[(k + u) * nO + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (go && bb[u] == b) acc += vv[u]; else go = false;
      }
    }
    Elem<T>::st(dW + (long)b * nO + c, acc);
  }
}
