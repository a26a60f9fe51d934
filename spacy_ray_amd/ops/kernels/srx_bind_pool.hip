// _srx_hip bindings: span pooling, attention pooling and SparseLinear.
#include "srx_bind.hip.h"

#include <type_traits>
#include <utility>

#include "srx_spanpool.hip.h"
#include "srx_attnpool.hip.h"
#include "srx_sparselinear.hip.h"

namespace {

// ------------------------------------------------------------ span pooling
// see srx_spanpool.hip.h.  X [T, W] bf16 (W % 8 == 0) or fp32 (W % 4 == 0),
// W <= 1024; starts / ends int32 [S].
namespace spanpool {

inline int sub_wave(long Q) { return Q <= 8 ? 8 : Q <= 16 ? 16 : Q <= 32 ? 32 : 64; }

// memory bound: at most 8 workgroups per CU, the rest is grid-strided
inline dim3 grid_for(long rows, int sw) {
  const long per_block = (SRX_SPANPOOL_THREADS / SRX_WAVE) * (SRX_WAVE / sw);
  const long cap = 8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  return dim3((unsigned)std::max<long>(
      1, std::min<long>((rows + per_block - 1) / per_block, cap)));
}

inline long check_x(const at::Tensor& X, const char* what) {
  check_dev(X);
  TORCH_CHECK(X.dim() == 2 && (X.scalar_type() == at::kBFloat16 ||
                               X.scalar_type() == at::kFloat),
              what, " must be bf16 or fp32 [rows, W]");
  const long V = X.scalar_type() == at::kBFloat16 ? 8 : 4;
  return V;
}

inline void check_spans(const at::Tensor& starts, const at::Tensor& ends) {
  check_dev(starts);
  check_dev(ends);
  TORCH_CHECK(starts.scalar_type() == at::kInt && ends.scalar_type() == at::kInt &&
                  starts.dim() == 1 && ends.dim() == 1 &&
                  starts.numel() == ends.numel(),
              "span_pool: starts and ends must be int32 [S]");
}

}  // namespace spanpool

#define SRX_SPANPOOL_DISPATCH(LAUNCH)                                          \
  if (bf16) {                                                                  \
    if (sw == 8) { LAUNCH(bf16_t, 8); }                                        \
    else if (sw == 16) { LAUNCH(bf16_t, 16); }                                 \
    else if (sw == 32) { LAUNCH(bf16_t, 32); }                                 \
    else { LAUNCH(bf16_t, 64); }                                               \
  } else {                                                                     \
    if (sw == 8) { LAUNCH(float, 8); }                                         \
    else if (sw == 16) { LAUNCH(float, 16); }                                  \
    else if (sw == 32) { LAUNCH(float, 32); }                                  \
    else { LAUNCH(float, 64); }                                                \
  }

// -> (R [rows, 4 W], which uint8 [S, W]); rows >= S, rows [S, rows) zero
std::vector<at::Tensor> span_pool_fwd(at::Tensor X, at::Tensor starts,
                                      at::Tensor ends, long rows) {
  const long V = spanpool::check_x(X, "span_pool_fwd: X");
  spanpool::check_spans(starts, ends);
  const long T = X.size(0), W = X.size(1), S = starts.numel();
  TORCH_CHECK(W >= V && W % V == 0 && W <= 1024,
              "span_pool_fwd: W must be a multiple of ", V, " and <= 1024");
  TORCH_CHECK(rows >= S && rows < (1L << 31) && T < (1L << 31),
              "span_pool_fwd: S <= rows < 2^31 and T < 2^31");
  TORCH_CHECK(aligned16(X.data_ptr()), "span_pool_fwd: X not 16-byte aligned");
  auto R = at::empty({rows, 4 * W}, X.options());
  auto which = at::empty({S, W}, X.options().dtype(at::kByte));
  if (rows == 0) return {R, which};
  const bool bf16 = X.scalar_type() == at::kBFloat16;
  const int sw = spanpool::sub_wave(W / V);
  const dim3 grid = spanpool::grid_for(rows, sw);
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_SPANPOOL_FWD(TT, SW)                                               \
  hipLaunchKernelGGL((span_pool_fwd_kernel<TT, SW>), grid,                     \
                     dim3(SRX_SPANPOOL_THREADS), 0, stream,                    \
                     (const TT*)X.data_ptr(), starts.data_ptr<int>(),          \
                     ends.data_ptr<int>(), (TT*)R.data_ptr(),                  \
                     which.data_ptr<uint8_t>(), (int)S, (int)rows, (int)T,     \
                     (int)W)
  SRX_SPANPOOL_DISPATCH(SRX_SPANPOOL_FWD)
#undef SRX_SPANPOOL_FWD
  return {R, which};
}

// dX [T, W] from dR [>= S, 4 W]; every row of dX is written
at::Tensor span_pool_bwd(at::Tensor dR, at::Tensor which, at::Tensor starts,
                         at::Tensor ends, at::Tensor tok_offsets,
                         at::Tensor tok_spans) {
  const long V = spanpool::check_x(dR, "span_pool_bwd: dR");
  spanpool::check_spans(starts, ends);
  check_dev(which);
  check_dev(tok_offsets);
  check_dev(tok_spans);
  const long S = starts.numel(), W = dR.size(1) / 4;
  TORCH_CHECK(dR.size(1) == 4 * W && W >= V && W % V == 0 && W <= 1024 &&
                  dR.size(0) >= S,
              "span_pool_bwd: dR must be [>= S, 4 W], W a multiple of ", V,
              " and <= 1024");
  TORCH_CHECK(which.scalar_type() == at::kByte && which.dim() == 2 &&
                  which.size(0) == S && which.size(1) == W,
              "span_pool_bwd: which must be uint8 [S, W]");
  TORCH_CHECK(tok_offsets.scalar_type() == at::kInt && tok_offsets.dim() == 1 &&
                  tok_offsets.numel() >= 1 &&
                  tok_spans.scalar_type() == at::kInt && tok_spans.dim() == 1,
              "span_pool_bwd: tok_offsets int32 [T + 1], tok_spans int32 [nnz]");
  const long T = tok_offsets.numel() - 1, nnz = tok_spans.numel();
  TORCH_CHECK(T < (1L << 31) && nnz < (1L << 31) && S < (1L << 31),
              "span_pool_bwd: sizes must fit in int32");
  TORCH_CHECK(aligned16(dR.data_ptr()), "span_pool_bwd: dR not 16-byte aligned");
  auto dX = at::empty({T, W}, dR.options());
  if (T == 0) return dX;
  const bool bf16 = dR.scalar_type() == at::kBFloat16;
  const int sw = spanpool::sub_wave(W / V);
  const dim3 grid = spanpool::grid_for(T, sw);
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_SPANPOOL_BWD(TT, SW)                                               \
  hipLaunchKernelGGL((span_pool_bwd_kernel<TT, SW>), grid,                     \
                     dim3(SRX_SPANPOOL_THREADS), 0, stream,                    \
                     (const TT*)dR.data_ptr(), which.data_ptr<uint8_t>(),      \
                     starts.data_ptr<int>(), ends.data_ptr<int>(),             \
                     tok_offsets.data_ptr<int>(), tok_spans.data_ptr<int>(),   \
                     (TT*)dX.data_ptr(), (int)S, (int)T, (int)W, (int)nnz)
  SRX_SPANPOOL_DISPATCH(SRX_SPANPOOL_BWD)
#undef SRX_SPANPOOL_BWD
  return dX;
}
#undef SRX_SPANPOOL_DISPATCH

// -------------------------------------------------------- attention pooling
// see srx_attnpool.hip.h.  X (and keys) [T, W] bf16 (W % 8 == 0) or fp32 (W %
// 4 == 0), W <= 768; offsets int32 [D + 1], ascending from 0 to T; q fp32 [W].
namespace attnpool {

struct Shape {
  long T, W, D, V, bound, n_slots;
  int sw, np;
  bool bf16, hask;
};

inline Shape check(const at::Tensor& X, const c10::optional<at::Tensor>& keys,
                   const at::Tensor& offsets, const at::Tensor& q, long sub_wave) {
  Shape s;
  s.V = spanpool::check_x(X, "attention_pool: X");
  check_dev(offsets);
  check_dev(q);
  s.T = X.size(0), s.W = X.size(1), s.D = offsets.numel() - 1;
  s.bf16 = X.scalar_type() == at::kBFloat16;
  s.hask = keys.has_value();
  TORCH_CHECK(s.W >= s.V && s.W % s.V == 0 && s.W <= SRX_ATTNPOOL_MAXW,
              "attention_pool: W must be a multiple of ", s.V, " and <= ",
              SRX_ATTNPOOL_MAXW);
  TORCH_CHECK(offsets.scalar_type() == at::kInt && offsets.dim() == 1 && s.D >= 0,
              "attention_pool: offsets must be int32 [D + 1]");
  TORCH_CHECK(q.scalar_type() == at::kFloat && q.dim() == 1 && q.numel() == s.W,
              "attention_pool: q must be fp32 [W]");
  TORCH_CHECK(aligned16(X.data_ptr()) && aligned16(q.data_ptr()),
              "attention_pool: X or q not 16-byte aligned");
  if (s.hask) {
    check_dev(*keys);
    TORCH_CHECK(keys->scalar_type() == X.scalar_type() && keys->sizes() == X.sizes() &&
                    aligned16(keys->data_ptr()),
                "attention_pool: keys must match X in dtype and shape");
  }
  s.bound = s.D + s.T / SRX_ATTNPOOL_CHUNK;
  s.n_slots = 2 * (s.T / SRX_ATTNPOOL_CHUNK);
  TORCH_CHECK(s.T < (1L << 31) - SRX_ATTNPOOL_CHUNK && s.bound < (1L << 30),
              "attention_pool: T and D + T / 64 must fit in int32");
  TORCH_CHECK(sub_wave == 0 || sub_wave == 8 || sub_wave == 16 || sub_wave == 32 ||
                  sub_wave == 64,
              "attention_pool: sub_wave must be 0, 8, 16, 32 or 64");
  const long Q = s.W / s.V;
  s.sw = sub_wave ? (int)sub_wave : spanpool::sub_wave(Q);
  while (3L * s.sw < Q) s.sw *= 2;  // a lane owns at most 3 pieces
  s.np = (int)((Q + s.sw - 1) / s.sw);
  return s;
}

inline dim3 grid_for(long units, long max_blocks) {
  long cap = 8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  if (max_blocks > 0) cap = max_blocks;
  const long blocks = (units + SRX_ATTNPOOL_UNITS - 1) / SRX_ATTNPOOL_UNITS;
  return dim3((unsigned)std::max<long>(1, std::min<long>(blocks, cap)));
}

template <int N>
using ic = std::integral_constant<int, N>;

// f(T{}, ic<SW>{}, ic<NP>{}, bool_constant<HASK>{}) for the shape's variant
template <typename F>
void dispatch(const Shape& s, F&& f) {
#define SRX_AP_CASE(SW, NP)                                                    \
  if (s.sw == SW && s.np == NP) {                                              \
    if (s.bf16) {                                                              \
      if (s.hask) f(bf16_t{}, ic<SW>{}, ic<NP>{}, std::true_type{});           \
      else f(bf16_t{}, ic<SW>{}, ic<NP>{}, std::false_type{});                 \
    } else {                                                                   \
      if (s.hask) f(float{}, ic<SW>{}, ic<NP>{}, std::true_type{});            \
      else f(float{}, ic<SW>{}, ic<NP>{}, std::false_type{});                  \
    }                                                                          \
    return;                                                                    \
  }
  SRX_AP_CASE(8, 1) SRX_AP_CASE(8, 2) SRX_AP_CASE(8, 3)
  SRX_AP_CASE(16, 1) SRX_AP_CASE(16, 2) SRX_AP_CASE(16, 3)
  SRX_AP_CASE(32, 1) SRX_AP_CASE(32, 2) SRX_AP_CASE(32, 3)
  SRX_AP_CASE(64, 1) SRX_AP_CASE(64, 2) SRX_AP_CASE(64, 3)
#undef SRX_AP_CASE
  TORCH_CHECK(false, "attention_pool: no kernel variant");
}

}  // namespace attnpool

// -> (P [rows, W], P32 fp32 [D, W], lse fp32 [D], unit_offsets int32 [D + 1]);
// rows >= D, rows [D, rows) of P zero.  sub_wave: 0 = the power of two >= W /
// V, or 8 / 16 / 32 / 64 (raised until a lane owns at most 3 pieces);
// max_blocks > 0 caps the grid.
std::vector<at::Tensor> attention_pool_fwd(at::Tensor X, c10::optional<at::Tensor> keys,
                                           at::Tensor offsets, at::Tensor q, long rows,
                                           long sub_wave, long max_blocks) {
  const auto s = attnpool::check(X, keys, offsets, q, sub_wave);
  TORCH_CHECK(rows >= s.D && rows < (1L << 30), "attention_pool_fwd: D <= rows < 2^30");
  auto f32 = X.options().dtype(at::kFloat);
  auto P = at::empty({rows, s.W}, X.options());
  auto P32 = at::empty({s.D, s.W}, f32);
  auto lse = at::empty({s.D}, f32);
  // units per doc: max(1, ceil(len / CH)) of the clamped lengths, as the kernel
  // clamps them
  auto o = offsets.clamp(0, s.T);
  auto len = (o.slice(0, 1) - o.slice(0, 0, s.D)).clamp_min(0);
  auto n = at::div(len + (SRX_ATTNPOOL_CHUNK - 1), SRX_ATTNPOOL_CHUNK, "floor").clamp_min(1);
  auto uo = at::zeros({s.D + 1}, offsets.options());
  if (s.D > 0) uo.slice(0, 1).copy_(at::cumsum(n, 0));
  if (rows == 0) return {P, P32, lse, uo};
  auto ws_ml = at::empty({s.n_slots, 2}, f32);
  auto ws_acc = at::empty({s.n_slots, s.W}, f32);
  const long n_units = s.bound + (rows - s.D);
  const dim3 grid = attnpool::grid_for(n_units, max_blocks);
  auto stream = at::cuda::getCurrentCUDAStream();
  attnpool::dispatch(s, [&](auto t, auto sw, auto np, auto hask) {
    using TT = decltype(t);
    hipLaunchKernelGGL(
        (attention_pool_fwd_kernel<TT, decltype(sw)::value, decltype(np)::value,
                                   decltype(hask)::value>),
        grid, dim3(SRX_ATTNPOOL_THREADS), 0, stream, (const TT*)X.data_ptr(),
        (const TT*)(keys ? keys->data_ptr() : nullptr), offsets.data_ptr<int>(),
        uo.data_ptr<int>(), q.data_ptr<float>(), (TT*)P.data_ptr(),
        P32.data_ptr<float>(), lse.data_ptr<float>(), ws_ml.data_ptr<float>(),
        ws_acc.data_ptr<float>(), (int)s.D, (int)rows, (int)s.T, (int)s.W,
        (int)s.bound, (int)s.n_slots);
  });
  if (s.n_slots > 0 && s.D > 0) {  // some doc may have more than one unit
    const long wpb = SRX_ATTNPOOL_THREADS / SRX_WAVE;
    const dim3 mgrid = attnpool::grid_for((s.D + wpb - 1) / wpb * SRX_ATTNPOOL_UNITS,
                                          max_blocks);
#define SRX_AP_MERGE(TT)                                                       \
  hipLaunchKernelGGL((attention_pool_merge_kernel<TT>), mgrid,                 \
                     dim3(SRX_ATTNPOOL_THREADS), 0, stream, uo.data_ptr<int>(),\
                     ws_ml.data_ptr<float>(), ws_acc.data_ptr<float>(),        \
                     (TT*)P.data_ptr(), P32.data_ptr<float>(),                 \
                     lse.data_ptr<float>(), (int)s.D, (int)s.W, (int)s.n_slots)
    if (s.bf16) SRX_AP_MERGE(bf16_t); else SRX_AP_MERGE(float);
#undef SRX_AP_MERGE
  }
  return {P, P32, lse, uo};
}

// -> (dX [T, W], dK [T, W] or an empty tensor, dq fp32 [W]); every row of dX
// (and dK) is written
std::vector<at::Tensor> attention_pool_bwd(at::Tensor X, c10::optional<at::Tensor> keys,
                                           at::Tensor offsets, at::Tensor uo,
                                           at::Tensor q, at::Tensor dP, at::Tensor P32,
                                           at::Tensor lse, long sub_wave,
                                           long max_blocks) {
  const auto s = attnpool::check(X, keys, offsets, q, sub_wave);
  check_dev(uo);
  check_dev(dP);
  check_dev(P32);
  check_dev(lse);
  TORCH_CHECK(uo.scalar_type() == at::kInt && uo.dim() == 1 && uo.numel() == s.D + 1,
              "attention_pool_bwd: unit_offsets must be int32 [D + 1]");
  TORCH_CHECK(dP.scalar_type() == X.scalar_type() && dP.dim() == 2 &&
                  dP.size(0) >= s.D && dP.size(1) == s.W && aligned16(dP.data_ptr()),
              "attention_pool_bwd: dP must be [>= D, W] in X's dtype");
  TORCH_CHECK(P32.scalar_type() == at::kFloat && P32.dim() == 2 && P32.size(0) == s.D &&
                  P32.size(1) == s.W && lse.scalar_type() == at::kFloat &&
                  lse.dim() == 1 && lse.numel() == s.D && aligned16(P32.data_ptr()),
              "attention_pool_bwd: P32 must be fp32 [D, W] and lse fp32 [D]");
  auto f32 = X.options().dtype(at::kFloat);
  if (s.D == 0 || s.T == 0)
    return {at::zeros_like(X), s.hask ? at::zeros_like(X) : at::empty({0}, X.options()),
            at::zeros({s.W}, f32)};
  auto dX = at::empty_like(X);
  auto dK = s.hask ? at::empty_like(X) : at::empty({0}, X.options());
  const long n_blocks = (s.bound + SRX_ATTNPOOL_UNITS - 1) / SRX_ATTNPOOL_UNITS;
  auto dq_part = at::empty({n_blocks, s.W}, f32);
  auto dq = at::empty({s.W}, f32);
  const dim3 grid = attnpool::grid_for(s.bound, max_blocks);
  auto stream = at::cuda::getCurrentCUDAStream();
  attnpool::dispatch(s, [&](auto t, auto sw, auto np, auto hask) {
    using TT = decltype(t);
    hipLaunchKernelGGL(
        (attention_pool_bwd_kernel<TT, decltype(sw)::value, decltype(np)::value,
                                   decltype(hask)::value>),
        grid, dim3(SRX_ATTNPOOL_THREADS), 0, stream, (const TT*)X.data_ptr(),
        (const TT*)(keys ? keys->data_ptr() : nullptr), offsets.data_ptr<int>(),
        uo.data_ptr<int>(), q.data_ptr<float>(), (const TT*)dP.data_ptr(),
        P32.data_ptr<float>(), lse.data_ptr<float>(), (TT*)dX.data_ptr(),
        (TT*)(s.hask ? dK.data_ptr() : nullptr), dq_part.data_ptr<float>(), (int)s.D,
        (int)s.T, (int)s.W, (int)s.bound);
  });
  hipLaunchKernelGGL(attention_pool_dq_kernel, dim3((unsigned)((s.W + 15) / 16)),
                     dim3(SRX_ATTNPOOL_THREADS), 0, stream, dq_part.data_ptr<float>(),
                     dq.data_ptr<float>(), (int)n_blocks, (int)s.W);
  return {dX, dK, dq};
}

// ------------------------------------------------- SparseLinear (TextCatBOW)
// see srx_sparselinear.hip.h.  ids int64 [T], offsets int32 [D + 1], weight
// bf16 / fp32 [L, nO], L a power of two <= 2^24, nO <= 128, G <= 4.
namespace spl {

inline dim3 grid_for(long blocks, long max_blocks) {
  long cap = 8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  if (max_blocks > 0) cap = max_blocks;
  return dim3((unsigned)std::max<long>(1, std::min<long>(blocks, cap)));
}

inline int pow2_ceil(long x) {
  int p = 1;
  while (p < x) p <<= 1;
  return p;
}

// -> (T, D); 2 G T < 2^31 keeps every entry index in int32 range
inline std::pair<long, long> check_docs(const at::Tensor& ids, const at::Tensor& offsets,
                                        long G, long L) {
  check_dev(ids);
  check_dev(offsets);
  TORCH_CHECK(ids.scalar_type() == at::kLong && ids.dim() == 1,
              "sparse_linear: ids must be int64 [T]");
  TORCH_CHECK(offsets.scalar_type() == at::kInt && offsets.dim() == 1 &&
                  offsets.numel() >= 1,
              "sparse_linear: offsets must be int32 [D + 1]");
  TORCH_CHECK(G >= 1 && G <= 4, "sparse_linear: ngram_size must be in 1..4");
  TORCH_CHECK(L >= 1 && L <= (1L << 24) && (L & (L - 1)) == 0,
              "sparse_linear: length must be a power of two <= 2^24");
  const long T = ids.numel(), D = offsets.numel() - 1;
  TORCH_CHECK(2 * G * T < (1L << 31) && D < (1L << 31),
              "sparse_linear: 2 * ngram_size * T and D must be < 2^31");
  return {T, D};
}

}  // namespace spl

// int32 [nnz, 2]; occ_offsets int64 [D + 1] = prefix sum of the docs'
// occurrence counts, nnz its last element
at::Tensor ngram_buckets(at::Tensor ids, at::Tensor offsets, at::Tensor occ_offsets,
                         long nnz, long G, long L) {
  const auto [T, D] = spl::check_docs(ids, offsets, G, L);
  check_dev(occ_offsets);
  TORCH_CHECK(occ_offsets.scalar_type() == at::kLong && occ_offsets.dim() == 1 &&
                  occ_offsets.numel() == D + 1 && nnz >= 0 && nnz < (1L << 30),
              "ngram_buckets: occ_offsets must be int64 [D + 1], nnz < 2^30");
  auto out = at::empty({nnz, 2}, offsets.options());
  if (nnz == 0 || T == 0) return out;
  const dim3 grid = spl::grid_for((T + SRX_SPL_THREADS - 1) / SRX_SPL_THREADS, 0);
  hipLaunchKernelGGL(ngram_buckets_kernel, grid, dim3(SRX_SPL_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(), ids.data_ptr<int64_t>(),
                     offsets.data_ptr<int>(), occ_offsets.data_ptr<int64_t>(),
                     out.data_ptr<int>(), (int)D, (int)T, (int)G, (uint32_t)(L - 1),
                     nnz);
  return out;
}

// scores fp32 [D, nO].  sub_wave: 0 = from the mean occurrences per doc, or
// 8 / 16 / 32 / 64 (raised to the lanes a row needs); max_blocks > 0 caps
// the grid.
at::Tensor sparse_linear_fwd(at::Tensor ids, at::Tensor offsets, at::Tensor weight,
                             at::Tensor bias, long G, long sub_wave, long max_blocks) {
  check_dev(weight);
  check_dev(bias);
  TORCH_CHECK(weight.dim() == 2 && (weight.scalar_type() == at::kBFloat16 ||
                                    weight.scalar_type() == at::kFloat),
              "sparse_linear_fwd: weight must be bf16 or fp32 [L, nO]");
  const long L = weight.size(0), nO = weight.size(1);
  const auto [T, D] = spl::check_docs(ids, offsets, G, L);
  TORCH_CHECK(nO >= 1 && nO <= 128, "sparse_linear_fwd: nO must be in 1..128");
  TORCH_CHECK(bias.scalar_type() == at::kFloat && bias.dim() == 1 && bias.numel() == nO,
              "sparse_linear_fwd: bias must be fp32 [nO]");
  TORCH_CHECK(aligned16(weight.data_ptr()), "sparse_linear_fwd: weight not 16-byte aligned");
  TORCH_CHECK(sub_wave == 0 || sub_wave == 8 || sub_wave == 16 || sub_wave == 32 ||
                  sub_wave == 64,
              "sparse_linear_fwd: sub_wave must be 0, 8, 16, 32 or 64");
  auto scores = at::empty({D, nO}, weight.options().dtype(at::kFloat));
  if (D == 0) return scores;
  const bool bf16 = weight.scalar_type() == at::kBFloat16;
  int C = bf16 ? 8 : 4;
  while (nO % C) C >>= 1;
  const int CL = std::min(spl::pow2_ceil(nO / C), 64);
  long sw = sub_wave;
  if (sw == 0) {  // occurrences per doc ~ G tokens-per-doc, CL lanes each
    const long per_doc = std::max<long>(1, G * T / D) * CL;
    sw = std::min<long>(64, std::max<long>(8, spl::pow2_ceil(per_doc)));
  }
  sw = std::max<long>(sw, CL);
  const long per_block = (SRX_SPL_THREADS / SRX_WAVE) * (SRX_WAVE / sw);
  const dim3 grid = spl::grid_for((D + per_block - 1) / per_block, max_blocks);
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_SPL_FWD(TT, SW, CC)                                                \
  hipLaunchKernelGGL((sparse_linear_fwd_kernel<TT, SW, CC>), grid,             \
                     dim3(SRX_SPL_THREADS), 0, stream, ids.data_ptr<int64_t>(),\
                     offsets.data_ptr<int>(), (const TT*)weight.data_ptr(),    \
                     bias.data_ptr<float>(), scores.data_ptr<float>(), (int)D, \
                     (int)T, (int)G, (int)nO, (uint32_t)(L - 1), CL)
#define SRX_SPL_FWD_SW(TT, CC)                                                 \
  if (sw == 8) { SRX_SPL_FWD(TT, 8, CC); }                                     \
  else if (sw == 16) { SRX_SPL_FWD(TT, 16, CC); }                              \
  else if (sw == 32) { SRX_SPL_FWD(TT, 32, CC); }                              \
  else { SRX_SPL_FWD(TT, 64, CC); }
  if (bf16) {
    if (C == 8) { SRX_SPL_FWD_SW(bf16_t, 8) }
    else if (C == 4) { SRX_SPL_FWD_SW(bf16_t, 4) }
    else if (C == 2) { SRX_SPL_FWD_SW(bf16_t, 2) }
    else { SRX_SPL_FWD_SW(bf16_t, 1) }
  } else {
    if (C == 4) { SRX_SPL_FWD_SW(float, 4) }
    else if (C == 2) { SRX_SPL_FWD_SW(float, 2) }
    else { SRX_SPL_FWD_SW(float, 1) }
  }
#undef SRX_SPL_FWD_SW
#undef SRX_SPL_FWD
  return scores;
}

// int64 [2 G T]: (bucket << 32) | doc per entry, the sentinel where an
// n-gram would cross its doc's end
at::Tensor sparse_linear_keys(at::Tensor ids, at::Tensor offsets, long G, long L) {
  const auto [T, D] = spl::check_docs(ids, offsets, G, L);
  auto keys = at::empty({2 * G * T}, ids.options());
  if (T == 0) return keys;
  const dim3 grid = spl::grid_for((T + SRX_SPL_THREADS - 1) / SRX_SPL_THREADS, 0);
  hipLaunchKernelGGL(sparse_linear_keys_kernel, grid, dim3(SRX_SPL_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(), ids.data_ptr<int64_t>(),
                     offsets.data_ptr<int>(), keys.data_ptr<int64_t>(), (int)D,
                     (int)T, (int)G, (uint32_t)(L - 1));
  return keys;
}

// dWeight [L, nO] (bf16: as_bf16) from the SORTED keys and dScores fp32 [D, nO]
at::Tensor sparse_linear_bwd(at::Tensor sorted, at::Tensor dS, long L, bool as_bf16,
                             long max_blocks) {
  check_dev(sorted);
  check_dev(dS);
  TORCH_CHECK(sorted.scalar_type() == at::kLong && sorted.dim() == 1,
              "sparse_linear_bwd: sorted must be int64 [N]");
  TORCH_CHECK(dS.scalar_type() == at::kFloat && dS.dim() == 2,
              "sparse_linear_bwd: dScores must be fp32 [D, nO]");
  const long N = sorted.numel(), D = dS.size(0), nO = dS.size(1);
  TORCH_CHECK(nO >= 1 && nO <= 128, "sparse_linear_bwd: nO must be in 1..128");
  TORCH_CHECK(L >= 1 && L <= (1L << 24) && N < (1L << 31) && D < (1L << 31),
              "sparse_linear_bwd: L <= 2^24, N and D < 2^31");
  TORCH_CHECK(aligned16(dS.data_ptr()), "sparse_linear_bwd: dScores not 16-byte aligned");
  auto dW = at::zeros({L, nO}, dS.options().dtype(as_bf16 ? at::kBFloat16 : at::kFloat));
  if (N == 0 || D == 0) return dW;
  const long n_chunks = (N + SRX_SPL_CHUNK - 1) / SRX_SPL_CHUNK;
  auto cbucket = at::empty({n_chunks, 2}, dS.options().dtype(at::kInt));
  auto crow = at::empty({n_chunks, 2, nO}, dS.options());
  const long wpb = SRX_SPL_THREADS / SRX_WAVE;
  const dim3 grid = spl::grid_for((n_chunks + wpb - 1) / wpb, max_blocks);
  const dim3 fgrid = spl::grid_for(
      (2 * n_chunks * nO + SRX_SPL_THREADS - 1) / SRX_SPL_THREADS, max_blocks);
  const bool vec = nO % 4 == 0;
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_SPL_BWD(TT, VEC)                                                   \
  hipLaunchKernelGGL((sparse_linear_bwd_kernel<TT, VEC>), grid,                \
                     dim3(SRX_SPL_THREADS), 0, stream,                         \
                     sorted.data_ptr<int64_t>(), dS.data_ptr<float>(),         \
                     (TT*)dW.data_ptr(), cbucket.data_ptr<int>(),              \
                     crow.data_ptr<float>(), N, n_chunks, (int)D, (int)L,      \
                     (int)nO);                                                 \
  hipLaunchKernelGGL((sparse_linear_fixup_kernel<TT>), fgrid,                  \
                     dim3(SRX_SPL_THREADS), 0, stream, cbucket.data_ptr<int>(),\
                     crow.data_ptr<float>(), (TT*)dW.data_ptr(), 2 * n_chunks, \
                     (int)L, (int)nO)
  if (as_bf16) {
    if (vec) { SRX_SPL_BWD(bf16_t, true); } else { SRX_SPL_BWD(bf16_t, false); }
  } else {
    if (vec) { SRX_SPL_BWD(float, true); } else { SRX_SPL_BWD(float, false); }
  }
#undef SRX_SPL_BWD
  return dW;
}

}  // namespace

void bind_pool(py::module_& m) {
  m.def("span_pool_fwd", &span_pool_fwd, py::arg("X"), py::arg("starts"),
        py::arg("ends"), py::arg("rows"));
  m.def("span_pool_bwd", &span_pool_bwd, py::arg("dR"), py::arg("which"),
        py::arg("starts"), py::arg("ends"), py::arg("tok_offsets"),
        py::arg("tok_spans"));
  m.def("attention_pool_fwd", &attention_pool_fwd, py::arg("X"), py::arg("keys"),
        py::arg("offsets"), py::arg("q"), py::arg("rows"), py::arg("sub_wave") = 0,
        py::arg("max_blocks") = 0);
  m.def("attention_pool_bwd", &attention_pool_bwd, py::arg("X"), py::arg("keys"),
        py::arg("offsets"), py::arg("unit_offsets"), py::arg("q"), py::arg("dP"),
        py::arg("P32"), py::arg("lse"), py::arg("sub_wave") = 0,
        py::arg("max_blocks") = 0);
  m.attr("ATTENTION_POOL_CHUNK") = SRX_ATTNPOOL_CHUNK;
  m.def("ngram_buckets", &ngram_buckets, py::arg("ids"), py::arg("offsets"),
        py::arg("occ_offsets"), py::arg("nnz"), py::arg("ngram_size"),
        py::arg("length"));
  m.def("sparse_linear_fwd", &sparse_linear_fwd, py::arg("ids"), py::arg("offsets"),
        py::arg("weight"), py::arg("bias"), py::arg("ngram_size"),
        py::arg("sub_wave") = 0, py::arg("max_blocks") = 0);
  m.def("sparse_linear_keys", &sparse_linear_keys, py::arg("ids"),
        py::arg("offsets"), py::arg("ngram_size"), py::arg("length"));
  m.def("sparse_linear_bwd", &sparse_linear_bwd, py::arg("sorted"),
        py::arg("dScores"), py::arg("length"), py::arg("as_bf16"),
        py::arg("max_blocks") = 0);
}
