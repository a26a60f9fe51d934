// spacy_ray_amd._srx_hip — gfx950 kernel bindings (torch extension).
// Kernels live in the *.hip.h headers; this TU instantiates fp32 + bf16
// variants and exposes the op surface consumed by ops/api.py and
// parallel/engine.py.  Tested on-GPU against ops/torch_ref.py fp32.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <mutex>
#include <unordered_map>
#include <utility>
#include <vector>

#include "srx_common.hip.h"
#include "srx_elementwise.hip.h"
#include "srx_embed_parser.hip.h"
#include "srx_softmax_reduce.hip.h"
#include "srx_mwe.hip.h"
#include "srx_mixer.hip.h"
#include "srx_mwe_dw.hip.h"
#include "srx_staticvec.hip.h"
#include "srx_floret.hip.h"
#include "srx_vecloss.hip.h"
#include "srx_activations.hip.h"
#include "srx_attn.hip.h"

namespace {

constexpr int kBlock = 256;

inline int grid_for(long total, int per_thread = 1) {
  long blocks = (total + (long)kBlock * per_thread - 1) / ((long)kBlock * per_thread);
  return (int)std::min<long>(blocks, 16384);
}

inline void check_dev(const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "expected a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), "expected contiguous");
}

#define DISPATCH_F(dtype, ...)                                        \
  if ((dtype) == at::kFloat) {                                        \
    using scalar_t = float;                                           \
    constexpr int kVec = 4;                                           \
    __VA_ARGS__;                                                      \
  } else if ((dtype) == at::kBFloat16) {                              \
    using scalar_t = bf16_t;                                          \
    constexpr int kVec = 8;                                           \
    __VA_ARGS__;                                                      \
  } else {                                                            \
    TORCH_CHECK(false, "unsupported dtype (need f32 or bf16)");       \
  }

// --------------------------------------------------------------- seq2col
// starts/ends: per-token doc-boundary uint8 masks, computed ONCE per batch
// on the python side (a masked_select/nonzero here would device-sync on
// every call — measured as a 33 ms/step stall in the encoder stack).
at::Tensor seq2col_fwd(at::Tensor X, at::Tensor starts, at::Tensor ends) {
  check_dev(X);
  long nT = X.size(0);
  int W = (int)X.size(1);
  auto Y = at::empty({nT, 3L * W}, X.options());
  if (nT == 0) return Y;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(X.scalar_type(), {
    const int V = (W % kVec == 0) ? kVec : 1;
    long total = nT * 3L * (W / V);
    if (V == kVec)
      hipLaunchKernelGGL((seq2col_fwd_kernel<scalar_t, kVec>), dim3(grid_for(total)),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)X.data_ptr(), (scalar_t*)Y.data_ptr(),
                         starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(), nT, W);
    else
      hipLaunchKernelGGL((seq2col_fwd_kernel<scalar_t, 1>), dim3(grid_for(nT * 3L * W)),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)X.data_ptr(), (scalar_t*)Y.data_ptr(),
                         starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(), nT, W);
  });
  return Y;
}

at::Tensor seq2col_bwd(at::Tensor dY, at::Tensor starts, at::Tensor ends,
                       c10::optional<at::Tensor> residual = c10::nullopt) {
  check_dev(dY);
  long nT = dY.size(0);
  int W3 = (int)dY.size(1);
  int W = W3 / 3;
  auto dX = at::empty({nT, (long)W}, dY.options());
  if (nT == 0) return dX;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(dY.scalar_type(), {
    const scalar_t* res =
        residual ? (const scalar_t*)residual->data_ptr() : nullptr;
    const int V = (W % kVec == 0) ? kVec : 1;
    if (V == kVec)
      hipLaunchKernelGGL((seq2col_bwd_kernel<scalar_t, kVec>),
                         dim3(grid_for(nT * (W / kVec))), dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), (scalar_t*)dX.data_ptr(),
                         starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(),
                         res, nT, W);
    else
      hipLaunchKernelGGL((seq2col_bwd_kernel<scalar_t, 1>),
                         dim3(grid_for(nT * (long)W)), dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), (scalar_t*)dX.data_ptr(),
                         starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(),
                         res, nT, W);
  });
  return dX;
}

// ---------------------------------------------------------------- maxout
std::vector<at::Tensor> maxout_fwd(at::Tensor X) {
  check_dev(X);
  int P = (int)X.size(-2);
  int W = (int)X.size(-1);
  long N = X.numel() / ((long)P * W);
  auto sizes = X.sizes().vec();
  sizes.erase(sizes.end() - 2);
  auto Y = at::empty(sizes, X.options());
  auto which = at::empty(sizes, X.options().dtype(at::kByte));
  if (N == 0) return {Y, which};
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(X.scalar_type(), {
    const int V = (W % kVec == 0) ? kVec : 1;
    if (V == kVec)
      hipLaunchKernelGGL((maxout_fwd_kernel<scalar_t, kVec>),
                         dim3(grid_for(N * (W / kVec))), dim3(kBlock), 0, stream,
                         (const scalar_t*)X.data_ptr(), (scalar_t*)Y.data_ptr(),
                         which.data_ptr<uint8_t>(), N, P, W);
    else
      hipLaunchKernelGGL((maxout_fwd_kernel<scalar_t, 1>),
                         dim3(grid_for(N * (long)W)), dim3(kBlock), 0, stream,
                         (const scalar_t*)X.data_ptr(), (scalar_t*)Y.data_ptr(),
                         which.data_ptr<uint8_t>(), N, P, W);
  });
  return {Y, which};
}

at::Tensor maxout_bwd(at::Tensor dY, at::Tensor which, long P) {
  check_dev(dY);
  int W = (int)dY.size(-1);
  long N = dY.numel() / W;
  auto sizes = dY.sizes().vec();
  sizes.insert(sizes.end() - 1, P);
  auto dX = at::empty(sizes, dY.options());
  if (N == 0) return dX;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(dY.scalar_type(), {
    const int V = (W % kVec == 0) ? kVec : 1;
    long total = N * P * (W / (V == kVec ? kVec : 1));
    if (V == kVec)
      hipLaunchKernelGGL((maxout_bwd_kernel<scalar_t, kVec>), dim3(grid_for(total)),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), which.data_ptr<uint8_t>(),
                         (scalar_t*)dX.data_ptr(), N, (int)P, W);
    else
      hipLaunchKernelGGL((maxout_bwd_kernel<scalar_t, 1>), dim3(grid_for(N * P * (long)W)),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), which.data_ptr<uint8_t>(),
                         (scalar_t*)dX.data_ptr(), N, (int)P, W);
  });
  return dX;
}

// ------------------------------------------------------------- layernorm
std::vector<at::Tensor> layernorm_fwd(at::Tensor X, at::Tensor g, at::Tensor b, double eps) {
  check_dev(X);
  int W = (int)X.size(-1);
  long N = X.numel() / W;
  auto Y = at::empty_like(X);
  auto mu = at::empty({N}, X.options().dtype(at::kFloat));
  auto rstd = at::empty({N}, X.options().dtype(at::kFloat));
  if (N == 0) return {Y, mu, rstd};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = grid_for(N * SRX_WAVE);
  DISPATCH_F(X.scalar_type(), {
    if (W % (2 * SRX_WAVE) == 0)
      hipLaunchKernelGGL((layernorm_fwd_v2_kernel<scalar_t>), dim3(grid), dim3(kBlock), 0,
                         stream, (const scalar_t*)X.data_ptr(),
                         (const scalar_t*)g.data_ptr(), (const scalar_t*)b.data_ptr(),
                         (scalar_t*)Y.data_ptr(), mu.data_ptr<float>(),
                         rstd.data_ptr<float>(), N, W, (float)eps);
    else
      hipLaunchKernelGGL((layernorm_fwd_kernel<scalar_t>), dim3(grid), dim3(kBlock), 0,
                         stream, (const scalar_t*)X.data_ptr(),
                         (const scalar_t*)g.data_ptr(), (const scalar_t*)b.data_ptr(),
                         (scalar_t*)Y.data_ptr(), mu.data_ptr<float>(),
                         rstd.data_ptr<float>(), N, W, (float)eps);
  });
  return {Y, mu, rstd};
}

std::vector<at::Tensor> layernorm_bwd(at::Tensor dY, at::Tensor X, at::Tensor g,
                                      at::Tensor mu, at::Tensor rstd,
                                      bool deterministic = false) {
  check_dev(dY);
  int W = (int)X.size(-1);
  long N = X.numel() / W;
  auto dX = at::empty_like(X);
  auto acc_dt = deterministic ? at::kLong : at::kFloat;
  auto dg32 = at::zeros({W}, X.options().dtype(acc_dt));
  auto db32 = at::zeros({W}, X.options().dtype(acc_dt));
  auto stream = at::cuda::getCurrentCUDAStream();
  TORCH_CHECK(W <= SRX_LN_MAX_W, "layernorm width > ", SRX_LN_MAX_W);
  if (N > 0) {
    // cap the grid so each wave covers many rows: the dg/db column sums are
    // register-accumulated per wave with one atomic per column at the end.
    // Narrow layers (CNN W=96) keep a tight cap — extra blocks only
    // serialize on the few dg/db addresses; wide layers (trf W=768) spread
    // the atomics over 8x the columns and need more waves to fill 256 CUs
    // at large N (measured 2.0 ms/call at N=260k W=768 under the 1024 cap).
    // (re-measured r2: the old 1024 cap for narrow layers starved the
    // 1M-row encoder backward of parallelism — 0.73 ms/call at 10x off
    // bandwidth; per-wave register accumulation keeps the dg/db atomic
    // count at waves*W regardless, so more waves are safe)
    long cap = 4096;
    int grid = (int)std::min<long>((N + 3) / 4, cap);
    bool v2 = W % (2 * SRX_WAVE) == 0;
    DISPATCH_F(X.scalar_type(), {
      if (v2 && deterministic)
        hipLaunchKernelGGL((layernorm_bwd_v2_kernel<scalar_t, true>), dim3(grid),
                           dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                           (const scalar_t*)X.data_ptr(), (const scalar_t*)g.data_ptr(),
                           mu.data_ptr<float>(), rstd.data_ptr<float>(),
                           (scalar_t*)dX.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), N, W);
      else if (v2)
        hipLaunchKernelGGL((layernorm_bwd_v2_kernel<scalar_t, false>), dim3(grid),
                           dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                           (const scalar_t*)X.data_ptr(), (const scalar_t*)g.data_ptr(),
                           mu.data_ptr<float>(), rstd.data_ptr<float>(),
                           (scalar_t*)dX.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), N, W);
      else if (deterministic)
        hipLaunchKernelGGL((layernorm_bwd_kernel<scalar_t, true>), dim3(grid),
                           dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                           (const scalar_t*)X.data_ptr(), (const scalar_t*)g.data_ptr(),
                           mu.data_ptr<float>(), rstd.data_ptr<float>(),
                           (scalar_t*)dX.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), N, W);
      else
        hipLaunchKernelGGL((layernorm_bwd_kernel<scalar_t, false>), dim3(grid),
                           dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                           (const scalar_t*)X.data_ptr(), (const scalar_t*)g.data_ptr(),
                           mu.data_ptr<float>(), rstd.data_ptr<float>(),
                           (scalar_t*)dX.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), N, W);
    });
  }
  if (deterministic) {
    // fixed-point -> float (deterministic elementwise divide)
    auto s = 1.0 / 16777216.0;
    return {dX, (dg32.to(at::kFloat) * s).to(X.scalar_type()),
            (db32.to(at::kFloat) * s).to(X.scalar_type())};
  }
  return {dX, dg32.to(X.scalar_type()), db32.to(X.scalar_type())};
}

// ------------------------------------------------------------- hashembed
// out_/col_off: optional preallocated [nT, ldY] destination + column
// offset — the 4 attr tables write straight into their block of the
// concatenated embed matrix (no separate cat copy).
std::vector<at::Tensor> hashembed_fwd(at::Tensor table, at::Tensor ids, int64_t seed,
                                      c10::optional<at::Tensor> out_ = c10::nullopt,
                                      int64_t col_off = 0) {
  check_dev(table);
  check_dev(ids);
  TORCH_CHECK(ids.scalar_type() == at::kLong, "ids must be int64 (bit-cast uint64)");
  long nT = ids.size(0);
  int nrows = (int)table.size(0);
  int W = (int)table.size(1);
  at::Tensor Y;
  long ldY = W;
  char* yptr = nullptr;
  if (out_) {
    Y = *out_;
    TORCH_CHECK(Y.size(0) == nT && Y.scalar_type() == table.scalar_type());
    ldY = Y.size(1);
    yptr = (char*)Y.data_ptr() + col_off * Y.element_size();
  } else {
    Y = at::empty({nT, (long)W}, table.options());
    yptr = (char*)Y.data_ptr();
  }
  auto rows = at::empty({nT, 4}, table.options().dtype(at::kInt));
  if (nT == 0) return {Y, rows};
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(table.scalar_type(), {
    hipLaunchKernelGGL((hashembed_fwd_kernel<scalar_t>), dim3(grid_for(nT * SRX_WAVE)),
                       dim3(kBlock), 0, stream, (const scalar_t*)table.data_ptr(),
                       (const uint64_t*)ids.data_ptr<int64_t>(), (scalar_t*)yptr,
                       rows.data_ptr<int32_t>(), nT, nrows, W, ldY, (uint32_t)seed);
  });
  return {Y, rows};
}

at::Tensor hashembed_bwd(at::Tensor dY, at::Tensor rows, int64_t nrows) {
  check_dev(dY);
  long nT = dY.size(0);
  int W = (int)dY.size(1);
  auto dT32 = at::zeros({nrows, (long)W}, dY.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (nT > 0) {
    DISPATCH_F(dY.scalar_type(), {
      hipLaunchKernelGGL((hashembed_bwd_kernel<scalar_t>), dim3(grid_for(nT * SRX_WAVE)),
                         dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                         rows.data_ptr<int32_t>(), dT32.data_ptr<float>(), nT, W);
    });
  }
  return dT32.to(dY.scalar_type());
}

// All n tables in one launch (multi_hashembed_fwd_kernel): writes column
// blocks [col_off, col_off + n W) of X [nT, ldX] and returns rows [n, nT, 4]
// and the int32 sort keys [n, nT].  Fast path only — equal W across tables,
// W a multiple of 8, bf16 or fp32; the caller uses the per-table launches
// for anything else.
std::vector<at::Tensor> multi_hashembed_fwd(at::Tensor ids4,
                                            std::vector<at::Tensor> tables,
                                            std::vector<int64_t> seeds, at::Tensor X,
                                            int64_t col_off) {
  const int n = (int)tables.size();
  TORCH_CHECK(n >= 1 && n <= SRX_MHE_MAX_TABLES, "multi_hashembed_fwd: 1..",
              SRX_MHE_MAX_TABLES, " tables");
  TORCH_CHECK((int)seeds.size() == n, "multi_hashembed_fwd: one seed per table");
  TORCH_CHECK(ids4.is_cuda() && ids4.dim() == 2 && ids4.scalar_type() == at::kLong &&
                  ids4.size(1) >= n && (ids4.stride(1) == 1 || ids4.size(1) == 1),
              "ids4 must be a GPU int64 [T, >= n] row view");
  const long nT = ids4.size(0);
  const int W = (int)tables[0].size(1);
  const auto dtype = tables[0].scalar_type();
  TORCH_CHECK(W % 8 == 0, "multi_hashembed_fwd: W % 8 == 0");
  MultiHashTables tabs;
  for (int i = 0; i < SRX_MHE_MAX_TABLES; i++) {
    const at::Tensor& tb = tables[i < n ? i : 0];
    check_dev(tb);
    TORCH_CHECK(tb.dim() == 2 && tb.size(1) == W && tb.scalar_type() == dtype &&
                    tb.size(0) >= 1 && tb.size(0) < 2147483648L,
                "multi_hashembed_fwd: tables must share W and dtype");
    TORCH_CHECK((uintptr_t)tb.data_ptr() % 16 == 0, "table not 16-byte aligned");
    tabs.table[i] = tb.data_ptr();
    tabs.seed[i] = (uint32_t)seeds[i < n ? i : 0];
    tabs.nrows[i] = (int32_t)tb.size(0);
  }
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.is_contiguous() && X.size(0) == nT &&
                  X.scalar_type() == dtype,
              "X must be a contiguous GPU [T, ldX] matrix of the tables' dtype");
  const long ldX = X.size(1);
  TORCH_CHECK(col_off >= 0 && col_off + (long)n * W <= ldX,
              "multi_hashembed_fwd: column blocks outside X");
  auto rows = at::empty({(long)n, nT, 4L}, X.options().dtype(at::kInt));
  auto keys = at::empty({(long)n, nT}, X.options().dtype(at::kInt));
  if (nT == 0) return {rows, keys};
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(dtype, {
    const long items = nT * n * (W / kVec);
    TORCH_CHECK(items < 2147483648L, "multi_hashembed_fwd: T * n * W too large");
    TORCH_CHECK(ldX % kVec == 0 && col_off % kVec == 0 &&
                    (uintptr_t)X.data_ptr() % 16 == 0,
                "multi_hashembed_fwd: X blocks not 16-byte aligned");
    hipLaunchKernelGGL((multi_hashembed_fwd_kernel<scalar_t, kVec>),
                       dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       stream, tabs, (const uint64_t*)ids4.data_ptr<int64_t>(),
                       (scalar_t*)X.data_ptr() + col_off, rows.data_ptr<int32_t>(),
                       keys.data_ptr<int32_t>(), nT, n, W, (long)ids4.stride(0), ldX);
  });
  return {rows, keys};
}

// dT32 [R, W] fp32 (zero-initialised by the caller) += the HashEmbed table
// gradient of dY, tokens visited in `order` (the int64 argsort of the
// forward's sort keys, taken as torch returns it).  dY is a row view
// (innermost stride 1, any row stride).
void hashembed_bwd_merged(at::Tensor order, at::Tensor rows, at::Tensor dY,
                          at::Tensor dT32) {
  TORCH_CHECK(dY.is_cuda() && dY.dim() == 2 && dY.stride(1) == 1,
              "dY must be a GPU row view (innermost stride 1)");
  const long nT = dY.size(0);
  const int W = (int)dY.size(1);
  const long ldY = dY.stride(0);
  TORCH_CHECK(W >= 1 && W <= 1024, "hashembed_bwd_merged W <= 1024");
  TORCH_CHECK(nT < 2147483648L, "hashembed_bwd_merged T < 2^31");
  check_dev(order);
  check_dev(rows);
  check_dev(dT32);
  TORCH_CHECK(order.scalar_type() == at::kLong && order.numel() == nT,
              "order must be int64 [T]");
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.numel() == nT * 4 &&
                  (uintptr_t)rows.data_ptr() % 16 == 0,
              "rows must be int32 [T, 4], 16-byte aligned");
  TORCH_CHECK(dT32.scalar_type() == at::kFloat && dT32.dim() == 2 && dT32.size(1) == W,
              "dT32 must be fp32 [R, W]");
  if (nT == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  const long waves = (nT + 2 * SRX_WAVE - 1) / (2 * SRX_WAVE);
  const dim3 grid((unsigned)((waves * SRX_WAVE + kBlock - 1) / kBlock));
#define SRX_HE_MERGED(V_, NC_, U_)                                                  \
  hipLaunchKernelGGL((hashembed_bwd_merged_kernel<scalar_t, V_, NC_, U_>), grid,    \
                     dim3(kBlock), 0, stream, order.data_ptr<int64_t>(),            \
                     rows.data_ptr<int32_t>(), (const scalar_t*)dY.data_ptr(),      \
                     dT32.data_ptr<float>(), nT, W, ldY)
  DISPATCH_F(dY.scalar_type(), {
    (void)kVec;
    // paired accesses need every row piece aligned to 2 elements
    const bool pairs = W % 2 == 0 && ldY % 2 == 0 &&
                       (uintptr_t)dY.data_ptr() % (2 * sizeof(scalar_t)) == 0;
    if (pairs && W <= 128)
      SRX_HE_MERGED(2, 1, 8);
    else if (pairs)
      SRX_HE_MERGED(2, 8, 4);
    else
      SRX_HE_MERGED(1, 16, 2);
  });
#undef SRX_HE_MERGED
}

// ----------------------------------------------------- parser step score
std::vector<at::Tensor> parser_step_fwd(at::Tensor pre, at::Tensor feats, at::Tensor bias) {
  check_dev(pre);
  check_dev(feats);
  TORCH_CHECK(feats.scalar_type() == at::kLong, "feats must be int64");
  long S = feats.size(0);
  int nF = (int)feats.size(1);
  int HP = (int)pre.size(-1);
  int H = HP / 2;
  auto hidden = at::empty({S, (long)H}, pre.options());
  auto which = at::empty({S, (long)H}, pre.options().dtype(at::kByte));
  if (S == 0) return {hidden, which};
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(pre.scalar_type(), {
    hipLaunchKernelGGL((parser_step_fwd_kernel<scalar_t>), dim3(grid_for(S * SRX_WAVE)),
                       dim3(kBlock), 0, stream, (const scalar_t*)pre.data_ptr(),
                       feats.data_ptr<int64_t>(), (const scalar_t*)bias.data_ptr(),
                       (scalar_t*)hidden.data_ptr(), which.data_ptr<uint8_t>(), S, nF, H);
  });
  return {hidden, which};
}

// Accumulating variant: scatter this step's dPre gradient into ONE
// persistent fp32 buffer (no per-step [T+1,nF,HP] allocation/zeroing — the
// parser step loop calls this once per transition step; the caller zeroes
// the buffer once per batch and injects dPre back into autograd via a
// surrogate product).  Returns the per-step dBias (small, differentiable
// path for the bias parameter).
at::Tensor parser_step_bwd_into(at::Tensor dHidden, at::Tensor feats,
                                at::Tensor which, at::Tensor dPre32) {
  check_dev(dHidden);
  long S = feats.size(0);
  int nF = (int)feats.size(1);
  int HP = (int)dPre32.size(-1);
  int H = HP / 2;
  auto dBiasStep = at::zeros({(long)HP}, dHidden.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (S > 0) {
    DISPATCH_F(dHidden.scalar_type(), {
      hipLaunchKernelGGL((parser_step_bwd_kernel<scalar_t>),
                         dim3(grid_for(S * SRX_WAVE)), dim3(kBlock), 0, stream,
                         (const scalar_t*)dHidden.data_ptr(), feats.data_ptr<int64_t>(),
                         which.data_ptr<uint8_t>(), dPre32.data_ptr<float>(),
                         dBiasStep.data_ptr<float>(), S, nF, H);
    });
  }
  return dBiasStep.to(dHidden.scalar_type());
}

std::vector<at::Tensor> parser_step_bwd(at::Tensor dHidden, at::Tensor feats,
                                        at::Tensor which, int64_t T1, int64_t nF,
                                        int64_t HP) {
  check_dev(dHidden);
  long S = feats.size(0);
  int H = (int)HP / 2;
  auto dPre32 = at::zeros({T1, nF, HP}, dHidden.options().dtype(at::kFloat));
  auto dBias32 = at::zeros({HP}, dHidden.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (S > 0) {
    DISPATCH_F(dHidden.scalar_type(), {
      hipLaunchKernelGGL((parser_step_bwd_kernel<scalar_t>),
                         dim3(grid_for(S * SRX_WAVE)), dim3(kBlock), 0, stream,
                         (const scalar_t*)dHidden.data_ptr(), feats.data_ptr<int64_t>(),
                         which.data_ptr<uint8_t>(), dPre32.data_ptr<float>(),
                         dBias32.data_ptr<float>(), S, (int)nF, H);
    });
  }
  return {dPre32.to(dHidden.scalar_type()), dBias32.to(dHidden.scalar_type())};
}

// OUT (fp32 [No, W]) += segmented sums of SRC rows; dst_sorted must be sorted.
// OUT fp32: plain float atomics.  OUT int64: deterministic fixed-point
// (caller converts back with /2^24).
void seg_scatter_add(at::Tensor dst_sorted, at::Tensor src_idx, at::Tensor SRC,
                     at::Tensor OUT) {
  TORCH_CHECK(SRC.is_cuda() && SRC.dim() == 2 && SRC.stride(1) == 1,
              "SRC must be a CUDA row-view (innermost stride 1)");
  bool det = OUT.scalar_type() == at::kLong;
  TORCH_CHECK(det || OUT.scalar_type() == at::kFloat);
  TORCH_CHECK(dst_sorted.scalar_type() == at::kInt && src_idx.scalar_type() == at::kInt);
  long M = dst_sorted.numel();
  int W = (int)SRC.size(-1);
  long ldSRC = SRC.stride(0);
  TORCH_CHECK(W <= 1024, "seg_scatter_add W <= 1024");
  if (M == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  constexpr int CHUNK = 128;
  long waves = (M + CHUNK - 1) / CHUNK;
  int grid = (int)std::min<long>((waves * SRX_WAVE + kBlock - 1) / kBlock, 16384);
  DISPATCH_F(SRC.scalar_type(), {
    if (det)
      hipLaunchKernelGGL((seg_scatter_add_kernel<scalar_t, CHUNK, true>), dim3(grid),
                         dim3(kBlock), 0, stream, dst_sorted.data_ptr<int32_t>(),
                         src_idx.data_ptr<int32_t>(), (const scalar_t*)SRC.data_ptr(),
                         OUT.data_ptr(), M, W, ldSRC);
    else
      hipLaunchKernelGGL((seg_scatter_add_kernel<scalar_t, CHUNK, false>), dim3(grid),
                         dim3(kBlock), 0, stream, dst_sorted.data_ptr<int32_t>(),
                         src_idx.data_ptr<int32_t>(), (const scalar_t*)SRC.data_ptr(),
                         OUT.data_ptr(), M, W, ldSRC);
  });
}

at::Tensor action_select(at::Tensor scores, at::Tensor is_gold, at::Tensor valid) {
  check_dev(scores);
  long S = scores.size(0);
  int A = (int)scores.size(1);
  auto actions = at::empty({S}, scores.options().dtype(at::kInt));
  if (S == 0) return actions;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(scores.scalar_type(), {
    hipLaunchKernelGGL((action_select_kernel<scalar_t>), dim3(grid_for(S * SRX_WAVE)),
                       dim3(kBlock), 0, stream, (const scalar_t*)scores.data_ptr(),
                       is_gold.data_ptr<uint8_t>(), valid.data_ptr<uint8_t>(),
                       actions.data_ptr<int32_t>(), S, A);
  });
  return actions;
}

// ------------------------------------------------------------ fused Adam
// clip_scale: 0-dim fp32 DEVICE tensor (or empty for no clip) — keeping the
// scale on-device avoids a host sync per optimizer step.
void adam_step(at::Tensor grad, at::Tensor master, at::Tensor m, at::Tensor v,
               at::Tensor param_out, at::Tensor clip_scale, double lr, double beta1,
               double beta2, double eps, double wd, double bc1, double bc2) {
  check_dev(grad);
  long n = grad.numel();
  if (n == 0) return;
  const float* scale_ptr =
      clip_scale.numel() > 0 ? clip_scale.data_ptr<float>() : nullptr;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(grad.scalar_type(), {
    hipLaunchKernelGGL((adam_step_kernel<scalar_t>), dim3(grid_for(n, 4)), dim3(kBlock),
                       0, stream, (const scalar_t*)grad.data_ptr(),
                       master.data_ptr<float>(), m.data_ptr<float>(),
                       v.data_ptr<float>(), (scalar_t*)param_out.data_ptr(), n,
                       scale_ptr, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, (float)wd, (float)bc1, (float)bc2);
  });
}

// ------------------------------------------- transition-pipe batched ops
// Fused CE over ALL transition steps (the C++ loop's arenas): returns
// (loss_count fp32 [2], dScores) — dScores = softmax_over_valid - target,
// zero for invalid columns / unsupervised rows (see transition_ce_kernel).
std::vector<at::Tensor> transition_ce(at::Tensor scores, at::Tensor gold,
                                      at::Tensor valid,
                                      bool deterministic = false) {
  check_dev(scores);
  long N = scores.size(0);
  int A = (int)scores.size(1);
  auto dScores = at::empty_like(scores);
  auto loss = at::zeros({2}, scores.options().dtype(at::kFloat));
  auto colsum = at::zeros(
      {(long)A}, scores.options().dtype(deterministic ? at::kLong : at::kFloat));
  if (N == 0) return {loss, dScores, colsum.to(at::kFloat)};
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(scores.scalar_type(), {
    if (deterministic)
      hipLaunchKernelGGL((transition_ce_kernel<scalar_t, true>),
                         dim3(grid_for(N * SRX_WAVE)), dim3(kBlock), 0, stream,
                         (const scalar_t*)scores.data_ptr(),
                         gold.data_ptr<uint8_t>(), valid.data_ptr<uint8_t>(),
                         (scalar_t*)dScores.data_ptr(), loss.data_ptr<float>(),
                         colsum.data_ptr(), N, A);
    else
      hipLaunchKernelGGL((transition_ce_kernel<scalar_t, false>),
                         dim3(grid_for(N * SRX_WAVE)), dim3(kBlock), 0, stream,
                         (const scalar_t*)scores.data_ptr(),
                         gold.data_ptr<uint8_t>(), valid.data_ptr<uint8_t>(),
                         (scalar_t*)dScores.data_ptr(), loss.data_ptr<float>(),
                         colsum.data_ptr(), N, A);
  });
  if (deterministic)
    colsum = colsum.to(at::kFloat) * (1.0 / 16777216.0);
  return {loss, dScores, colsum};
}

// Batched dPre scatter over all steps: direct atomics for the near-uniform
// token destinations (packed-bf16 atomics when dPre is bf16 — halves the
// traffic and skips the fp32->bf16 convert of the whole buffer); the
// Zipf-hot PAD row and the bias column-sum are register-accumulated per
// wave into SEPARATE fp32 buffers.  Returns (dBias32 [HP], dPad32 [nF,HP]);
// the caller writes dPad into dPre's pad row.
std::vector<at::Tensor> dpre_scatter(at::Tensor dSummed, at::Tensor feats,
                                     at::Tensor dPre, int64_t pad_row) {
  check_dev(dSummed);
  TORCH_CHECK(feats.scalar_type() == at::kLong);
  long S = feats.size(0);
  int nF = (int)feats.size(1);
  int HP = (int)dPre.size(-1);
  TORCH_CHECK(HP <= 256, "dpre_scatter HP <= 256");
  TORCH_CHECK(nF <= 16, "dpre_scatter nF <= 16");
  int mode = dPre.scalar_type() == at::kBFloat16 ? 1
           : dPre.scalar_type() == at::kLong      ? 2
                                                  : 0;
  TORCH_CHECK(mode != 0 || dPre.scalar_type() == at::kFloat,
              "dPre must be bf16, fp32 or int64 (deterministic)");
  TORCH_CHECK(mode != 1 || HP % 2 == 0, "bf16 dPre needs even HP");
  auto acc_dt = mode == 2 ? at::kLong : at::kFloat;
  auto dBias32 = at::zeros({(long)HP}, dSummed.options().dtype(acc_dt));
  auto dPad32 = at::zeros({(long)nF, (long)HP}, dSummed.options().dtype(acc_dt));
  auto finish = [&](at::Tensor t) {
    return mode == 2 ? (t.to(at::kFloat) * (1.0 / 16777216.0)) : t;
  };
  if (S == 0) return {finish(dBias32), finish(dPad32)};
  auto stream = at::cuda::getCurrentCUDAStream();
  long waves = (S + 63) / 64;  // >=64 states per wave target
  int grid = (int)std::min<long>((waves * SRX_WAVE + kBlock - 1) / kBlock, 4096);
  grid = std::max(grid, 64);
  DISPATCH_F(dSummed.scalar_type(), {
    if (mode == 1)
      hipLaunchKernelGGL((dpre_scatter_kernel<scalar_t, 1>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)dSummed.data_ptr(),
                         feats.data_ptr<int64_t>(), dPre.data_ptr(),
                         dBias32.data_ptr(), dPad32.data_ptr(),
                         S, nF, HP, pad_row);
    else if (mode == 2)
      hipLaunchKernelGGL((dpre_scatter_kernel<scalar_t, 2>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)dSummed.data_ptr(),
                         feats.data_ptr<int64_t>(), dPre.data_ptr(),
                         dBias32.data_ptr(), dPad32.data_ptr(),
                         S, nF, HP, pad_row);
    else
      hipLaunchKernelGGL((dpre_scatter_kernel<scalar_t, 0>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)dSummed.data_ptr(),
                         feats.data_ptr<int64_t>(), dPre.data_ptr(),
                         dBias32.data_ptr(), dPad32.data_ptr(),
                         S, nF, HP, pad_row);
  });
  return {finish(dBias32), finish(dPad32)};
}

// Doc-major atomic-free variant (GPU-state-machine arenas): one block per
// doc, LDS accumulation, plain stores into an UNINITIALIZED dPre — see
// dpre_docmajor_kernel.  Same return contract as dpre_scatter.
std::vector<at::Tensor> dpre_scatter_docmajor(at::Tensor dSummed,
                                              at::Tensor feats, at::Tensor dPre,
                                              at::Tensor off, at::Tensor lens,
                                              int64_t pad_row, int64_t cap_mult,
                                              int64_t maxlen) {
  check_dev(dSummed);
  TORCH_CHECK(feats.scalar_type() == at::kLong);
  TORCH_CHECK(dPre.scalar_type() == dSummed.scalar_type(),
              "docmajor dPre accumulates in the compute dtype");
  int nF = (int)feats.size(1);
  int HP = (int)dPre.size(-1);
  long n_docs = off.size(0);
  TORCH_CHECK(HP % SRX_WAVE == 0 && HP <= 128, "docmajor needs HP in {64,128}");
  TORCH_CHECK(nF <= 16, "docmajor nF <= 16");
  size_t lds = (size_t)maxlen * HP * sizeof(float);
  TORCH_CHECK(lds <= 64 * 1024, "docmajor maxlen*HP too large for LDS");
  auto dBias32 = at::zeros({(long)HP}, dSummed.options().dtype(at::kFloat));
  auto dPad32 =
      at::zeros({(long)nF, (long)HP}, dSummed.options().dtype(at::kFloat));
  if (n_docs == 0) return {dBias32, dPad32};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = (int)std::min<long>(n_docs, 65535);
  DISPATCH_F(dSummed.scalar_type(), {
    hipLaunchKernelGGL((dpre_docmajor_kernel<scalar_t>),
                       dim3(grid, (unsigned)nF), dim3(256), lds, stream,
                       (const scalar_t*)dSummed.data_ptr(),
                       feats.data_ptr<int64_t>(),
                       (scalar_t*)dPre.data_ptr(),
                       dBias32.data_ptr<float>(), dPad32.data_ptr<float>(),
                       off.data_ptr<int32_t>(), lens.data_ptr<int32_t>(),
                       n_docs, pad_row, nF, HP, (int)cap_mult);
  });
  return {dBias32, dPad32};
}

// ----------------------------------------------------- activations
// Thinc's elementwise activation surface (mish/swish/gelu/clipped_linear
// — srx_activations.hip.h); OP codes shared with ops/api.py.
template <int OP>
static void act_launch(bool bwd, const at::Tensor& A, const at::Tensor& B,
                       at::Tensor& out, double slope, double offset, double lo,
                       double hi) {
  long n = out.numel();
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(out.scalar_type(), {
    constexpr int V = sizeof(scalar_t) == 2 ? 8 : 4;
    if (n % V == 0) {
      long chunks = n / V;
      if (bwd)
        hipLaunchKernelGGL((act_bwd_kernel<scalar_t, V, OP>),
                           dim3(grid_for(chunks)), dim3(kBlock), 0, stream,
                           (const scalar_t*)A.data_ptr(),
                           (const scalar_t*)B.data_ptr(),
                           (scalar_t*)out.data_ptr(), chunks, (float)slope,
                           (float)offset, (float)lo, (float)hi);
      else
        hipLaunchKernelGGL((act_fwd_kernel<scalar_t, V, OP>),
                           dim3(grid_for(chunks)), dim3(kBlock), 0, stream,
                           (const scalar_t*)A.data_ptr(),
                           (scalar_t*)out.data_ptr(), chunks, (float)slope,
                           (float)offset, (float)lo, (float)hi);
    } else {
      if (bwd)
        hipLaunchKernelGGL((act_bwd_kernel<scalar_t, 1, OP>),
                           dim3(grid_for(n)), dim3(kBlock), 0, stream,
                           (const scalar_t*)A.data_ptr(),
                           (const scalar_t*)B.data_ptr(),
                           (scalar_t*)out.data_ptr(), n, (float)slope,
                           (float)offset, (float)lo, (float)hi);
      else
        hipLaunchKernelGGL((act_fwd_kernel<scalar_t, 1, OP>),
                           dim3(grid_for(n)), dim3(kBlock), 0, stream,
                           (const scalar_t*)A.data_ptr(),
                           (scalar_t*)out.data_ptr(), n, (float)slope,
                           (float)offset, (float)lo, (float)hi);
    }
  });
}

at::Tensor act_fwd(at::Tensor X, int64_t op, double slope, double offset,
                   double lo, double hi) {
  check_dev(X);
  auto Xc = X.contiguous();
  auto Y = at::empty_like(Xc);
  if (Y.numel() == 0) return Y;
  at::Tensor dummy;
  switch (op) {
    case SRX_ACT_MISH: act_launch<SRX_ACT_MISH>(false, Xc, dummy, Y, slope, offset, lo, hi); break;
    case SRX_ACT_SWISH: act_launch<SRX_ACT_SWISH>(false, Xc, dummy, Y, slope, offset, lo, hi); break;
    case SRX_ACT_GELU: act_launch<SRX_ACT_GELU>(false, Xc, dummy, Y, slope, offset, lo, hi); break;
    default: act_launch<SRX_ACT_CLIPPED_LINEAR>(false, Xc, dummy, Y, slope, offset, lo, hi); break;
  }
  return Y;
}

at::Tensor act_bwd(at::Tensor dY, at::Tensor X, int64_t op, double slope,
                   double offset, double lo, double hi) {
  check_dev(dY);
  auto dYc = dY.contiguous();
  auto Xc = X.contiguous();
  auto dX = at::empty_like(Xc);
  if (dX.numel() == 0) return dX;
  switch (op) {
    case SRX_ACT_MISH: act_launch<SRX_ACT_MISH>(true, dYc, Xc, dX, slope, offset, lo, hi); break;
    case SRX_ACT_SWISH: act_launch<SRX_ACT_SWISH>(true, dYc, Xc, dX, slope, offset, lo, hi); break;
    case SRX_ACT_GELU: act_launch<SRX_ACT_GELU>(true, dYc, Xc, dX, slope, offset, lo, hi); break;
    default: act_launch<SRX_ACT_CLIPPED_LINEAR>(true, dYc, Xc, dX, slope, offset, lo, hi); break;
  }
  return dX;
}

// ----------------------------------------------------- attention softmax
// Fused masked softmax (+dropout) between the two attention bmm GEMMs —
// srx_attn.hip.h.  S/P/dS: [NH, L, L]; lens: [NH/heads] int32.
// Shared argument guards of the attention launchers: the kernels index raw
// pointers, so every operand must be a dense GPU tensor of the expected
// dtype and lens must hold exactly one int32 per window.
static void check_attn_lens(const at::Tensor& lens, long NH, int64_t heads) {
  TORCH_CHECK(lens.is_cuda() && lens.is_contiguous(),
              "attention: lens must be a contiguous GPU tensor");
  TORCH_CHECK(lens.scalar_type() == at::kInt, "attention: lens must be int32");
  TORCH_CHECK(heads > 0 && NH % heads == 0 && lens.numel() == NH / heads,
              "attention: lens must have NH / heads entries");
}

static void check_attn_like(const at::Tensor& t, const at::Tensor& ref,
                            const char* what) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), what,
              ": expected a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == ref.scalar_type() && t.sizes() == ref.sizes(),
              what, ": dtype/shape mismatch");
}

static void check_attn_lse(const at::Tensor& lse, long NH, int L) {
  TORCH_CHECK(lse.is_cuda() && lse.is_contiguous() &&
                  lse.scalar_type() == at::kFloat && lse.dim() == 2 &&
                  lse.size(0) == NH && lse.size(1) == L,
              "attention: lse must be a contiguous fp32 [NH, L] GPU tensor");
}

std::vector<at::Tensor> attn_softmax_fwd(at::Tensor S, at::Tensor lens,
                                         int64_t heads, double scale,
                                         double drop_p, int64_t seed) {
  check_dev(S);
  long NH = S.size(0);
  int L = (int)S.size(-1);
  TORCH_CHECK(L <= SRX_ATTN_MAX_L, "attn softmax: L <= 256");
  TORCH_CHECK(S.dim() == 3 && S.size(1) == L, "attn softmax: S must be [NH, L, L]");
  check_attn_lens(lens, NH, heads);
  auto P = at::empty_like(S);
  auto lse = at::empty({NH, (long)L}, S.options().dtype(at::kFloat));
  long n_rows = NH * L;
  if (n_rows == 0) return {P, lse};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = grid_for(n_rows * SRX_WAVE);
  float keep = 1.0f - (float)drop_p;
  DISPATCH_F(S.scalar_type(), {
    if (drop_p > 0.0)
      hipLaunchKernelGGL((attn_softmax_fwd_kernel<scalar_t, true>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)S.data_ptr(), (scalar_t*)P.data_ptr(),
                         lse.data_ptr<float>(), lens.data_ptr<int32_t>(),
                         n_rows, L, (int)heads, (float)scale, keep,
                         (unsigned long long)seed);
    else
      hipLaunchKernelGGL((attn_softmax_fwd_kernel<scalar_t, false>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)S.data_ptr(), (scalar_t*)P.data_ptr(),
                         lse.data_ptr<float>(), lens.data_ptr<int32_t>(),
                         n_rows, L, (int)heads, (float)scale, keep,
                         (unsigned long long)seed);
  });
  return {P, lse};
}

at::Tensor attn_softmax_bwd(at::Tensor S, at::Tensor lse, at::Tensor dPt,
                            at::Tensor lens, int64_t heads, double scale,
                            double drop_p, int64_t seed) {
  check_dev(S);
  long NH = S.size(0);
  int L = (int)S.size(-1);
  TORCH_CHECK(L <= SRX_ATTN_MAX_L, "attn softmax: L <= 256");
  TORCH_CHECK(S.dim() == 3 && S.size(1) == L, "attn softmax: S must be [NH, L, L]");
  check_attn_like(dPt, S, "attn softmax dP");
  check_attn_lse(lse, NH, L);
  check_attn_lens(lens, NH, heads);
  auto dS = at::empty_like(S);
  long n_rows = NH * L;
  if (n_rows == 0) return dS;
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = grid_for(n_rows * SRX_WAVE);
  float keep = 1.0f - (float)drop_p;
  DISPATCH_F(S.scalar_type(), {
    if (drop_p > 0.0)
      hipLaunchKernelGGL((attn_softmax_bwd_kernel<scalar_t, true>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)S.data_ptr(), lse.data_ptr<float>(),
                         (const scalar_t*)dPt.data_ptr(),
                         (scalar_t*)dS.data_ptr(), lens.data_ptr<int32_t>(),
                         n_rows, L, (int)heads, (float)scale, keep,
                         (unsigned long long)seed);
    else
      hipLaunchKernelGGL((attn_softmax_bwd_kernel<scalar_t, false>), dim3(grid),
                         dim3(kBlock), 0, stream,
                         (const scalar_t*)S.data_ptr(), lse.data_ptr<float>(),
                         (const scalar_t*)dPt.data_ptr(),
                         (scalar_t*)dS.data_ptr(), lens.data_ptr<int32_t>(),
                         n_rows, L, (int)heads, (float)scale, keep,
                         (unsigned long long)seed);
  });
  return dS;
}

// ------------------------------------------- fused flash-style attention
std::vector<at::Tensor> attn_fused_fwd(at::Tensor Q, at::Tensor K,
                                       at::Tensor V, at::Tensor lens,
                                       int64_t heads, double scale,
                                       double drop_p, int64_t seed) {
  check_dev(Q);
  TORCH_CHECK(Q.scalar_type() == at::kBFloat16, "fused attention is bf16-only");
  long NH = Q.size(0);
  int L = (int)Q.size(1);
  TORCH_CHECK((int)Q.size(2) == 64, "fused attention needs D == 64");
  TORCH_CHECK(L <= SRX_ATTN_FUSED_MAX_L, "fused attention: L <= 96");
  TORCH_CHECK(Q.dim() == 3, "fused attention: Q must be [NH, L, 64]");
  check_attn_like(K, Q, "fused attention K");
  check_attn_like(V, Q, "fused attention V");
  check_attn_lens(lens, NH, heads);
  auto O = at::empty_like(Q);
  auto lse = at::empty({NH, (long)L}, Q.options().dtype(at::kFloat));
  if (NH == 0) return {O, lse};
  int Lp = (L + 31) & ~31;
  int NT = Lp / 32;
  size_t lds =
      ((size_t)2 * Lp * SRX_ATTN_LDQ + 64 * SRX_ATTN_LDT + (size_t)Lp * SRX_ATTN_LDT) * 2;
  static std::once_flag attr_f;
  std::call_once(attr_f, []() {
#define AF_ATTR(DR, NTV)                                                      \
    (void)hipFuncSetAttribute((const void*)attn_fused_fwd_kernel<DR, NTV>,    \
                              hipFuncAttributeMaxDynamicSharedMemorySize,     \
                              100 * 1024)
    AF_ATTR(true, 1); AF_ATTR(true, 2); AF_ATTR(true, 3);
    AF_ATTR(false, 1); AF_ATTR(false, 2); AF_ATTR(false, 3);
#undef AF_ATTR
  });
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = (int)std::min<long>(NH, 65535);
  float keep = 1.0f - (float)drop_p;
#define LAUNCH_AF(DR, NTV)                                                    \
  hipLaunchKernelGGL((attn_fused_fwd_kernel<DR, NTV>), dim3(grid),            \
                     dim3(64 * NTV), lds, stream,                             \
                     (const bf16_t*)Q.data_ptr(), (const bf16_t*)K.data_ptr(),\
                     (const bf16_t*)V.data_ptr(), lens.data_ptr<int32_t>(),   \
                     (bf16_t*)O.data_ptr(), lse.data_ptr<float>(), NH, L,     \
                     (int)heads, (float)scale, keep, (unsigned long long)seed)
  if (drop_p > 0.0) {
    if (NT == 1) LAUNCH_AF(true, 1); else if (NT == 2) LAUNCH_AF(true, 2); else LAUNCH_AF(true, 3);
  } else {
    if (NT == 1) LAUNCH_AF(false, 1); else if (NT == 2) LAUNCH_AF(false, 2); else LAUNCH_AF(false, 3);
  }
#undef LAUNCH_AF
  return {O, lse};
}

std::vector<at::Tensor> attn_fused_bwd(at::Tensor Q, at::Tensor K,
                                       at::Tensor V, at::Tensor dO,
                                       at::Tensor lse, at::Tensor lens,
                                       int64_t heads, double scale,
                                       double drop_p, int64_t seed) {
  check_dev(Q);
  TORCH_CHECK(Q.scalar_type() == at::kBFloat16, "fused attention is bf16-only");
  TORCH_CHECK(Q.dim() == 3 && Q.size(2) == 64, "fused attention needs D == 64");
  long NH = Q.size(0);
  int L = (int)Q.size(1);
  TORCH_CHECK(L <= SRX_ATTN_FUSED_MAX_L, "fused attention: L <= 96");
  check_attn_like(K, Q, "fused attention K");
  check_attn_like(V, Q, "fused attention V");
  check_attn_like(dO, Q, "fused attention dO");
  check_attn_lse(lse, NH, L);
  check_attn_lens(lens, NH, heads);
  auto dQ = at::empty_like(Q);
  auto dK = at::empty_like(Q);
  auto dV = at::empty_like(Q);
  if (NH == 0) return {dQ, dK, dV};
  int Lp = (L + 31) & ~31;
  int NT = Lp / 32;
  size_t lds = ((size_t)4 * Lp * SRX_ATTN_LDQ + (size_t)3 * 64 * SRX_ATTN_LDT +
                (size_t)2 * Lp * SRX_ATTN_LDT) * 2;
  static std::once_flag attr_b;
  std::call_once(attr_b, []() {
#define AB_ATTR(DR, NTV)                                                      \
    (void)hipFuncSetAttribute((const void*)attn_fused_bwd_kernel<DR, NTV>,    \
                              hipFuncAttributeMaxDynamicSharedMemorySize,     \
                              144 * 1024)
    AB_ATTR(true, 1); AB_ATTR(true, 2); AB_ATTR(true, 3);
    AB_ATTR(false, 1); AB_ATTR(false, 2); AB_ATTR(false, 3);
#undef AB_ATTR
  });
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = (int)std::min<long>(NH, 65535);
  float keep = 1.0f - (float)drop_p;
#define LAUNCH_AB(DR, NTV)                                                    \
  hipLaunchKernelGGL((attn_fused_bwd_kernel<DR, NTV>), dim3(grid),            \
                     dim3(64 * NTV), lds, stream,                             \
                     (const bf16_t*)Q.data_ptr(), (const bf16_t*)K.data_ptr(),\
                     (const bf16_t*)V.data_ptr(), (const bf16_t*)dO.data_ptr(),\
                     lse.data_ptr<float>(), lens.data_ptr<int32_t>(),         \
                     (bf16_t*)dQ.data_ptr(), (bf16_t*)dK.data_ptr(),          \
                     (bf16_t*)dV.data_ptr(), NH, L, (int)heads,               \
                     (float)scale, keep, (unsigned long long)seed)
  if (drop_p > 0.0) {
    if (NT == 1) LAUNCH_AB(true, 1); else if (NT == 2) LAUNCH_AB(true, 2); else LAUNCH_AB(true, 3);
  } else {
    if (NT == 1) LAUNCH_AB(false, 1); else if (NT == 2) LAUNCH_AB(false, 2); else LAUNCH_AB(false, 3);
  }
#undef LAUNCH_AB
  return {dQ, dK, dV};
}

// ----------------------------------------------------- dropout mask
at::Tensor dropout_mask(at::Tensor like, double p, int64_t seed, int64_t offset) {
  check_dev(like);
  auto out = at::empty_like(like);
  long n = out.numel();
  if (n == 0 || p <= 0.0) {
    out.fill_(1.0);
    return out;
  }
  float keep = 1.0f - (float)p;
  float scale = 1.0f / keep;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(like.scalar_type(), {
    hipLaunchKernelGGL((dropout_mask_kernel<scalar_t>), dim3(grid_for(n, 4)),
                       dim3(kBlock), 0, stream, (scalar_t*)out.data_ptr(), n,
                       keep, scale, (unsigned long long)seed,
                       (unsigned long long)offset);
  });
  return out;
}

// ------------------------------------------------------- softmax + CE
// returns (loss_and_count fp32 [2], dScores) — dScores = softmax - onehot
// (unnormalized; the python wrapper divides by the valid count).
std::vector<at::Tensor> softmax_ce(at::Tensor scores, at::Tensor gold) {
  check_dev(scores);
  TORCH_CHECK(gold.scalar_type() == at::kLong);
  long N = scores.size(0);
  int C = (int)scores.size(1);
  auto dScores = at::empty_like(scores);
  auto loss = at::zeros({2}, scores.options().dtype(at::kFloat));
  if (N == 0) return {loss, dScores};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = (int)std::min<long>((N + 3) / 4, 2048);
  DISPATCH_F(scores.scalar_type(), {
    hipLaunchKernelGGL((softmax_ce_kernel<scalar_t>), dim3(grid), dim3(kBlock), 0,
                       stream, (const scalar_t*)scores.data_ptr(),
                       gold.data_ptr<int64_t>(), (scalar_t*)dScores.data_ptr(),
                       loss.data_ptr<float>(), N, C);
  });
  return {loss, dScores};
}

// ---------------------------------------------- segmented reductions
std::vector<at::Tensor> reduce_ragged(at::Tensor X, at::Tensor offsets, int64_t mode) {
  check_dev(X);
  long N = offsets.size(0) - 1;
  int W = (int)X.size(1);
  auto out = at::empty({N, (long)W}, X.options());
  auto argmax = mode == 2 ? at::empty({N, (long)W}, X.options().dtype(at::kInt))
                          : at::empty({0}, X.options().dtype(at::kInt));
  if (N == 0) return {out, argmax};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = grid_for(N * SRX_WAVE);
  DISPATCH_F(X.scalar_type(), {
    if (mode == 0)
      hipLaunchKernelGGL((reduce_ragged_kernel<scalar_t, 0>), dim3(grid), dim3(kBlock),
                         0, stream, (const scalar_t*)X.data_ptr(),
                         offsets.data_ptr<int32_t>(), (scalar_t*)out.data_ptr(),
                         nullptr, N, W);
    else if (mode == 1)
      hipLaunchKernelGGL((reduce_ragged_kernel<scalar_t, 1>), dim3(grid), dim3(kBlock),
                         0, stream, (const scalar_t*)X.data_ptr(),
                         offsets.data_ptr<int32_t>(), (scalar_t*)out.data_ptr(),
                         nullptr, N, W);
    else
      hipLaunchKernelGGL((reduce_ragged_kernel<scalar_t, 2>), dim3(grid), dim3(kBlock),
                         0, stream, (const scalar_t*)X.data_ptr(),
                         offsets.data_ptr<int32_t>(), (scalar_t*)out.data_ptr(),
                         argmax.data_ptr<int32_t>(), N, W);
  });
  return {out, argmax};
}

at::Tensor reduce_ragged_bwd(at::Tensor dY, at::Tensor doc_of, at::Tensor offsets,
                             int64_t Ttot, int64_t mode) {
  check_dev(dY);
  int W = (int)dY.size(1);
  auto dX = at::empty({Ttot, (long)W}, dY.options());
  if (Ttot == 0) return dX;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(dY.scalar_type(), {
    if (mode == 0)
      hipLaunchKernelGGL((reduce_ragged_bwd_kernel<scalar_t, 0>),
                         dim3(grid_for(Ttot * (long)W)), dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), doc_of.data_ptr<int32_t>(),
                         offsets.data_ptr<int32_t>(), (scalar_t*)dX.data_ptr(), Ttot, W);
    else
      hipLaunchKernelGGL((reduce_ragged_bwd_kernel<scalar_t, 1>),
                         dim3(grid_for(Ttot * (long)W)), dim3(kBlock), 0, stream,
                         (const scalar_t*)dY.data_ptr(), doc_of.data_ptr<int32_t>(),
                         offsets.data_ptr<int32_t>(), (scalar_t*)dX.data_ptr(), Ttot, W);
  });
  return dX;
}

at::Tensor reduce_max_bwd(at::Tensor dY, at::Tensor argmax, int64_t Ttot) {
  check_dev(dY);
  long N = dY.size(0);
  int W = (int)dY.size(1);
  auto dX = at::zeros({Ttot, (long)W}, dY.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(dY.scalar_type(), {
    hipLaunchKernelGGL((reduce_max_bwd_kernel<scalar_t>), dim3(grid_for(N * (long)W)),
                       dim3(kBlock), 0, stream, (const scalar_t*)dY.data_ptr(),
                       argmax.data_ptr<int32_t>(), (scalar_t*)dX.data_ptr(), N, W);
  });
  return dX;
}

// ----------------------------------------- fused MWE backward stage 1
// (dropmask x dY -> LN bwd -> maxout scatter) + dg/db/dbias column sums in
// ONE kernel; see mwe_bwd_stage1_kernel.
std::vector<at::Tensor> mwe_bwd_stage1(at::Tensor dY,
                                       c10::optional<at::Tensor> dropmask,
                                       at::Tensor Mout, at::Tensor g,
                                       at::Tensor mu, at::Tensor rstd,
                                       at::Tensor which,
                                       bool deterministic = false) {
  check_dev(dY);
  long N = dY.size(0);
  int W = (int)dY.size(1);
  TORCH_CHECK(W <= 256, "mwe_bwd_stage1 W <= 256");
  auto dPre = at::empty({N, 3L * W}, dY.options());
  auto acc_dt = deterministic ? at::kLong : at::kFloat;
  auto dg32 = at::zeros({W}, dY.options().dtype(acc_dt));
  auto db32 = at::zeros({W}, dY.options().dtype(acc_dt));
  auto dbias32 = at::zeros({3L * W}, dY.options().dtype(acc_dt));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (N > 0) {
    int grid = (int)std::min<long>((N + 3) / 4, 4096);
    DISPATCH_F(dY.scalar_type(), {
      const scalar_t* mask =
          dropmask ? (const scalar_t*)dropmask->data_ptr() : nullptr;
      if (deterministic)
        hipLaunchKernelGGL((mwe_bwd_stage1_kernel<scalar_t, true>), dim3(grid),
                           dim3(kBlock), 0, stream,
                           (const scalar_t*)dY.data_ptr(), mask,
                           (const scalar_t*)Mout.data_ptr(),
                           (const scalar_t*)g.data_ptr(), mu.data_ptr<float>(),
                           rstd.data_ptr<float>(), which.data_ptr<uint8_t>(),
                           (scalar_t*)dPre.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), dbias32.data_ptr(), N, W);
      else
        hipLaunchKernelGGL((mwe_bwd_stage1_kernel<scalar_t, false>), dim3(grid),
                           dim3(kBlock), 0, stream,
                           (const scalar_t*)dY.data_ptr(), mask,
                           (const scalar_t*)Mout.data_ptr(),
                           (const scalar_t*)g.data_ptr(), mu.data_ptr<float>(),
                           rstd.data_ptr<float>(), which.data_ptr<uint8_t>(),
                           (scalar_t*)dPre.data_ptr(), dg32.data_ptr(),
                           db32.data_ptr(), dbias32.data_ptr(), N, W);
    });
  }
  if (deterministic) {
    double s = 1.0 / 16777216.0;
    return {dPre, (dg32.to(at::kFloat) * s), (db32.to(at::kFloat) * s),
            (dbias32.to(at::kFloat) * s)};
  }
  return {dPre, dg32, db32, dbias32};
}

// ------------------------------------------------ fused MWE layer (MFMA)
template <int W>
void launch_mwe(const at::Tensor& X, const at::Tensor& Wt, const at::Tensor& bias,
                const at::Tensor& g, const at::Tensor& b, const at::Tensor& starts,
                const at::Tensor& ends, const c10::optional<at::Tensor>& dropmask,
                at::Tensor& Y, at::Tensor& Mout,
                at::Tensor& which, at::Tensor& mu, at::Tensor& rstd, long T,
                double eps, hipStream_t stream) {
  using C = MweCfg<W, false>;
  // X halo image + double-buffered B chunks + LN partials / row stats
  // (77 KB at W=96 -> two 6-wave workgroups per CU; 102 KB at W=128 -> one
  // 8-wave workgroup)
  size_t lds_bytes = (size_t)(C::A_ELEMS + C::B_ELEMS) * sizeof(bf16_t) +
                     (size_t)(2 * C::NW * C::MT + 2 * C::MT) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_layer_fwd_kernel<W>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mwe_layer_fwd_kernel<W>), grid, dim3(C::NT), lds_bytes,
                     stream, (const bf16_t*)X.data_ptr(), (const bf16_t*)Wt.data_ptr(),
                     (const bf16_t*)bias.data_ptr(), (const bf16_t*)g.data_ptr(),
                     (const bf16_t*)b.data_ptr(), starts.data_ptr<uint8_t>(),
                     ends.data_ptr<uint8_t>(),
                     dropmask ? (const bf16_t*)dropmask->data_ptr() : nullptr,
                     (bf16_t*)Y.data_ptr(),
                     (bf16_t*)Mout.data_ptr(), which.data_ptr<uint8_t>(),
                     mu.data_ptr<float>(), rstd.data_ptr<float>(), T, (float)eps);
}

std::vector<at::Tensor> mwe_layer_fwd(at::Tensor X, at::Tensor Wt, at::Tensor bias,
                                      at::Tensor g, at::Tensor b, at::Tensor starts,
                                      at::Tensor ends,
                                      c10::optional<at::Tensor> dropmask, double eps) {
  check_dev(X);
  TORCH_CHECK(X.scalar_type() == at::kBFloat16, "mwe_layer is bf16-only");
  long T = X.size(0);
  int W = (int)X.size(1);
  TORCH_CHECK(W == 96 || W == 128, "mwe_layer supports W in {96,128}");
  TORCH_CHECK(T % 64 == 0, "mwe_layer needs T % 64 == 0 (TokenBatch pads)");
  TORCH_CHECK(Wt.size(0) == 3 * W && Wt.size(1) == 3 * W, "weight must be [3W,3W]");
  auto Y = at::empty_like(X);
  auto Mout = at::empty_like(X);
  auto which = at::empty({T, (long)W}, X.options().dtype(at::kByte));
  auto mu = at::empty({T}, X.options().dtype(at::kFloat));
  auto rstd = at::empty({T}, X.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (T > 0) {
    if (W == 96)
      launch_mwe<96>(X, Wt, bias, g, b, starts, ends, dropmask, Y, Mout, which, mu,
                     rstd, T, eps, stream);
    else
      launch_mwe<128>(X, Wt, bias, g, b, starts, ends, dropmask, Y, Mout, which, mu,
                      rstd, T, eps, stream);
  }
  return {Y, Mout, which, mu, rstd};
}

// ------------------------------------------------ fused MWE backward dX
template <int W>
void launch_mwe_bwd_dx(const at::Tensor& dPre, const at::Tensor& WT,
                       const at::Tensor& starts, const at::Tensor& ends,
                       const at::Tensor& dY, at::Tensor& dX, long T,
                       hipStream_t stream) {
  using C = MweCfg<W, true>;
  // dPre halo image (K = 3W) + double-buffered B chunks: 117 KB at W=96,
  // 152 KB at W=128 -> one workgroup per CU
  size_t lds_bytes = (size_t)(C::A_ELEMS + C::B_ELEMS) * sizeof(bf16_t);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_bwd_dx_kernel<W>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mwe_bwd_dx_kernel<W>), grid, dim3(C::NT), lds_bytes, stream,
                     (const bf16_t*)dPre.data_ptr(), (const bf16_t*)WT.data_ptr(),
                     starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(),
                     (const bf16_t*)dY.data_ptr(), (bf16_t*)dX.data_ptr(), T);
}

// dX = dY + seq2col_bwd(dPre @ weight) in one kernel (no [T,3W] product,
// no atomics); see mwe_bwd_dx_kernel.
at::Tensor mwe_bwd_dx(at::Tensor dPre, at::Tensor weight, at::Tensor starts,
                      at::Tensor ends, at::Tensor dY) {
  check_dev(dPre);
  check_dev(dY);
  TORCH_CHECK(weight.is_cuda(), "expected a GPU tensor");
  TORCH_CHECK(dPre.scalar_type() == at::kBFloat16 &&
                  weight.scalar_type() == at::kBFloat16 &&
                  dY.scalar_type() == at::kBFloat16,
              "mwe_bwd_dx is bf16-only");
  TORCH_CHECK(dPre.dim() == 2 && dY.dim() == 2 && weight.dim() == 2,
              "mwe_bwd_dx expects 2-d tensors");
  long T = dY.size(0);
  int W = (int)dY.size(1);
  TORCH_CHECK(W == 96 || W == 128, "mwe_bwd_dx supports W in {96,128}");
  TORCH_CHECK(T % 64 == 0, "mwe_bwd_dx needs T % 64 == 0 (TokenBatch pads)");
  TORCH_CHECK(dPre.size(0) == T && dPre.size(1) == 3 * W, "dPre must be [T,3W]");
  TORCH_CHECK(weight.size(0) == 3 * W && weight.size(1) == 3 * W,
              "weight must be [3W,3W]");
  TORCH_CHECK(starts.numel() == T && ends.numel() == T,
              "starts/ends must have T entries");
  auto dX = at::empty_like(dY);
  if (T == 0) return dX;
  // k-contiguous B rows: section s, output column n -> WT[sW + n, :]
  auto WT = weight.t().contiguous();
  auto stream = at::cuda::getCurrentCUDAStream();
  if (W == 96)
    launch_mwe_bwd_dx<96>(dPre, WT, starts, ends, dY, dX, T, stream);
  else
    launch_mwe_bwd_dx<128>(dPre, WT, starts, ends, dY, dX, T, stream);
  return dX;
}

// per-tile column-sum rows [n, ncols] -> one row: 64 rows per block per
// level, added in row order (mwe_colsum_kernel)
at::Tensor mwe_fold_partials(at::Tensor part, int ncols, hipStream_t stream) {
  long n = part.size(0);
  const int R = 64;
  do {
    long nb = (n + R - 1) / R;
    auto out = at::empty({nb, (long)ncols}, part.options());
    hipLaunchKernelGGL(mwe_colsum_kernel, dim3((unsigned)nb, (ncols + 63) / 64),
                       dim3(64), 0, stream, part.data_ptr<float>(),
                       out.data_ptr<float>(), n, R, ncols);
    part = out;
    n = nb;
  } while (n > 1);
  return part.view({(long)ncols});
}

// ------------------------------------- fused MWE backward (stage 1 + dX)
template <int W, bool COMPACT>
void launch_mwe_bwd_fused(const at::Tensor& dY,
                          const c10::optional<at::Tensor>& dropmask,
                          const at::Tensor& Mout, const at::Tensor& g,
                          const at::Tensor& mu, const at::Tensor& rstd,
                          const at::Tensor& which, const at::Tensor& WT,
                          const at::Tensor& starts, const at::Tensor& ends,
                          at::Tensor& dPre, at::Tensor& dX, at::Tensor& partials,
                          long T, hipStream_t stream) {
  using C = MweCfg<W, true>;
  // the dX kernel's LDS: dPre halo image + double-buffered B chunks; the
  // epilogue tiles and the column-sum partials reuse both regions
  size_t lds_bytes = (size_t)(C::A_ELEMS + C::B_ELEMS) * sizeof(bf16_t);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_bwd_fused_kernel<W, COMPACT>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mwe_bwd_fused_kernel<W, COMPACT>), grid, dim3(C::NT), lds_bytes,
                     stream, (const bf16_t*)dY.data_ptr(),
                     dropmask ? (const bf16_t*)dropmask->data_ptr() : nullptr,
                     (const bf16_t*)Mout.data_ptr(), (const bf16_t*)g.data_ptr(),
                     mu.data_ptr<float>(), rstd.data_ptr<float>(),
                     which.data_ptr<uint8_t>(), (const bf16_t*)WT.data_ptr(),
                     starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(),
                     (bf16_t*)dPre.data_ptr(), (bf16_t*)dX.data_ptr(),
                     partials.data_ptr<float>(), T);
}

// mwe_bwd_stage1 + mwe_bwd_dx in one kernel: dPre is computed per 128-row
// tile straight into the dX GEMM's LDS image and written to memory once
// (for the dW GEMM), never read back.  The column sums leave as one fp32
// row per tile and are added in a fixed order (no atomics): the same
// kernel serves SRX_DETERMINISTIC.  Returns {dPre, dX, dg32, db32, dbias32}.
// compact: the first output is dM [T, W] (dPre[t, which[t,c] W + c], the
// input of mwe_bwd_dw) instead of the expanded dPre [T, 3W]; the others are
// bit-identical.
std::vector<at::Tensor> mwe_bwd_fused(at::Tensor dY,
                                      c10::optional<at::Tensor> dropmask,
                                      at::Tensor Mout, at::Tensor g,
                                      at::Tensor mu, at::Tensor rstd,
                                      at::Tensor which, at::Tensor weight,
                                      at::Tensor starts, at::Tensor ends,
                                      bool compact) {
  check_dev(dY);
  check_dev(Mout);
  check_dev(g);
  check_dev(mu);
  check_dev(rstd);
  check_dev(which);
  check_dev(starts);
  check_dev(ends);
  TORCH_CHECK(weight.is_cuda(), "expected a GPU tensor");
  TORCH_CHECK(dY.scalar_type() == at::kBFloat16 &&
                  Mout.scalar_type() == at::kBFloat16 &&
                  g.scalar_type() == at::kBFloat16 &&
                  weight.scalar_type() == at::kBFloat16,
              "mwe_bwd_fused is bf16-only");
  TORCH_CHECK(dY.dim() == 2 && weight.dim() == 2,
              "mwe_bwd_fused expects 2-d tensors");
  long T = dY.size(0);
  int W = (int)dY.size(1);
  TORCH_CHECK(W == 96 || W == 128, "mwe_bwd_fused supports W in {96,128}");
  TORCH_CHECK(T % 64 == 0, "mwe_bwd_fused needs T % 64 == 0 (TokenBatch pads)");
  TORCH_CHECK(weight.size(0) == 3 * W && weight.size(1) == 3 * W,
              "weight must be [3W,3W]");
  TORCH_CHECK(starts.numel() == T && ends.numel() == T,
              "starts/ends must have T entries");
  TORCH_CHECK(starts.scalar_type() == at::kByte && ends.scalar_type() == at::kByte,
              "starts/ends must be uint8");
  TORCH_CHECK(Mout.dim() == 2 && Mout.size(0) == T && Mout.size(1) == W,
              "Mout must be [T,W]");
  TORCH_CHECK(which.scalar_type() == at::kByte && which.dim() == 2 &&
                  which.size(0) == T && which.size(1) == W,
              "which must be uint8 [T,W]");
  TORCH_CHECK(mu.scalar_type() == at::kFloat && rstd.scalar_type() == at::kFloat &&
                  mu.numel() == T && rstd.numel() == T,
              "mu/rstd must be fp32 with T entries");
  TORCH_CHECK(g.numel() == W, "g must have W entries");
  if (dropmask) {
    check_dev(*dropmask);
    TORCH_CHECK(dropmask->scalar_type() == at::kBFloat16 && dropmask->dim() == 2 &&
                    dropmask->size(0) == T && dropmask->size(1) == W,
                "dropmask must be bf16 [T,W]");
  }
  auto dPre = at::empty({T, (compact ? 1L : 3L) * W}, dY.options());
  auto dX = at::empty_like(dY);
  auto f32 = dY.options().dtype(at::kFloat);
  if (T == 0) {
    return {dPre, dX, at::zeros({W}, f32), at::zeros({W}, f32),
            at::zeros({3L * W}, f32)};
  }
  // k-contiguous B rows: section s, output column n -> WT[sW + n, :]
  auto WT = weight.t().contiguous();
  auto stream = at::cuda::getCurrentCUDAStream();
  const int ncols = 5 * W;
  long n = (T + 127) / 128;
  auto part = at::empty({n, (long)ncols}, f32);
  if (W == 96 && compact)
    launch_mwe_bwd_fused<96, true>(dY, dropmask, Mout, g, mu, rstd, which, WT,
                                   starts, ends, dPre, dX, part, T, stream);
  else if (W == 96)
    launch_mwe_bwd_fused<96, false>(dY, dropmask, Mout, g, mu, rstd, which, WT,
                                    starts, ends, dPre, dX, part, T, stream);
  else if (compact)
    launch_mwe_bwd_fused<128, true>(dY, dropmask, Mout, g, mu, rstd, which, WT,
                                    starts, ends, dPre, dX, part, T, stream);
  else
    launch_mwe_bwd_fused<128, false>(dY, dropmask, Mout, g, mu, rstd, which, WT,
                                     starts, ends, dPre, dX, part, T, stream);
  auto sums = mwe_fold_partials(part, ncols, stream);
  return {dPre, dX, sums.narrow(0, 0, W), sums.narrow(0, W, W),
          sums.narrow(0, 2L * W, 3L * W)};
}

// ------------------------------------------------ MWE dW (srx_mwe_dw.hip.h)
// dW [3W, 3W] bf16 from dM (compact mwe_bwd_fused), which, X and the doc
// boundaries: persistent MFMA kernel + fixed-order reduction of the
// per-workgroup fp32 partials.  max_groups caps the number of workgroups
// (default: one per CU), so tests can force several tiles per workgroup.
at::Tensor mwe_bwd_dw(at::Tensor dM, at::Tensor which, at::Tensor X,
                      at::Tensor starts, at::Tensor ends, int64_t max_groups) {
  check_dev(dM);
  check_dev(which);
  check_dev(X);
  check_dev(starts);
  check_dev(ends);
  TORCH_CHECK(which.device() == dM.device() && X.device() == dM.device() &&
                  starts.device() == dM.device() && ends.device() == dM.device(),
              "mwe_bwd_dw: all tensors must be on one device");
  TORCH_CHECK(dM.scalar_type() == at::kBFloat16 && X.scalar_type() == at::kBFloat16,
              "mwe_bwd_dw is bf16-only");
  TORCH_CHECK(dM.dim() == 2 && X.dim() == 2 && which.dim() == 2,
              "mwe_bwd_dw expects 2-d tensors");
  TORCH_CHECK(dM.is_contiguous() && X.is_contiguous() && which.is_contiguous() &&
                  starts.is_contiguous() && ends.is_contiguous(),
              "mwe_bwd_dw expects contiguous tensors");
  const long T = dM.size(0);
  const int W = (int)dM.size(1);
  TORCH_CHECK(W == 96, "mwe_bwd_dw supports W = 96");
  TORCH_CHECK(T % 64 == 0, "mwe_bwd_dw needs T % 64 == 0 (TokenBatch pads)");
  TORCH_CHECK(X.size(0) == T && X.size(1) == W, "X must be [T,W]");
  TORCH_CHECK(which.scalar_type() == at::kByte && which.size(0) == T &&
                  which.size(1) == W,
              "which must be uint8 [T,W]");
  TORCH_CHECK(starts.scalar_type() == at::kByte && ends.scalar_type() == at::kByte,
              "starts/ends must be uint8");
  TORCH_CHECK(starts.dim() == 1 && ends.dim() == 1 && starts.numel() == T &&
                  ends.numel() == T,
              "starts/ends must have T entries");
  if (T == 0) return at::zeros({3L * W, 3L * W}, dM.options());
  using C = MweDwCfg<96>;
  const long ntiles = (T + C::MT - 1) / C::MT;
  long G = std::min<long>(ntiles,
                          at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  if (max_groups > 0) G = std::min<long>(G, max_groups);
  const int n = 9 * W * W;
  auto ws = at::empty({G, 3L * W, 3L * W}, dM.options().dtype(at::kFloat));
  auto dW = at::empty({3L * W, 3L * W}, dM.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_bwd_dw_kernel<96>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)C::LDS_BYTES);
    attr_set = true;
  }
  hipLaunchKernelGGL((mwe_bwd_dw_kernel<96>), dim3((unsigned)G), dim3(C::NT),
                     (size_t)C::LDS_BYTES, stream, (const bf16_t*)dM.data_ptr(),
                     which.data_ptr<uint8_t>(), (const bf16_t*)X.data_ptr(),
                     starts.data_ptr<uint8_t>(), ends.data_ptr<uint8_t>(),
                     ws.data_ptr<float>(), T, (int)ntiles);
  hipLaunchKernelGGL(mwe_dw_reduce_kernel, dim3((n + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, stream, ws.data_ptr<float>(),
                     (bf16_t*)dW.data_ptr(), (int)G, n);
  return dW;
}

// ------------------------------------------ fused embedding mixer (MFMA)
// see srx_mixer.hip.h
void mixer_check_shape(const char* name, long T, int W, int NS) {
  TORCH_CHECK(W == 96 || W == 128, name, " supports W in {96,128}");
  TORCH_CHECK(NS == 4 || NS == 5, name, " supports 4 or 5 input blocks of width W");
  TORCH_CHECK(T % 64 == 0, name, " needs T % 64 == 0 (TokenBatch pads)");
}

void mixer_check_mask(const c10::optional<at::Tensor>& dropmask, long T, int W) {
  if (!dropmask) return;
  check_dev(*dropmask);
  TORCH_CHECK(dropmask->scalar_type() == at::kBFloat16 && dropmask->dim() == 2 &&
                  dropmask->size(0) == T && dropmask->size(1) == W,
              "dropmask must be bf16 [T,W]");
}

template <int W, int NS>
void launch_mixer_fwd(const at::Tensor& E, const at::Tensor& Wm,
                      const at::Tensor& bias, const at::Tensor& g,
                      const at::Tensor& b,
                      const c10::optional<at::Tensor>& dropmask, at::Tensor& Y,
                      at::Tensor& Mout, at::Tensor& which, at::Tensor& mu,
                      at::Tensor& rstd, long T, double eps, hipStream_t stream) {
  using C = MixCfg<W, NS, false>;
  // streamed A and B chunks, reused by the epilogue tiles, + LN partials /
  // row stats: 70 KB at W=96 -> two 6-wave workgroups per CU; 91 KB at
  // W=128 -> one 8-wave workgroup
  size_t lds_bytes = MixFwdLds<W, NS>::BYTES;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mixer_fwd_kernel<W, NS>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mixer_fwd_kernel<W, NS>), grid, dim3(C::NT), lds_bytes,
                     stream, (const bf16_t*)E.data_ptr(), (const bf16_t*)Wm.data_ptr(),
                     (const bf16_t*)bias.data_ptr(), (const bf16_t*)g.data_ptr(),
                     (const bf16_t*)b.data_ptr(),
                     dropmask ? (const bf16_t*)dropmask->data_ptr() : nullptr,
                     (bf16_t*)Y.data_ptr(), (bf16_t*)Mout.data_ptr(),
                     which.data_ptr<uint8_t>(), mu.data_ptr<float>(),
                     rstd.data_ptr<float>(), T, (float)eps);
}

// Y = dropmask * LN(maxout_3(E @ Wm^T + bias)) in one kernel.
// Returns {Y, Mout, which, mu, rstd}.
std::vector<at::Tensor> mixer_fwd(at::Tensor E, at::Tensor Wm, at::Tensor bias,
                                  at::Tensor g, at::Tensor b,
                                  c10::optional<at::Tensor> dropmask, double eps) {
  check_dev(E);
  check_dev(Wm);
  check_dev(bias);
  check_dev(g);
  check_dev(b);
  TORCH_CHECK(E.scalar_type() == at::kBFloat16 &&
                  Wm.scalar_type() == at::kBFloat16 &&
                  bias.scalar_type() == at::kBFloat16 &&
                  g.scalar_type() == at::kBFloat16 &&
                  b.scalar_type() == at::kBFloat16,
              "mixer_fwd is bf16-only");
  TORCH_CHECK(E.dim() == 2 && Wm.dim() == 2, "mixer_fwd expects 2-d tensors");
  TORCH_CHECK(Wm.size(0) % 3 == 0, "weight must be [3W, NS*W]");
  long T = E.size(0);
  int W = (int)(Wm.size(0) / 3);
  TORCH_CHECK(W > 0 && E.size(1) % W == 0 && Wm.size(1) == E.size(1),
              "E must be [T, NS*W] and weight [3W, NS*W]");
  int NS = (int)(E.size(1) / W);
  mixer_check_shape("mixer_fwd", T, W, NS);
  TORCH_CHECK(bias.numel() == 3 * W && g.numel() == W && b.numel() == W,
              "bias must have 3W entries, g and b W");
  mixer_check_mask(dropmask, T, W);
  auto Y = at::empty({T, (long)W}, E.options());
  auto Mout = at::empty({T, (long)W}, E.options());
  auto which = at::empty({T, (long)W}, E.options().dtype(at::kByte));
  auto mu = at::empty({T}, E.options().dtype(at::kFloat));
  auto rstd = at::empty({T}, E.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (T > 0) {
#define SRX_MIXER_FWD(W_, NS_)                                                 \
  if (W == W_ && NS == NS_)                                                    \
    launch_mixer_fwd<W_, NS_>(E, Wm, bias, g, b, dropmask, Y, Mout, which, mu, \
                              rstd, T, eps, stream);
    SRX_MIXER_FWD(96, 4) SRX_MIXER_FWD(96, 5)
    SRX_MIXER_FWD(128, 4) SRX_MIXER_FWD(128, 5)
#undef SRX_MIXER_FWD
  }
  return {Y, Mout, which, mu, rstd};
}

template <int W, int NS>
void launch_mixer_bwd_fused(const at::Tensor& dY,
                            const c10::optional<at::Tensor>& dropmask,
                            const at::Tensor& Mout, const at::Tensor& g,
                            const at::Tensor& mu, const at::Tensor& rstd,
                            const at::Tensor& which, const at::Tensor& WT,
                            at::Tensor& dPre, at::Tensor& dE, at::Tensor& partials,
                            long T, hipStream_t stream) {
  using C = MixCfg<W, NS, true>;
  // stage-1 image [128][3W] + double-buffered B chunks + one section's
  // output tile: 139 KB at W=96, 152 KB at W=128 -> one workgroup per CU
  size_t lds_bytes =
      (size_t)(C::A_ELEMS + C::B_ELEMS + C::MT * C::OP) * sizeof(bf16_t);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mixer_bwd_fused_kernel<W, NS>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mixer_bwd_fused_kernel<W, NS>), grid, dim3(C::NT), lds_bytes,
                     stream, (const bf16_t*)dY.data_ptr(),
                     dropmask ? (const bf16_t*)dropmask->data_ptr() : nullptr,
                     (const bf16_t*)Mout.data_ptr(), (const bf16_t*)g.data_ptr(),
                     mu.data_ptr<float>(), rstd.data_ptr<float>(),
                     which.data_ptr<uint8_t>(), (const bf16_t*)WT.data_ptr(),
                     (bf16_t*)dPre.data_ptr(), (bf16_t*)dE.data_ptr(),
                     partials.data_ptr<float>(), T);
}

// Mixer backward in one kernel: stage 1 (dropmask x LayerNorm backward x
// maxout scatter) per 128-row tile into LDS, dPre written once for the dW
// GEMM, dE = dPre @ weight.  Fixed-order column sums (no atomics).
// Returns {dPre, dE, dg32, db32, dbias32}.
std::vector<at::Tensor> mixer_bwd_fused(at::Tensor dY,
                                        c10::optional<at::Tensor> dropmask,
                                        at::Tensor Mout, at::Tensor g,
                                        at::Tensor mu, at::Tensor rstd,
                                        at::Tensor which, at::Tensor weight) {
  check_dev(dY);
  check_dev(Mout);
  check_dev(g);
  check_dev(mu);
  check_dev(rstd);
  check_dev(which);
  check_dev(weight);
  TORCH_CHECK(dY.scalar_type() == at::kBFloat16 &&
                  Mout.scalar_type() == at::kBFloat16 &&
                  g.scalar_type() == at::kBFloat16 &&
                  weight.scalar_type() == at::kBFloat16,
              "mixer_bwd_fused is bf16-only");
  TORCH_CHECK(dY.dim() == 2 && weight.dim() == 2,
              "mixer_bwd_fused expects 2-d tensors");
  long T = dY.size(0);
  int W = (int)dY.size(1);
  TORCH_CHECK(W > 0 && weight.size(0) == 3 * W && weight.size(1) % W == 0,
              "weight must be [3W, NS*W]");
  int NS = (int)(weight.size(1) / W);
  mixer_check_shape("mixer_bwd_fused", T, W, NS);
  TORCH_CHECK(Mout.dim() == 2 && Mout.size(0) == T && Mout.size(1) == W,
              "Mout must be [T,W]");
  TORCH_CHECK(which.scalar_type() == at::kByte && which.dim() == 2 &&
                  which.size(0) == T && which.size(1) == W,
              "which must be uint8 [T,W]");
  TORCH_CHECK(mu.scalar_type() == at::kFloat && rstd.scalar_type() == at::kFloat &&
                  mu.numel() == T && rstd.numel() == T,
              "mu/rstd must be fp32 with T entries");
  TORCH_CHECK(g.numel() == W, "g must have W entries");
  mixer_check_mask(dropmask, T, W);
  auto dPre = at::empty({T, 3L * W}, dY.options());
  auto dE = at::empty({T, (long)NS * W}, dY.options());
  auto f32 = dY.options().dtype(at::kFloat);
  if (T == 0) {
    return {dPre, dE, at::zeros({W}, f32), at::zeros({W}, f32),
            at::zeros({3L * W}, f32)};
  }
  // k-contiguous B rows: section s, output column n -> WT[sW + n, :]
  auto WT = weight.t().contiguous();
  auto stream = at::cuda::getCurrentCUDAStream();
  const int ncols = 5 * W;
  auto part = at::empty({(T + 127) / 128, (long)ncols}, f32);
#define SRX_MIXER_BWD(W_, NS_)                                                \
  if (W == W_ && NS == NS_)                                                   \
    launch_mixer_bwd_fused<W_, NS_>(dY, dropmask, Mout, g, mu, rstd, which, WT, \
                                    dPre, dE, part, T, stream);
  SRX_MIXER_BWD(96, 4) SRX_MIXER_BWD(96, 5)
  SRX_MIXER_BWD(128, 4) SRX_MIXER_BWD(128, 5)
#undef SRX_MIXER_BWD
  auto sums = mwe_fold_partials(part, ncols, stream);
  return {dPre, dE, sums.narrow(0, 0, W), sums.narrow(0, W, W),
          sums.narrow(0, 2L * W, 3L * W)};
}

// ------------------------------------------------- static word vectors
// see srx_staticvec.hip.h.  `rows` must be < V: vocab.Vectors.find_rows
// guarantees it on the host where the rows are built (no device sync here);
// the kernels treat anything else as out of vocabulary.
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

void check_static_vectors(const at::Tensor& table, const at::Tensor& rows,
                          int nO, int nM) {
  check_dev(table);
  check_dev(rows);
  TORCH_CHECK(table.scalar_type() == at::kBFloat16 && table.dim() == 2,
              "static_vectors: table must be bf16 [V, nMp]");
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.dim() == 1,
              "static_vectors: rows must be int32 [T]");
  const long nMp = table.size(1);
  TORCH_CHECK(nMp % 32 == 0 && nMp >= 32 && nMp <= 320,
              "static_vectors: table row stride must be a multiple of 32, <= 320");
  TORCH_CHECK(nM <= nMp && nMp - nM < 32,
              "static_vectors: table stride must be roundup(nM, 32)");
  TORCH_CHECK(nO == 96 || nO == 128, "static_vectors supports nO in {96,128}");
  TORCH_CHECK(table.size(0) < (1L << 31), "static_vectors: too many rows");
}

template <int NO>
void launch_static_vectors_fwd(const at::Tensor& table, const at::Tensor& rows,
                               const at::Tensor& W, at::Tensor& Y, int col_off,
                               hipStream_t stream) {
  using C = SvCfg<NO>;
  const long T = rows.size(0);
  const int nMp = (int)table.size(1), nM = (int)W.size(1);
  auto lds_for = [](int k) {
    size_t img = (size_t)(C::MT * (k + 8) + C::B_ELEMS) * sizeof(bf16_t) +
                 C::MT * sizeof(int);
    return std::max(img, (size_t)C::MT * C::YP * sizeof(bf16_t));
  };
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)static_vectors_fwd_kernel<NO>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_for(C::MAXK));
    attr_set = true;
  }
  const long ldY = Y.stride(0);
  const int w_vec = (nM % 8 == 0) && aligned16(W.data_ptr());
  bf16_t* yp = (bf16_t*)Y.data_ptr();
  const int y_vec = (ldY % 8 == 0) && (col_off % 8 == 0) && aligned16(yp);
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((static_vectors_fwd_kernel<NO>), grid, dim3(C::NT),
                     lds_for(nMp), stream, (const bf16_t*)table.data_ptr(),
                     rows.data_ptr<int>(), (const bf16_t*)W.data_ptr(), yp, ldY,
                     col_off, T, (int)table.size(0), nM, nMp, w_vec, y_vec);
}

void static_vectors_fwd(at::Tensor table, at::Tensor rows, at::Tensor W,
                        at::Tensor Y, int64_t col_off) {
  check_dev(W);
  TORCH_CHECK(W.scalar_type() == at::kBFloat16 && W.dim() == 2,
              "static_vectors_fwd: W must be bf16 [nO, nM]");
  const int nO = (int)W.size(0);
  check_static_vectors(table, rows, nO, (int)W.size(1));
  const long T = rows.size(0);
  TORCH_CHECK(Y.is_cuda() && Y.scalar_type() == at::kBFloat16 && Y.dim() == 2 &&
                  Y.stride(1) == 1,
              "static_vectors_fwd: Y must be a bf16 matrix with unit column stride");
  TORCH_CHECK(Y.size(0) >= T && col_off >= 0 && col_off + nO <= Y.size(1) &&
                  Y.stride(0) >= Y.size(1),
              "static_vectors_fwd: column block outside Y");
  if (T == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  if (nO == 96)
    launch_static_vectors_fwd<96>(table, rows, W, Y, (int)col_off, stream);
  else
    launch_static_vectors_fwd<128>(table, rows, W, Y, (int)col_off, stream);
}

template <int NO>
void launch_static_vectors_bwd(const at::Tensor& table, const at::Tensor& rows,
                               const at::Tensor& dX, int col_off, at::Tensor& ws,
                               int G, int ntiles, hipStream_t stream) {
  using C = SvCfg<NO>;
  const int nMp = (int)table.size(1);
  auto lds_for = [](int k) {
    return (size_t)(NO + k) * C::TP * sizeof(bf16_t) + C::MT * sizeof(int);
  };
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)static_vectors_bwd_dw_kernel<NO>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_for(C::MAXK));
    attr_set = true;
  }
  const long ldX = dX.stride(0);
  const bf16_t* xp = (const bf16_t*)dX.data_ptr();
  const int x_vec = (ldX % 8 == 0) && (col_off % 8 == 0) && aligned16(xp);
  hipLaunchKernelGGL((static_vectors_bwd_dw_kernel<NO>), dim3((unsigned)G),
                     dim3(C::NT), lds_for(nMp), stream,
                     (const bf16_t*)table.data_ptr(), rows.data_ptr<int>(), xp, ldX,
                     col_off, ws.data_ptr<float>(), (long)rows.size(0),
                     (int)table.size(0), nMp, ntiles, x_vec);
}

at::Tensor static_vectors_bwd_dw(at::Tensor table, at::Tensor rows, at::Tensor dX,
                                 int64_t col_off, int64_t nO,
                                 int64_t max_groups, int64_t nM) {
  if (nM <= 0) nM = table.size(1);
  check_static_vectors(table, rows, (int)nO, (int)nM);
  const long T = rows.size(0);
  TORCH_CHECK(dX.is_cuda() && dX.scalar_type() == at::kBFloat16 && dX.dim() == 2 &&
                  dX.stride(1) == 1,
              "static_vectors_bwd_dw: dX must be a bf16 matrix with unit column stride");
  TORCH_CHECK(dX.size(0) >= T && col_off >= 0 && col_off + nO <= dX.size(1) &&
                  dX.stride(0) >= dX.size(1),
              "static_vectors_bwd_dw: column block outside dX");
  auto f32 = table.options().dtype(at::kFloat);
  if (T == 0) return at::zeros({nO, nM}, f32);
  const long ntiles = (T + 127) / 128;
  // one workgroup per CU (122 KB of LDS at nMp = 320)
  long G = std::min<long>(ntiles,
                          at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  if (max_groups > 0) G = std::min<long>(G, max_groups);
  const long nMp = table.size(1);
  auto ws = at::empty({G, nO, nMp}, f32);
  auto dW = at::empty({nO, nM}, f32);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (nO == 96)
    launch_static_vectors_bwd<96>(table, rows, dX, (int)col_off, ws, (int)G,
                                  (int)ntiles, stream);
  else
    launch_static_vectors_bwd<128>(table, rows, dX, (int)col_off, ws, (int)G,
                                   (int)ntiles, stream);
  const int total = (int)(nO * nM);
  hipLaunchKernelGGL(static_vectors_reduce_kernel, dim3((total + kBlock - 1) / kBlock),
                     dim3(kBlock), 0, stream, ws.data_ptr<float>(),
                     dW.data_ptr<float>(), (int)G, (int)nO, (int)nM, (int)nMp);
  return dW;
}

// ------------------------------------------------------- floret vectors
// see srx_floret.hip.h.  out[u] = mean of table[idx[offsets[u] : offsets[u+1]]]
// for u < U = offsets.numel() - 1; rows >= U of `out` are left alone.
void floret_words_mean(at::Tensor table, at::Tensor offsets, at::Tensor idx,
                       at::Tensor out) {
  check_dev(table);
  check_dev(offsets);
  check_dev(idx);
  check_dev(out);
  TORCH_CHECK(table.scalar_type() == at::kBFloat16 && table.dim() == 2,
              "floret_words_mean: table must be bf16 [R, nMp]");
  TORCH_CHECK(offsets.scalar_type() == at::kInt && offsets.dim() == 1 &&
                  offsets.numel() >= 1,
              "floret_words_mean: offsets must be int32 [U + 1]");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.dim() == 1,
              "floret_words_mean: idx must be int32 [nnz]");
  const long U = offsets.numel() - 1;
  const long nMp = table.size(1);
  TORCH_CHECK(nMp >= 8 && nMp % 8 == 0,
              "floret_words_mean: table row stride must be a multiple of 8");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.dim() == 2 &&
                  out.size(1) == nMp && out.size(0) >= U,
              "floret_words_mean: out must be bf16 [>= U, nMp] with "
              "offsets.numel() == U + 1");
  TORCH_CHECK(table.size(0) < (1L << 31) && idx.numel() < (1L << 31) &&
                  U < (1L << 31),
              "floret_words_mean: sizes must fit in int32");
  if (U == 0) return;
  const int wpb = SRX_FLORET_THREADS / SRX_WAVE;
  // memory bound: at most 8 workgroups per CU, the rest is grid-strided
  const long cap = 8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  dim3 grid((unsigned)std::min<long>((U + wpb - 1) / wpb, cap));
  auto stream = at::cuda::getCurrentCUDAStream();
  const long Q = nMp / 8;
#define SRX_FLORET_LAUNCH(SW)                                                  \
  hipLaunchKernelGGL((floret_words_mean_kernel<SW>), grid,                     \
                     dim3(SRX_FLORET_THREADS), 0, stream,                      \
                     (const bf16_t*)table.data_ptr(), offsets.data_ptr<int>(), \
                     idx.data_ptr<int>(), (bf16_t*)out.data_ptr(), (int)U,     \
                     (int)table.size(0), (int)nMp, (int)idx.numel())
  if (Q <= 8) SRX_FLORET_LAUNCH(8);
  else if (Q <= 16) SRX_FLORET_LAUNCH(16);
  else if (Q <= 32) SRX_FLORET_LAUNCH(32);
  else SRX_FLORET_LAUNCH(64);
#undef SRX_FLORET_LAUNCH
}

// ---------------------------------------------------------- vectors loss
// see srx_vecloss.hip.h.  One launch: row_loss[i] (fp32) and dpred[i, :nM]
// (bf16) for i < N = rows.numel(); rows >= N of either output and columns
// >= nM of dpred are left alone.  pred and dpred may be row-strided views.
void vectors_loss(at::Tensor pred, at::Tensor table, at::Tensor rows,
                  at::Tensor row_loss, at::Tensor dpred, bool l2, double scale) {
  check_dev(table);
  check_dev(rows);
  check_dev(row_loss);
  TORCH_CHECK(table.scalar_type() == at::kBFloat16 && table.dim() == 2,
              "vectors_loss: table must be bf16 [V, nMp]");
  TORCH_CHECK(rows.scalar_type() == at::kInt && rows.dim() == 1,
              "vectors_loss: rows must be int32 [N]");
  const long N = rows.size(0);
  const long nMp = table.size(1), V = table.size(0);
  TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == at::kBFloat16 &&
                  pred.dim() == 2 && pred.size(0) == N,
              "vectors_loss: pred must be bf16 [N, nM]");
  const long nM = pred.size(1);
  TORCH_CHECK(nMp % 32 == 0 && nMp >= 32 && nMp <= 320 && nM <= nMp &&
                  nMp - nM < 32,
              "vectors_loss: table row stride must be roundup(nM, 32) <= 320");
  TORCH_CHECK(V >= 1 && V < (1L << 31), "vectors_loss: 1 <= V < 2^31");
  TORCH_CHECK(aligned16(table.data_ptr()), "vectors_loss: table not 16-byte aligned");
  TORCH_CHECK(dpred.is_cuda() && dpred.scalar_type() == at::kBFloat16 &&
                  dpred.dim() == 2 && dpred.size(0) >= N && dpred.size(1) == nM,
              "vectors_loss: dpred must be bf16 [>= N, nM]");
  TORCH_CHECK(row_loss.scalar_type() == at::kFloat && row_loss.numel() >= N,
              "vectors_loss: row_loss must be fp32 [>= N]");
  if (N == 0) return;
  // a one-row matrix may carry any row stride; it is never used
  const long ldP = N > 1 ? pred.stride(0) : nM;
  const long ldD = dpred.size(0) > 1 ? dpred.stride(0) : nM;
  TORCH_CHECK(pred.stride(1) == 1 && dpred.stride(1) == 1 && ldP >= nM && ldD >= nM,
              "vectors_loss: pred and dpred need unit column stride and "
              "non-overlapping rows");
  // widest access (in bf16 elements) that the base pointers, the row
  // strides and the row length all allow
  const uintptr_t mix = (uintptr_t)pred.data_ptr() | (uintptr_t)dpred.data_ptr() |
                        (uintptr_t)(2 * ldP) | (uintptr_t)(2 * ldD) |
                        (uintptr_t)(2 * nM);
  const int pv = (mix % 16 == 0) ? 8 : (mix % 8 == 0) ? 4 : (mix % 4 == 0) ? 2 : 1;
  const long Q = nMp / 8;
  const int sw = Q <= 8 ? 8 : Q <= 16 ? 16 : Q <= 32 ? 32 : 64;
  const long wpb = SRX_VECLOSS_THREADS / SRX_WAVE;
  const long groups = (N + (SRX_WAVE / sw) - 1) / (SRX_WAVE / sw);
  // memory bound: at most 8 workgroups per CU, the rest is grid-strided
  const long cap = 8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  dim3 grid((unsigned)std::min<long>((groups + wpb - 1) / wpb, cap));
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_VECLOSS_LAUNCH(SW, PV)                                             \
  hipLaunchKernelGGL((vectors_loss_kernel<SW, PV>), grid,                      \
                     dim3(SRX_VECLOSS_THREADS), 0, stream,                     \
                     (const bf16_t*)pred.data_ptr(),                           \
                     (const bf16_t*)table.data_ptr(), rows.data_ptr<int>(),    \
                     row_loss.data_ptr<float>(), (bf16_t*)dpred.data_ptr(),    \
                     ldP, ldD, N, (int)V, (int)nM, (int)nMp, (int)l2,          \
                     (float)scale)
#define SRX_VECLOSS_PV(SW)                                                     \
  switch (pv) {                                                                \
    case 8: SRX_VECLOSS_LAUNCH(SW, 8); break;                                  \
    case 4: SRX_VECLOSS_LAUNCH(SW, 4); break;                                  \
    case 2: SRX_VECLOSS_LAUNCH(SW, 2); break;                                  \
    default: SRX_VECLOSS_LAUNCH(SW, 1); break;                                 \
  }
  if (sw == 8) { SRX_VECLOSS_PV(8) }
  else if (sw == 16) { SRX_VECLOSS_PV(16) }
  else if (sw == 32) { SRX_VECLOSS_PV(32) }
  else { SRX_VECLOSS_PV(64) }
#undef SRX_VECLOSS_PV
#undef SRX_VECLOSS_LAUNCH
}

// --------------------------------------------- fused transition step (C++)
// One python call per transition step: state scorer kernel + upper GEMM +
// on-device action selection, with a C++ autograd node so the per-step
// python op count collapses (~10 -> 1).  Backward stashes the compact
// (feats, dSummed) pair into a session store keyed by task id; the python
// side drains it for the batched sorted dPre scatter.
// NOTE: backward runs on autograd worker threads WITHOUT the GIL — only
// ATen ops and the mutex-guarded store are touched there.
namespace fusedstep {

struct Store {
  std::mutex mu;
  std::unordered_map<int64_t, std::vector<std::pair<at::Tensor, at::Tensor>>> m;
};
Store& store() {
  static Store s;
  return s;
}

class Fn : public torch::autograd::Function<Fn> {
 public:
  static torch::autograd::variable_list forward(
      torch::autograd::AutogradContext* ctx, at::Tensor pre_d, at::Tensor feats,
      at::Tensor lower_b, at::Tensor upperW, at::Tensor upperB,
      at::Tensor is_gold, at::Tensor valid, int64_t task_id, bool train) {
    auto hw = parser_step_fwd(pre_d, feats, lower_b);
    auto hidden = hw[0];
    auto which = hw[1];
    auto scores = at::addmm(upperB, hidden, upperW.t());
    auto actions = action_select(scores, is_gold, valid);
    ctx->save_for_backward({feats, which, hidden, upperW});
    ctx->saved_data["task_id"] = task_id;
    ctx->saved_data["train"] = train;
    ctx->mark_non_differentiable({actions});
    return {scores, actions};
  }

  static torch::autograd::variable_list backward(
      torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
    auto saved = ctx->get_saved_variables();
    auto feats = saved[0];
    auto which = saved[1];
    auto hidden = saved[2];
    auto upperW = saved[3];
    auto dScores = grads[0].contiguous();
    auto dUpperW = dScores.t().mm(hidden);
    auto dUpperB = dScores.sum(0);
    auto dHidden = dScores.mm(upperW).contiguous();
    auto dSummed = maxout_bwd(dHidden, which, 2).view({dHidden.size(0), -1});
    auto dLowerB = dSummed.to(at::kFloat).sum(0);  // mirrors the python accum path
    int64_t task_id = ctx->saved_data["task_id"].toInt();
    {
      auto& s = store();
      std::lock_guard<std::mutex> lock(s.mu);
      s.m[task_id].emplace_back(feats, dSummed);
    }
    // pre_d is detached by contract (its gradient flows via the batched
    // scatter + inject_grad); feats/is_gold/valid are integer masks.
    return {at::Tensor(), at::Tensor(), dLowerB, dUpperW, dUpperB,
            at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
  }
};

std::vector<at::Tensor> fused_step(at::Tensor pre_d, at::Tensor feats,
                                   at::Tensor lower_b, at::Tensor upperW,
                                   at::Tensor upperB, at::Tensor is_gold,
                                   at::Tensor valid, int64_t task_id, bool train) {
  auto out = Fn::apply(pre_d, feats, lower_b, upperW, upperB, is_gold, valid,
                       task_id, train);
  return {out[0], out[1]};
}

std::vector<std::vector<at::Tensor>> fused_entries_take(int64_t task_id) {
  auto& s = store();
  std::lock_guard<std::mutex> lock(s.mu);
  std::vector<std::vector<at::Tensor>> out;
  auto it = s.m.find(task_id);
  if (it != s.m.end()) {
    for (auto& pr : it->second) out.push_back({pr.first, pr.second});
    s.m.erase(it);
  }
  return out;
}

}  // namespace fusedstep

}  // namespace

// srx_steploop.hip — the C++-owned transition loop (one python call/batch)
std::vector<std::vector<at::Tensor>> srx_run_transition_loop(
    std::vector<std::tuple<int64_t, at::Tensor, at::Tensor, at::Tensor,
                           at::Tensor, bool>>
        tasks);

// srx_gpustate.hip — fully GPU-resident state machines (one wave per doc)
std::vector<at::Tensor> srx_gpu_arceager(
    at::Tensor pre, at::Tensor off, at::Tensor lens, at::Tensor gh,
    at::Tensor gl, at::Tensor kids_off, at::Tensor kids, at::Tensor lowerB,
    at::Tensor upperW, at::Tensor upperB, int64_t total, int64_t n_labels,
    bool train, bool fuse_ce);
std::vector<at::Tensor> srx_gpu_biluo(
    at::Tensor pre, at::Tensor off, at::Tensor lens, at::Tensor gold,
    at::Tensor lowerB, at::Tensor upperW, at::Tensor upperB, int64_t total,
    int64_t n_types, bool train, bool fuse_ce);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("seq2col_fwd", &seq2col_fwd);
  m.def("seq2col_bwd", &seq2col_bwd, py::arg("dY"), py::arg("starts"),
        py::arg("ends"), py::arg("residual") = py::none());
  m.def("mwe_bwd_stage1", &mwe_bwd_stage1, py::arg("dY"), py::arg("dropmask"),
        py::arg("Mout"), py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("which"), py::arg("deterministic") = false);
  m.def("maxout_fwd", &maxout_fwd);
  m.def("maxout_bwd", &maxout_bwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dY"), py::arg("X"),
        py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("deterministic") = false);
  m.def("hashembed_fwd", &hashembed_fwd, py::arg("table"), py::arg("ids"),
        py::arg("seed"), py::arg("out") = py::none(), py::arg("col_off") = 0);
  m.def("hashembed_bwd", &hashembed_bwd);
  m.def("multi_hashembed_fwd", &multi_hashembed_fwd, py::arg("ids4"),
        py::arg("tables"), py::arg("seeds"), py::arg("X"), py::arg("col_off") = 0);
  m.def("hashembed_bwd_merged", &hashembed_bwd_merged, py::arg("order"),
        py::arg("rows"), py::arg("dY"), py::arg("dT32"));
  m.def("parser_step_fwd", &parser_step_fwd);
  m.def("parser_step_bwd", &parser_step_bwd);
  m.def("parser_step_bwd_into", &parser_step_bwd_into);
  m.def("action_select", &action_select);
  m.def("seg_scatter_add", &seg_scatter_add);
  m.def("adam_step", &adam_step);
  m.def("dropout_mask", &dropout_mask);
  m.def("act_fwd", &act_fwd);
  m.def("attn_softmax_fwd", &attn_softmax_fwd);
  m.def("attn_fused_fwd", &attn_fused_fwd);
  m.def("attn_fused_bwd", &attn_fused_bwd);
  m.def("attn_softmax_bwd", &attn_softmax_bwd);
  m.def("act_bwd", &act_bwd);
  m.def("softmax_ce", &softmax_ce);
  m.def("reduce_ragged", &reduce_ragged);
  m.def("reduce_ragged_bwd", &reduce_ragged_bwd);
  m.def("reduce_max_bwd", &reduce_max_bwd);
  m.def("mwe_layer_fwd", &mwe_layer_fwd);
  m.def("mwe_bwd_dx", &mwe_bwd_dx, py::arg("dPre"), py::arg("weight"),
        py::arg("starts"), py::arg("ends"), py::arg("dY"));
  m.def("mwe_bwd_fused", &mwe_bwd_fused, py::arg("dY"), py::arg("dropmask"),
        py::arg("Mout"), py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("which"), py::arg("weight"), py::arg("starts"), py::arg("ends"),
        py::arg("compact") = false);
  m.def("mwe_bwd_dw", &mwe_bwd_dw, py::arg("dM"), py::arg("which"), py::arg("X"),
        py::arg("starts"), py::arg("ends"), py::arg("max_groups") = 0);
  m.def("mixer_fwd", &mixer_fwd, py::arg("E"), py::arg("weight"), py::arg("bias"),
        py::arg("g"), py::arg("b"), py::arg("dropmask"), py::arg("eps"));
  m.def("mixer_bwd_fused", &mixer_bwd_fused, py::arg("dY"), py::arg("dropmask"),
        py::arg("Mout"), py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("which"), py::arg("weight"));
  m.def("static_vectors_fwd", &static_vectors_fwd, py::arg("table"),
        py::arg("rows"), py::arg("W"), py::arg("Y"), py::arg("col_off") = 0);
  m.def("static_vectors_bwd_dw", &static_vectors_bwd_dw, py::arg("table"),
        py::arg("rows"), py::arg("dX"), py::arg("col_off"), py::arg("nO"),
        py::arg("max_groups") = 0, py::arg("nM") = 0);
  m.def("floret_words_mean", &floret_words_mean, py::arg("table"),
        py::arg("offsets"), py::arg("idx"), py::arg("out"));
  m.def("vectors_loss", &vectors_loss, py::arg("pred"), py::arg("table"),
        py::arg("rows"), py::arg("row_loss"), py::arg("dpred"), py::arg("l2"),
        py::arg("scale"));
  m.def("fused_step", &fusedstep::fused_step);
  m.def("fused_entries_take", &fusedstep::fused_entries_take);
  m.def("transition_ce", &transition_ce, py::arg("scores"), py::arg("gold"),
        py::arg("valid"), py::arg("deterministic") = false);
  m.attr("FIXED_SCALE") = 16777216.0;
  m.def("dpre_scatter", &dpre_scatter);
  m.def("dpre_scatter_docmajor", &dpre_scatter_docmajor);
  m.def("run_transition_loop", &srx_run_transition_loop,
        py::call_guard<py::gil_scoped_release>());
  m.def("gpu_arceager", &srx_gpu_arceager, py::arg("pre"), py::arg("off"),
        py::arg("lens"), py::arg("gh"), py::arg("gl"), py::arg("kids_off"),
        py::arg("kids"), py::arg("lowerB"), py::arg("upperW"),
        py::arg("upperB"), py::arg("total"), py::arg("n_labels"),
        py::arg("train"), py::arg("fuse_ce") = false);
  m.def("gpu_biluo", &srx_gpu_biluo, py::arg("pre"), py::arg("off"),
        py::arg("lens"), py::arg("gold"), py::arg("lowerB"), py::arg("upperW"),
        py::arg("upperB"), py::arg("total"), py::arg("n_types"),
        py::arg("train"), py::arg("fuse_ce") = false);
  m.attr("GPU_STATE_MAXLEN") = 128;
}
