// _srx_hip bindings: the fused MWE (maxout window encoder) block, its dW
// kernel and the fused embedding mixer (MFMA kernels).
#include "srx_bind.hip.h"

#include "srx_mwe.hip.h"
#include "srx_mwe_wide.hip.h"
#include "srx_mixer.hip.h"
#include "srx_mwe_dw.hip.h"

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

namespace {

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

// W = 256: 64 whole rows per workgroup (srx_mwe_wide.hip.h)
void launch_mwe_wide(const at::Tensor& X, const at::Tensor& Wt,
                     const at::Tensor& bias, const at::Tensor& g,
                     const at::Tensor& b, const at::Tensor& starts,
                     const at::Tensor& ends,
                     const c10::optional<at::Tensor>& dropmask, at::Tensor& Y,
                     at::Tensor& Mout, at::Tensor& which, at::Tensor& mu,
                     at::Tensor& rstd, long T, double eps, hipStream_t stream) {
  using C = MweWideFwdCfg;
  // X halo image + double-buffered B chunks (the epilogue tiles reuse the
  // B region): 154 KB -> one 8-wave workgroup per CU
  size_t lds_bytes = C::LDS_BYTES;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_wide_fwd_kernel<256>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mwe_wide_fwd_kernel<256>), grid, dim3(C::NT), lds_bytes,
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
  TORCH_CHECK(W == 96 || W == 128 || W == 256,
              "mwe_layer supports W in {96,128,256}");
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
    else if (W == 256)
      launch_mwe_wide(X, Wt, bias, g, b, starts, ends, dropmask, Y, Mout, which,
                      mu, rstd, T, eps, stream);
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

// W = 256: compact dM + tag bytes in LDS, the A fragment of each piece
// formed in registers (srx_mwe_wide.hip.h)
void launch_mwe_wide_bwd_fused(const at::Tensor& dY,
                               const c10::optional<at::Tensor>& dropmask,
                               const at::Tensor& Mout, const at::Tensor& g,
                               const at::Tensor& mu, const at::Tensor& rstd,
                               const at::Tensor& which, const at::Tensor& WT,
                               const at::Tensor& starts, const at::Tensor& ends,
                               at::Tensor& dPre, at::Tensor& dX,
                               at::Tensor& partials, long T, hipStream_t stream) {
  using C = MweWideBwdCfg;
  // dM halo image + tag bytes + double-buffered B chunks: 142 KB -> one
  // 8-wave workgroup per CU
  size_t lds_bytes = C::LDS_BYTES;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)mwe_wide_bwd_fused_kernel<256>,
                              hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)lds_bytes);
    attr_set = true;
  }
  dim3 grid((unsigned)((T + C::MT - 1) / C::MT));
  hipLaunchKernelGGL((mwe_wide_bwd_fused_kernel<256>), grid, dim3(C::NT), lds_bytes,
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
// bit-identical.  W = 256 has no compact form (there is no dW kernel at that
// width to read it).
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
  TORCH_CHECK(W == 96 || W == 128 || W == 256,
              "mwe_bwd_fused supports W in {96,128,256}");
  TORCH_CHECK(!(compact && W == 256),
              "mwe_bwd_fused: compact=True is not available at W = 256");
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
  if (W == 256)
    launch_mwe_wide_bwd_fused(dY, dropmask, Mout, g, mu, rstd, which, WT, starts,
                              ends, dPre, dX, part, T, stream);
  else if (W == 96 && compact)
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

}  // namespace

void bind_mwe(py::module_& m) {
  m.def("mwe_bwd_stage1", &mwe_bwd_stage1, py::arg("dY"), py::arg("dropmask"),
        py::arg("Mout"), py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("which"), py::arg("deterministic") = false);
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
}
