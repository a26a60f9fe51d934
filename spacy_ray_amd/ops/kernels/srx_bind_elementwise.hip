// _srx_hip bindings: elementwise layers, the optimizer step, softmax
// cross-entropy, ragged reductions and the activation surface.
#include "srx_bind.hip.h"

#include "srx_elementwise.hip.h"
#include "srx_softmax_reduce.hip.h"
#include "srx_activations.hip.h"

namespace {

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

}  // namespace

// external linkage: the fused transition step's backward
// (srx_bind_parser.hip) calls it too
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

namespace {

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
  // fp32 rows sum dg/db by fp64 atomics: fp32 adds in arrival order over
  // thousands of waves would cost the fp32 result several digits
  auto acc_dt = deterministic ? at::kLong
                : X.scalar_type() == at::kFloat ? at::kDouble : at::kFloat;
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
                       scale_ptr, (float)(1.0 - lr * wd), (float)(lr / bc1),
                       (float)beta1, (float)beta2, (float)(1.0 - beta1),
                       (float)(1.0 - beta2), (float)eps, (float)bc2);
  });
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
  auto loss = at::zeros({2}, scores.options().dtype(at::kDouble));
  if (N == 0) return {loss.to(at::kFloat), dScores};
  auto stream = at::cuda::getCurrentCUDAStream();
  int grid = (int)std::min<long>((N + 3) / 4, 2048);
  DISPATCH_F(scores.scalar_type(), {
    hipLaunchKernelGGL((softmax_ce_kernel<scalar_t>), dim3(grid), dim3(kBlock), 0,
                       stream, (const scalar_t*)scores.data_ptr(),
                       gold.data_ptr<int64_t>(), (scalar_t*)dScores.data_ptr(),
                       loss.data_ptr<double>(), N, C);
  });
  return {loss.to(at::kFloat), dScores};
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

}  // namespace

void bind_elementwise(py::module_& m) {
  m.def("seq2col_fwd", &seq2col_fwd);
  m.def("seq2col_bwd", &seq2col_bwd, py::arg("dY"), py::arg("starts"),
        py::arg("ends"), py::arg("residual") = py::none());
  m.def("maxout_fwd", &maxout_fwd);
  m.def("maxout_bwd", &maxout_bwd);
  m.def("layernorm_fwd", &layernorm_fwd);
  m.def("layernorm_bwd", &layernorm_bwd, py::arg("dY"), py::arg("X"),
        py::arg("g"), py::arg("mu"), py::arg("rstd"),
        py::arg("deterministic") = false);
  m.def("adam_step", &adam_step);
  m.def("dropout_mask", &dropout_mask);
  m.def("act_fwd", &act_fwd);
  m.def("act_bwd", &act_bwd);
  m.def("softmax_ce", &softmax_ce);
  m.def("reduce_ragged", &reduce_ragged);
  m.def("reduce_ragged_bwd", &reduce_ragged_bwd);
  m.def("reduce_max_bwd", &reduce_max_bwd);
}
