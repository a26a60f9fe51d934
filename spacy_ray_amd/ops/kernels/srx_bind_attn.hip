// _srx_hip bindings: attention softmax and the fused flash-style attention.
#include "srx_bind.hip.h"

#include <mutex>

#include "srx_attn.hip.h"

namespace {

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

}  // namespace

void bind_attn(py::module_& m) {
  m.def("attn_softmax_fwd", &attn_softmax_fwd);
  m.def("attn_softmax_bwd", &attn_softmax_bwd);
  m.def("attn_fused_fwd", &attn_fused_fwd);
  m.def("attn_fused_bwd", &attn_fused_bwd);
}
