// Host-side helpers shared by the _srx_hip binding files (srx_bind_*.hip and
// srx_ext.hip): launch geometry, argument checks, the fp32/bf16 dispatch and
// the few launchers that more than one family calls.  No kernels here.
#pragma once

#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "srx_common.hip.h"

constexpr int kBlock = 256;

inline int grid_for(long total, int per_thread = 1) {
  long blocks = (total + (long)kBlock * per_thread - 1) / ((long)kBlock * per_thread);
  return (int)std::min<long>(blocks, 16384);
}

inline void check_dev(const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "expected a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), "expected contiguous");
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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

// srx_bind_mwe.hip; also folds dpre_gather's per-wave partials
at::Tensor mwe_fold_partials(at::Tensor part, int ncols, hipStream_t stream);
// srx_bind_elementwise.hip; also the fused transition step's backward
at::Tensor maxout_bwd(at::Tensor dY, at::Tensor which, long P);

// one per binding file: registers the family's launchers on the module
void bind_elementwise(pybind11::module_& m);
void bind_parser(pybind11::module_& m);
void bind_mwe(pybind11::module_& m);
void bind_attn(pybind11::module_& m);
void bind_vectors(pybind11::module_& m);
void bind_pool(pybind11::module_& m);
