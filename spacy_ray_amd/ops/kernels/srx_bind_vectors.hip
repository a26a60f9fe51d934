// _srx_hip bindings: static and floret word vectors, the vectors loss and
// CharacterEmbed.
#include "srx_bind.hip.h"

#include "srx_staticvec.hip.h"
#include "srx_floret.hip.h"
#include "srx_vecloss.hip.h"
#include "srx_charembed.hip.h"

namespace {

// ------------------------------------------------- static word vectors
// see srx_staticvec.hip.h.  `rows` must be < V: vocab.Vectors.find_rows
// guarantees it on the host where the rows are built (no device sync here);
// the kernels treat anything else as out of vocabulary.
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

// ------------------------------------------------- CharacterEmbed
// see srx_charembed.hip.h.  E bf16 / fp32 [nC, 256, nM], ids uint8 [T, nC];
// nM % 8 == 0, 8 <= nM <= 128, 1 <= nC <= 16, 16-byte-aligned blocks.
namespace ce {

constexpr long kMinTokensPerSlice = 4096;

inline void check_shape(long nC, long nM) {
  TORCH_CHECK(nC >= 1 && nC <= 16, "char_embed: nC must be in 1..16");
  TORCH_CHECK(nM >= 8 && nM <= 128 && nM % 8 == 0,
              "char_embed: nM must be a multiple of 8 in 8..128");
}

inline void check_ids(const at::Tensor& ids, long nC) {
  check_dev(ids);
  TORCH_CHECK(ids.scalar_type() == at::kByte && ids.dim() == 2 && ids.size(1) == nC,
              "char_embed: ids must be uint8 [T, nC]");
}

}  // namespace ce

// -> (S, tokens per slice) of char_embed_bwd's grid (nC, S): nC * S is about
// twice the CU count, but a slice never holds fewer than kMinTokensPerSlice
// tokens (each slice costs a zero fill, a write and a read of [256, nM]
// floats), so small batches run S = 1.
std::vector<int64_t> char_embed_slices(int64_t T, int64_t nC) {
  ce::check_shape(nC, 8);
  const long cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  long S = std::max<long>(1, (2 * cus + nC / 2) / nC);
  S = std::max<long>(1, std::min<long>(S, T / ce::kMinTokensPerSlice));
  const long per = std::max<long>(1, (T + S - 1) / S);
  S = std::max<long>(1, (T + per - 1) / per);  // no empty slice
  return {S, per};
}

void char_embed_fwd(at::Tensor E, at::Tensor ids, at::Tensor X, int64_t col_off) {
  check_dev(E);
  TORCH_CHECK(E.dim() == 3 && E.size(1) == SRX_CE_BINS,
              "char_embed_fwd: E must be [nC, 256, nM]");
  const long nC = E.size(0), nM = E.size(2);
  ce::check_shape(nC, nM);
  ce::check_ids(ids, nC);
  const long nT = ids.size(0);
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.is_contiguous() && X.size(0) == nT &&
                  X.scalar_type() == E.scalar_type(),
              "X must be a contiguous GPU [T, ldX] matrix of the table's dtype");
  const long ldX = X.size(1);
  TORCH_CHECK(col_off >= 0 && col_off + nC * nM <= ldX,
              "char_embed_fwd: column block outside X");
  if (nT == 0) return;
  auto stream = at::cuda::getCurrentCUDAStream();
  DISPATCH_F(E.scalar_type(), {
    const long items = nT * nC * (nM / kVec);
    TORCH_CHECK(items < 2147483648L, "char_embed_fwd: T * nC * nM too large");
    TORCH_CHECK(ldX % kVec == 0 && col_off % kVec == 0 && aligned16(X.data_ptr()) &&
                    aligned16(E.data_ptr()),
                "char_embed_fwd: blocks not 16-byte aligned");
    hipLaunchKernelGGL((char_embed_fwd_kernel<scalar_t, kVec>),
                       dim3((unsigned)((items + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                       stream, (const scalar_t*)E.data_ptr(), ids.data_ptr<uint8_t>(),
                       (scalar_t*)X.data_ptr() + col_off, nT, (int)nC, (int)nM, ldX);
  });
}

// dE [nC, 256, nM] in dX's dtype; dX is the [T, nC * nM] column block of the
// embed gradient (a row view, innermost stride 1, read in place).
at::Tensor char_embed_bwd(at::Tensor dX, at::Tensor ids, int64_t nC, int64_t nM,
                          bool deterministic) {
  ce::check_shape(nC, nM);
  ce::check_ids(ids, nC);
  const long nT = ids.size(0);
  TORCH_CHECK(dX.is_cuda() && dX.dim() == 2 && dX.stride(1) == 1 && dX.size(0) == nT &&
                  dX.size(1) == nC * nM,
              "char_embed_bwd: dX must be a GPU [T, nC * nM] row view");
  const long ldX = nT > 1 ? dX.stride(0) : nC * nM;
  auto dE = at::empty({nC, (long)SRX_CE_BINS, nM}, dX.options());
  if (nT == 0) return dE.zero_();
  const auto sl = char_embed_slices(nT, nC);
  const long S = sl[0], per = sl[1];
  const long n = nC * SRX_CE_BINS * nM;
  auto part = at::empty({S, n}, dX.options().dtype(at::kFloat));
  const size_t lds = (size_t)SRX_CE_BINS * nM * sizeof(float);
  const dim3 grid((unsigned)nC, (unsigned)S);
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_CE_BWD(DET_, NT_)                                                       \
  {                                                                                 \
    static bool attr_set = false;                                                   \
    if (!attr_set) {                                                                \
      (void)hipFuncSetAttribute(                                                    \
          (const void*)char_embed_bwd_kernel<scalar_t, kVec, DET_>,                 \
          hipFuncAttributeMaxDynamicSharedMemorySize, SRX_CE_BINS * 128 * 4);       \
      attr_set = true;                                                              \
    }                                                                               \
    hipLaunchKernelGGL((char_embed_bwd_kernel<scalar_t, kVec, DET_>), grid,         \
                       dim3(NT_), lds, stream, (const scalar_t*)dX.data_ptr(),      \
                       ids.data_ptr<uint8_t>(), part.data_ptr<float>(), nT, per,    \
                       (int)nC, (int)nM, ldX);                                      \
  }
  DISPATCH_F(dX.scalar_type(), {
    TORCH_CHECK(ldX % kVec == 0 && aligned16(dX.data_ptr()),
                "char_embed_bwd: dX rows not 16-byte aligned");
    if (deterministic)
      SRX_CE_BWD(true, SRX_WAVE)
    else
      SRX_CE_BWD(false, SRX_CE_THREADS)
    hipLaunchKernelGGL((char_embed_reduce_kernel<scalar_t, kVec>),
                       dim3((unsigned)((n / kVec + kBlock - 1) / kBlock)), dim3(kBlock),
                       0, stream, part.data_ptr<float>(), (scalar_t*)dE.data_ptr(), n, S);
  });
#undef SRX_CE_BWD
  return dE;
}

}  // namespace

void bind_vectors(py::module_& m) {
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
  m.def("char_embed_slices", &char_embed_slices, py::arg("T"), py::arg("nC"));
  m.def("char_embed_fwd", &char_embed_fwd, py::arg("E"), py::arg("ids"), py::arg("X"),
        py::arg("col_off") = 0);
  m.def("char_embed_bwd", &char_embed_bwd, py::arg("dX_view"), py::arg("ids"),
        py::arg("nC"), py::arg("nM"), py::arg("deterministic") = false);
}
