// _srx_hip bindings: HashEmbed, the parser/NER state scorer, the batched
// transition ops (cross-entropy, dPre scatter/gather) and the fused
// transition step's autograd node.
#include "srx_bind.hip.h"

#include <mutex>
#include <unordered_map>
#include <utility>

#include "srx_embed_parser.hip.h"
#include "srx_softmax_reduce.hip.h"

namespace {

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

// LDS bytes of one wave's slice in dpre_gather_kernel: cap_mult*maxlen rows
// of min(row dwords, 64) dwords.  Python asks this before choosing the path.
int64_t dpre_gather_slice_bytes(int64_t HP, int64_t elem_size,
                                int64_t cap_mult, int64_t maxlen) {
  int64_t row_dwords = HP * elem_size / 4;
  return cap_mult * maxlen * std::min<int64_t>(row_dwords, SRX_WAVE) * 4;
}

// Doc-major atomic-free dPre (GPU-state-machine arenas): one wave per doc
// gathers every (token, slot) row of its doc from LDS and stores it once
// into an UNINITIALIZED dPre — see dpre_gather_kernel.  Rows [0, pad_row)
// are all written (batch-padding tokens [doc_total, pad_row) as zeros); the
// caller fills the pad row from dPad32.  maxlen must be >= max(lens).
// Same return contract as dpre_scatter.
std::vector<at::Tensor> dpre_gather(at::Tensor dSummed, at::Tensor feats,
                                    at::Tensor dPre, at::Tensor off,
                                    at::Tensor lens, int64_t pad_row,
                                    int64_t cap_mult, int64_t maxlen,
                                    int64_t doc_total) {
  check_dev(dSummed);
  check_dev(feats);
  check_dev(dPre);
  check_dev(off);
  check_dev(lens);
  TORCH_CHECK(feats.scalar_type() == at::kLong && feats.dim() == 2);
  TORCH_CHECK(off.scalar_type() == at::kInt && lens.scalar_type() == at::kInt &&
                  off.numel() == lens.numel(),
              "dpre_gather off/lens must be int32 of one length");
  TORCH_CHECK(dSummed.is_contiguous() && feats.is_contiguous() &&
                  dPre.is_contiguous() && off.is_contiguous() &&
                  lens.is_contiguous(),
              "dpre_gather needs contiguous tensors");
  TORCH_CHECK(dPre.scalar_type() == dSummed.scalar_type(),
              "dpre_gather writes dPre in the dtype of dSummed");
  TORCH_CHECK(dSummed.dim() == 2 && dPre.dim() == 3);
  long S = dSummed.size(0);
  int nF = (int)feats.size(1);
  int HP = (int)dPre.size(2);
  long n_docs = off.numel();
  TORCH_CHECK(HP == 64 || HP == 128, "dpre_gather needs HP in {64, 128}");
  TORCH_CHECK(nF >= 1 && nF <= 16, "dpre_gather nF <= 16");
  TORCH_CHECK(feats.size(0) == S && dSummed.size(1) == HP &&
                  dPre.size(1) == nF,
              "dpre_gather shape mismatch");
  TORCH_CHECK(0 <= doc_total && doc_total <= pad_row && pad_row < dPre.size(0),
              "dpre_gather needs doc_total <= pad_row < dPre rows");
  TORCH_CHECK(cap_mult >= 1 && maxlen >= 0 && cap_mult * maxlen <= 4 * SRX_WAVE,
              "dpre_gather holds at most 256 rows per doc");
  int slice_rows = (int)std::max<int64_t>(cap_mult * maxlen, 1);
  size_t slice_bytes = (size_t)dpre_gather_slice_bytes(
      HP, dSummed.element_size(), slice_rows, 1);
  TORCH_CHECK(slice_bytes <= 64 * 1024, "dpre_gather slice exceeds 64 KB LDS");
  int nw = (int)std::min<size_t>(4, (64 * 1024) / slice_bytes);
  // 8 waves per CU cover the LDS-bound occupancy at any slice size
  long target = std::min<long>(
      std::max<long>(n_docs, 1),
      8L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount);
  int grid = (int)((target + nw - 1) / nw);
  long n_waves = (long)grid * nw;
  int ncols = HP + nF * HP;
  auto partials =
      at::empty({n_waves, (long)ncols}, dSummed.options().dtype(at::kFloat));
  auto stream = at::cuda::getCurrentCUDAStream();
#define SRX_DPRE_GATHER(HPV)                                                  \
  hipLaunchKernelGGL((dpre_gather_kernel<scalar_t, HPV>), dim3(grid),         \
                     dim3(nw * SRX_WAVE), nw * slice_bytes, stream,           \
                     (const scalar_t*)dSummed.data_ptr(),                     \
                     feats.data_ptr<int64_t>(), (scalar_t*)dPre.data_ptr(),   \
                     partials.data_ptr<float>(), off.data_ptr<int32_t>(),     \
                     lens.data_ptr<int32_t>(), n_docs, S, (long)pad_row,      \
                     (long)doc_total, nF, (int)cap_mult, slice_rows)
  DISPATCH_F(dSummed.scalar_type(), {
    if (HP == 64)
      SRX_DPRE_GATHER(64);
    else
      SRX_DPRE_GATHER(128);
  });
#undef SRX_DPRE_GATHER
  auto sums = mwe_fold_partials(partials, ncols, stream);
  return {sums.slice(0, 0, HP), sums.slice(0, HP).view({(long)nF, (long)HP})};
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

void bind_parser(py::module_& m) {
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
  m.def("fused_step",&fusedstep::fused_step);
  m.def("fused_entries_take", &fusedstep::fused_entries_take);
  m.def("transition_ce", &transition_ce, py::arg("scores"), py::arg("gold"),
        py::arg("valid"), py::arg("deterministic") = false);
  m.attr("FIXED_SCALE") = 16777216.0;
  m.def("dpre_scatter", &dpre_scatter);
  m.def("dpre_gather", &dpre_gather);
  m.def("dpre_gather_slice_bytes", &dpre_gather_slice_bytes);
}
