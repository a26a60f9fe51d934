// spacy_ray_amd._srx_hip_vecsim — launcher and binding of the cosine top-n
// kernels (srx_vecsim.hip.h).  A translation unit and an extension module of
// its own, because it is compiled with packed fp32 instructions off
// (setup.py) while _srx_hip keeps the flags it was measured with.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <algorithm>
#include <climits>
#include <tuple>

#include "srx_vecsim.hip.h"

namespace {

void check_vecsim_table(const at::Tensor& table, const char* what) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kBFloat16 &&
                  table.dim() == 2 && table.is_contiguous(),
              what, ": table must be a contiguous bf16 GPU matrix [V, nMp]");
  const long nMp = table.size(1);
  TORCH_CHECK(nMp % 32 == 0 && nMp >= 32 && nMp <= 320, what,
              ": table row stride must be a multiple of 32, 32..320");
  TORCH_CHECK(table.size(0) >= 1 && table.size(0) <= INT_MAX - 2 * SRX_VECSIM_TR,
              what, ": 1 <= V < 2^31 - 128");
  TORCH_CHECK(((uintptr_t)table.data_ptr() & 15) == 0, what,
              ": table not 16-byte aligned");
}

// inv(t_r) = 1 / |t_r| (0 for an all-zero row), fp32 [V]
at::Tensor vectors_row_inv(at::Tensor table) {
  check_vecsim_table(table, "vectors_row_inv");
  const long V = table.size(0);
  auto inv = at::empty({V}, table.options().dtype(at::kFloat));
  const long threads = V * 16;
  hipLaunchKernelGGL(vecsim_rowinv_kernel, dim3((unsigned)((threads + 255) / 256)),
                     dim3(256), 0, at::cuda::getCurrentCUDAStream(),
                     (const bf16_t*)table.data_ptr(), inv.data_ptr<float>(), (int)V,
                     (int)table.size(1));
  return inv;
}

struct VecsimArgs {
  const bf16_t* queries;
  const bf16_t* table;
  const float* invt;
  int* out_rows;
  float* out_scores;
  float* ws_s;
  int* ws_r;
  float* ws_invq;
  long nQ;
  int V, n, ntiles, qtiles, splits;
  hipStream_t stream;
};

template <int KC, int N>
void launch_vecsim(const VecsimArgs& a) {
  constexpr int lds = vecsim_lds_bytes(KC);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)vecsim_topn_kernel<KC, N>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_set = true;
  }
  hipLaunchKernelGGL((vecsim_topn_kernel<KC, N>),
                     dim3((unsigned)a.qtiles, (unsigned)a.splits),
                     dim3(SRX_VECSIM_THREADS), lds, a.stream, a.queries, a.table,
                     a.invt, a.out_rows, a.out_scores, a.ws_s, a.ws_r, a.ws_invq,
                     a.nQ, a.V, a.n, a.ntiles);
  if (a.splits > 1)
    hipLaunchKernelGGL((vecsim_merge_kernel<N>),
                       dim3((unsigned)((a.nQ + 3) / 4)), dim3(256), 0, a.stream,
                       (const float*)a.ws_s, (const int*)a.ws_r,
                       (const float*)a.ws_invq, a.out_rows, a.out_scores, a.nQ,
                       a.splits, a.n);
}

template <int N>
void launch_vecsim_kc(int kc, const VecsimArgs& a) {
  switch (kc) {
    case 1: launch_vecsim<1, N>(a); break;
    case 2: launch_vecsim<2, N>(a); break;
    case 3: launch_vecsim<3, N>(a); break;
    case 4: launch_vecsim<4, N>(a); break;
    case 5: launch_vecsim<5, N>(a); break;
    case 6: launch_vecsim<6, N>(a); break;
    case 7: launch_vecsim<7, N>(a); break;
    case 8: launch_vecsim<8, N>(a); break;
    case 9: launch_vecsim<9, N>(a); break;
    default: launch_vecsim<10, N>(a); break;
  }
}

// rows int32 [nQ, n], scores fp32 [nQ, n]: per query the n best table rows by
// cosine similarity, sorted by (score descending, row ascending).  splits = 0
// lets the launcher choose how many workgroups share the table rows of one
// query tile; a positive value forces it (clamped to the number of 64-row
// table tiles).  table_inv is vectors_row_inv(table), computed here when it
// is not given.
std::tuple<at::Tensor, at::Tensor> vectors_most_similar(
    at::Tensor queries, at::Tensor table, int64_t n, int64_t splits,
    c10::optional<at::Tensor> table_inv) {
  check_vecsim_table(table, "vectors_most_similar");
  const long V = table.size(0), nMp = table.size(1);
  TORCH_CHECK(queries.is_cuda() && queries.scalar_type() == at::kBFloat16 &&
                  queries.dim() == 2 && queries.is_contiguous() &&
                  queries.size(1) == nMp,
              "vectors_most_similar: queries must be a contiguous bf16 GPU matrix "
              "[nQ, nMp] of the table's row stride");
  TORCH_CHECK(queries.get_device() == table.get_device(),
              "vectors_most_similar: queries and table on different devices");
  TORCH_CHECK(((uintptr_t)queries.data_ptr() & 15) == 0,
              "vectors_most_similar: queries not 16-byte aligned");
  TORCH_CHECK(n >= 1 && n <= 8 && n <= V,
              "vectors_most_similar: need 1 <= n <= min(8, V), got n = ", n);
  TORCH_CHECK(splits >= 0, "vectors_most_similar: splits must be >= 0");
  const long nQ = queries.size(0);
  auto rows = at::empty({nQ, n}, table.options().dtype(at::kInt));
  auto scores = at::empty({nQ, n}, table.options().dtype(at::kFloat));
  if (nQ == 0) return {rows, scores};

  at::Tensor invt;
  if (table_inv.has_value()) {
    invt = *table_inv;
    TORCH_CHECK(invt.is_cuda() && invt.scalar_type() == at::kFloat &&
                    invt.dim() == 1 && invt.size(0) == V && invt.is_contiguous() &&
                    invt.get_device() == table.get_device(),
                "vectors_most_similar: table_inv must be fp32 [V] on the table's "
                "device");
  } else {
    invt = vectors_row_inv(table);
  }

  const long ntiles = (V + SRX_VECSIM_TR - 1) / SRX_VECSIM_TR;
  const long qtiles = (nQ + SRX_VECSIM_QT - 1) / SRX_VECSIM_QT;
  TORCH_CHECK(qtiles < (1L << 31), "vectors_most_similar: too many queries");
  long S = splits;
  if (S == 0) {
    // one workgroup per CU (up to 84 KB of LDS, 8 waves).  With fewer query
    // tiles than two per CU the table rows are shared out, a split keeping
    // at least 8 tiles so that the merge stays small against the scan.
    const long want = 2L * at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    S = qtiles >= want ? 1 : (want + qtiles - 1) / qtiles;
    S = std::min(S, std::max<long>(ntiles / 8, 1));
  }
  S = std::min<long>(std::min(S, ntiles), 65535);
  const int N = n == 1 ? 1 : 8;

  at::Tensor ws_s, ws_r, ws_invq;
  if (S > 1) {
    ws_s = at::empty({S, nQ, N}, scores.options());
    ws_r = at::empty({S, nQ, N}, rows.options());
    ws_invq = at::empty({nQ}, scores.options());
  }
  VecsimArgs a;
  a.queries = (const bf16_t*)queries.data_ptr();
  a.table = (const bf16_t*)table.data_ptr();
  a.invt = invt.data_ptr<float>();
  a.out_rows = rows.data_ptr<int>();
  a.out_scores = scores.data_ptr<float>();
  a.ws_s = S > 1 ? ws_s.data_ptr<float>() : nullptr;
  a.ws_r = S > 1 ? ws_r.data_ptr<int>() : nullptr;
  a.ws_invq = S > 1 ? ws_invq.data_ptr<float>() : nullptr;
  a.nQ = nQ;
  a.V = (int)V;
  a.n = (int)n;
  a.ntiles = (int)ntiles;
  a.qtiles = (int)qtiles;
  a.splits = (int)S;
  a.stream = at::cuda::getCurrentCUDAStream();
  if (N == 1)
    launch_vecsim_kc<1>((int)(nMp / 32), a);
  else
    launch_vecsim_kc<8>((int)(nMp / 32), a);
  return {rows, scores};
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("vectors_row_inv", &vectors_row_inv, py::arg("table"));
  m.def("vectors_most_similar", &vectors_most_similar, py::arg("queries"),
        py::arg("table"), py::arg("n"), py::arg("splits") = 0,
        py::arg("table_inv") = py::none());
  m.attr("VECSIM_TABLE_TILE") = SRX_VECSIM_TR;
  m.attr("VECSIM_QUERY_TILE") = SRX_VECSIM_QT;
}
