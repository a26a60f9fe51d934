// spacy_ray_amd._srx_hip — gfx950 kernel bindings (torch extension).
// Kernels live in the *.hip.h headers; each srx_bind_<family>.hip
// instantiates its family's fp32 + bf16 variants, holds the launchers and
// registers them in bind_<family>.  Together they expose the op surface
// consumed by ops/api.py and parallel/engine.py.  Tested on-GPU against
// ops/torch_ref.py fp32.
#include "srx_bind.hip.h"

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
  bind_elementwise(m);
  bind_parser(m);
  bind_mwe(m);
  bind_attn(m);
  bind_vectors(m);
  bind_pool(m);
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
