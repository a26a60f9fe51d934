// _srx_cpu: CPU-side native core (pybind11 + numpy, no torch headers).
// Round 1 contents: MurmurHash3 hashing (StringStore + HashEmbed row hashing,
// SURVEY.md §2.2 N3).  Transition systems (arc-eager parser / BILUO NER,
// SURVEY.md §2.2 N7) live in transitions.cpp, same module.
#include <pybind11/pybind11.h>
#include <pybind11/numpy.h>
#include <pybind11/stl.h>

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "murmur3.h"

namespace py = pybind11;

static py::array_t<uint64_t> hash_strings(const std::vector<std::string>& strs) {
  py::array_t<uint64_t> out((py::ssize_t)strs.size());
  auto r = out.mutable_unchecked<1>();
  for (py::ssize_t i = 0; i < (py::ssize_t)strs.size(); i++) {
    r(i) = srx::hash_utf8(strs[i].data(), (int)strs[i].size());
  }
  return out;
}

static uint64_t hash_string(const std::string& s) {
  return srx::hash_utf8(s.data(), (int)s.size());
}

// Thinc Ops.hash contract: (n,) uint64 ids -> (n, 4) uint32 hash lanes.
static py::array_t<uint32_t> hash4(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ids,
                                   uint32_t seed) {
  py::ssize_t n = ids.shape(0);
  py::array_t<uint32_t> out({n, (py::ssize_t)4});
  auto in = ids.unchecked<1>();
  auto r = out.mutable_unchecked<2>();
  for (py::ssize_t i = 0; i < n; i++) {
    uint32_t h[4];
    srx::murmur3_hash4_u64(in(i), seed, h);
    r(i, 0) = h[0]; r(i, 1) = h[1]; r(i, 2) = h[2]; r(i, 3) = h[3];
  }
  return out;
}

// HashEmbed row ids: (n,) uint64 keys -> (n,4) int32 rows in [0, nrows).
static py::array_t<int32_t> hashembed_rows(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> ids,
                                           uint32_t seed, uint32_t nrows) {
  py::ssize_t n = ids.shape(0);
  py::array_t<int32_t> out({n, (py::ssize_t)4});
  auto in = ids.unchecked<1>();
  auto r = out.mutable_unchecked<2>();
  for (py::ssize_t i = 0; i < n; i++) {
    uint32_t h[4];
    srx::murmur3_hash4_u64(in(i), seed, h);
    r(i, 0) = (int32_t)(h[0] % nrows);
    r(i, 1) = (int32_t)(h[1] % nrows);
    r(i, 2) = (int32_t)(h[2] % nrows);
    r(i, 3) = (int32_t)(h[3] % nrows);
  }
  return out;
}

// Floret n-gram rows (vocab/vectors.py, floret mode): every word expands to
// the table rows of `bow + word + eow` itself and of its character n-grams,
// n = minn..maxn, by code point; an n-gram's rows are the first
// `hash_count` little-endian uint32 of murmur3_x64_128(utf8, seed) modulo
// `nrows`.  Returns the CSR (offsets int32 [U + 1], idx int32 [nnz]),
// entries n-gram-major, then hash index.  "" has no entries.
static py::tuple floret_ngram_rows(const std::vector<std::string>& words,
                                   int minn, int maxn, int hash_count,
                                   uint32_t seed, const std::string& bow,
                                   const std::string& eow, uint32_t nrows) {
  if (minn < 1 || maxn < minn)
    throw std::invalid_argument("floret: need 1 <= minn <= maxn");
  if (hash_count < 1 || hash_count > 4)
    throw std::invalid_argument("floret: hash_count must be in 1..4");
  if (nrows == 0) throw std::invalid_argument("floret: the table has no rows");
  const size_t U = words.size();
  if (U >= (size_t)std::numeric_limits<int32_t>::max())
    throw std::overflow_error("floret: too many words for int32 offsets");
  std::vector<int32_t> offsets(U + 1, 0);
  std::vector<int32_t> idx;
  std::string padded;
  std::vector<int> cp;  // byte offset of every code point, plus the end
  auto emit = [&](const char* p, int len) {
    uint64_t h[2];
    srx::murmur3_x64_128(p, len, seed, h);
    const uint32_t lanes[4] = {(uint32_t)(h[0] & 0xffffffffULL), (uint32_t)(h[0] >> 32),
                               (uint32_t)(h[1] & 0xffffffffULL), (uint32_t)(h[1] >> 32)};
    for (int k = 0; k < hash_count; k++) idx.push_back((int32_t)(lanes[k] % nrows));
  };
  for (size_t u = 0; u < U; u++) {
    if (!words[u].empty()) {
      padded.assign(bow);
      padded += words[u];
      padded += eow;
      cp.clear();
      for (size_t b = 0; b < padded.size(); b++)
        if (((unsigned char)padded[b] & 0xC0) != 0x80) cp.push_back((int)b);
      const int L = (int)cp.size();
      cp.push_back((int)padded.size());
      emit(padded.data(), (int)padded.size());
      for (int n = minn; n <= maxn && n <= L; n++)
        for (int i = 0; i + n <= L; i++)
          emit(padded.data() + cp[i], cp[i + n] - cp[i]);
    }
    if (idx.size() > (size_t)std::numeric_limits<int32_t>::max())
      throw std::overflow_error(
          "floret: the batch's n-gram entries do not fit in int32; "
          "split the batch");
    offsets[u + 1] = (int32_t)idx.size();
  }
  py::array_t<int32_t> off_arr((py::ssize_t)offsets.size());
  py::array_t<int32_t> idx_arr((py::ssize_t)idx.size());
  std::memcpy(off_arr.mutable_data(), offsets.data(), offsets.size() * sizeof(int32_t));
  if (!idx.empty())
    std::memcpy(idx_arr.mutable_data(), idx.data(), idx.size() * sizeof(int32_t));
  return py::make_tuple(off_arr, idx_arr);
}

// Distinct 64-bit keys of a batch, in order of first occurrence:
// (inverse int32 [n], first int64 [U]).  keys[i] == skip_key gets
// inverse -1 and is not counted.  Open addressing over the keys' low bits
// (they are murmur hashes already); no sort.
static py::tuple dedupe_keys(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> keys,
                             uint64_t skip_key) {
  const py::ssize_t n = keys.shape(0);
  if (n >= (py::ssize_t)std::numeric_limits<int32_t>::max())
    throw std::overflow_error("dedupe_keys: too many keys for int32");
  auto in = keys.unchecked<1>();
  py::array_t<int32_t> inverse(n);
  auto inv = inverse.mutable_unchecked<1>();
  size_t cap = 16;
  while (cap < (size_t)n * 2) cap <<= 1;
  const size_t mask = cap - 1;
  std::vector<int32_t> slot(cap, -1);
  std::vector<int64_t> first;
  for (py::ssize_t i = 0; i < n; i++) {
    const uint64_t k = in(i);
    if (k == skip_key) {
      inv(i) = -1;
      continue;
    }
    size_t h = (size_t)(k ^ (k >> 32)) & mask;
    for (;;) {
      const int32_t id = slot[h];
      if (id < 0) {
        slot[h] = (int32_t)first.size();
        inv(i) = (int32_t)first.size();
        first.push_back((int64_t)i);
        break;
      }
      if (in(first[id]) == k) {
        inv(i) = id;
        break;
      }
      h = (h + 1) & mask;
    }
  }
  py::array_t<int64_t> first_arr((py::ssize_t)first.size());
  if (!first.empty())
    std::memcpy(first_arr.mutable_data(), first.data(), first.size() * sizeof(int64_t));
  return py::make_tuple(inverse, first_arr);
}

void init_transitions(py::module_& m);  // transitions.cpp

PYBIND11_MODULE(_srx_cpu, m) {
  m.doc() = "spacy_ray_amd CPU native core (murmur hashing, transition systems)";
  m.def("hash_strings", &hash_strings, "hash a list of UTF-8 strings to uint64");
  m.def("hash_string", &hash_string, "hash one UTF-8 string to uint64");
  m.def("spacy_hash_strings",
        [](const std::vector<std::string>& strs) {
          // spaCy StringStore hash (MurmurHash64A seed 1) — the `.spacy`
          // DocBin string-reference values
          py::array_t<uint64_t> out((py::ssize_t)strs.size());
          auto r = out.mutable_unchecked<1>();
          for (py::ssize_t i = 0; i < (py::ssize_t)strs.size(); i++)
            r(i) = srx::murmur2_64a(strs[i].data(), (int)strs[i].size(), 1);
          return out;
        },
        "spaCy-compatible string hashes (MurmurHash64A, seed 1)");
  m.def("spacy_hash_string", [](const std::string& s) {
    return srx::murmur2_64a(s.data(), (int)s.size(), 1);
  });
  m.def("hash4", &hash4, py::arg("ids"), py::arg("seed"),
        "murmur3 x86_128 of 8-byte keys -> (n,4) uint32");
  m.def("hashembed_rows", &hashembed_rows, py::arg("ids"), py::arg("seed"), py::arg("nrows"),
        "murmur3 row ids for HashEmbed: (n,4) int32 in [0, nrows)");
  m.def("floret_ngram_rows", &floret_ngram_rows, py::arg("words"),
        py::arg("minn"), py::arg("maxn"), py::arg("hash_count"),
        py::arg("hash_seed"), py::arg("bow"), py::arg("eow"), py::arg("nrows"),
        "floret n-gram table rows of each word as a CSR (offsets, idx)");
  m.def("dedupe_keys", &dedupe_keys, py::arg("keys"), py::arg("skip_key"),
        "distinct uint64 keys in first-occurrence order: (inverse, first)");
  init_transitions(m);
}
