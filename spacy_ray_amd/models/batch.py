"""TokenBatch: the device-side representation of a batch of Docs.

MI355X-first design (SURVEY.md §2.2 N6 disposition): attr hashes are
precomputed per Doc on the CPU once, and a batch ships to the GPU as ONE
int64 [T, 4] tensor (bit-cast uint64) + a lengths vector — no per-token
Python objects anywhere near the hot path.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from spacy_ray_amd.vocab.doc import Doc


class TokenBatch:
    __slots__ = ("attr_ids", "lengths", "n_tokens", "n_real_tokens", "docs",
                 "staged", "lengths_np", "vec_rows", "vec_rows_attr")

    def __init__(self, docs: Sequence[Doc], device: torch.device,
                 pad_to: int = 0):
        """pad_to > 0: round the token count up to a multiple by appending a
        pad pseudo-doc (zero attr ids, no annotations).  Keeps the GEMM M
        dims on a small set of repeating shapes so hipBLASLt's solution
        cache hits instead of re-selecting per batch.  Defaults: 2048 on
        GPU, none on CPU."""
        if isinstance(device, str):
            device = torch.device(device)
        self.docs = list(docs)
        lens_list = [len(d) for d in docs]
        # real (pre-pad) per-doc lengths; reused by the transition pipes'
        # state construction (a fresh 50k-doc list comprehension per pipe
        # per step showed up in profiles)
        self.lengths_np = np.asarray(lens_list, dtype=np.int32)
        real = int(sum(lens_list))
        self.n_real_tokens = real
        if pad_to == 0:
            if device.type == "cuda":
                # coarser buckets at larger T: hipBLASLt re-runs solution
                # selection per distinct M, so keep the distinct-M count tiny
                pad_to = 2048 if real < 32768 else 8192
            else:
                pad_to = 1
        padded = -(-max(real, 1) // pad_to) * pad_to if pad_to > 1 else real
        n_pad = padded - real
        if n_pad > 0:
            lens_list = lens_list + [n_pad]
        lens = np.array(lens_list, dtype=np.int64)
        arrs = [d.attr_hashes for d in docs]
        if n_pad > 0:
            arrs.append(np.zeros((n_pad, 4), dtype=np.uint64))
        attr = (np.concatenate(arrs, axis=0) if arrs
                else np.zeros((0, 4), dtype=np.uint64))
        self.n_tokens = int(lens.sum())
        from spacy_ray_amd.utils.pinned import to_device

        # bit-cast uint64 -> int64 (torch has no uint64); kernels re-interpret
        self.attr_ids = to_device(attr.view(np.int64), device)
        self.lengths = to_device(lens, device)
        # per-pipe staged device data (e.g. tagger gold ids), uploaded at
        # step start while the GPU queue is empty — a pageable H2D later in
        # the step blocks the host behind every queued kernel.  Replayed
        # batches (bench) keep the cache across steps.
        self.staged = {}
        # static vectors: one int32 [T] row tensor (-1 = OOV and pad rows),
        # shipped only when the vocab has a table AND a model asked for it
        self.vec_rows = None
        self.vec_rows_attr = None
        vocab = self.docs[0].vocab if self.docs else None
        if (vocab is not None and getattr(vocab, "vectors", None) is not None
                and vocab.vector_key_attrs):
            if vocab.vectors.is_floret:
                # floret: (inverse, offsets, idx) instead of rows, see
                # get_floret; vec_rows stays None
                self.get_floret(vocab.vector_key_attrs[0])
            else:
                self.vec_rows_attr = vocab.vector_key_attrs[0]
                self.vec_rows = self._build_vec_rows(self.vec_rows_attr)

    def _build_vec_rows(self, key_attr: str) -> torch.Tensor:
        from spacy_ray_amd.utils.pinned import to_device

        parts = [d.get_vector_rows(key_attr) for d in self.docs]
        n_pad = self.n_tokens - self.n_real_tokens
        if n_pad > 0:
            parts.append(np.full(n_pad, -1, dtype=np.int32))
        rows = (np.concatenate(parts) if parts
                else np.zeros(0, dtype=np.int32)).astype(np.int32, copy=False)
        return to_device(rows, self.attr_ids.device)

    def get_vec_rows(self, key_attr: str) -> torch.Tensor:
        """Vector rows under `key_attr`; the tensor built at construction
        when it matches, otherwise built once and kept in `staged`."""
        if self.vec_rows is not None and key_attr == self.vec_rows_attr:
            return self.vec_rows
        key = ("vec_rows", key_attr)
        if key not in self.staged:
            self.staged[key] = self._build_vec_rows(key_attr)
        return self.staged[key]

    # -------------------------------------------------------------- floret
    def _build_floret(self, key_attr: str):
        """Host side of the floret path: deduplicate the tokens over their
        64-bit key hashes (C++ hash map, no sort), expand only the distinct
        words to their n-gram rows.  Returns numpy (inverse int32 [T], -1 for
        pad tokens and empty strings; offsets int32 [U + 1]; idx int32
        [nnz]) and the U distinct strings."""
        from spacy_ray_amd import _srx_cpu
        from spacy_ray_amd.vocab.vectors import hash_words

        if not self.docs:
            return (np.full(self.n_tokens, -1, dtype=np.int32),
                    np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), [])
        vectors = self.docs[0].vocab.vectors
        parts = [d.get_vector_keys(key_attr) for d in self.docs]
        keys = (np.concatenate(parts) if parts
                else np.zeros(0, dtype=np.uint64))
        inverse, first = _srx_cpu.dedupe_keys(keys, int(hash_words([""])[0]))
        # first-occurrence token -> (doc, position): only U strings are built
        ends = np.cumsum(self.lengths_np, dtype=np.int64)
        doc_of = np.searchsorted(ends, first, side="right")
        pos_of = first - (ends[doc_of] - self.lengths_np[doc_of])
        lower = key_attr != "ORTH"
        words = []
        for di, pi in zip(doc_of.tolist(), pos_of.tolist()):
            w = self.docs[di].words[pi]
            words.append(w.lower() if lower else w)
        offsets, idx = vectors.ngram_rows(words)
        n_pad = self.n_tokens - self.n_real_tokens
        if n_pad > 0:
            inverse = np.concatenate([inverse, np.full(n_pad, -1, dtype=np.int32)])
        return inverse, offsets, idx, words

    def get_floret(self, key_attr: str):
        """Device (inverse [T], offsets [U + 1], idx [nnz]) int32 tensors of
        this batch under `key_attr`, built once and kept in `staged`."""
        key = ("floret", key_attr)
        if key not in self.staged:
            from spacy_ray_amd.utils.pinned import to_device

            device = self.attr_ids.device
            inverse, offsets, idx, _ = self._build_floret(key_attr)
            self.staged[key] = tuple(to_device(a, device)
                                     for a in (inverse, offsets, idx))
        return self.staged[key]

    def get_floret_table(self, vectors, key_attr: str, device, dtype):
        """(temporary table [U, C], inverse [T]): one averaged vector per
        distinct word, in the layout of the Vectors device table, and the
        token -> word map that stands in for the vector rows.  Computed on
        first use per (device, dtype) and kept in `staged`, so replayed
        batches and several listeners share it.  Data, not a parameter."""
        from spacy_ray_amd.ops import api as ops

        inverse, offsets, idx = self.get_floret(key_attr)
        key = ("floret_table", key_attr, str(torch.device(device)), str(dtype))
        cached = self.staged.get(key)
        if cached is None or cached[0] is not vectors:
            table = vectors.device_table(device, dtype)
            temp = ops.floret_words_mean(table, offsets, idx)
            if temp.shape[0] == 0:
                # no word at all: keep one zero row so that the table can be
                # indexed (every inverse entry is -1)
                temp = temp.new_zeros(1, temp.shape[1])
            cached = (vectors, temp)
            self.staged[key] = cached
        return cached[1], inverse

    def __len__(self) -> int:
        return len(self.docs)
