"""Static word vectors: the table behind `include_static_vectors`.

A `Vectors` object is three arrays: `data` [V, nM] float32, `keys` (sorted
uint64 MurmurHash64A of the word, the same hash the StringStore and the
NORM column of `Doc.attr_hashes` use) and `rows` (int32, parallel to `keys`;
several keys may share a row).  Lookup is one `np.searchsorted` over a whole
batch of hashes: -1 means out of vocabulary.

The table is data, not a parameter: it hangs on the `Vocab`, is shared by
every component, never enters a module's `state_dict`, the optimizer or the
gradient buckets, and is copied to a device once per (device, dtype).  The
GPU copy is bf16 with the row stride padded with zeros to a multiple of 32,
which makes every row 16-byte aligned for the gather kernels
(ops/kernels/srx_staticvec.hip.h).
"""
from __future__ import annotations

import gzip
import json
from pathlib import Path
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from spacy_ray_amd import _srx_cpu

KEY_ATTRS = ("ORTH", "LOWER", "NORM")


def roundup(n: int, m: int) -> int:
    return -(-n // m) * m


def hash_words(words: Sequence[str]) -> np.ndarray:
    if not len(words):
        return np.zeros(0, dtype=np.uint64)
    return np.asarray(_srx_cpu.hash_strings(list(words)), dtype=np.uint64)


class Vectors:
    def __init__(self, data: np.ndarray, keys: np.ndarray,
                 rows: Optional[np.ndarray] = None, *, name: str = "vectors",
                 key_attr: str = "ORTH") -> None:
        data = np.ascontiguousarray(data, dtype=np.float32)
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
        if data.ndim != 2:
            raise ValueError(f"vectors data must be [V, nM], got {data.shape}")
        if rows is None:
            if len(keys) != data.shape[0]:
                raise ValueError(
                    f"{len(keys)} keys for {data.shape[0]} vector rows")
            rows = np.arange(len(keys), dtype=np.int32)
        rows = np.asarray(rows, dtype=np.int32).reshape(-1)
        if len(rows) != len(keys):
            raise ValueError("vectors keys and rows must be parallel")
        if len(rows) and (rows.min() < 0 or rows.max() >= data.shape[0]):
            raise ValueError("vectors rows point outside the data")
        if key_attr not in KEY_ATTRS:
            raise ValueError(f"vectors key_attr must be one of {KEY_ATTRS}")
        order = np.argsort(keys, kind="stable")
        keys, rows = keys[order], rows[order]
        if len(keys) > 1:
            # a word listed twice keeps its first entry
            first = np.concatenate([[True], keys[1:] != keys[:-1]])
            keys, rows = keys[first], rows[first]
        self.data = data
        self.keys = np.ascontiguousarray(keys)
        self.rows = np.ascontiguousarray(rows)
        self.name = name
        self.key_attr = key_attr
        self._device: Dict[Tuple[str, str], object] = {}

    # ------------------------------------------------------------ building
    @classmethod
    def from_words(cls, words: Sequence[str], data: np.ndarray, **kw) -> "Vectors":
        return cls(data, hash_words(words), **kw)

    @property
    def shape(self) -> Tuple[int, int]:
        return tuple(self.data.shape)

    @property
    def width(self) -> int:
        return int(self.data.shape[1])

    def __len__(self) -> int:
        return int(self.data.shape[0])

    def __repr__(self) -> str:
        return (f"Vectors(name={self.name!r}, shape={self.shape}, "
                f"keys={len(self.keys)}, key_attr={self.key_attr!r})")

    # -------------------------------------------------------------- lookup
    def find_rows(self, hashes: np.ndarray) -> np.ndarray:
        """uint64 hashes [n] -> int32 rows [n], -1 = out of vocabulary.
        Every returned row is < len(self): the range check the kernels rely
        on is done here, on the host."""
        hashes = np.asarray(hashes, dtype=np.uint64).reshape(-1)
        if not len(self.keys) or not len(hashes):
            return np.full(len(hashes), -1, dtype=np.int32)
        pos = np.searchsorted(self.keys, hashes)
        pos[pos == len(self.keys)] = 0
        hit = self.keys[pos] == hashes
        return np.where(hit, self.rows[pos], -1).astype(np.int32)

    def find_words(self, words: Sequence[str]) -> np.ndarray:
        return self.find_rows(hash_words(words))

    # --------------------------------------------------------- device copy
    def device_table(self, device, dtype):
        """The table on `device`, cached per (device, dtype).  bf16 copies
        are [V, roundup(nM, 32)] with zero padding; others are [V, nM]."""
        import torch

        device = torch.device(device)
        key = (str(device), str(dtype))
        table = self._device.get(key)
        if table is None:
            src = torch.from_numpy(self.data)
            if dtype == torch.bfloat16:
                V, nM = self.shape
                table = torch.zeros(V, roundup(nM, 32), dtype=dtype)
                table[:, :nM] = src.to(dtype)
            else:
                table = src.to(dtype)
            table = table.to(device)
            self._device[key] = table
        return table

    # ------------------------------------------------------- serialisation
    def to_disk(self, vocab_dir) -> None:
        from safetensors.numpy import save_file

        vocab_dir = Path(vocab_dir)
        vocab_dir.mkdir(parents=True, exist_ok=True)
        save_file({"data": self.data, "keys": self.keys.view(np.int64),
                   "rows": self.rows}, str(vocab_dir / "vectors.safetensors"))
        (vocab_dir / "vectors.json").write_text(json.dumps(
            {"name": self.name, "shape": list(self.shape),
             "key_attr": self.key_attr}, indent=2))

    @classmethod
    def from_disk(cls, vocab_dir) -> Optional["Vectors"]:
        """None when the directory holds no vectors."""
        from safetensors.numpy import load_file

        vocab_dir = Path(vocab_dir)
        if not (vocab_dir / "vectors.safetensors").exists():
            return None
        meta = json.loads((vocab_dir / "vectors.json").read_text())
        arrs = load_file(str(vocab_dir / "vectors.safetensors"))
        return cls(arrs["data"], arrs["keys"].view(np.uint64), arrs["rows"],
                   name=meta.get("name", "vectors"),
                   key_attr=meta.get("key_attr", "ORTH"))


def load_vectors_dir(path) -> Vectors:
    """Vectors of a pipeline directory (as written by `init vectors` or
    `Language.to_disk`)."""
    path = Path(path)
    vectors = Vectors.from_disk(path / "vocab")
    if vectors is None:
        raise ValueError(
            f"{path} holds no vectors (expected vocab/vectors.safetensors) — "
            f"create it with `spacy-mi init vectors <lang> <vectors.txt> {path}`")
    return vectors


def read_word2vec_text(path, truncate: int = 0):
    """word2vec text format -> (words, data).  The `V D` header line is
    optional; every other line is a word and D floats."""
    path = Path(path)
    opener = gzip.open if path.suffix == ".gz" else open
    words, vecs = [], []
    dim = None
    with opener(path, "rt", encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip():
                continue
            parts = line.rstrip().split(" ")
            if lineno == 1 and len(parts) == 2:
                try:
                    int(parts[0]), int(parts[1])
                    dim = int(parts[1])
                    continue
                except ValueError:
                    pass
            if truncate and len(words) >= truncate:
                break
            if dim is None:
                dim = len(parts) - 1
            if len(parts) != dim + 1 or dim < 1:
                raise ValueError(
                    f"{path}: line {lineno}: expected a word and {dim} "
                    f"floats, got {len(parts)} fields")
            try:
                vec = np.asarray(parts[1:], dtype=np.float32)
            except ValueError:
                raise ValueError(
                    f"{path}: line {lineno}: vector values must be floats"
                ) from None
            words.append(parts[0])
            vecs.append(vec)
    if not words:
        raise ValueError(f"{path}: no vectors found")
    return words, np.stack(vecs)


def cosine(a: np.ndarray, b: np.ndarray) -> float:
    na, nb = float(np.linalg.norm(a)), float(np.linalg.norm(b))
    if na == 0.0 or nb == 0.0:
        return 0.0
    return float(np.dot(a, b) / (na * nb))
