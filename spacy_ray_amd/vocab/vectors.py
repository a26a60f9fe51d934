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

Floret mode (`mode="floret"`) has no word-to-row map: `data` is a hashed
n-gram table and a word's vector is the mean of the rows its character
n-grams hash to (`ngram_rows`), so no word is out of vocabulary.  The batch
path deduplicates the words, expands only the distinct ones and averages
their rows on the device (ops/kernels/srx_floret.hip.h).
"""
from __future__ import annotations

import gzip
import json
from pathlib import Path
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from spacy_ray_amd import _srx_cpu

KEY_ATTRS = ("ORTH", "LOWER", "NORM")
MODES = ("default", "floret")
# floret needs the string itself; only ORTH and LOWER can be rebuilt from a
# Doc's words
FLORET_KEY_ATTRS = ("ORTH", "LOWER")
FLORET_SETTINGS = ("minn", "maxn", "hash_count", "hash_seed", "bow", "eow")


def roundup(n: int, m: int) -> int:
    return -(-n // m) * m


def hash_words(words: Sequence[str]) -> np.ndarray:
    if not len(words):
        return np.zeros(0, dtype=np.uint64)
    return np.asarray(_srx_cpu.hash_strings(list(words)), dtype=np.uint64)


def floret_key_attr_error(key_attr: str) -> Optional[str]:
    """Why `key_attr` cannot key a floret table, or None when it can."""
    if key_attr in FLORET_KEY_ATTRS:
        return None
    if key_attr == "NORM":
        return ("floret vectors cannot use key_attr = 'NORM': floret hashes "
                "the character n-grams of the string, and only the hash of "
                "NORM is kept on a Doc; use 'ORTH' or 'LOWER'")
    return (f"floret vectors key_attr must be one of {FLORET_KEY_ATTRS}, "
            f"got {key_attr!r}")


class Vectors:
    def __init__(self, data: np.ndarray, keys: Optional[np.ndarray] = None,
                 rows: Optional[np.ndarray] = None, *, name: str = "vectors",
                 key_attr: str = "ORTH", mode: str = "default",
                 minn: int = 0, maxn: int = 0, hash_count: int = 1,
                 hash_seed: int = 0, bow: str = "<", eow: str = ">") -> None:
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim != 2:
            raise ValueError(f"vectors data must be [V, nM], got {data.shape}")
        if mode not in MODES:
            raise ValueError(f"vectors mode must be one of {MODES}, got {mode!r}")
        self.mode = mode
        self.minn, self.maxn = int(minn), int(maxn)
        self.hash_count, self.hash_seed = int(hash_count), int(hash_seed)
        self.bow, self.eow = str(bow), str(eow)
        if mode == "floret":
            if keys is not None or rows is not None:
                raise ValueError("floret vectors have no keys / rows")
            if not 1 <= self.minn <= self.maxn:
                raise ValueError(
                    f"floret vectors need 1 <= minn <= maxn, got minn = "
                    f"{minn}, maxn = {maxn}")
            if not 1 <= self.hash_count <= 4:
                raise ValueError(
                    f"floret vectors need hash_count in 1..4, got {hash_count}")
            if not 0 <= self.hash_seed < 2 ** 32:
                raise ValueError("floret hash_seed must fit in uint32")
            if not data.shape[0]:
                raise ValueError("a floret table needs at least one row")
            err = floret_key_attr_error(key_attr)
            if err:
                raise ValueError(err)
            self.data = data
            self.keys = np.zeros(0, dtype=np.uint64)
            self.rows = np.zeros(0, dtype=np.int32)
            self.name = name
            self.key_attr = key_attr
            self._device = {}
            return
        if keys is None:
            raise ValueError("vectors in default mode need keys")
        keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
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

    @property
    def is_floret(self) -> bool:
        return self.mode == "floret"

    def floret_settings(self) -> Dict[str, object]:
        return {k: getattr(self, k) for k in FLORET_SETTINGS}

    def __repr__(self) -> str:
        if self.is_floret:
            return (f"Vectors(name={self.name!r}, shape={self.shape}, "
                    f"mode='floret', minn={self.minn}, maxn={self.maxn}, "
                    f"hash_count={self.hash_count}, hash_seed={self.hash_seed}, "
                    f"bow={self.bow!r}, eow={self.eow!r}, "
                    f"key_attr={self.key_attr!r})")
        return (f"Vectors(name={self.name!r}, shape={self.shape}, "
                f"keys={len(self.keys)}, key_attr={self.key_attr!r})")

    # -------------------------------------------------------------- lookup
    def find_rows(self, hashes: np.ndarray) -> np.ndarray:
        """uint64 hashes [n] -> int32 rows [n], -1 = out of vocabulary.
        Every returned row is < len(self): the range check the kernels rely
        on is done here, on the host."""
        self._no_rows("find_rows")
        hashes = np.asarray(hashes, dtype=np.uint64).reshape(-1)
        if not len(self.keys) or not len(hashes):
            return np.full(len(hashes), -1, dtype=np.int32)
        pos = np.searchsorted(self.keys, hashes)
        pos[pos == len(self.keys)] = 0
        hit = self.keys[pos] == hashes
        return np.where(hit, self.rows[pos], -1).astype(np.int32)

    def find_words(self, words: Sequence[str]) -> np.ndarray:
        self._no_rows("find_words")
        return self.find_rows(hash_words(words))

    def _no_rows(self, what: str) -> None:
        if self.is_floret:
            raise ValueError(
                f"Vectors.{what}: floret vectors have no word-to-row map (a "
                f"word's vector is the mean of its n-gram rows); use "
                f"ngram_rows / get_batch, or TokenBatch.get_floret_table on "
                f"the batch path")

    # -------------------------------------------------------------- floret
    def ngram_rows(self, words: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """The n-gram table rows of each word as a CSR: (offsets int32
        [n + 1], idx int32 [nnz]).  For `padded = bow + word + eow` the
        n-grams are `padded` itself, then every code-point slice
        `padded[i:i + n]` for n = minn..maxn; each one's UTF-8 bytes go
        through murmur3_x64_128(seed = hash_seed) and the first `hash_count`
        little-endian uint32 of the result, modulo the table's rows, are its
        entries.  "" has none."""
        if not self.is_floret:
            raise ValueError("Vectors.ngram_rows needs mode = 'floret'")
        return _srx_cpu.floret_ngram_rows(
            list(words), self.minn, self.maxn, self.hash_count, self.hash_seed,
            self.bow, self.eow, len(self))

    def get_batch(self, words: Sequence[str]) -> np.ndarray:
        """float32 [n, nM]: each word's vector.  Floret: the mean of the
        word's n-gram rows (zero for "").  Default mode: the word's row, zero
        when it is out of vocabulary."""
        out = np.zeros((len(words), self.width), dtype=np.float32)
        if not len(words):
            return out
        if not self.is_floret:
            rows = self.find_words(words)
            out[rows >= 0] = self.data[rows[rows >= 0]]
            return out
        offsets, idx = self.ngram_rows(words)
        counts = np.diff(offsets)
        full = counts > 0
        if full.any():
            # reduceat over the starts of the non-empty slices only: an
            # empty slice would otherwise return the row at its offset
            sums = np.add.reduceat(self.data[idx], offsets[:-1][full], axis=0)
            out[full] = sums / counts[full, None].astype(np.float32)
        return out

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
             "key_attr": self.key_attr, **self._mode_meta()}, indent=2))

    def _mode_meta(self) -> Dict[str, object]:
        # default-mode files keep their earlier form
        if not self.is_floret:
            return {}
        return {"mode": self.mode, **self.floret_settings()}

    @classmethod
    def from_disk(cls, vocab_dir) -> Optional["Vectors"]:
        """None when the directory holds no vectors."""
        from safetensors.numpy import load_file

        vocab_dir = Path(vocab_dir)
        if not (vocab_dir / "vectors.safetensors").exists():
            return None
        meta = json.loads((vocab_dir / "vectors.json").read_text())
        arrs = load_file(str(vocab_dir / "vectors.safetensors"))
        if meta.get("mode", "default") == "floret":
            return cls(arrs["data"], mode="floret",
                       name=meta.get("name", "vectors"),
                       key_attr=meta.get("key_attr", "ORTH"),
                       **{k: meta[k] for k in FLORET_SETTINGS})
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


def read_floret_text(path):
    """floret's `.floret` text format (`.gz` too) -> (data float32 [rows,
    dim], settings).  The header is one line of eight fields, `rows dim minn
    maxn hash_count hash_seed bow eow`; every other line is a row index and
    `dim` floats.  Rows may come in any order; each index 0..rows-1 must
    appear exactly once."""
    path = Path(path)
    opener = gzip.open if path.suffix == ".gz" else open
    data = None
    seen = None
    settings: Dict[str, object] = {}
    with opener(path, "rt", encoding="utf8") as f:
        for lineno, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if data is None:
                parts = line.split(" ")
                if len(parts) != 8:
                    raise ValueError(
                        f"{path}: line {lineno}: expected the floret header "
                        f"`rows dim minn maxn hash_count hash_seed bow eow`, "
                        f"got {len(parts)} fields")
                try:
                    nrows, dim, minn, maxn, hash_count, hash_seed = (
                        int(x) for x in parts[:6])
                except ValueError:
                    raise ValueError(
                        f"{path}: line {lineno}: the first six header fields "
                        f"must be integers") from None
                if nrows < 1 or dim < 1:
                    raise ValueError(
                        f"{path}: line {lineno}: rows and dim must be positive")
                settings = {"minn": minn, "maxn": maxn, "hash_count": hash_count,
                            "hash_seed": hash_seed, "bow": parts[6],
                            "eow": parts[7]}
                data = np.zeros((nrows, dim), dtype=np.float32)
                seen = np.zeros(nrows, dtype=bool)
                continue
            if not line.strip():
                continue
            parts = line.rstrip().split(" ")
            if len(parts) != data.shape[1] + 1:
                raise ValueError(
                    f"{path}: line {lineno}: expected a row index and "
                    f"{data.shape[1]} floats, got {len(parts)} fields")
            try:
                row = int(parts[0])
            except ValueError:
                raise ValueError(
                    f"{path}: line {lineno}: the row index must be an integer"
                ) from None
            if not 0 <= row < data.shape[0]:
                raise ValueError(
                    f"{path}: line {lineno}: row index {row} outside "
                    f"0..{data.shape[0] - 1}")
            if seen[row]:
                raise ValueError(
                    f"{path}: line {lineno}: row index {row} appears twice")
            try:
                data[row] = np.asarray(parts[1:], dtype=np.float32)
            except ValueError:
                raise ValueError(
                    f"{path}: line {lineno}: vector values must be floats"
                ) from None
            seen[row] = True
    if data is None:
        raise ValueError(f"{path}: no floret header found")
    if not seen.all():
        missing = int(np.flatnonzero(~seen)[0])
        raise ValueError(
            f"{path}: {int((~seen).sum())} of {len(seen)} rows are missing "
            f"(first: {missing})")
    return data, settings


def cosine(a: np.ndarray, b: np.ndarray) -> float:
    na, nb = float(np.linalg.norm(a)), float(np.linalg.norm(b))
    if na == 0.0 or nb == 0.0:
        return 0.0
    return float(np.dot(a, b) / (na * nb))
