"""Building-block layers (torch modules over the ops API)."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from spacy_ray_amd.ops import api as ops


def glorot_uniform_(w: torch.Tensor) -> torch.Tensor:
    """Thinc-style Glorot/Xavier uniform init."""
    fan_in, fan_out = w.shape[-1], w.shape[0]
    limit = math.sqrt(6.0 / (fan_in + fan_out))
    with torch.no_grad():
        w.uniform_(-limit, limit)
    return w


class Maxout(nn.Module):
    """Linear (nI -> P*nO, pieces-major) followed by max over P pieces — the
    Thinc Maxout layer (SURVEY.md §2.5 maxout_fwd/bwd).  Weight rows are laid
    out pieces-major so each piece is a contiguous nO block in the GEMM
    output (coalesced maxout kernel)."""

    def __init__(self, nI: int, nO: int, pieces: int = 3, normalize: bool = False):
        super().__init__()
        self.nI, self.nO, self.pieces = nI, nO, pieces
        self.weight = nn.Parameter(glorot_uniform_(torch.empty(pieces * nO, nI)))
        self.bias = nn.Parameter(torch.zeros(pieces * nO))
        self.norm = LayerNorm(nO) if normalize else None

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        Y = ops.linear_cdw(X, self.weight, self.bias)
        Y = ops.maxout(Y.view(*Y.shape[:-1], self.pieces, self.nO))
        if self.norm is not None:
            Y = self.norm(Y)
        return Y


class LayerNorm(nn.Module):
    def __init__(self, width: int, eps: float = 1e-5):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(width))
        self.bias = nn.Parameter(torch.zeros(width))
        self.eps = eps

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return ops.layernorm(X, self.weight, self.bias, self.eps)


class StaticVectors(nn.Module):
    """spaCy's StaticVectors layer: vectors[rows] @ W^T.  One trainable
    projection `W` [nO, nM], Glorot-initialised; no bias, no dropout.  The
    output row is zero for out-of-vocabulary tokens and the pad pseudo-doc.

    The vector table itself is NOT part of the module: `vectors` is the
    vocab's Vectors object (a plain attribute, so it is in no state_dict,
    parameter list or gradient bucket), and its device copy is shared by
    every layer that uses it."""

    def __init__(self, nO: int, nM: int, key_attr: str = "ORTH", vectors=None):
        super().__init__()
        self.nO, self.nM, self.key_attr = nO, nM, key_attr
        self.W = nn.Parameter(glorot_uniform_(torch.empty(nO, nM)))
        self._check_key_attr(vectors)
        self.__dict__["vectors"] = vectors

    def _check_key_attr(self, vectors) -> None:
        if vectors is not None and vectors.is_floret:
            from spacy_ray_amd.vocab.vectors import floret_key_attr_error

            err = floret_key_attr_error(self.key_attr)
            if err:
                raise ValueError(err)

    def bind(self, vectors) -> None:
        self._check_key_attr(vectors)
        if vectors.width != self.nM:
            raise ValueError(
                f"StaticVectors was built for {self.nM}-dimensional vectors "
                f"but the vocab's table {vectors.name!r} has width "
                f"{vectors.width}")
        self.__dict__["vectors"] = vectors

    def table(self) -> torch.Tensor:
        if self.vectors is None:
            raise ValueError(
                "StaticVectors has no vector table: load one into "
                "nlp.vocab.vectors ([initialize] vectors = <path>)")
        return self.vectors.device_table(self.W.device, self.W.dtype)

    def table_and_rows(self, batch):
        """(table, rows) for ops.static_vectors / ops.multi_hashembed.  In
        floret mode the table is the batch's temporary one (a vector per
        distinct word) and the rows are the token -> word map."""
        if self.vectors is not None and self.vectors.is_floret:
            return batch.get_floret_table(self.vectors, self.key_attr,
                                          self.W.device, self.W.dtype)
        return self.table(), batch.get_vec_rows(self.key_attr)

    def forward(self, batch) -> torch.Tensor:
        table, rows = self.table_and_rows(batch)
        return ops.static_vectors(self.W, table, rows)


class Linear(nn.Module):
    def __init__(self, nI: int, nO: int, bias: bool = True):
        super().__init__()
        self.weight = nn.Parameter(glorot_uniform_(torch.empty(nO, nI)))
        self.bias = nn.Parameter(torch.zeros(nO)) if bias else None

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.linear(X, self.weight, self.bias)
