"""Tok2vec pretraining (spaCy's `spacy pretrain` role).

spaCy pretrains tok2vec on raw text with approximate-LM objectives
("characters" / "vectors") and `[initialize] init_tok2vec` then loads the
weights before supervised training.  Offline equivalent here: a masked-
token objective over the murmur-hashed vocabulary — 15% of tokens have
their attr-hash rows replaced by the "[MASK]" word's hashes and a linear
head predicts the ORIGINAL token's NORM-hash bucket from the tok2vec
output (cross-entropy over `n_buckets` classes).  The trained encoder
weights save as `tok2vec.safetensors`, loadable via
``training.init_tok2vec`` (config key or dotted CLI override) or
``spacy-mi ray train --init-tok2vec path``.

With a vectors table in the vocab, ``objective="vectors"`` is spaCy's
`PretrainVectors`: the same 15% mask, but a maxout + layer-norm + linear
head predicts the ORIGINAL token's static vector and the loss is the cosine
or L2 distance to it (``ops.vectors_loss``).
"""
from __future__ import annotations

import copy
from pathlib import Path
from typing import Iterator

import numpy as np
import torch

from spacy_ray_amd.models.batch import TokenBatch
from spacy_ray_amd.models.layers import Linear, Maxout, StaticVectors
from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.vocab.attrs import extract_attr_hashes

OBJECTIVES = ("masked", "vectors")
LOSSES = ("cosine", "L2")
PRETRAIN_VECTORS_ARCH = "spacy.PretrainVectors.v1"


def masked_batches(examples, batch_size: int, mask_rate: float, seed: int):
    """Yield lists of docs of ~batch_size docs (pretraining is raw-text:
    only the words are used)."""
    docs = [eg.reference if hasattr(eg, "reference") else eg
            for eg in examples]
    rng = np.random.RandomState(seed)
    order = rng.permutation(len(docs))
    for i in range(0, len(order), batch_size):
        yield [docs[j] for j in order[i:i + batch_size]]


def objective_from_config(cfg) -> dict:
    """Keyword arguments for pretrain_tok2vec from a config's
    `[pretraining.objective]` block (`@architectures =
    "spacy.PretrainVectors.v1"`); empty when there is none."""
    block = (cfg.get("pretraining") or {}).get("objective")
    if not block:
        return {}
    from spacy_ray_amd.config.registry import resolve_registry_ref

    block = dict(block)
    name = block.pop("@architectures", None)
    if name is None:
        raise ValueError("[pretraining.objective] needs an @architectures name "
                         f"({PRETRAIN_VECTORS_ARCH!r})")
    settings = resolve_registry_ref("architectures", name)(**block)
    if not isinstance(settings, dict) or "objective" not in settings:
        raise ValueError(
            f"[pretraining.objective]: {name!r} is not a pretraining objective")
    return settings


class VectorsHead(torch.nn.Module):
    """The output layer of `spacy.PretrainVectors.v1`: maxout (`hidden_size`
    units, `maxout_pieces` pieces) with layer norm, then a linear layer to
    the width of the vectors table.  Trained with the tok2vec, then thrown
    away."""

    def __init__(self, width: int, nM: int, hidden_size: int = 300,
                 maxout_pieces: int = 3):
        super().__init__()
        self.hidden = Maxout(width, hidden_size, pieces=maxout_pieces,
                             normalize=True)
        self.output = Linear(hidden_size, nM)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self.output(self.hidden(X))


def _masked_batch(batch: TokenBatch, ids: torch.Tensor, module, total: int,
                  mask: torch.Tensor) -> TokenBatch:
    """The batch as the tok2vec may see it: a shallow per-step copy with the
    masked attr ids and, for every StaticVectors layer of `module`, a copy of
    the vector rows (floret: of the token -> word map) with -1 at the masked
    positions, so that the input cannot carry the vector it has to predict.
    `batch` itself, which holds the target rows and may be cached or
    replayed, is not modified."""
    mb = copy.copy(batch)
    mb.staged = dict(batch.staged)
    mb.attr_ids = ids
    for layer in module.modules():
        if not isinstance(layer, StaticVectors) or layer.vectors is None:
            continue
        key = layer.key_attr
        if layer.vectors.is_floret:
            inverse, offsets, idx = batch.get_floret(key)
            inverse = inverse.clone()
            inverse[:total][mask] = -1
            mb.staged[("floret", key)] = (inverse, offsets, idx)
        else:
            rows = batch.get_vec_rows(key).clone()
            rows[:total][mask] = -1
            if mb.vec_rows is not None and key == mb.vec_rows_attr:
                mb.vec_rows = rows
            else:
                mb.staged[("vec_rows", key)] = rows
    return mb


def pretrain_tok2vec(nlp, corpus, *, steps: int = 1000, batch_docs: int = 64,
                     n_buckets: int = 4096, mask_rate: float = 0.15,
                     learn_rate: float = 1e-3, seed: int = 0,
                     log_every: int = 50, log=print,
                     objective: str = "masked", loss: str = "cosine",
                     hidden_size: int = 300, maxout_pieces: int = 3):
    """Train nlp's tok2vec on the corpus.  objective="masked" (default):
    predict the masked token's NORM-hash bucket.  objective="vectors"
    (spaCy's PretrainVectors): predict its static vector, `loss` = "cosine"
    or "L2"; needs nlp.vocab.vectors.  Returns the per-interval mean losses
    (callers assert they fall)."""
    if objective not in OBJECTIVES:
        raise ValueError(
            f"pretrain objective must be one of {OBJECTIVES}, got {objective!r}")
    if loss not in LOSSES:
        raise ValueError(f"pretrain loss must be one of {LOSSES}, got {loss!r}")
    t2v_pipe = nlp.tok2vec
    assert t2v_pipe is not None and t2v_pipe.module is not None, \
        "pretrain needs an initialized tok2vec pipe"
    module = t2v_pipe.module
    device = nlp.device
    width = t2v_pipe.width
    dtype = next(module.parameters()).dtype
    vectors = getattr(nlp.vocab, "vectors", None)
    if objective == "vectors":
        if vectors is None:
            raise ValueError(
                "the vectors pretraining objective needs a vectors table in "
                "nlp.vocab.vectors: build one with `spacy-mi init vectors` "
                "and load it with `[initialize] vectors = <path>`")
        head = VectorsHead(width, vectors.width, hidden_size, maxout_pieces)
    else:
        head = torch.nn.Linear(width, n_buckets)
    head = head.to(device).to(dtype)
    # on a GPU the loss runs in bf16, the training engine's compute type and
    # the one the fused kernel and the padded device table are made for: the
    # head's output is rounded to it, parameters and Adam state stay as they are
    loss_dtype = torch.bfloat16 if device.type == "cuda" else dtype
    params = list(module.parameters()) + list(head.parameters())
    opt = torch.optim.Adam(params, lr=learn_rate)
    mask_hashes = torch.from_numpy(
        extract_attr_hashes(["[MASK]"]).view(np.int64)).to(device)  # [1, 4]
    rng = np.random.RandomState(seed)
    examples = list(corpus(nlp))
    losses, interval = [], []
    step = 0
    while step < steps:
        for docs in masked_batches(examples, batch_docs, mask_rate,
                                   seed + step):
            if step >= steps:
                break
            batch = TokenBatch(docs, device)
            total = batch.n_real_tokens
            if total == 0:
                continue
            mask = torch.from_numpy(
                (rng.random_sample(total) < mask_rate)).to(device)
            if not bool(mask.any()):
                continue
            ids = batch.attr_ids.clone()
            # original NORM hash -> target bucket (before masking)
            targets = (ids[:total, 0].view(torch.int64).remainder(n_buckets))
            ids[:total][mask] = mask_hashes[0]
            if objective == "vectors":
                # targets: the ORIGINAL tokens' rows, from the unmasked batch
                if vectors.is_floret:
                    table, rows = batch.get_floret_table(
                        vectors, vectors.key_attr, device, loss_dtype)
                else:
                    table = vectors.device_table(device, loss_dtype)
                    rows = batch.get_vec_rows(vectors.key_attr)
                rows = rows[:total][mask]
                t2v = t2v_pipe.forward(
                    _masked_batch(batch, ids, module, total, mask))
                pred = head(t2v[:total][mask]).to(loss_dtype)
                step_loss = ops.vectors_loss(pred, table, rows, loss=loss,
                                             scale=1.0 / rows.shape[0])
            else:
                batch.attr_ids = ids
                t2v = t2v_pipe.forward(batch)
                logits = head(t2v[:total][mask])
                step_loss = torch.nn.functional.cross_entropy(
                    logits.float(), targets[mask])
            opt.zero_grad(set_to_none=True)
            step_loss.backward()
            opt.step()
            interval.append(float(step_loss.detach()))
            step += 1
            if step % log_every == 0:
                losses.append(sum(interval) / len(interval))
                log(f"[pretrain] step {step}  loss {losses[-1]:.4f}")
                interval = []
    if interval:
        losses.append(sum(interval) / len(interval))
    return losses


def save_tok2vec(nlp, out_dir) -> Path:
    from safetensors.torch import save_file

    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    module = nlp.tok2vec.module
    state = {k: v.detach().cpu().contiguous()
             for k, v in module.state_dict().items()}
    path = out / "tok2vec.safetensors"
    save_file(state, str(path))
    return path


def load_init_tok2vec(nlp, path) -> int:
    """Load pretrained tok2vec weights into the pipeline's tok2vec
    (spaCy's `[initialize] init_tok2vec` contract).  Returns the number of
    tensors loaded; shape mismatches fail loudly."""
    from safetensors.torch import load_file

    p = Path(path)
    if p.is_dir():
        p = p / "tok2vec.safetensors"
    state = load_file(str(p))
    module = nlp.tok2vec.module
    module.load_state_dict(state)
    module.to(nlp.device)
    return len(state)
