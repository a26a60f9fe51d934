"""CharacterEmbed on the CPU: byte features against a pure-Python version, the
module against a float64 loop, the registry entry, the example config."""
import os

import numpy as np
import pytest
import torch

from spacy_ray_amd.config.config import Config
from spacy_ray_amd.models.batch import TokenBatch
from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.vocab.doc import Doc, Vocab

CFG = os.path.join(os.path.dirname(__file__), "..", "examples", "configs",
                   "xx_tagger_charembed.cfg")


def py_utf8_row(word, n):
    b, row = word.encode("utf8"), []
    start, end = 0, len(b) - 1
    while start <= end and len(row) < n:
        row.append(b[start])
        start += 1
        if start <= end and len(row) < n:
            row.append(b[end])
            end -= 1
    return row + [255] * (n - len(row))


def reference(E, ids, dX):
    """float64, one term at a time -> (X, dE, sum|terms| per element, terms
    per bin)."""
    nC, _, nM = E.shape
    E64, dX64 = E.double().numpy().reshape(-1, nM), dX.double().numpy().reshape(-1, nM)
    flat = (ids.long().numpy() + 256 * np.arange(nC)).reshape(-1)
    X = E64[flat].reshape(len(ids), nC * nM)
    dE, mag, k = np.zeros_like(E64), np.zeros_like(E64), np.zeros((nC * 256, 1))
    np.add.at(dE, flat, dX64)
    np.add.at(mag, flat, np.abs(dX64))
    np.add.at(k, flat, 1)
    return (torch.from_numpy(X), *(torch.from_numpy(a).view(nC, 256, -1)
                                   for a in (dE, mag, k)))


@pytest.mark.parametrize("n", [1, 4, 8])
def test_to_utf8_array_matches_python(n):
    words = ["", "a", "x" * n, "y" * n + "z", "abcdefghijklmnopqrstuvwxyz", "naïve€日本"]
    doc = Doc(Vocab(), words)
    got = doc.to_utf8_array(n)
    assert got.dtype == np.uint8 and got.shape == (len(words), n)
    assert got.tolist() == [py_utf8_row(w, n) for w in words]
    assert doc.to_utf8_array(n) is got  # cached per (doc, nr_char)


def test_get_char_ids_pads_with_255():
    docs = [Doc(Vocab(), ["ab", "c"]), Doc(Vocab(), ["def"])]
    batch = TokenBatch(docs, torch.device("cpu"), pad_to=8)
    ids = batch.get_char_ids(4)
    assert ids.dtype == torch.uint8 and tuple(ids.shape) == (8, 4)
    assert ids[:3].tolist() == [py_utf8_row(w, 4) for w in ("ab", "c", "def")]
    assert (ids[3:] == 255).all() and batch.get_char_ids(4) is ids


def test_registry_resolves_and_rejects_static_vectors():
    from spacy_ray_amd.models.tok2vec import CharacterEmbed
    from spacy_ray_amd.pipeline.language import build_nlp

    text = open(CFG).read()
    nlp = build_nlp(Config.from_str(text))
    assert nlp.pipe_names == ["tok2vec", "tagger"]
    with pytest.raises(ValueError, match="not supported yet"):
        build_nlp(Config.from_str(text.replace(
            "include_static_vectors = false", "include_static_vectors = true")))
    with pytest.raises(ValueError, match="feature"):
        CharacterEmbed(16, rows=10, nM=8, nC=2, feature="LEMMA")


def test_cpu_forward_backward_match_float64_loop():
    g = torch.Generator().manual_seed(0)
    nC, nM, W, T = 3, 5, 7, 40
    E = torch.randn(nC, 256, nM, generator=g, dtype=torch.float64, requires_grad=True)
    table = torch.randn(11, W, generator=g, dtype=torch.float64, requires_grad=True)
    ids = torch.randint(0, 256, (T, nC), generator=g).to(torch.uint8)
    ids[::3] = 255
    hash_ids = torch.randint(0, 2 ** 40, (T,), generator=g)
    dX = torch.randn(T, nC * nM + W, generator=g, dtype=torch.float64)
    X = ops.char_embed(E, ids, table, hash_ids, 5)
    X.backward(dX)
    X64, dE64, _, _ = reference(E.detach(), ids, dX[:, :nC * nM])
    assert torch.equal(X[:, :nC * nM].detach(), X64)
    assert torch.allclose(E.grad, dE64, rtol=0, atol=1e-12)
    hashed = ops.hashembed(table, hash_ids, 5)
    assert torch.equal(X[:, nC * nM:], hashed)
    assert torch.allclose(table.grad, torch.autograd.grad(hashed, table, dX[:, nC * nM:])[0])


def test_example_config_trains_and_round_trips(tmp_path):
    import spacy_ray_amd
    from spacy_ray_amd.config.config import resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example

    torch.manual_seed(0)
    cfg = Config.from_disk(CFG)
    nlp = init_nlp(cfg, device="cpu", sample_size=32)
    embed = nlp.tok2vec.module.embed
    assert tuple(embed.E.shape) == (8, 256, 48) and embed.mixer.weight.shape[1] == 512
    docs = make_synthetic_docs(nlp.vocab, n_docs=32, words_per_doc=12, vocab_size=200,
                               n_tags=20, n_deps=10, n_ent_types=3, seed=0)
    examples = [Example.from_doc(d) for d in docs]
    T = resolve(cfg.interpolate()["training"], validate=False)
    engine = ZeRO1Engine(nlp, T["optimizer"], LocalComm())
    seen = []
    for _ in range(8):
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        engine.apply_step()
        seen.append(float(losses["tagger"]))
    assert seen[-1] < seen[0], seen
    nlp.to_disk(str(tmp_path))
    nlp2 = spacy_ray_amd.load(str(tmp_path), device="cpu")
    outs1 = nlp.predict_docs([d.copy_unannotated() for d in docs[:8]])
    outs2 = nlp2.predict_docs([d.copy_unannotated() for d in docs[:8]])
    assert [o.tags for o in outs1] == [o.tags for o in outs2]
