"""SparseLinear / TextCatBOW on the CPU: the host hash against Python-int
hashes, the composed path against a float64 loop, the BOW textcat pipe."""
import numpy as np
import pytest
import torch

from spacy_ray_amd import _srx_cpu
from spacy_ray_amd.ops import torch_ref as ref

M64 = (1 << 64) - 1


def murmur2_64a(words):
    """MurmurHash64A of little-endian uint64 words, seed 0."""
    m, r = 0xC6A4A7935BD1E995, 47
    h = (8 * len(words) * m) & M64
    for k in words:
        k = (k * m) & M64
        k ^= k >> r
        k = (k * m) & M64
        h = ((h ^ k) * m) & M64
    h ^= h >> r
    h = (h * m) & M64
    return h ^ (h >> r)


def fmix64(k):
    k ^= k >> 33
    k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33
    k = (k * 0xC4CEB9FE1A85EC53) & M64
    return k ^ (k >> 33)


def hash4_lanes01(key):
    """First two uint32 lanes of MurmurHash3 x64_128 of one 8-byte key, seed 0."""
    k1 = (key * 0x87C37B91114253D5) & M64
    k1 = ((k1 << 31) | (k1 >> 33)) & M64
    h1 = ((k1 * 0x4CF5AD432745937F) & M64) ^ 8
    h2 = 8
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1 = (fmix64(h1) + fmix64(h2)) & M64
    return h1 & 0xFFFFFFFF, h1 >> 32


def py_buckets(docs, G, L):
    """Per doc, the (b0, b1) of its n-grams: n-major, then position."""
    out = []
    for doc in docs:
        rows = []
        for n in range(1, G + 1):
            for i in range(len(doc) - n + 1):
                h0, h1 = hash4_lanes01(murmur2_64a(doc[i:i + n]))
                rows.append((h0 & (L - 1), h1 & (L - 1)))
        out.append(rows)
    return out


def pack(docs):
    """(ids int64 [T], offsets int32 [D + 1]) tensors of lists of uint64."""
    ids = np.array([w for d in docs for w in d], dtype=np.uint64)
    offsets = np.cumsum([0] + [len(d) for d in docs]).astype(np.int32)
    return torch.from_numpy(ids.view(np.int64)), torch.from_numpy(offsets)


def reference(docs, G, weight, bias, dS):
    """float64 loop -> (scores, sum|terms| per doc, entries per doc, dWeight,
    sum|terms| per row element, entries per row)."""
    L, nO = weight.shape
    W, dS = weight.double().numpy(), dS.double().numpy()
    rows = py_buckets(docs, G, L)
    b = np.array([x for r in rows for pair in r for x in pair], dtype=np.int64)
    d = np.repeat(np.arange(len(docs)), [2 * len(r) for r in rows])
    scores = np.tile(bias.double().numpy(), (len(docs), 1))
    mag, m = np.abs(scores), np.zeros((len(docs), 1))
    dW, dmag, k = np.zeros((L, nO)), np.zeros((L, nO)), np.zeros((L, 1))
    np.add.at(scores, d, W[b])  # one entry at a time, in float64
    np.add.at(mag, d, np.abs(W[b]))
    np.add.at(m, d, 1)
    np.add.at(dW, b, dS[d])
    np.add.at(dmag, b, np.abs(dS[d]))
    np.add.at(k, b, 1)
    return tuple(torch.from_numpy(a) for a in (scores, mag, m, dW, dmag, k))


DOCS = [[], [5], [2 ** 64 - 1, 0], [7, 8, 7, 8, 9, 0, 3]]  # lengths 0, 1, 2, 7


@pytest.mark.parametrize("G", [1, 2, 3])
def test_host_buckets_match_python_hashes(G):
    ids, offsets = pack(DOCS)
    got = _srx_cpu.ngram_buckets(ids.numpy().view(np.uint64), offsets.numpy(), G, 64)
    want = py_buckets(DOCS, G, 64)
    counts = [sum(max(0, len(d) - n + 1) for n in range(1, G + 1)) for d in DOCS]
    assert [len(w) for w in want] == counts and got.shape == (sum(counts), 2)
    assert got.tolist() == [list(p) for rows in want for p in rows]
    assert ref.ngram_counts(offsets, G).tolist() == counts


def test_composed_path_matches_float64_loop_and_gradcheck():
    g = torch.Generator().manual_seed(0)
    ids, offsets = pack(DOCS)
    weight = torch.randn(16, 3, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(3, generator=g, dtype=torch.float64, requires_grad=True)
    dS = torch.randn(len(DOCS), 3, generator=g, dtype=torch.float64)
    scores = ref.sparse_linear(ids, offsets, weight, bias, 3)
    scores.backward(dS)
    s64, _, _, dW64, _, _ = reference(DOCS, 3, weight.detach(), bias.detach(), dS)
    assert torch.allclose(scores, s64, rtol=0, atol=1e-12)
    assert torch.allclose(weight.grad, dW64, rtol=0, atol=1e-12)
    assert torch.allclose(bias.grad, dS.sum(0), rtol=0, atol=1e-12)
    assert torch.autograd.gradcheck(
        lambda w, b: ref.sparse_linear(ids, offsets, w, b, 3), (weight, bias))


BOW_CFG = """
[nlp]
lang = "en"
pipeline = ["textcat"]

[components]

[components.textcat]
factory = "textcat"

[components.textcat.model]
@architectures = "spacy.TextCatBOW.v2"
exclusive_classes = true
ngram_size = 2
no_output_layer = false

[corpora]

[corpora.train]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 96
words_per_doc = 14
vocab_size = 120
n_tags = 10
seed = 5

[training]
seed = 0
train_corpus = "corpora.train"
"""


def test_bow_pipe_trains_and_round_trips(tmp_path):
    import spacy_ray_amd
    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.train.scorer import score_examples
    from spacy_ray_amd.vocab.doc import Example

    torch.manual_seed(0)
    nlp = init_nlp(Config.from_str(BOW_CFG), device="cpu", sample_size=64)
    pipe = nlp.pipeline[0][1]
    assert nlp.tok2vec is None and pipe.listens_to is None
    assert tuple(pipe.module.weight.shape) == (262144, len(pipe.labels))
    docs = make_synthetic_docs(nlp.vocab, n_docs=96, words_per_doc=14, vocab_size=120,
                               n_tags=10, n_deps=10, n_ent_types=3, seed=5)
    examples = [Example.from_doc(d) for d in docs]
    opt = resolve({"o": {"@optimizers": "Adam.v1", "learn_rate": 0.01}}, validate=False)["o"]
    engine = ZeRO1Engine(nlp, opt, LocalComm())
    seen = []
    for _ in range(30):
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        engine.apply_step()
        seen.append(float(losses["textcat"]))
    assert seen[-1] < seen[0]
    nlp.predict_docs([eg.predicted for eg in examples])
    scores = score_examples(examples, ["textcat"])
    assert scores["cats_macro_acc"] > 0.5, scores

    nlp.to_disk(str(tmp_path))
    nlp2 = spacy_ray_amd.load(str(tmp_path), device="cpu")
    assert nlp2.pipeline[0][1].cfg["ngram_size"] == 2
    outs1 = nlp.predict_docs([d.copy_unannotated() for d in docs[:8]])
    outs2 = nlp2.predict_docs([d.copy_unannotated() for d in docs[:8]])
    assert [o.cats for o in outs1] == [o.cats for o in outs2]


def test_length_must_be_a_power_of_two():
    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.pipeline.language import build_nlp

    cfg = BOW_CFG.replace("TextCatBOW.v2", "TextCatBOW.v3").replace(
        "ngram_size = 2", "ngram_size = 2\nlength = 1000")
    with pytest.raises(ValueError, match="length"):
        build_nlp(Config.from_str(cfg))
