"""Fused static-vectors kernels (srx_staticvec.hip.h) against float64.

Inputs are built on the CPU from a seeded generator and rounded to bf16
(as ref64.mwe_inputs does); the float64 reference is computed here from
exactly those values, the baseline is the same operation in stock bf16
torch ops on the GPU, and the rule is ref64.check_parity(factor=2)."""
import math

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

V = 257
NEG_POS = (0, 63, 64, 127, 128)


def _hip():
    from spacy_ray_amd.ops.api import hip_ext

    hip = hip_ext()
    assert hip is not None
    return hip


def _rows(T, gen, all_oov_from=None):
    """Random rows with row 0, row V-1, one row repeated 64 times, and -1 at
    positions 0, 63, 64, 127, 128 and T-1 where they exist."""
    rows = torch.randint(0, V, (T,), generator=gen, dtype=torch.int32)
    neg = {p for p in NEG_POS + (T - 1,) if 0 <= p < T}
    free = [p for p in range(T) if p not in neg]
    if len(free) >= 2:
        rows[free[0]] = 0
        rows[free[1]] = V - 1
    for p in free[2:66]:
        rows[p] = 7
    for p in neg:
        rows[p] = -1
    if all_oov_from is not None:
        rows[all_oov_from:] = -1
    return rows


def _inputs(nO, nM, seed):
    gen = torch.Generator().manual_seed(seed)
    table = (torch.randn(V, nM, generator=gen) * 0.5).to(torch.bfloat16)
    W = (torch.randn(nO, nM, generator=gen) / math.sqrt(nM)).to(torch.bfloat16)
    return gen, table, W


def _padded(table):
    nM = table.shape[1]
    nMp = -(-nM // 32) * 32
    out = torch.zeros(table.shape[0], nMp, dtype=table.dtype)
    out[:, :nM] = table
    return out.cuda()


def _gather64(table, rows):
    G = table.double()[rows.long().clamp(min=0)]
    return G * (rows >= 0)[:, None]


def _gather_bf16(table_d, rows_d, nM):
    G = table_d[rows_d.long().clamp(min=0)][:, :nM]
    return G.masked_fill((rows_d < 0)[:, None], 0)


@need_gpu
@pytest.mark.parametrize("T", [1, 64, 129, 192])
@pytest.mark.parametrize("nM", [300, 96, 50])
@pytest.mark.parametrize("nO", [96, 128])
def test_static_vectors_fwd(nO, nM, T):
    hip = _hip()
    gen, table, W = _inputs(nO, nM, 1000 * nO + 10 * nM + T)
    rows = _rows(T, gen, all_oov_from=128 if T == 192 else None)
    ref = _gather64(table, rows) @ W.double().t()

    table_d, rows_d, W_d = _padded(table), rows.cuda(), W.cuda()
    sentinel = 1.5
    Y = torch.full((T + 3, 5 * nO), sentinel, dtype=torch.bfloat16, device="cuda")
    before = Y.clone()
    hip.static_vectors_fwd(table_d, rows_d, W_d, Y, 4 * nO)
    base = _gather_bf16(table_d, rows_d, nM) @ W_d.t()

    got = Y[:T, 4 * nO:]
    ref64.check_parity(f"sv_fwd nO={nO} nM={nM} T={T}", got.cpu(), base.cpu(), ref)
    # nothing outside the block, nothing past row T
    assert torch.equal(Y[:, :4 * nO].view(torch.int16),
                       before[:, :4 * nO].view(torch.int16))
    assert torch.equal(Y[T:].view(torch.int16), before[T:].view(torch.int16))
    oov = (rows < 0).cuda()
    assert bool((got[oov].view(torch.int16) == 0).all())
    if T > 1:
        assert bool((got[~oov] != 0).any())


@need_gpu
@pytest.mark.parametrize("T,max_groups", [(129, 0), (384, 2)])
@pytest.mark.parametrize("nM", [300, 96, 50])
@pytest.mark.parametrize("nO", [96, 128])
def test_static_vectors_bwd_dw(nO, nM, T, max_groups):
    hip = _hip()
    gen, table, _ = _inputs(nO, nM, 7000 * nO + 10 * nM + T)
    rows = _rows(T, gen)
    dX = (torch.randn(T, 5 * nO, generator=gen) * 0.1).to(torch.bfloat16)
    dY = dX[:, 4 * nO:]
    ref = dY.double().t() @ _gather64(table, rows)

    table_d, rows_d, dX_d = _padded(table), rows.cuda(), dX.cuda()
    dW = hip.static_vectors_bwd_dw(table_d, rows_d, dX_d, 4 * nO, nO,
                                   max_groups, nM)
    assert dW.shape == (nO, nM) and dW.dtype == torch.float32
    base = dX_d[:, 4 * nO:].t() @ _gather_bf16(table_d, rows_d, nM)
    ref64.check_parity(f"sv_dw nO={nO} nM={nM} T={T}", dW.cpu(), base.cpu(), ref)

    again = hip.static_vectors_bwd_dw(table_d, rows_d, dX_d, 4 * nO, nO,
                                      max_groups, nM)
    assert torch.equal(dW, again)
    # OOV tokens contribute nothing, whatever their dY is
    dX2 = dX_d.clone()
    dX2[(rows < 0).cuda()] = 3.0
    other = hip.static_vectors_bwd_dw(table_d, rows_d, dX2, 4 * nO, nO,
                                      max_groups, nM)
    assert torch.equal(dW, other)


def _embed_inputs(width, T, seed):
    gen = torch.Generator().manual_seed(seed)
    ids4 = torch.randint(-2 ** 62, 2 ** 62, (T, 4), generator=gen,
                         dtype=torch.int64).cuda()
    tables = [(torch.randn(r, width, generator=gen) * 0.1)
              .to(torch.bfloat16).cuda().requires_grad_(True)
              for r in (50, 30, 30, 30)]
    return gen, ids4, tables


@need_gpu
def test_multi_hashembed_with_vectors_uses_the_kernels(monkeypatch):
    from spacy_ray_amd.ops import api as ops

    monkeypatch.setenv("SRX_STATIC_VECTORS", "fused")
    hip = _hip()
    width, nM, T = 96, 300, 129
    _, table, W = _inputs(width, nM, 5)
    gen, ids4, tables = _embed_inputs(width, T, 6)
    rows_d = _rows(T, gen).cuda()
    table_d = _padded(table)
    vW = W.cuda().requires_grad_(True)
    seeds = [0, 1, 2, 3]
    assert ops.static_vectors_available(table_d, vW)

    X0 = ops.multi_hashembed(ids4, seeds, tables)
    X1 = ops.multi_hashembed(ids4, seeds, tables, (table_d, rows_d, vW))
    assert X1.shape == (T, 5 * width)
    assert torch.equal(X0, X1[:, :4 * width])
    Y = torch.zeros(T, width, dtype=torch.bfloat16, device="cuda")
    hip.static_vectors_fwd(table_d, rows_d, vW.detach(), Y, 0)
    assert torch.equal(Y, X1[:, 4 * width:])

    dX = (torch.randn(T, 5 * width, generator=gen) * 0.1).to(torch.bfloat16).cuda()
    X1.backward(dX)
    want = hip.static_vectors_bwd_dw(table_d, rows_d, dX, 4 * width, width, 0, nM)
    assert torch.equal(vW.grad, want.to(torch.bfloat16))
    assert all(t.grad is not None for t in tables)


@need_gpu
def test_static_vectors_composed_fallback_parity():
    """nO = 64 has no fused kernel: index_select + mm on the GPU."""
    from spacy_ray_amd.ops import api as ops

    nO, nM, T = 64, 300, 129
    gen, table, W = _inputs(nO, nM, 9)
    rows = _rows(T, gen)
    dY = (torch.randn(T, nO, generator=gen) * 0.1).to(torch.bfloat16)
    G64 = _gather64(table, rows)
    table_d, rows_d = _padded(table), rows.cuda()
    vW = W.cuda().requires_grad_(True)
    assert not ops.static_vectors_available(table_d, vW)
    Y = ops.static_vectors(vW, table_d, rows_d)
    Y.backward(dY.cuda())
    Gb = _gather_bf16(table_d, rows_d, nM)
    ref64.check_parity("sv_composed fwd", Y.detach().cpu(),
                       (Gb @ vW.detach().t()).cpu(), G64 @ W.double().t())
    ref64.check_parity("sv_composed dW", vW.grad.cpu(),
                       (dY.cuda().t() @ Gb).cpu(), dY.double().t() @ G64)
    assert bool((Y[(rows < 0).cuda()] == 0).all())


E2E_CFG = """
[paths]
vectors = null

[nlp]
lang = "en"
pipeline = ["tok2vec", "tagger"]

[components]

[components.tok2vec]
factory = "tok2vec"

[components.tok2vec.model]
@architectures = "spacy.Tok2Vec.v2"

[components.tok2vec.model.embed]
@architectures = "spacy.MultiHashEmbed.v2"
width = 96
attrs = ["NORM", "PREFIX", "SUFFIX", "SHAPE"]
rows = [500, 250, 250, 250]
include_static_vectors = true

[components.tok2vec.model.encode]
@architectures = "spacy.MaxoutWindowEncoder.v2"
width = 96
depth = 2
window_size = 1
maxout_pieces = 3

[components.tagger]
factory = "tagger"

[components.tagger.model]
@architectures = "spacy.Tagger.v2"

[components.tagger.model.tok2vec]
@architectures = "spacy.Tok2VecListener.v1"
width = 96

[corpora]

[corpora.train]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 150
words_per_doc = 14
vocab_size = 300
n_tags = 12
seed = 0

[corpora.dev]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 10
words_per_doc = 14
vocab_size = 300
n_tags = 12
seed = 1

[training]
train_corpus = "corpora.train"
dev_corpus = "corpora.dev"
seed = 0

[training.optimizer]
@optimizers = "Adam.v1"
learn_rate = 0.01

[initialize]
vectors = ${paths.vectors}
"""


@need_gpu
@pytest.mark.parametrize("mode", ["fused", "composed"])
def test_static_vectors_end_to_end(tmp_path, monkeypatch, mode):
    import numpy as np

    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example
    from spacy_ray_amd.vocab.vectors import Vectors

    monkeypatch.setenv("SRX_STATIC_VECTORS", mode)
    rng = np.random.default_rng(0)
    lexicon = [f"w{i}" for i in range(250)]  # w250.. are out of vocabulary
    Vectors.from_words(lexicon, rng.standard_normal((250, 50)).astype("f")
                       ).to_disk(tmp_path / "vec" / "vocab")
    cfg = Config.from_str(E2E_CFG, overrides={"paths.vectors": str(tmp_path / "vec")})
    nlp = init_nlp(cfg, device="cuda:0", sample_size=32)
    table_before = nlp.vocab.vectors.data.copy()
    T = resolve(cfg.interpolate()["training"], validate=False)
    engine = ZeRO1Engine(nlp, T["optimizer"], LocalComm())
    docs = make_synthetic_docs(nlp.vocab, n_docs=150, words_per_doc=14,
                               vocab_size=300, n_tags=12, seed=0)
    examples = [Example.from_doc(d) for d in docs]
    assert 1500 < sum(len(d) for d in docs) < 3000
    seen = []
    for _ in range(3):
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        engine.apply_step()
        seen.append(losses["tagger"])
    assert all(math.isfinite(x) for x in seen), seen
    assert seen[-1] < seen[0], seen
    assert np.array_equal(nlp.vocab.vectors.data, table_before)
    dev = nlp.vocab.vectors.device_table("cuda:0", torch.bfloat16)
    assert torch.equal(dev[:, :50].float().cpu(),
                       torch.from_numpy(table_before).to(torch.bfloat16).float())

    sub = [d.copy_unannotated() for d in docs[:20]]
    nlp.predict_docs(sub)
    out = tmp_path / "ckpt"
    nlp.to_disk(out)
    assert (out / "vocab" / "vectors.safetensors").exists()
    nlp2 = init_nlp(cfg, device="cuda:0", sample_size=32)
    nlp2.from_disk(out)
    sub2 = [d.copy_unannotated() for d in docs[:20]]
    for d in sub2:
        d.vocab = nlp2.vocab
        d.vector_rows = {}
    nlp2.predict_docs(sub2)
    assert [d.tags for d in sub] == [d.tags for d in sub2]
