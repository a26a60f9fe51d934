"""sparse_linear kernels against a float64 loop; the BOW textcat pipe end to end."""
import functools

import numpy as np
import pytest
import torch

from spacy_ray_amd import _srx_cpu
from spacy_ray_amd.ops import api as ops
from tests.test_sparse_linear import BOW_CFG, pack, reference

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF, F32 = torch.bfloat16, torch.float32
# dtype, nO, G, D, L: nO single piece / odd / several pieces, one doc up to
# several workgroups, a colliding and the default table
CASES = [(BF, 1, 1, 1, 64), (BF, 5, 1, 63, 64), (BF, 8, 3, 64, 64),
         (BF, 32, 3, 65, 262144), (BF, 4, 3, 600, 64), (F32, 4, 3, 63, 64),
         (F32, 32, 1, 64, 64), (F32, 5, 3, 65, 64), (F32, 2, 3, 600, 262144)]


def make_docs(D, seed=0):
    """Lengths from {1, 2, 3, 20, 70} (70 > one trip at 64 lanes), doc 1
    empty; ids from 50 types that include 0 and 2^64 - 1; every non-empty
    doc starts with the same token (at D = 600 its rows are runs of more
    than two 256-entry chunks); doc 0 repeats a bigram."""
    rng = np.random.RandomState(seed)
    types = [0, 2 ** 64 - 1] + [int(x) for x in rng.randint(1, 2 ** 62, 48)]
    docs = [[types[2]] + [types[j] for j in rng.randint(0, 50, n - 1)]
            for n in rng.choice([1, 2, 3, 20, 70], D)]
    docs[0] = [types[2], 7, 8, 7, 8, 0, 2 ** 64 - 1] + docs[0][1:14]
    if D > 1:
        docs[1] = []
    return docs


@functools.lru_cache(maxsize=None)  # the float64 reference is the slow part
def case(dtype, nO, G, D, L):
    g = torch.Generator().manual_seed(1)
    docs = make_docs(D)
    weight = torch.randn(L, nO, generator=g).to(dtype)
    bias = torch.randn(nO, generator=g)
    dS = torch.randn(D, nO, generator=g)
    return docs, weight, bias, dS, reference(docs, G, weight, bias, dS)


def run(docs, weight, bias, dS, G, **kw):
    ids, offsets = (t.cuda() for t in pack(docs))
    w, b = weight.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
    scores = ops.sparse_linear(ids, offsets, w, b, G, **kw)
    scores.backward(dS.cuda())
    return scores.detach().cpu(), w.grad.cpu(), b.grad.cpu()


def check(dtype, scores, dW, dB, dS, ref):
    s64, mag, m, dW64, dmag, k = ref
    assert scores.dtype == torch.float32 and dW.dtype == dtype
    err, bound = (scores.double() - s64).abs(), 2 * (m + 2) * U * mag
    print("scores err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    rel = 2.0 ** -8 if dtype == BF else 0.0
    err, bound = (dW.double() - dW64).abs(), 2 * (k + 1) * U * dmag + rel * dW64.abs()
    print("dWeight err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    assert not dW[k[:, 0] == 0].any()
    assert torch.allclose(dB.double(), dS.double().sum(0), rtol=0,
                          atol=2 * (len(dS) + 1) * U * float(dS.abs().sum(0).max()))


@pytest.mark.parametrize("G", [1, 2, 3, 4])
def test_device_hash_is_bit_equal_to_host(G):
    ids, offsets = pack(make_docs(65))
    got = ops.ngram_buckets(ids.cuda(), offsets.cuda(), G, 262144).cpu().numpy()
    want = _srx_cpu.ngram_buckets(ids.numpy().view(np.uint64), offsets.numpy(), G, 262144)
    assert got.dtype == np.int32 and np.array_equal(got, want)


@pytest.mark.parametrize("dtype,nO,G,D,L", CASES)
def test_forward_and_backward_match_float64(dtype, nO, G, D, L):
    docs, weight, bias, dS, ref = case(dtype, nO, G, D, L)
    check(dtype, *run(docs, weight, bias, dS, G), dS, ref)


@pytest.mark.parametrize("sub_wave", [8, 16, 32, 64])
@pytest.mark.parametrize("dtype,nO,G,D,L", [CASES[2], CASES[3], CASES[7]])
def test_every_sub_wave(sub_wave, dtype, nO, G, D, L):
    docs, weight, bias, dS, ref = case(dtype, nO, G, D, L)
    check(dtype, *run(docs, weight, bias, dS, G, sub_wave=sub_wave), dS, ref)


@pytest.mark.parametrize("dtype,nO,G,D,L", [CASES[4], CASES[8]])
def test_backward_is_reproducible_and_grid_independent(dtype, nO, G, D, L):
    docs, weight, bias, dS, _ = case(dtype, nO, G, D, L)
    first = run(docs, weight, bias, dS, G)
    again = run(docs, weight, bias, dS, G)
    one_block = run(docs, weight, bias, dS, G, max_blocks=1)
    for a, b, c in zip(first, again, one_block):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_mode_switch_and_fallback(monkeypatch):
    dtype, nO, G, D, L = CASES[3]
    docs, weight, bias, dS, ref = case(dtype, nO, G, D, L)
    for mode in ("fused", "composed"):
        monkeypatch.setenv("SRX_SPARSE_LINEAR", mode)
        check(dtype, *run(docs, weight, bias, dS, G), dS, ref)
    monkeypatch.setenv("SRX_SPARSE_LINEAR", "atomic")
    with pytest.raises(ValueError, match="SRX_SPARSE_LINEAR"):
        run(docs, weight, bias, dS, G)
    monkeypatch.delenv("SRX_SPARSE_LINEAR")
    docs, weight, bias, dS, ref = case(F32, 129, 1, 63, 64)  # nO > 128: composed
    ids, _ = pack(docs)
    assert not ops.sparse_linear_available(ids.cuda(), weight.cuda(), 1)
    check(F32, *run(docs, weight, bias, dS, 1), dS, ref)


def test_bow_pipe_fused_against_composed(monkeypatch):
    """The pipe's loss and dWeight on a 64-doc batch, both routes.  The loss
    (mean softmax cross-entropy) is 2-Lipschitz in the scores' sup norm and
    dScores = (softmax - gold) / n moves by at most 2 delta / n when the
    scores move by delta, so with delta = the two routes' forward bounds the
    routes differ by at most 2 delta in the loss and, in a row with k
    entries, by both dWeight bounds plus k * 2 delta / n."""
    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.models.batch import TokenBatch
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example

    cfg = BOW_CFG.replace("ngram_size = 2", "ngram_size = 3")
    nlp = init_nlp(Config.from_str(cfg), device="cuda:0", sample_size=64)
    pipe = nlp.pipeline[0][1]
    head = pipe.module
    with torch.no_grad():
        head.weight.normal_(generator=torch.Generator("cuda").manual_seed(3))
    examples = [Example.from_doc(d) for d in make_synthetic_docs(
        nlp.vocab, n_docs=64, words_per_doc=14, vocab_size=120, n_tags=10,
        n_deps=10, n_ent_types=3, seed=5)]
    batch = TokenBatch([eg.predicted for eg in examples], nlp.device)
    out = {}
    for mode in ("fused", "composed"):
        monkeypatch.setenv("SRX_SPARSE_LINEAR", mode)
        head.zero_grad(set_to_none=True)
        loss, _ = pipe.get_loss(examples, None, batch)
        loss.backward()
        out[mode] = (float(loss.detach()), head.weight.grad.cpu().double())
    ids, offsets = (t.cpu().numpy() for t in pipe._bow_inputs(batch, None))
    assert len(offsets) == 65  # the batch's pad pseudo-doc is left out
    docs = [[int(x) for x in ids.view(np.uint64)[a:b]] for a, b in zip(offsets, offsets[1:])]
    weight, bias = head.weight.detach().cpu(), head.bias.detach().cpu()
    s64, mag, m, _, _, _ = reference(docs, 3, weight, bias, torch.zeros(64, len(bias)))
    gold = torch.from_numpy(pipe._gold_matrix(examples)).double()
    dS64 = (torch.softmax(s64, -1) - gold) / 64
    _, _, _, dW64, dmag, k = reference(docs, 3, weight, bias, dS64)
    delta = 2 * float((2 * (m + 2) * U * mag).max())
    assert abs(out["fused"][0] - out["composed"][0]) <= 2 * delta
    err = (out["fused"][1] - out["composed"][1]).abs()
    bound = 2 * (2 * (k + 1) * U * dmag) + k * 2 * delta / 64
    print("pipe dWeight err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    assert ((out["fused"][1] - dW64).abs() <= bound).all()  # and not both wrong
