"""attention_pool kernels against the float64 loop of tests/test_attention_pool.py
(the bound is derived in that module's docstring); the ensemble pipe end to end."""
import pytest
import torch

from spacy_ray_amd.ops import api as ops
from tests.test_attention_pool import (BF, ENSEMBLE, F32, WIDTHS, case, check,
                                       reference, run)

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fused(monkeypatch):
    monkeypatch.setenv("SRX_ATTENTION_POOL", "fused")


@pytest.mark.parametrize("D", [1, 3, 70])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("keys", [False, True])
@pytest.mark.parametrize("dtype", [BF, F32])
def test_forward_and_backward_match_float64(dtype, keys, W, D):
    X, offsets, q, K, dP, want = case(dtype, W, D, keys)
    assert ops.attention_pool_available(X.cuda(), q.cuda(), None if K is None else K.cuda())
    check(run(X, offsets, q, K, dP, "cuda"), want, dtype)


# a lane owns at most 3 pieces: sub_wave lanes serve W <= 3 * sub_wave * V
@pytest.mark.parametrize("sub_wave", [8, 16, 32, 64])
@pytest.mark.parametrize("dtype,keys", [(BF, False), (F32, True)])
def test_every_sub_wave(sub_wave, dtype, keys):
    V = 8 if dtype == BF else 4
    for W in [w for w in WIDTHS if w <= 3 * sub_wave * V]:
        X, offsets, q, K, dP, want = case(dtype, W, 70, keys)
        check(run(X, offsets, q, K, dP, "cuda", sub_wave=sub_wave), want, dtype)


@pytest.mark.parametrize("dtype,W,keys", [(BF, 96, False), (BF, 768, True), (F32, 520, True)])
def test_reproducible_and_grid_independent(dtype, W, keys):
    X, offsets, q, K, dP, _ = case(dtype, W, 70, keys)
    first = run(X, offsets, q, K, dP, "cuda")
    again = run(X, offsets, q, K, dP, "cuda")
    one_block = run(X, offsets, q, K, dP, "cuda", max_blocks=1)
    for name in first:
        assert torch.equal(first[name], again[name]), name
        assert torch.equal(first[name], one_block[name]), name


def test_mode_switch_and_fallback(monkeypatch):
    X, offsets, q, K, dP, want = case(BF, 96, 70, True)
    for mode in ("fused", "composed"):
        monkeypatch.setenv("SRX_ATTENTION_POOL", mode)
        check(run(X, offsets, q, K, dP, "cuda"), want, BF)
    monkeypatch.setenv("SRX_ATTENTION_POOL", "flash")
    with pytest.raises(ValueError, match="SRX_ATTENTION_POOL"):
        run(X, offsets, q, K, dP, "cuda")
    monkeypatch.setenv("SRX_ATTENTION_POOL", "fused")
    g = torch.Generator().manual_seed(0)  # W = 12 in bf16: no 16-byte pieces
    X, q = torch.randn(9, 12, generator=g).to(BF), torch.randn(12, generator=g)
    dP, lengths = torch.randn(3, 12, generator=g).to(BF), [4, 0, 5]
    offsets = torch.tensor([0, 4, 4, 9], dtype=torch.int32)
    assert not ops.attention_pool_available(X.cuda(), q.cuda())
    check(run(X, offsets, q, None, dP, "cuda"), reference(X, lengths, q, None, dP), BF)


def test_ensemble_pipe_fused_against_composed(monkeypatch):
    """The pipe's loss and Q.grad on a 64-doc batch, both routes and a
    float64 copy of the head.  The two routes share every launch but the
    pooling, whose outputs R differ by at most both forward bounds, delta.
    The head's scores are differentiable in R, so to first order the loss
    moves by at most sum |dLoss/dR| delta (the float64 gradient), and by
    twice that against float64, where the fp32 head adds its own rounding.
    Q.grad = dq is linear in dP = dLoss/dR: both routes' dq bounds at the
    float64 dP, doubled for the first-order change of dP itself."""
    import copy

    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.models.batch import TokenBatch
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example

    nlp = init_nlp(Config.from_str(ENSEMBLE), device="cuda:0", sample_size=48)
    pipe = nlp.pipeline[-1][1]
    head = pipe.module
    gen = torch.Generator("cuda").manual_seed(3)
    with torch.no_grad():
        for p in (head.attend.Q, head.output.weight, head.bow.weight):
            p.normal_(std=0.3, generator=gen)
    examples = [Example.from_doc(d) for d in make_synthetic_docs(
        nlp.vocab, n_docs=64, words_per_doc=14, vocab_size=120, n_tags=10,
        n_deps=10, n_ent_types=3, seed=5)]
    batch = TokenBatch([eg.predicted for eg in examples], nlp.device)
    with torch.no_grad():
        t2v = nlp.tok2vec.forward(batch).float()
    out = {}
    for mode in ("fused", "composed"):
        monkeypatch.setenv("SRX_ATTENTION_POOL", mode)
        head.zero_grad(set_to_none=True)
        loss, _ = pipe.get_loss(examples, t2v, batch)
        loss.backward()
        out[mode] = (float(loss.detach()), head.attend.Q.grad.cpu().double())

    # float64 on the CPU: the same head, the composed ops
    head64 = copy.deepcopy(head).double().cpu()
    lengths = batch.lengths.cpu()
    offsets = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    offsets[1:] = torch.cumsum(lengths, 0)
    X64 = t2v[:batch.n_tokens].double().cpu()
    ids, bow_offsets = (t.cpu() for t in pipe._bow_inputs(batch, None))
    R = ops.attention_pool(X64, offsets, head64.attend.Q).detach().requires_grad_(True)
    monkeypatch.setattr(ops, "attention_pool", lambda *a, **k: R)
    scores = head64(X64, offsets, 64, ids, bow_offsets)
    gold = torch.from_numpy(pipe._gold_matrix(examples)).double()
    loss64 = -(gold * torch.log_softmax(scores, -1)).sum() / 64
    loss64.backward()
    want = reference(X64, lengths.tolist(), head64.attend.Q.detach(), None, R.grad)
    delta = 2 * want["P"][1]
    dloss = float((R.grad.abs() * delta).sum())
    print("pipe loss: fused - composed", out["fused"][0] - out["composed"][0],
          "fused - float64", out["fused"][0] - float(loss64.detach()), "bound", dloss)
    assert abs(out["fused"][0] - out["composed"][0]) <= dloss
    assert abs(out["fused"][0] - float(loss64.detach())) <= 2 * dloss
    dq64, bq = want["dq"]
    err = (out["fused"][1] - out["composed"][1]).abs()
    print("pipe Q.grad err / bound", float((err / (4 * bq).clamp(min=1e-300)).max()))
    assert (err <= 4 * bq).all()
    assert ((out["fused"][1] - dq64).abs() <= 4 * bq).all()  # and not both wrong
