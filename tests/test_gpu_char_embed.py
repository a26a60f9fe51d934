"""char_embed kernels against a float64 loop; the example config on the GPU."""
import functools

import pytest
import torch

from spacy_ray_amd.ops import api as ops
from tests.test_char_embed import CFG, reference

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF, F32 = torch.bfloat16, torch.float32
SLICED = -1  # T from the host's slice rule: S >= 2 with a ragged last slice
# dtype, nC, nM, T: one vector per cell / the default / the LDS ceiling, one
# token up to several passes of a workgroup, several slices
CASES = [(BF, 1, 8, 1), (BF, 5, 64, 63), (BF, 8, 128, 257), (BF, 8, 64, SLICED),
         (F32, 5, 8, 257), (F32, 8, 64, 63), (F32, 1, 128, 1), (F32, 5, 128, SLICED),
         (BF, 5, 24, 257)]
# all-pad and 0-and-255 ids on one bf16 and one fp32 shape
PARAMS = [(*c, "mixed") for c in CASES] + [
    (*c, kind) for c in (CASES[3], CASES[4]) for kind in ("pad", "ends")]


def n_tokens(nC, T):
    if T != SLICED:
        return T
    floor = 1
    while ops.hip_ext().char_embed_slices(2 * floor, nC)[0] < 2:
        floor *= 2
    T = 2 * floor + 37
    S, per = ops.hip_ext().char_embed_slices(T, nC)
    assert S >= 2 and T % per != 0
    return T


@functools.lru_cache(maxsize=None)  # the float64 loop is the slow part
def case(dtype, nC, nM, T, kind):
    """ids: "mixed" = letter-heavy with a third of the cells 255, bin 7 of
    every position never hit; "pad" = all 255; "ends" = only 0 and 255."""
    g = torch.Generator().manual_seed(1)
    T = n_tokens(nC, T)
    E = torch.randn(nC, 256, nM, generator=g).to(dtype)
    ids = 97 + torch.randint(0, 26, (T, nC), generator=g)
    ids[torch.rand(T, nC, generator=g) < 0.1] = 200
    ids[torch.rand(T, nC, generator=g) < 0.33] = 255
    if kind == "pad":
        ids.fill_(255)
    elif kind == "ends":
        ids = 255 * torch.randint(0, 2, (T, nC), generator=g)
    ids = ids.to(torch.uint8)
    dX = torch.randn(T, nC * nM + 24, generator=g).to(dtype)  # a wider matrix
    return E, ids, dX, reference(E, ids, dX[:, 8:8 + nC * nM])


def check_bwd(dtype, dE, ref):
    _, dE64, mag, k = ref
    assert dE.dtype == dtype
    rel = 2.0 ** -8 if dtype == BF else 0.0
    err = (dE.double().cpu() - dE64).abs()
    bound = 2 * (k + 1) * U * mag + rel * dE64.abs()
    print("dE err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    assert not dE.cpu()[(k == 0).expand_as(dE64)].any()  # untouched bins: exactly 0


@pytest.mark.parametrize("dtype,nC,nM,T,kind", PARAMS)
def test_kernels_match_float64(dtype, nC, nM, T, kind):
    E, ids, dX, ref = case(dtype, nC, nM, T, kind)
    hip = ops.hip_ext()
    X = torch.full((len(ids), nC * nM + 16), 3.0, dtype=dtype, device="cuda")
    hip.char_embed_fwd(E.cuda(), ids.cuda(), X, 8)
    X = X.cpu()
    assert torch.equal(X[:, 8:8 + nC * nM].double(), ref[0])  # the table's bits
    assert (X[:, :8] == 3).all() and (X[:, 8 + nC * nM:] == 3).all()
    view = dX.cuda()[:, 8:8 + nC * nM]
    check_bwd(dtype, hip.char_embed_bwd(view, ids.cuda(), nC, nM, False), ref)
    check_bwd(dtype, hip.char_embed_bwd(view, ids.cuda(), nC, nM, True), ref)


def run_op(E, ids, table, hash_ids, dX):
    E, table = (t.cuda().requires_grad_(True) for t in (E, table))
    X = ops.char_embed(E, ids.cuda(), table, hash_ids.cuda(), 5)
    X.backward(dX.cuda())
    return X.detach(), E.grad, table.grad


@pytest.mark.parametrize("mode", ["fused", "composed"])
def test_op_blocks_and_hashed_block_equals_hashembed(monkeypatch, mode):
    dtype, nC, nM, T = CASES[1]
    E, ids, dX, ref = case(dtype, nC, nM, T, "mixed")
    g = torch.Generator().manual_seed(2)
    table = torch.randn(50, 24, generator=g).to(dtype)
    hash_ids = torch.randint(0, 2 ** 40, (T, 4), generator=g)[:, 1]  # a column view
    dX = torch.cat([dX[:, 8:8 + nC * nM], dX[:, :24]], dim=1)
    monkeypatch.setenv("SRX_CHAR_EMBED", mode)
    X, dE, dT = run_op(E, ids, table, hash_ids, dX)
    assert torch.equal(X[:, :nC * nM].double().cpu(), ref[0])
    check_bwd(dtype, dE, ref)
    t = table.cuda().requires_grad_(True)
    H = ops.hashembed(t, hash_ids.cuda().contiguous(), 5)
    assert torch.equal(X[:, nC * nM:], H.detach())
    dH = dX[:, nC * nM:].contiguous()
    (dT_alone,) = torch.autograd.grad(H, t, dH.cuda())
    # two fp32 sums of at most 4 T terms each, rounded once to bf16
    atol = 2 * 2 * (4 * T + 1) * U * 4 * float(dH.abs().sum(0).max())
    assert torch.allclose(dT.float(), dT_alone.float(), rtol=2.0 ** -7, atol=atol)
    monkeypatch.setenv("SRX_CHAR_EMBED", "lds")
    with pytest.raises(ValueError, match="SRX_CHAR_EMBED"):
        run_op(E, ids, table, hash_ids, dX)


def test_deterministic_backward_is_bit_identical(monkeypatch):
    dtype, nC, nM, T = CASES[3]
    E, ids, dX, ref = case(dtype, nC, nM, T, "mixed")
    g = torch.Generator().manual_seed(2)
    table = torch.randn(50, 24, generator=g).to(dtype)
    hash_ids = torch.randint(0, 2 ** 40, (len(ids),), generator=g)
    dX = torch.cat([dX[:, 8:8 + nC * nM], dX[:, :24]], dim=1)
    monkeypatch.setenv("SRX_DETERMINISTIC", "1")
    monkeypatch.setenv("SRX_CHAR_EMBED", "fused")
    first = run_op(E, ids, table, hash_ids, dX)
    again = run_op(E, ids, table, hash_ids, dX)
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    check_bwd(dtype, first[1], ref)


def test_example_config_steps_on_gpu():
    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example

    cfg = Config.from_disk(CFG)
    nlp = init_nlp(cfg, device="cuda:0", sample_size=16)
    T = resolve(cfg.interpolate()["training"], validate=False)
    engine = ZeRO1Engine(nlp, T["optimizer"], LocalComm())
    docs = make_synthetic_docs(nlp.vocab, n_docs=16, words_per_doc=12, vocab_size=200,
                               n_tags=20, n_deps=10, n_ent_types=3, seed=0)
    examples = [Example.from_doc(d) for d in docs]
    for _ in range(3):
        losses = {}
        engine.accumulate(examples, drop=0.1, losses=losses)
        engine.apply_step()
    torch.cuda.synchronize()
    assert 0 < float(losses["tagger"]) < float("inf")
    E = nlp.tok2vec.module.embed.E
    assert torch.isfinite(E.float()).all()
