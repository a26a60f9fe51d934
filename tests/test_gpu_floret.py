"""floret_words_mean (srx_floret.hip.h) against float64, and the floret
batch path through the static-vectors ops and a training run.

Inputs are built on the CPU from a seeded generator and rounded to bf16 (as
test_gpu_static_vectors.py does); the float64 reference is computed here
from exactly those values.

The kernel's bound is derived, not tuned.  A word's row is the fp32 sum of
n bf16 values in a fixed order, one fp32 division and one round-to-nearest-
even to bf16, so per element
    |got - ref| <= 2^-8 |ref| + 2 n 2^-24 mean_e |x_e|
The first term is the one rounding to bf16; the second is the fp32 sum and
divide (n roundings of magnitudes bounded by sum |x_e|, divided by n), with
a factor 2 for second-order terms."""
import math

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

R = 257
NS = (0, 1, 2, 63, 64, 65, 257)
SENTINEL = 1.5


def _hip():
    from spacy_ray_amd.ops.api import hip_ext

    hip = hip_ext()
    assert hip is not None
    return hip


def _padded(table):
    nM = table.shape[1]
    nMp = -(-nM // 32) * 32
    out = torch.zeros(table.shape[0], nMp, dtype=table.dtype)
    out[:, :nM] = table
    return out


_TABLES = {}


def _table(nM):
    """(bf16 table [R, nM] on the CPU, its padded copy on the GPU), built
    once per width and never modified."""
    if nM not in _TABLES:
        gen = torch.Generator().manual_seed(100 + nM)
        table = (torch.randn(R, nM, generator=gen) * 0.5).to(torch.bfloat16)
        _TABLES[nM] = (table, _padded(table).cuda())
    return _TABLES[nM]


def _csr(U, seed):
    """U words with n_u cycling through NS (the cycle starts at U % 7, so
    that U = 1 is not the empty word).  Every other 64-entry word repeats
    one row 64 times; everything else is random rows, row 0 and row R - 1
    included."""
    gen = torch.Generator().manual_seed(seed)
    slices, repeated = [], []
    for u in range(U):
        n = NS[(u + U) % len(NS)]
        rows = torch.randint(0, R, (n,), generator=gen, dtype=torch.int32)
        if n == 64 and (u // len(NS)) % 2 == 0:
            rows[:] = int(rows[0])
            repeated.append(u)
        elif n >= 2:
            rows[0], rows[-1] = 0, R - 1
        slices.append(rows)
    return slices, repeated


def _pack(slices):
    offsets = [0]
    for s in slices:
        offsets.append(offsets[-1] + len(s))
    idx = torch.cat(slices) if slices else torch.zeros(0, dtype=torch.int32)
    return torch.tensor(offsets, dtype=torch.int32), idx.to(torch.int32)


def _run(table_d, offsets, idx, extra_rows=3):
    """The kernel into an over-allocated, sentinel-filled `out`."""
    U = offsets.numel() - 1
    out = torch.full((U + extra_rows, table_d.shape[1]), SENTINEL,
                     dtype=torch.bfloat16, device="cuda")
    _hip().floret_words_mean(table_d, offsets.cuda(), idx.cuda(), out)
    torch.cuda.synchronize()
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _check_bound(name, got, table, slices):
    """The derived bound of the module docstring, per element."""
    worst = 0.0
    for u, rows in enumerate(slices):
        n = len(rows)
        if n == 0:
            continue
        x = table.double()[rows.long()]
        ref = x.mean(dim=0)
        tol = 2.0 ** -8 * ref.abs() + 2 * n * 2.0 ** -24 * x.abs().mean(dim=0)
        err = (got[u].double() - ref).abs()
        worst = max(worst, float((err / tol).max()))
        assert bool((err <= tol).all()), (
            f"{name}: word {u} (n = {n}) err/tol = {float((err / tol).max()):.3f}")
    print(f"floret bound {name}: worst err/tol = {worst:.3f}")


@need_gpu
@pytest.mark.parametrize("U", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("nM", [300, 96, 50])
def test_floret_words_mean(nM, U):
    table, table_d = _table(nM)
    nMp = table_d.shape[1]
    slices, repeated = _csr(U, 1000 * nM + U)
    offsets, idx = _pack(slices)
    out = _run(table_d, offsets, idx)
    got = out[:U, :nM]

    # rows >= U untouched, pad columns zero
    assert bool((_bits(out[U:]) == _bits(torch.tensor(SENTINEL, dtype=torch.bfloat16))).all())
    assert bool((_bits(out[:U, nM:]) == 0).all())
    # exact cases
    for u, rows in enumerate(slices):
        if len(rows) == 0:
            assert bool((_bits(out[u]) == 0).all()), u
        elif len(rows) == 1:
            assert torch.equal(_bits(got[u]), _bits(table[int(rows[0])])), u
    for u in repeated:
        assert torch.equal(_bits(got[u]), _bits(table[int(slices[u][0])])), u
    if U == 130:
        assert len(repeated) >= 1
        assert {len(s) for s in slices} == set(NS)
    _check_bound(f"nM={nM} U={U}", got, table, slices)
    # two runs, identical bits
    assert torch.equal(_bits(out), _bits(_run(table_d, offsets, idx)))
    assert nMp % 32 == 0


@need_gpu
@pytest.mark.parametrize("nM", [300, 96, 50])
def test_floret_words_mean_order_independence(nM):
    """The same word at two positions of one call, and in two calls with
    different U, gives identical bits."""
    table, table_d = _table(nM)
    slices, _ = _csr(130, 77 + nM)
    offsets, idx = _pack(slices)
    full = _run(table_d, offsets, idx)[:130]
    # every word twice in one call: positions u and 130 + (129 - u)
    twice = slices + slices[::-1]
    o2, i2 = _pack(twice)
    both = _run(table_d, o2, i2)[:260]
    assert torch.equal(_bits(both[:130]), _bits(full))
    assert torch.equal(_bits(both[130:]), _bits(full.flip(0)))
    # a smaller call, the words in another order
    pick = [129, 3, 64, 65, 66, 67, 68, 0, 5, 6, 128, 70, 71]
    o3, i3 = _pack([slices[p] for p in pick])
    sub = _run(table_d, o3, i3)[:len(pick)]
    assert torch.equal(_bits(sub), _bits(full[pick]))


@need_gpu
@pytest.mark.parametrize("nM", [300, 96, 50])
def test_floret_words_mean_guards(nM):
    """Entries equal to R and -1, and an offsets[U] past idx.numel(),
    contribute nothing and touch nothing (ordinary inputs to a guarded
    kernel).  n_u stays the length of the slice inside idx."""
    table, table_d = _table(nM)
    idx = torch.tensor([5, R, -1,            # word 0: one valid entry of 3
                        R, -1,               # word 1: none valid
                        7, 9, 11], dtype=torch.int32)  # word 2: cut short
    offsets = torch.tensor([0, 3, 5, 8 + 100], dtype=torch.int32)
    out = _run(table_d, offsets, idx)
    t32 = table.float()
    want0 = (t32[5] / 3).to(torch.bfloat16)
    want2 = (((t32[7] + t32[9]) + t32[11]) / 3).to(torch.bfloat16)
    assert torch.equal(_bits(out[0, :nM]), _bits(want0))
    assert bool((_bits(out[1]) == 0).all())
    assert torch.equal(_bits(out[2, :nM]), _bits(want2))
    assert bool((_bits(out[:3, nM:]) == 0).all())
    assert bool((_bits(out[3:]) == _bits(torch.tensor(SENTINEL, dtype=torch.bfloat16))).all())
    # negative and descending offsets are clamped to an empty slice
    bad = torch.tensor([-4, 2, 1, 3], dtype=torch.int32)
    out = _run(table_d, bad, idx)
    assert torch.equal(_bits(out[0, :nM]),
                       _bits(((t32[5] + 0) / 2).to(torch.bfloat16)))
    assert bool((_bits(out[1]) == 0).all())
    assert bool((_bits(out[3:]) == _bits(torch.tensor(SENTINEL, dtype=torch.bfloat16))).all())


@need_gpu
def test_floret_words_mean_launcher_checks():
    hip = _hip()
    _, table_d = _table(96)
    offsets = torch.tensor([0, 1], dtype=torch.int32).cuda()
    idx = torch.tensor([3], dtype=torch.int32).cuda()
    out = torch.zeros(1, 96, dtype=torch.bfloat16, device="cuda")
    hip.floret_words_mean(table_d, offsets, idx, out)
    with pytest.raises(RuntimeError, match="offsets"):
        hip.floret_words_mean(table_d, offsets.long(), idx, out)
    with pytest.raises(RuntimeError, match="idx"):
        hip.floret_words_mean(table_d, offsets, idx.long(), out)
    with pytest.raises(RuntimeError, match="table"):
        hip.floret_words_mean(table_d.float(), offsets, idx, out)
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.floret_words_mean(table_d[:, :64], offsets, idx, out[:, :64])
    with pytest.raises(RuntimeError, match="U \\+ 1"):
        hip.floret_words_mean(table_d, torch.tensor([0, 1, 1], dtype=torch.int32).cuda(),
                              idx, out)
    with pytest.raises(RuntimeError, match="U \\+ 1"):
        hip.floret_words_mean(table_d, offsets, idx, out[:, :64].contiguous())


# ------------------------------------------ through the static-vectors ops
T_TOKENS = 129


def _floret_batch(nM, seed):
    """A floret batch built directly: 40 words as a CSR, T = 129 tokens
    that repeat them, -1 at the positions test_gpu_static_vectors uses."""
    table, table_d = _table(nM)
    slices, _ = _csr(40, seed)
    offsets, idx = _pack(slices)
    gen = torch.Generator().manual_seed(seed + 1)
    inverse = torch.randint(0, 40, (T_TOKENS,), generator=gen, dtype=torch.int32)
    inverse[10:30] = 3                       # one word 20 times
    for p in (0, 63, 64, 127, 128):
        inverse[p] = -1
    means64 = torch.stack([
        table.double()[s.long()].mean(dim=0) if len(s) else
        torch.zeros(nM, dtype=torch.float64) for s in slices])
    G64 = means64[inverse.long().clamp(min=0)] * (inverse >= 0)[:, None]
    return table_d, offsets.cuda(), idx.cuda(), inverse.cuda(), G64, gen


def _baseline_gather(table_d, offsets, idx, inverse, nM):
    """Stock torch in bf16: the composed mean, then the gather."""
    from spacy_ray_amd.ops import torch_ref as ref

    temp = ref.floret_words_mean(table_d, offsets, idx)
    G = temp[inverse.long().clamp(min=0)][:, :nM]
    return G.masked_fill((inverse < 0)[:, None], 0)


@need_gpu
@pytest.mark.parametrize("nM", [300, 50])
@pytest.mark.parametrize("nO", [96, 128, 64])
def test_floret_static_vectors_forward_and_dw(monkeypatch, nO, nM):
    from spacy_ray_amd.ops import api as ops

    monkeypatch.setenv("SRX_STATIC_VECTORS", "fused")
    table_d, offsets, idx, inverse, G64, gen = _floret_batch(nM, 31 * nO + nM)
    W = (torch.randn(nO, nM, generator=gen) / math.sqrt(nM)).to(torch.bfloat16)
    dY = (torch.randn(T_TOKENS, nO, generator=gen) * 0.1).to(torch.bfloat16)
    vW = W.cuda().requires_grad_(True)

    assert ops.floret_words_mean_available(table_d)
    temp = ops.floret_words_mean(table_d, offsets, idx)
    assert temp.shape == (40, table_d.shape[1]) and not temp.requires_grad
    assert ops.static_vectors_available(temp, vW) == (nO in (96, 128))
    Y = ops.static_vectors(vW, temp, inverse)
    Y.backward(dY.cuda())
    Gb = _baseline_gather(table_d, offsets, idx, inverse, nM)
    tag = f"nO={nO} nM={nM}"
    ref64.check_parity(f"floret sv fwd {tag}", Y.detach().cpu(),
                       (Gb @ vW.detach().t()).cpu(), G64 @ W.double().t())
    ref64.check_parity(f"floret sv dW {tag}", vW.grad.cpu(),
                       (dY.cuda().t() @ Gb).cpu(), dY.double().t() @ G64)
    assert bool((Y[inverse < 0] == 0).all())


@need_gpu
@pytest.mark.parametrize("width", [96, 128, 64])
def test_floret_multi_hashembed_forward_and_dw(monkeypatch, width):
    from spacy_ray_amd.ops import api as ops

    monkeypatch.setenv("SRX_STATIC_VECTORS", "fused")
    nM = 300
    table_d, offsets, idx, inverse, G64, gen = _floret_batch(nM, 500 + width)
    W = (torch.randn(width, nM, generator=gen) / math.sqrt(nM)).to(torch.bfloat16)
    ids4 = torch.randint(-2 ** 62, 2 ** 62, (T_TOKENS, 4), generator=gen,
                         dtype=torch.int64).cuda()
    tables = [(torch.randn(r, width, generator=gen) * 0.1)
              .to(torch.bfloat16).cuda().requires_grad_(True)
              for r in (50, 30, 30, 30)]
    dX = (torch.randn(T_TOKENS, 5 * width, generator=gen) * 0.1).to(torch.bfloat16)
    vW = W.cuda().requires_grad_(True)
    seeds = [0, 1, 2, 3]

    temp = ops.floret_words_mean(table_d, offsets, idx)
    X0 = ops.multi_hashembed(ids4, seeds, tables)
    X1 = ops.multi_hashembed(ids4, seeds, tables, (temp, inverse, vW))
    assert X1.shape == (T_TOKENS, 5 * width)
    assert torch.equal(X0, X1[:, :4 * width])
    X1.backward(dX.cuda())
    Gb = _baseline_gather(table_d, offsets, idx, inverse, nM)
    dY = dX[:, 4 * width:]
    tag = f"width={width}"
    ref64.check_parity(f"floret mhe fwd {tag}", X1[:, 4 * width:].detach().cpu(),
                       (Gb @ vW.detach().t()).cpu(), G64 @ W.double().t())
    ref64.check_parity(f"floret mhe dW {tag}", vW.grad.cpu(),
                       (dY.cuda().t() @ Gb).cpu(), dY.double().t() @ G64)
    assert all(t.grad is not None for t in tables)


@need_gpu
def test_floret_composed_switch_matches_the_kernel(monkeypatch):
    """SRX_STATIC_VECTORS=composed covers this step too; both paths agree
    to one bf16 rounding of an fp32 mean."""
    from spacy_ray_amd.ops import api as ops

    table_d, offsets, idx, _, _, _ = _floret_batch(300, 9)
    monkeypatch.setenv("SRX_STATIC_VECTORS", "fused")
    fused = ops.floret_words_mean(table_d, offsets, idx)
    monkeypatch.setenv("SRX_STATIC_VECTORS", "composed")
    composed = ops.floret_words_mean(table_d, offsets, idx)
    assert fused.shape == composed.shape and composed.dtype == torch.bfloat16
    err = (fused.float() - composed.float()).abs()
    # two bf16 roundings of fp32 means that differ by summation order only
    assert bool((err <= 2.0 ** -7 * composed.float().abs() + 1e-6).all())


# ---------------------------------------------------------------- training
@need_gpu
@pytest.mark.parametrize("mode", ["fused", "composed"])
def test_floret_vectors_end_to_end(tmp_path, monkeypatch, mode):
    import numpy as np
    from typer.testing import CliRunner

    from test_gpu_static_vectors import E2E_CFG

    from spacy_ray_amd.cli.main import app
    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.models.batch import TokenBatch
    from spacy_ray_amd.ops import api as ops
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Doc, Example

    monkeypatch.setenv("SRX_STATIC_VECTORS", mode)
    rng = np.random.default_rng(0)
    data = rng.standard_normal((500, 50)).astype("f")
    src = tmp_path / "v.floret"
    lines = ["500 50 3 5 2 0 < >"]
    for r in rng.permutation(500).tolist():
        lines.append(f"{r} " + " ".join(repr(float(x)) for x in data[r]))
    src.write_text("\n".join(lines) + "\n")
    r = CliRunner().invoke(app, ["init", "vectors", "en", str(src),
                                 str(tmp_path / "vec"), "--mode", "floret"])
    assert r.exit_code == 0, r.output

    cfg = Config.from_str(E2E_CFG, overrides={"paths.vectors": str(tmp_path / "vec")})
    nlp = init_nlp(cfg, device="cuda:0", sample_size=32)
    assert nlp.vocab.vectors.is_floret
    table_before = nlp.vocab.vectors.data.copy()
    assert np.array_equal(table_before, data)
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
    embed = nlp.tok2vec.module.embed
    assert not any("table" in k and "static" in k
                   for k in nlp.tok2vec.module.state_dict())

    # a doc made only of never-seen words: non-zero static-vector columns
    unseen = Doc(nlp.vocab, ["qwrtzx", "blorptangle", "żółwik", "日本語"])
    batch = TokenBatch([unseen], nlp.device)
    sv = embed.static_vectors
    with torch.no_grad():
        X = ops.multi_hashembed(batch.attr_ids, embed.seeds, list(embed.tables),
                                (*sv.table_and_rows(batch), sv.W))
    block = X[:, 4 * 96:].float()
    assert bool((block[:4].abs().sum(dim=1) > 0).all())
    assert bool((block[4:] == 0).all())      # the pad pseudo-doc

    sub = [d.copy_unannotated() for d in docs[:20]]
    nlp.predict_docs(sub)
    out = tmp_path / "ckpt"
    nlp.to_disk(out)
    assert (out / "vocab" / "vectors.safetensors").exists()
    nlp2 = init_nlp(cfg, device="cuda:0", sample_size=32)
    nlp2.from_disk(out)
    # the trained pipeline computes in the engine's bf16; give the reloaded
    # one the same compute type (the checkpoint holds bf16 values, so the
    # cast is exact): fp32 against bf16 scores may break a near-tie apart
    ZeRO1Engine(nlp2, T["optimizer"], LocalComm())
    assert nlp2.vocab.vectors.is_floret
    assert nlp2.vocab.vectors.floret_settings() == nlp.vocab.vectors.floret_settings()
    sub2 = [d.copy_unannotated() for d in docs[:20]]
    for d in sub2:
        d.vocab = nlp2.vocab
        d.vector_rows = {}
    nlp2.predict_docs(sub2)
    assert [d.tags for d in sub] == [d.tags for d in sub2]
