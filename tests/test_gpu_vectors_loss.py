"""vectors_loss (srx_vecloss.hip.h) against float64, its dispatch through
ops.vectors_loss, and pretrain_tok2vec(objective="vectors") on the GPU.

Inputs are built on the CPU from a seeded generator and rounded to bf16; the
float64 reference (torch_ref.vectors_loss in float64, itself checked against
a numpy transcription in test_vectors_loss.py) is computed from exactly
those values.

The bound is derived, not tuned.  u = 2^-24.  Products of two bf16 values
are exact in fp32, so each of p.p, y.y, p.y is an fp32 sum of nM exact
terms: in any order its error is at most nM u sum |terms|, that is a
relative e = nM u for |p|^2 and |y|^2 and an absolute e |p| |y| for p.y
(Cauchy-Schwarz).  First order, with c = p.y / (|p| |y|), |c| <= 1:

  inv = 1 / (sqrt(pp) sqrt(yy))   relative e + 7u  (two square roots of 2u,
                                  a product, a division of 2u)
  c = py inv                      absolute 2e + 8u
  loss_i = 1 - c                  absolute 2e + 10u
  ca = -scale inv                 relative e + 9u  (scale itself is rounded)
  cb = scale c / pp               absolute (3e + 11u) scale / |p|^2
  g = ca y + cb p                 absolute
        scale ((e + 10u) |y_e| / (|p| |y|) + (3e + 12u) |p_e| / |p|^2)
        + u |g|

and g is rounded to bf16 once (2^-8 |ref|, which also covers u |g|).  For
L2, d = p - y, g = scale d and loss_i = sum d^2 give (2^-8 + 8u) |ref| per
gradient element and a relative e + 3u for the row loss.  Every fp32 term is
doubled for the second-order terms, as in test_gpu_floret.py:

  cosine  |dg|    <= 2^-8 |ref| + 2 scale u ((nM + 10) |y_e| / (|p| |y|)
                                             + (3 nM + 12) |p_e| / |p|^2)
          |dloss| <= 2 (2 nM + 10) u
  L2      |dg|    <= (2^-8 + 8u) |ref|,   |dloss| <= 2 (nM + 3) u |ref|

The total is scale * torch.sum of N fp32 row losses: the row bounds summed,
plus 2 (N + 2) u sum |loss_i|, times scale.  The composed bf16 path does the
same arithmetic in another order with no more roundings than counted above,
so it is held to the same bound."""
import math

import pytest
import torch

from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.ops import torch_ref as ref

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

V = 257
ZERO_ROW = 7
NMS = (32, 50, 96, 300)
NS = (1, 63, 64, 65, 257)
LOSSES = ("cosine", "L2")
SENTINEL = 1.5
U = 2.0 ** -24


def _hip():
    hip = ops.hip_ext()
    assert hip is not None
    return hip


def _bits(t):
    return t.contiguous().view(torch.int16)


_TABLES, _INPUTS, _REFS = {}, {}, {}


def _table(nM, nMp=None):
    """(bf16 table [V, nM] on the CPU, its zero-padded copy on the GPU);
    row ZERO_ROW is all zero.  Built once per width, never modified."""
    nMp = nMp or -(-nM // 32) * 32
    if (nM, nMp) not in _TABLES:
        gen = torch.Generator().manual_seed(300 + nM)
        table = (torch.randn(V, nM, generator=gen) * 0.5).to(torch.bfloat16)
        table[ZERO_ROW] = 0
        padded = torch.zeros(V, nMp, dtype=torch.bfloat16)
        padded[:, :nM] = table
        _TABLES[(nM, nMp)] = (table, padded.cuda())
    return _TABLES[(nM, nMp)]


def _inputs(nM, N):
    """(pred bf16 [N, nM], rows int32 [N]) on the CPU.  The rows cycle
    through 0, V - 1, -1, V, V + 5, the all-zero row and four random rows;
    token 8 (a random row) predicts zero."""
    if (nM, N) not in _INPUTS:
        gen = torch.Generator().manual_seed(7000 + 10 * nM + N)
        pred = torch.randn(N, nM, generator=gen).to(torch.bfloat16)
        rows = torch.randint(0, V, (N,), generator=gen, dtype=torch.int32)
        rows[rows == ZERO_ROW] = ZERO_ROW + 1
        special = [0, V - 1, -1, V, V + 5, ZERO_ROW]
        for i in range(N):
            if i % 10 < len(special):
                rows[i] = special[i % 10]
        if N > 8:
            pred[8] = 0
        _INPUTS[(nM, N)] = (pred, rows)
    return _INPUTS[(nM, N)]


def _skipped(pred, rows, loss):
    skip = (rows < 0) | (rows >= V)
    if loss == "cosine":
        skip = skip | (rows == ZERO_ROW) | ~pred.bool().any(dim=1)
    return skip


def _reference(nM, N, loss):
    """float64 (row_loss, dpred, row tolerance, dpred tolerance, total,
    total tolerance) for scale = 1 / N; computed once per case."""
    key = (nM, N, loss)
    if key in _REFS:
        return _REFS[key]
    table, _ = _table(nM)
    pred, rows = _inputs(nM, N)
    scale = 1.0 / N
    p, t = pred.double(), table.double()
    rl, dp = ref.vectors_loss(p, t, rows, loss, scale)
    skip = _skipped(pred, rows, loss)
    assert bool((rl[skip] == 0).all()) and not bool(dp[skip].any())
    if loss == "cosine":
        y = t[rows.long().clamp(0, V - 1)]
        pn = p.norm(dim=1, keepdim=True).clamp_min(1e-300)
        yn = y.norm(dim=1, keepdim=True).clamp_min(1e-300)
        tol_d = 2.0 ** -8 * dp.abs() + 2 * scale * U * (
            (nM + 10) * y.abs() / (pn * yn) + (3 * nM + 12) * p.abs() / pn ** 2)
        tol_l = torch.full_like(rl, 2 * (2 * nM + 10) * U)
    else:
        tol_d = (2.0 ** -8 + 8 * U) * dp.abs()
        tol_l = 2 * (nM + 3) * U * rl.abs()
    tol_d = tol_d.masked_fill(skip[:, None], 0)
    tol_l = tol_l.masked_fill(skip, 0)
    total = scale * rl.sum()
    tol_t = scale * (tol_l.sum() + 2 * (N + 2) * U * rl.abs().sum())
    _REFS[key] = (rl, dp, tol_l, tol_d, float(total), float(tol_t))
    return _REFS[key]


def _check(name, nM, N, loss, row_loss, dpred):
    rl, dp, tol_l, tol_d, _, _ = _reference(nM, N, loss)
    err_d = (dpred.double() - dp).abs()
    err_l = (row_loss.double() - rl).abs()
    live = tol_d > 0
    print(f"vectors_loss {name} nM={nM} N={N} {loss}: worst dPred err/tol = "
          f"{float((err_d[live] / tol_d[live]).max()) if bool(live.any()) else 0:.3f}, "
          f"row loss err/tol = "
          f"{float((err_l / tol_l.clamp_min(1e-300)).max()):.3f}")
    assert bool((err_d <= tol_d).all()), name
    assert bool((err_l <= tol_l).all()), name


def _run(pred_d, table_d, rows, loss, scale, extra_rows=3):
    """The kernel into over-allocated, sentinel-filled outputs."""
    N, nM = pred_d.shape
    row_loss = torch.full((N + extra_rows,), SENTINEL, device="cuda")
    dpred = torch.full((N + extra_rows, nM), SENTINEL, dtype=torch.bfloat16,
                       device="cuda")
    _hip().vectors_loss(pred_d, table_d, rows.cuda(), row_loss, dpred,
                        loss == "L2", scale)
    torch.cuda.synchronize()
    return row_loss.cpu(), dpred.cpu()


def _sentinel_only(t):
    return bool((_bits(t.to(torch.bfloat16))
                 == _bits(torch.tensor(SENTINEL, dtype=torch.bfloat16))).all())


@need_gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nM", NMS)
def test_vectors_loss_kernel(nM, N, loss):
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    row_loss, dpred = _run(pred.cuda(), table_d, rows, loss, 1.0 / N)
    # rows beyond N untouched
    assert _sentinel_only(row_loss[N:]) and _sentinel_only(dpred[N:])
    _check("kernel", nM, N, loss, row_loss[:N], dpred[:N])
    # skipped rows: loss 0, gradient bit-exact zero
    skip = _skipped(pred, rows, loss)
    assert bool((_bits(dpred[:N][skip]) == 0).all())
    assert bool((row_loss[:N][skip] == 0).all())
    if N >= 63:
        # per ten rows: -1, V, V + 5, and for the cosine the all-zero row
        assert int(skip.sum()) >= (4 if loss == "cosine" else 3) * (N // 10)
    # a second run gives the same bits
    row_loss2, dpred2 = _run(pred.cuda(), table_d, rows, loss, 1.0 / N)
    assert torch.equal(row_loss2, row_loss)
    assert torch.equal(_bits(dpred2), _bits(dpred))


@need_gpu
def test_vectors_loss_empty_batch():
    _, table_d = _table(50)
    pred = torch.zeros(0, 50, dtype=torch.bfloat16, device="cuda")
    rows = torch.zeros(0, dtype=torch.int32)
    row_loss, dpred = _run(pred, table_d, rows, "cosine", 1.0)
    assert _sentinel_only(row_loss) and _sentinel_only(dpred)  # no launch
    p = pred.clone().requires_grad_()
    out = ops.vectors_loss(p, table_d, rows.cuda(), loss="cosine", scale=1.0)
    out.backward()
    assert float(out.detach()) == 0.0 and p.grad.shape == (0, 50)


@need_gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("nM", NMS)
def test_strided_views_write_only_their_window(nM, loss):
    """pred and dPred as windows of larger sentinel-filled buffers (extra
    rows on both sides, extra columns): same bits as the contiguous run,
    nothing outside the window is written."""
    N = 65
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    want_l, want_d = _run(pred.cuda(), table_d, rows, loss, 1.0 / N)
    for extra_cols in (3, 8):  # a 2-byte and a 16-byte aligned row stride
        ld = nM + extra_cols
        pbuf = torch.full((N + 4, ld), float("nan"), dtype=torch.bfloat16,
                          device="cuda")
        pbuf[2:2 + N, :nM] = pred.cuda()
        dbuf = torch.full((N + 4, ld), SENTINEL, dtype=torch.bfloat16,
                          device="cuda")
        row_loss = torch.full((N + 3,), SENTINEL, device="cuda")
        _hip().vectors_loss(pbuf[2:2 + N, :nM], table_d, rows.cuda(), row_loss,
                            dbuf[2:, :nM], loss == "L2", 1.0 / N)
        torch.cuda.synchronize()
        dbuf, row_loss = dbuf.cpu(), row_loss.cpu()
        assert torch.equal(_bits(dbuf[2:2 + N, :nM]), _bits(want_d[:N]))
        assert torch.equal(row_loss[:N], want_l[:N])
        assert _sentinel_only(row_loss[N:])
        assert _sentinel_only(dbuf[:2]) and _sentinel_only(dbuf[2 + N:])
        assert _sentinel_only(dbuf[:, nM:])


@need_gpu
@pytest.mark.parametrize("nM,offset", [(50, 50), (50, 1), (300, 300), (300, 2),
                                       (32, 4), (96, 1)])
def test_misaligned_base_matches_the_aligned_run(nM, offset):
    """A view that starts `offset` elements into its buffer (one row of nM =
    50: a 4-byte aligned base; one row of 300: 8 bytes; one element: 2
    bytes) takes narrower loads and stores and gives the same bits."""
    N = 65
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    for loss in LOSSES:
        want_l, want_d = _run(pred.cuda(), table_d, rows, loss, 1.0 / N)
        pflat = torch.full((offset + N * nM + 8,), float("nan"),
                           dtype=torch.bfloat16, device="cuda")
        pview = pflat[offset:offset + N * nM].view(N, nM)
        pview.copy_(pred)
        assert pview.data_ptr() % 16 == (2 * offset) % 16
        dflat = torch.full((offset + N * nM + 8,), SENTINEL,
                           dtype=torch.bfloat16, device="cuda")
        row_loss = torch.full((N,), SENTINEL, device="cuda")
        _hip().vectors_loss(pview, table_d, rows.cuda(), row_loss,
                            dflat[offset:offset + N * nM].view(N, nM),
                            loss == "L2", 1.0 / N)
        torch.cuda.synchronize()
        dflat = dflat.cpu()
        assert torch.equal(row_loss.cpu(), want_l[:N])
        assert torch.equal(_bits(dflat[offset:offset + N * nM].view(N, nM)),
                           _bits(want_d[:N]))
        assert _sentinel_only(dflat[:offset])
        assert _sentinel_only(dflat[offset + N * nM:])


@need_gpu
@pytest.mark.parametrize("loss", LOSSES)
def test_nan_in_skipped_rows_reaches_no_output(loss):
    nM, N = 50, 65
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    want_l, want_d = _run(pred.cuda(), table_d, rows, loss, 1.0 / N)
    bad = pred.clone()
    hidden = (rows < 0) | (rows >= V)
    if loss == "cosine":
        hidden = hidden | (rows == ZERO_ROW)
    bad[hidden] = float("nan")
    bad[torch.nonzero(hidden)[0, 0], 3] = float("inf")
    row_loss, dpred = _run(bad.cuda(), table_d, rows, loss, 1.0 / N)
    assert torch.equal(row_loss, want_l)
    assert torch.equal(_bits(dpred), _bits(want_d))


@need_gpu
@pytest.mark.parametrize("mode", ["fused", "composed"])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("nM", [50, 300])
def test_op_dispatch_and_autograd(monkeypatch, nM, loss, mode):
    N = 257
    monkeypatch.setenv("SRX_VECTORS_LOSS", mode)
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    assert ops.vectors_loss_available(pred.cuda(), table_d)
    calls = []
    hip = _hip()
    real = hip.vectors_loss
    monkeypatch.setattr(hip, "vectors_loss",
                        lambda *a: (calls.append(1), real(*a))[1])
    p = pred.cuda().requires_grad_()
    out = ops.vectors_loss(p, table_d, rows.cuda(), loss=loss, scale=1.0 / N)
    assert len(calls) == (1 if mode == "fused" else 0)
    assert out.dim() == 0 and out.dtype == torch.float32
    _, dp, _, tol_d, total, tol_t = _reference(nM, N, loss)
    print(f"vectors_loss op {mode} nM={nM} {loss}: total {float(out):.7f} "
          f"ref {total:.7f} tol {tol_t:.3g}")
    assert abs(float(out) - total) <= tol_t
    # a non-unit upstream gradient scales dPred; 0.75 dp is exact in fp32
    # but rounds once more in bf16
    (0.75 * out).backward()
    assert p.grad.dtype == torch.bfloat16
    err = (p.grad.cpu().double() - 0.75 * dp).abs()
    assert bool((err <= 0.75 * tol_d
                 + 2.0 ** -8 * 0.75 * (dp.abs() + tol_d)).all())
    skip = _skipped(pred, rows, loss)
    assert bool((_bits(p.grad.cpu()[skip]) == 0).all())


@need_gpu
def test_op_mode_errors_and_composed_fallbacks(monkeypatch):
    nM, N = 50, 65
    _, table_d = _table(nM)
    pred, rows = _inputs(nM, N)
    monkeypatch.setenv("SRX_VECTORS_LOSS", "hip")
    with pytest.raises(ValueError, match="SRX_VECTORS_LOSS"):
        ops.vectors_loss(pred.cuda(), table_d, rows.cuda())
    monkeypatch.setenv("SRX_VECTORS_LOSS", "fused")
    hip = _hip()
    monkeypatch.setattr(hip, "vectors_loss", lambda *a: pytest.fail(
        "the kernel cannot take these inputs"))
    _, dp, _, tol_d, total, tol_t = _reference(nM, N, "cosine")
    # fp32 pred: composed, and well inside the bf16 bound
    p = pred.float().cuda().requires_grad_()
    assert not ops.vectors_loss_available(p, table_d)
    out = ops.vectors_loss(p, table_d, rows.cuda(), scale=1.0 / N)
    out.backward()
    assert abs(float(out) - total) <= tol_t
    assert bool(((p.grad.cpu().double() - dp).abs() <= tol_d).all())
    # a table wider than the kernel takes: nM = 340, nMp = 352
    table, wide_d = _table(340, 352)
    gen = torch.Generator().manual_seed(9)
    wp = torch.randn(N, 340, generator=gen).to(torch.bfloat16)
    p = wp.cuda().requires_grad_()
    assert not ops.vectors_loss_available(p, wide_d)
    out = ops.vectors_loss(p, wide_d, rows.cuda(), loss="L2", scale=1.0 / N)
    out.backward()
    want_l, want_d = ref.vectors_loss(wp.double(), table.double(), rows, "L2",
                                      1.0 / N)
    assert math.isclose(float(out), float(want_l.sum() / N), rel_tol=1e-4)
    assert bool(((p.grad.cpu().double() - want_d).abs()
                 <= (2.0 ** -8 + 8 * U) * want_d.abs()).all())


# ------------------------------------------------------------- end to end
E2E_CFG = """
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
n_docs = 40
words_per_doc = 12
vocab_size = 120
n_tags = 10
seed = 0

[corpora.dev]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 5
words_per_doc = 12
vocab_size = 120
n_tags = 10
seed = 1

[training]
train_corpus = "corpora.train"
dev_corpus = "corpora.dev"
seed = 0

[training.optimizer]
@optimizers = "Adam.v1"
learn_rate = 0.01
"""


@need_gpu
@pytest.mark.parametrize("mode", ["default", "floret"])
def test_pretrain_vectors_end_to_end(monkeypatch, mode):
    import numpy as np

    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.train.pretrain import pretrain_tok2vec
    from spacy_ray_amd.vocab.doc import Example
    from spacy_ray_amd.vocab.vectors import Vectors

    torch.manual_seed(0)
    nlp = init_nlp(Config.from_str(E2E_CFG), device="cuda:0", sample_size=16)
    rng = np.random.default_rng(5)
    if mode == "floret":
        nlp.vocab.vectors = Vectors(rng.standard_normal((64, 50)).astype("f"),
                                    mode="floret", minn=2, maxn=3)
    else:
        nlp.vocab.vectors = Vectors.from_words(
            [f"w{i}" for i in range(120)],
            rng.standard_normal((120, 50)).astype("f"))
    docs = make_synthetic_docs(nlp.vocab, n_docs=96, words_per_doc=12,
                               vocab_size=120, n_tags=10, n_deps=5,
                               n_ent_types=2, seed=3)
    examples = [Example.from_doc(d) for d in docs]
    calls = []
    hip = _hip()
    real = hip.vectors_loss
    monkeypatch.setattr(hip, "vectors_loss",
                        lambda *a: (calls.append(1), real(*a))[1])
    losses = pretrain_tok2vec(nlp, lambda n: iter(examples), steps=30,
                              batch_docs=24, learn_rate=5e-3, log_every=10,
                              log=lambda *a: None, objective="vectors",
                              hidden_size=64)
    assert len(losses) == 3 and all(math.isfinite(x) for x in losses), losses
    assert losses[-1] < losses[0], losses
    if ops.VECTORS_LOSS_FUSED_DEFAULT:
        assert len(calls) == 30  # the kernel ran, not the composed path
