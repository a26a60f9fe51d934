"""The vectors pretraining objective on the CPU: ops.vectors_loss against a
plain-numpy transcription of its formulas, its gradient, and
pretrain_tok2vec(objective="vectors") through the public surface."""
import numpy as np
import pytest
import torch

from spacy_ray_amd.config.config import Config
from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.ops import torch_ref as ref
from spacy_ray_amd.pipeline.language import (check_static_vectors_config,
                                             init_nlp)
from spacy_ray_amd.train.pretrain import (load_init_tok2vec, pretrain_tok2vec,
                                          save_tok2vec)
from spacy_ray_amd.vocab.vectors import Vectors

CFG = "examples/configs/en_tagger_cpu.cfg"
LOSSES = ("cosine", "L2")


# ------------------------------------------------------------------ the op
def _numpy_vectors_loss(pred, table, rows, loss, scale):
    """The formulas of ops.vectors_loss, row by row."""
    N, nM = pred.shape
    V = table.shape[0]
    row_loss = np.zeros(N)
    dpred = np.zeros((N, nM))
    for i in range(N):
        r = int(rows[i])
        if r < 0 or r >= V:
            continue
        p, y = pred[i], table[r, :nM]
        if loss == "cosine":
            if not y.any() or float(p @ p) == 0.0:
                continue
            norm = np.sqrt(p @ p) * np.sqrt(y @ y)
            c = float(p @ y) / norm
            row_loss[i] = 1.0 - c
            dpred[i] = -scale * (y / norm - c * p / (p @ p))
        else:
            row_loss[i] = ((p - y) ** 2).sum()
            dpred[i] = scale * (p - y)
    return scale * row_loss.sum(), row_loss, dpred


def _case():
    """N = 7, nM = 5, V = 6 with a padded table; rows 2 and 3 are outside
    the table, row 4 points at an all-zero vector, row 5 predicts zero."""
    g = torch.Generator().manual_seed(11)
    N, nM, V = 7, 5, 6
    table = torch.randn(V, 8, generator=g, dtype=torch.float64)
    table[:, nM:] = 0
    table[3] = 0
    pred = torch.randn(N, nM, generator=g, dtype=torch.float64)
    pred[5] = 0
    rows = torch.tensor([0, V - 1, -1, V, 3, 1, 2], dtype=torch.int32)
    return pred, table, rows


@pytest.mark.parametrize("loss", LOSSES)
def test_reference_matches_numpy_transcription(loss):
    pred, table, rows = _case()
    scale = 1.0 / 7
    want, want_rows, want_d = _numpy_vectors_loss(
        pred.numpy(), table.numpy(), rows.numpy(), loss, scale)
    row_loss, dpred = ref.vectors_loss(pred, table, rows, loss, scale)
    assert row_loss.dtype == torch.float64 and dpred.dtype == torch.float64
    np.testing.assert_allclose(row_loss.numpy(), want_rows, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dpred.numpy(), want_d, rtol=1e-12, atol=1e-14)
    skipped = [2, 3, 4, 5] if loss == "cosine" else [2, 3]
    for i in range(7):
        assert (want_rows[i] == 0 and not want_d[i].any()) == (i in skipped), i
    # through the public op: value and autograd
    p = pred.clone().requires_grad_()
    out = ops.vectors_loss(p, table, rows, loss=loss, scale=scale)
    assert out.dim() == 0 and out.dtype == torch.float64
    np.testing.assert_allclose(out.item(), want, rtol=1e-12)
    (3.0 * out).backward()
    np.testing.assert_allclose(p.grad.numpy(), 3.0 * want_d, rtol=1e-12, atol=1e-14)
    assert not p.grad[skipped].any()  # exactly zero


def test_skipped_rows_hide_non_finite_predictions():
    pred, table, rows = _case()
    pred[2] = float("nan")
    pred[3] = float("inf")
    pred[4, 1] = float("nan")  # all-zero target: skipped by the cosine only
    p = pred.clone().requires_grad_()
    out = ops.vectors_loss(p, table, rows, loss="cosine", scale=0.5)
    out.backward()
    assert torch.isfinite(out) and torch.isfinite(p.grad).all()
    assert not p.grad[[2, 3, 4, 5]].any()


def test_gradient_cosine_gradcheck():
    pred, table, rows = _case()
    live = [0, 1, 6]
    p = pred[live].clone().requires_grad_()
    assert torch.autograd.gradcheck(
        lambda x: ops.vectors_loss(x, table, rows[live], loss="cosine", scale=0.3),
        (p,), eps=1e-6, atol=1e-7)


def test_gradient_l2_is_thinc_half_gradient():
    """thinc's L2Distance returns (p - y) for the loss sum (p - y)^2: the
    op's gradient is HALF the derivative of its value, by definition.  The
    value is quadratic, so a central difference is its exact derivative."""
    pred, table, rows = _case()
    live = [0, 1, 4, 5, 6]  # the L2 loss skips out-of-table rows only
    x = pred[live].clone()
    r = rows[live]
    f = lambda v: ops.vectors_loss(v, table, r, loss="L2", scale=0.3)
    p = x.clone().requires_grad_()
    f(p).backward()
    numeric = torch.zeros_like(x)
    h = 1e-3
    for i in range(x.shape[0]):
        for j in range(x.shape[1]):
            e = torch.zeros_like(x)
            e[i, j] = h
            numeric[i, j] = (f(x + e) - f(x - e)) / (2 * h)
    np.testing.assert_allclose(p.grad.numpy(), 0.5 * numeric.numpy(),
                               rtol=1e-8, atol=1e-10)
    y = table[r.long(), :5]
    np.testing.assert_allclose(p.grad.numpy(), 0.3 * (x - y).numpy(), rtol=1e-12)


def test_op_argument_errors(monkeypatch):
    pred, table, rows = _case()
    with pytest.raises(ValueError, match="cosine"):
        ops.vectors_loss(pred, table, rows, loss="l1")
    with pytest.raises(ValueError, match="rows"):
        ops.vectors_loss(pred, table, rows[:3])
    monkeypatch.setenv("SRX_VECTORS_LOSS", "bogus")
    with pytest.raises(ValueError, match="SRX_VECTORS_LOSS"):
        ops.vectors_loss(pred, table, rows)
    monkeypatch.setenv("SRX_VECTORS_LOSS", "fused")  # CPU: composed anyway
    assert torch.isfinite(ops.vectors_loss(pred, table, rows))
    assert not ops.vectors_loss_available(pred, table)


# ----------------------------------------------------------- the objective
def _corpus(nlp):
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.vocab.doc import Example

    docs = make_synthetic_docs(nlp.vocab, n_docs=96, words_per_doc=12,
                               vocab_size=120, n_tags=10, n_deps=5,
                               n_ent_types=2, seed=3)
    return [Example.from_doc(d) for d in docs]


def _vectors(mode):
    rng = np.random.default_rng(5)
    if mode == "floret":
        return Vectors(rng.standard_normal((64, 16)).astype("f"), mode="floret",
                       minn=2, maxn=3)
    return Vectors.from_words([f"w{i}" for i in range(120)],
                              rng.standard_normal((120, 16)).astype("f"))


def _pretrain(nlp, examples, **kw):
    return pretrain_tok2vec(nlp, lambda n: iter(examples), batch_docs=24,
                            learn_rate=5e-3, log=lambda *a: None,
                            objective="vectors", hidden_size=32, **kw)


@pytest.mark.parametrize("mode,loss", [("default", "cosine"), ("default", "L2"),
                                       ("floret", "cosine")])
def test_pretrain_vectors_loss_falls_and_weights_roundtrip(tmp_path, mode, loss):
    torch.manual_seed(0)
    cfg = Config.from_disk(CFG)
    nlp = init_nlp(cfg, device="cpu", sample_size=16)
    nlp.vocab.vectors = _vectors(mode)
    before = {k: v.clone() for k, v in nlp.tok2vec.module.state_dict().items()}
    losses = _pretrain(nlp, _corpus(nlp), steps=40, log_every=10, loss=loss)
    assert len(losses) == 4 and all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses
    state = nlp.tok2vec.module.state_dict()
    assert any(not torch.equal(before[k], state[k]) for k in state)
    # only the tok2vec is saved: the head is gone
    save_tok2vec(nlp, tmp_path)
    torch.manual_seed(1)
    nlp2 = init_nlp(cfg, device="cpu", sample_size=16)
    assert load_init_tok2vec(nlp2, tmp_path) == len(state)
    after = nlp2.tok2vec.module.state_dict()
    assert list(after) == list(state)
    for k in state:
        assert torch.equal(after[k], state[k]), k


def test_pretrain_vectors_needs_a_table():
    cfg = Config.from_disk(CFG)
    nlp = init_nlp(cfg, device="cpu", sample_size=16)
    assert nlp.vocab.vectors is None
    with pytest.raises(ValueError, match=r"init vectors.*\[initialize\] vectors"):
        _pretrain(nlp, _corpus(nlp), steps=1)
    with pytest.raises(ValueError, match="objective"):
        pretrain_tok2vec(nlp, lambda n: iter([]), objective="characters")
    with pytest.raises(ValueError, match="loss"):
        pretrain_tok2vec(nlp, lambda n: iter([]), objective="vectors", loss="l1")


VEC_CFG = """
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
width = 32
attrs = ["NORM", "PREFIX", "SUFFIX", "SHAPE"]
rows = [200, 100, 100, 100]
include_static_vectors = %(static)s

[components.tok2vec.model.encode]
@architectures = "spacy.MaxoutWindowEncoder.v2"
width = 32
depth = 1
window_size = 1
maxout_pieces = 3

[components.tagger]
factory = "tagger"

[components.tagger.model]
@architectures = "spacy.Tagger.v2"

[components.tagger.model.tok2vec]
@architectures = "spacy.Tok2VecListener.v1"
width = 32

[corpora]

[corpora.train]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 40
words_per_doc = 10
vocab_size = 120
n_tags = 6
seed = 0

[corpora.dev]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 5
words_per_doc = 10
vocab_size = 120
n_tags = 6
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

OBJECTIVE_BLOCK = """
[pretraining]

[pretraining.objective]
@architectures = "spacy.PretrainVectors.v1"
maxout_pieces = 2
hidden_size = 24
loss = "L2"
"""


def _vec_dir(tmp_path, mode="default"):
    _vectors(mode).to_disk(tmp_path / "vec" / "vocab")
    return tmp_path / "vec"


@pytest.mark.parametrize("mode", ["default", "floret"])
def test_masked_tokens_are_oov_on_the_input_side(tmp_path, monkeypatch, mode):
    """include_static_vectors = true: the embed layer must not see the
    vector that the head has to predict."""
    from spacy_ray_amd.models.batch import TokenBatch
    from spacy_ray_amd.models.layers import StaticVectors
    from spacy_ray_amd.train import pretrain as mod

    cfg = Config.from_str(VEC_CFG % {"static": "true"},
                          overrides={"paths.vectors": str(_vec_dir(tmp_path, mode))})
    torch.manual_seed(0)
    nlp = init_nlp(cfg, device="cpu", sample_size=8)
    examples = _corpus(nlp)[:24]

    def originals(batch):
        if mode == "floret":
            return batch.get_floret("ORTH")[0]
        return batch.get_vec_rows("ORTH")

    seen, batches, targets = [], [], []
    inner = StaticVectors.table_and_rows

    def spy_rows(self, batch):
        table, rows = inner(self, batch)
        seen.append(rows.clone())
        return table, rows

    class SpyBatch(TokenBatch):
        __slots__ = ()

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            batches.append((self, originals(self).clone()))

    real_loss = ops.vectors_loss

    def spy_loss(pred, table, rows, **kw):
        targets.append(rows.clone())
        return real_loss(pred, table, rows, **kw)

    monkeypatch.setattr(StaticVectors, "table_and_rows", spy_rows)
    monkeypatch.setattr(mod, "TokenBatch", SpyBatch)
    monkeypatch.setattr(mod.ops, "vectors_loss", spy_loss)
    _pretrain(nlp, examples, steps=1, mask_rate=0.3, seed=4)

    assert len(seen) == 1 and len(batches) == 1 and len(targets) == 1
    batch, before = batches[0]
    total = batch.n_real_tokens
    mask = torch.from_numpy(
        np.random.RandomState(4).random_sample(total) < 0.3)
    assert 0 < int(mask.sum()) < total
    got = seen[0]
    assert got.shape == before.shape
    assert bool((before[:total] >= 0).all())  # every corpus word has a vector
    assert bool((got[:total][mask] == -1).all())
    assert torch.equal(got[:total][~mask], before[:total][~mask])
    assert torch.equal(got[total:], before[total:])
    # the targets are the originals, and the batch itself is untouched
    assert torch.equal(targets[0], before[:total][mask])
    assert torch.equal(originals(batch), before)


# -------------------------------------------------------------------- CLI
def _write_cfg(tmp_path, text, name="config.cfg"):
    path = tmp_path / name
    path.write_text(text)
    return path


def test_cli_pretrain_vectors(tmp_path, monkeypatch):
    from typer.testing import CliRunner

    from spacy_ray_amd.cli.main import app
    from spacy_ray_amd.train import pretrain as mod

    vec = _vec_dir(tmp_path)
    plain = _write_cfg(tmp_path, VEC_CFG % {"static": "false"})
    calls = []
    real = mod.pretrain_tok2vec

    def spy(*a, **kw):
        calls.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(mod, "pretrain_tok2vec", spy)
    run = CliRunner().invoke
    out = tmp_path / "out1"
    r = run(app, ["pretrain", str(plain), str(out), "--objective", "vectors",
                  "--steps", "3", "--batch-docs", "16", "--hidden-size", "16",
                  f"--paths.vectors={vec}"])
    assert r.exit_code == 0, r.output
    assert (out / "tok2vec.safetensors").exists()
    assert calls[-1]["objective"] == "vectors" and calls[-1]["hidden_size"] == 16
    assert "loss" not in calls[-1]  # the function's default: cosine

    # the [pretraining.objective] block selects it without the flag ...
    block = _write_cfg(tmp_path, VEC_CFG % {"static": "false"} + OBJECTIVE_BLOCK,
                       "block.cfg")
    out = tmp_path / "out2"
    r = run(app, ["pretrain", str(block), str(out), "--steps", "3",
                  "--batch-docs", "16", f"--paths.vectors={vec}"])
    assert r.exit_code == 0, r.output
    assert (out / "tok2vec.safetensors").exists()
    assert calls[-1] == {**calls[-1], "objective": "vectors", "loss": "L2",
                         "hidden_size": 24, "maxout_pieces": 2}
    # ... and flags override the block
    r = run(app, ["pretrain", str(block), str(tmp_path / "out3"), "--steps", "2",
                  "--batch-docs", "16", "--loss", "cosine", "--maxout-pieces", "3",
                  f"--paths.vectors={vec}"])
    assert r.exit_code == 0, r.output
    assert calls[-1]["loss"] == "cosine" and calls[-1]["maxout_pieces"] == 3
    assert calls[-1]["hidden_size"] == 24
    r = run(app, ["pretrain", str(block), str(tmp_path / "out4"), "--steps", "2",
                  "--batch-docs", "16", "--objective", "masked",
                  f"--paths.vectors={vec}"])
    assert r.exit_code == 0, r.output
    assert calls[-1]["objective"] == "masked"

    n = len(calls)
    r = run(app, ["pretrain", str(plain), str(tmp_path / "bad"), "--objective",
                  "vectors", "--loss", "manhattan", f"--paths.vectors={vec}"])
    assert r.exit_code != 0 and "--loss" in r.output
    r = run(app, ["pretrain", str(plain), str(tmp_path / "bad"), "--objective",
                  "characters", f"--paths.vectors={vec}"])
    assert r.exit_code != 0 and "--objective" in r.output
    # the vectors objective without a table names the way to get one
    r = run(app, ["pretrain", str(plain), str(tmp_path / "bad"), "--objective",
                  "vectors", "--steps", "1"])
    assert r.exit_code != 0 and "init vectors" in r.output
    assert len(calls) == n + 1 and not (tmp_path / "bad").exists()


def test_objective_is_registered_and_checked_by_debug_config(tmp_path):
    from spacy_ray_amd.config.registry import resolve_registry_ref

    make = resolve_registry_ref("architectures", "spacy.PretrainVectors.v1")
    assert make() == {"objective": "vectors", "loss": "cosine",
                      "hidden_size": 300, "maxout_pieces": 3}
    with pytest.raises(ValueError, match="loss"):
        make(loss="manhattan")
    text = VEC_CFG % {"static": "false"} + OBJECTIVE_BLOCK
    with pytest.raises(ValueError,
                       match=r"vectors objective without \[initialize\] vectors"):
        check_static_vectors_config(Config.from_str(text).interpolate())
    cfg = Config.from_str(text, overrides={"paths.vectors": str(_vec_dir(tmp_path))})
    lines = check_static_vectors_config(cfg.interpolate())
    assert any("vectors objective" in line and "L2" in line for line in lines)
    assert init_nlp(cfg, device="cpu", sample_size=8).vocab.vectors is not None
