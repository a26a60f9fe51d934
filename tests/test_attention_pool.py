"""attention_pool on the CPU: the composed path against a float64 per-doc
loop, and the TextCatEnsemble / TextCatParametricAttention pipes.

The error bound (shared with tests/test_gpu_attention_pool.py).  u = 2^-24;
every output is compared as |err| <= k u M + r |ref|, M the float64
expression with absolute values, r = 2^-8 for a bf16 output and 0 for fp32.

* logits: s_t = k_t . q is a W-term fp32 dot, and the exponent s_t - m is
  rounded again each time the running maximum moves, |s - m| <= 2 S with S =
  max_t sum_i |k_ti q_i| over the doc: |ds| <= (W + 6) u S.  Moving every
  logit of a doc by that much moves a_t by the factor exp(+-2 ds): the logit
  error enters a_t twice.
* chain(n): the fp32 roundings between one exp(s_t - m) x_t and P_d: n for
  the n-term sum, 3 (an exp, a product) for each of the at most CH / 2 trips
  that rescale the accumulator, 4 for each of the 6 row-group merges, 3 per
  chunk merge, 4 for the exp, the product, the division and the log.  The
  denominator has the same chain, so
      k_P = 2 chain(n) + 2 (W + 6) S          M_P = sum_t a_t |x_t|.
* backward: a_t = exp(s_t - lse) has P's relative error; g_t = x_t . dP and
  c = P32 . dP are W-term dots over G_t = |x_t| . |dP| and Cm = sum_t a_t G_t
  (c also carries P32's error, relative to Cm); ds_t = a_t (g_t - c) so
      |d ds_t| <= (W + 5 + 2 k_P) u a_t (G_t + Cm) = k_b u M_ds,
  and dX_t = a_t dP + ds_t q, dK_t = ds_t q take k_b with M = a_t |dP| +
  M_ds |q|.  dq = sum over all T rows of ds_t k_t: k = max k_b + T, M = sum_t
  M_ds |k_t|.
"""
import functools
import math

import numpy as np
import pytest
import torch

from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.ops import torch_ref as ref

U = 2.0 ** -24
CH = ops.ATTENTION_POOL_CHUNK
BF, F32 = torch.bfloat16, torch.float32
WIDTHS = [8, 96, 128, 520, 768]
# lengths 0, 1, 2 and 64 / SW - 1 .. 64 / SW + 1 rows for every sub-wave (0 ..
# 9), the chunk edges, then fillers; docs 14 and 15 are rewritten by case()
EDGES = list(range(10)) + [CH - 1, CH, CH + 1, 2 * CH + 3, 20, 40]
LENGTHS = {1: [2 * CH + 3], 3: [0, CH + 1, 5],
           70: EDGES + [int(n) for n in np.random.RandomState(0).randint(0, 12, 54)]}


def reference(X, lengths, q, K, dP):
    """float64 loop -> {name: (value, k u M)} for P, dX, dK, dq."""
    W = X.shape[1]
    x, qq, dp = X.double().numpy(), q.double().numpy(), dP.double().numpy()
    k = x if K is None else K.double().numpy()
    P, bP = np.zeros((len(lengths), W)), np.zeros((len(lengths), W))
    dX, bX, dK, bK = (np.zeros_like(x) for _ in range(4))
    dq, mq, kmax, t0 = np.zeros(W), np.zeros(W), 0.0, 0
    for d, n in enumerate(lengths):
        if n == 0:
            continue
        xs, ks = x[t0:t0 + n], k[t0:t0 + n]
        s = ks @ qq
        S = (np.abs(ks) * np.abs(qq)).sum(1).max()
        a = np.exp(s - s.max())
        a /= a.sum()
        chain = n + 3 * (CH // 2) + 4 * 6 + 3 * math.ceil(n / CH) + 4
        kP = 2 * chain + 2 * (W + 6) * S
        P[d], bP[d] = a @ xs, kP * U * (a @ np.abs(xs))
        g, G = xs @ dp[d], np.abs(xs) @ np.abs(dp[d])
        ds, mds = a * (g - a @ g), a * (G + a @ G)
        kb = W + 5 + 2 * kP
        da, ma = a[:, None] * dp[d], a[:, None] * np.abs(dp[d])
        dsq, mdsq = ds[:, None] * qq, mds[:, None] * np.abs(qq)
        if K is None:
            dX[t0:t0 + n], bX[t0:t0 + n] = da + dsq, kb * U * (ma + mdsq)
        else:
            dX[t0:t0 + n], bX[t0:t0 + n] = da, kb * U * ma
            dK[t0:t0 + n], bK[t0:t0 + n] = dsq, kb * U * mdsq
        dq += ds @ ks
        mq += mds @ np.abs(ks)
        kmax, t0 = max(kmax, kb), t0 + n
    out = {"P": (P, bP), "dX": (dX, bX), "dq": (dq, (kmax + len(x)) * U * mq)}
    if K is not None:
        out["dK"] = (dK, bK)
    return {n: (torch.from_numpy(v), torch.from_numpy(b)) for n, (v, b) in out.items()}


@functools.lru_cache(maxsize=None)  # the float64 reference is the slow part
def case(dtype, W, D, keys):
    """Random rows with logits of order 1; in the D = 70 list doc 14 is one
    row repeated and doc 15's logits rise by about 80 from its first to its
    last row, so that every trip rescales the accumulator."""
    g = torch.Generator().manual_seed(W + D)
    lengths = LENGTHS[D]
    T = sum(lengths)
    X = torch.randn(T, W, generator=g)
    K = torch.randn(T, W, generator=g) if keys else None
    q = torch.randn(W, generator=g) / math.sqrt(W)
    if D == 70:
        a, b = sum(lengths[:14]), sum(lengths[:15])
        X[a:b] = X[a]
        if keys:
            K[a:b] = K[a]
        ramp = torch.linspace(0, 80, lengths[15])[:, None] * (q / (q @ q))
        (K if keys else X)[b:b + lengths[15]] += ramp
    X = X.to(dtype)
    K = None if K is None else K.to(dtype)
    dP = torch.randn(len(lengths), W, generator=g).to(dtype)
    offsets = torch.tensor(np.cumsum([0] + lengths), dtype=torch.int32)
    return X, offsets, q, K, dP, reference(X, lengths, q, K, dP)


def run(X, offsets, q, K, dP, device="cpu", **kw):
    ins = [t.clone().to(device).requires_grad_(True) for t in (X, q) + (() if K is None else (K,))]
    P = ops.attention_pool(ins[0], offsets.to(device), ins[1],
                           ins[2] if K is not None else None, **kw)
    P.backward(dP.to(device))
    out = {"P": P, "dX": ins[0].grad, "dq": ins[1].grad}
    if K is not None:
        out["dK"] = ins[2].grad
    return {n: t.detach().cpu() for n, t in out.items()}


def check(got, want, dtype):
    for name, (value, bound) in want.items():
        out = got[name]
        assert out.dtype == (F32 if name == "dq" else dtype) and out.shape == value.shape
        rel = 2.0 ** -8 if out.dtype == BF else 0.0
        err, bound = (out.double() - value).abs(), bound + rel * value.abs()
        print(name, "err / bound", float((err / bound.clamp(min=1e-300)).max()))
        assert (err <= bound).all(), name


@pytest.mark.parametrize("keys", [False, True])
def test_composed_path_matches_float64_loop(keys):
    X, offsets, q, K, dP, want = case(F32, 8, 70, keys)
    got = run(X.double(), offsets, q.double(), None if K is None else K.double(),
              dP.double())
    for name, (value, _) in want.items():
        assert torch.allclose(got[name], value, rtol=0, atol=1e-11), name
    assert not got["P"][0].any()  # an empty doc: a zero row


@pytest.mark.parametrize("D", [1, 3, 70])
@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("keys", [False, True])
def test_fp32_composed_path_is_inside_the_bound(keys, W, D):
    """The condition on the GPU test's inputs: plain fp32 already passes."""
    X, offsets, q, K, dP, want = case(F32, W, D, keys)
    check(run(X, offsets, q, K, dP), want, F32)


def test_zero_query_is_the_mean_and_pad_rows_are_zero():
    X, offsets, q, _, dP, _ = case(F32, 96, 70, False)
    mean, bound = reference(X, LENGTHS[70], 0 * q, None, dP)["P"]
    P = ops.attention_pool(X, offsets, 0 * q, pad_rows=64)
    assert P.shape == (128, 96) and not P[70:].any()
    lengths = (offsets[1:] - offsets[:-1]).long()
    for got in (P[:70], ops.reduce_mean_ragged(X, lengths)):
        assert ((got.double() - mean).abs() <= bound).all()


CFG = """
[nlp]
lang = "en"
pipeline = ["tok2vec", "%(factory)s"]

[components]

[components.tok2vec]
factory = "tok2vec"

[components.tok2vec.model]
@architectures = "spacy.HashEmbedCNN.v2"
width = 32
depth = 1
embed_size = 200

[components.%(factory)s]
factory = "%(factory)s"

[components.%(factory)s.model]
%(model)s

[components.%(factory)s.model.tok2vec]
@architectures = "spacy.Tok2VecListener.v1"
width = 32
%(linear)s
[corpora]

[corpora.train]
@readers = "spacy-mi.SyntheticCorpus.v1"
n_docs = 48
words_per_doc = 14
vocab_size = 120
n_tags = 10
seed = 5

[training]
seed = 0
train_corpus = "corpora.train"
"""
BOW = """
[components.%(factory)s.model.linear_model]
@architectures = "%(arch)s"
exclusive_classes = true
ngram_size = 2
no_output_layer = false
"""
ENSEMBLE = CFG % {"factory": "textcat", "model": '@architectures = "spacy.TextCatEnsemble.v2"',
                  "linear": BOW % {"factory": "textcat", "arch": "spacy.TextCatBOW.v2"}}
PARAMETRIC = CFG % {"factory": "textcat_multilabel", "linear": "", "model":
                    '@architectures = "spacy.TextCatParametricAttention.v1"\n'
                    "exclusive_classes = false"}


@pytest.mark.parametrize("cfg,head", [(ENSEMBLE, "TextcatEnsembleHead"),
                                      (PARAMETRIC, "TextcatAttentionHead")],
                         ids=["ensemble", "parametric_attention"])
def test_pipe_trains_and_round_trips(cfg, head, tmp_path):
    import spacy_ray_amd
    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.vocab.doc import Example

    torch.manual_seed(0)
    nlp = init_nlp(Config.from_str(cfg), device="cpu", sample_size=48)
    pipe = nlp.pipeline[-1][1]
    assert type(pipe.module).__name__ == head and pipe.listens_to == "tok2vec"
    assert not pipe.module.attend.Q.any()  # attention starts uniform
    docs = make_synthetic_docs(nlp.vocab, n_docs=48, words_per_doc=14, vocab_size=120,
                               n_tags=10, n_deps=10, n_ent_types=3, seed=5)
    examples = [Example.from_doc(d) for d in docs]
    opt = resolve({"o": {"@optimizers": "Adam.v1", "learn_rate": 0.01}}, validate=False)["o"]
    engine = ZeRO1Engine(nlp, opt, LocalComm())
    seen = []
    for _ in range(12):
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        engine.apply_step()
        seen.append(float(losses[pipe.name]))
    assert seen[-1] < seen[0] and pipe.module.attend.Q.any()

    nlp.to_disk(str(tmp_path))
    nlp2 = spacy_ray_amd.load(str(tmp_path), device="cpu")
    outs1 = nlp.predict_docs([d.copy_unannotated() for d in docs[:8]])
    outs2 = nlp2.predict_docs([d.copy_unannotated() for d in docs[:8]])
    assert [o.cats for o in outs1] == [o.cats for o in outs2]


def test_linear_model_must_be_bow_and_bow_cfg_is_unchanged():
    from spacy_ray_amd.config.config import Config
    from spacy_ray_amd.pipeline.language import build_nlp, init_nlp
    from tests.test_sparse_linear import BOW_CFG

    bad = ENSEMBLE.replace("spacy.TextCatBOW.v2", "spacy.TextCatCNN.v2").replace(
        "ngram_size = 2\nno_output_layer = false\n",
        '\n[components.textcat.model.linear_model.tok2vec]\n'
        '@architectures = "spacy.Tok2VecListener.v1"\nwidth = 32\n')
    with pytest.raises(ValueError, match="linear_model"):
        build_nlp(Config.from_str(bad))
    v3 = build_nlp(Config.from_str(ENSEMBLE.replace(
        "TextCatBOW.v2", "TextCatBOW.v3").replace("false", "true")))
    assert v3.pipeline[-1][1].attention == {
        "keys": False, "bow": {"ngram_size": 2, "length": 262144},
        "no_output_layer": True}
    bow = init_nlp(Config.from_str(BOW_CFG), device="cpu", sample_size=8).pipeline[0][1]
    assert sorted(bow.cfg) == ["exclusive", "labels", "length", "ngram_size"]
