"""Span pooling on the CPU: torch_ref, ops.span_index, ops.span_pool and the
spancat pipe with and without a `reducer` block."""
import os

import pytest
import torch

from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.ops import torch_ref


def reference(X, starts, ends, dR):
    """float64 forward (R, which) and backward (dX, sum|term|, n terms) of
    the definitions (last | first | mean | max, first-occurrence argmax, zero
    row for an empty span), by a loop over the spans of CPU tensors."""
    X, dR = X.double(), dR.double()
    S, W = len(starts), X.shape[1]
    R = torch.zeros(S, 4 * W, dtype=torch.float64)
    which = torch.zeros(S, W, dtype=torch.int64)
    dX, mag, n = (torch.zeros_like(X) for _ in range(3))
    cols = torch.arange(W)

    def add(t, term):
        dX[t] += term
        mag[t] += term.abs()
        n[t] += 1

    for s, (a, e) in enumerate(zip(starts, ends)):
        if e <= a:
            continue
        mx, wh = X[a].clone(), torch.zeros(W, dtype=torch.int64)
        for t in range(a + 1, e):
            gt = X[t] > mx
            mx, wh = torch.where(gt, X[t], mx), torch.where(gt, t - a, wh)
        R[s] = torch.cat([X[e - 1], X[a], X[a:e].sum(0) / (e - a), mx])
        which[s] = wh
        dlast, dfirst, dmean, dmax = dR[s].split(W)
        for t in range(a, e):
            add(t, dmean / (e - a))
        add(e - 1, dlast)
        add(a, dfirst)
        dX[a + wh, cols] += dmax
        mag[a + wh, cols] += dmax.abs()
        n[a + wh, cols] += 1
    return R, which, dX, mag, n


SPANS = [(0, 1), (0, 5), (3, 3), (2, 9), (2, 9), (11, 12), (0, 12), (7, 10)]


@pytest.mark.parametrize("ties", [False, True])
def test_torch_ref_matches_loop(ties):
    g = torch.Generator().manual_seed(3)
    X = torch.randn(12, 8, generator=g)
    if ties:
        X = torch.randint(-4, 5, (12, 8), generator=g).float() / 4
    starts, ends = (torch.tensor(v) for v in zip(*SPANS))
    R, which = torch_ref.span_pool(X, starts, ends)
    R64, which64 = reference(X, starts.tolist(), ends.tolist(),
                             torch.zeros(len(SPANS), 32))[:2]
    W = X.shape[1]
    # copies are exact; an fp32 mean of L <= 12 terms: (L + 2) u max|x|
    assert torch.equal(R[:, :2 * W].double(), R64[:, :2 * W])
    assert torch.equal(R[:, 3 * W:].double(), R64[:, 3 * W:])
    assert torch.equal(which.long(), which64)
    assert (R[:, 2 * W:3 * W].double() - R64[:, 2 * W:3 * W]).abs().max() <= 14 * 2.0 ** -24 * X.abs().max()
    assert not R[2].any() and not which[2].any()


def test_span_pool_gradcheck():
    g = torch.Generator().manual_seed(4)
    X = torch.randn(12, 4, dtype=torch.float64, generator=g, requires_grad=True)
    starts, ends = zip(*SPANS)
    index = ops.span_index(starts, ends, 12, "cpu")
    assert index.max_len == 12 and index.n_spans == len(SPANS)
    assert index.tok_offsets.tolist()[:4] == [0, 3, 5, 9]
    assert index.tok_spans.tolist()[:5] == [0, 1, 6, 1, 6]
    assert ops.span_pool(X, index, pad_rows=64).shape == (64, 16)
    assert torch.autograd.gradcheck(lambda x: ops.span_pool(x, index, 3), (X,))


@pytest.mark.parametrize("starts,ends", [([3], [2]), ([0], [13]), ([-1], [2])])
def test_span_index_rejects(starts, ends):
    with pytest.raises(ValueError):
        ops.span_index(starts, ends, 12, "cpu")


CFG_PATH = os.path.join(os.path.dirname(__file__), "..", "examples", "configs",
                        "en_spancat.cfg")
REDUCER_BLOCKS = """[components.spancat.model.reducer]
@layers = "spacy.mean_max_reducer.v1"
hidden_size = 96

[components.spancat.model.scorer]
@layers = "spacy.LinearLogistic.v1"
"""


def spancat_cfg(reducer: bool):
    from spacy_ray_amd.config.config import Config

    with open(CFG_PATH) as f:
        text = f.read()
    assert REDUCER_BLOCKS in text
    return Config.from_str(text if reducer else text.replace(REDUCER_BLOCKS, ""))


def test_spancat_without_reducer_keeps_old_head():
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.pipeline.pipes import SpancatHead

    nlp = init_nlp(spancat_cfg(False), device="cpu", sample_size=8)
    pipe = nlp.get_pipe("spancat")
    assert type(pipe.module) is SpancatHead
    assert "hidden_size" not in pipe.cfg
    assert sorted(pipe.module.state_dict()) == ["output.bias", "output.weight"]


def test_spancat_reducer_trains_and_roundtrips(tmp_path):
    import spacy_ray_amd
    from spacy_ray_amd.config.config import resolve
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.pipeline.pipes import SpancatReducerHead
    from spacy_ray_amd.vocab.doc import Example

    torch.manual_seed(0)
    nlp = init_nlp(spancat_cfg(True), device="cpu", sample_size=8)
    docs = make_synthetic_docs(nlp.vocab, n_docs=64, words_per_doc=10,
                               vocab_size=60, n_tags=6, n_deps=5,
                               n_ent_types=2, seed=7)
    # the synthetic spans of test_pipeline.test_spancat_trains_and_predicts
    for d in docs:
        ids = [int(w[1:]) for w in d.words]
        d.spans["sc"] = (
            [(i, i + 1, "LONE") for i, wid in enumerate(ids) if wid % 10 == 0]
            + [(i, i + 2, "PAIR") for i, wid in enumerate(ids[:-1]) if wid % 2 == 0])
    pipe = nlp.get_pipe("spancat")
    pipe.labels = []
    pipe.module = None
    examples = [Example.from_doc(d) for d in docs]
    pipe.initialize(examples, "cpu")
    assert type(pipe.module) is SpancatReducerHead and pipe.cfg["hidden_size"] == 96
    opt = {"@optimizers": "Adam.v1", "learn_rate": 0.02}
    engine = ZeRO1Engine(nlp, resolve({"o": opt}, validate=False)["o"], LocalComm())
    seen = []
    for _ in range(40):
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        engine.apply_step()
        seen.append(losses["spancat"])
    assert seen[-1] < seen[0], (seen[0], seen[-1])
    outs1 = nlp.predict_docs([d.copy_unannotated() for d in docs[:8]])
    nlp.to_disk(str(tmp_path))
    nlp2 = spacy_ray_amd.load(str(tmp_path), device="cpu")
    assert type(nlp2.get_pipe("spancat").module) is SpancatReducerHead
    outs2 = nlp2.predict_docs([d.copy_unannotated() for d in docs[:8]])
    assert [d.spans for d in outs2] == [d.spans for d in outs1]
