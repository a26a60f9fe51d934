"""span_pool kernels against a float64 loop; the reducer head end to end."""
import functools

import numpy as np
import pytest
import torch

from spacy_ray_amd.ops import api as ops
from tests.test_span_pool import reference

pytestmark = pytest.mark.gpu

T = 300
U = 2.0 ** -24
CASES = [(torch.bfloat16, 64), (torch.bfloat16, 96), (torch.bfloat16, 128),
         (torch.bfloat16, 768), (torch.float32, 96)]
SIZES = [1, 63, 64, 65, 257]


def make_spans(S, seed=0):
    """[0,1), [T-1,T), [0,255), one empty span and one exact duplicate as far
    as S allows, then lengths from {0,1,2,3,9,255} with starts in [0, 250);
    tokens 259..298 stay uncovered."""
    rng = np.random.RandomState(seed)
    spans = [(0, 1), (T - 1, T), (0, 255), (7, 7), (0, 255)][:S]
    while len(spans) < S:
        L = int(rng.choice([0, 1, 2, 3, 9, 255]))
        a = int(rng.randint(0, 250))
        if L == 255:
            a = min(a, 4)
        elif a + L > 259:
            a = 259 - L
        spans.append((a, a + L))
    return [s for s, _ in spans], [e for _, e in spans]


def make_x(dtype, W, ties):
    g = torch.Generator().manual_seed(1)
    X = torch.randint(-4, 5, (T, W), generator=g) / 4 if ties else torch.randn(T, W, generator=g)
    return X.to(dtype)


@functools.lru_cache(maxsize=2)  # the float64 loop is the slow part
def case(dtype, W, S, ties):
    starts, ends = make_spans(S)
    X = make_x(dtype, W, ties)
    dR = torch.randn((S + 63) // 64 * 64, 4 * W,
                     generator=torch.Generator().manual_seed(2)).to(dtype)
    return starts, ends, X, dR, reference(X, starts, ends, dR[:S])


def run(X, dR, index):
    x = X.cuda().requires_grad_(True)
    R = ops.span_pool(x, index, pad_rows=64)
    R.backward(dR.cuda()[:R.shape[0]])
    return R.detach().cpu(), x.grad.cpu()


def check(dtype, X, starts, ends, R, dX, ref):
    R64, which64, dX64, mag, n = ref
    S, W = len(starts), X.shape[1]
    rel = 2.0 ** -8 if dtype == torch.bfloat16 else 0.0
    last, first, mean, mx = R[:S].double().split(W, dim=1)
    assert torch.equal(last, R64[:, :W]) and torch.equal(first, R64[:, W:2 * W])
    assert torch.equal(mx, R64[:, 3 * W:])
    L = (torch.tensor(ends) - torch.tensor(starts)).double()[:, None]
    absmean = torch.stack([X[a:e].double().abs().sum(0) / max(e - a, 1)
                           for a, e in zip(starts, ends)])
    err = (mean - R64[:, 2 * W:3 * W]).abs()
    bound = 2 * (L + 2) * U * absmean + rel * R64[:, 2 * W:3 * W].abs()
    print("mean err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    assert not R[S:].any()
    if S >= 5:
        assert torch.equal(R[4], R[2])
    err = (dX.double() - dX64).abs()
    bound = 2 * (n + 1) * U * mag + rel * dX64.abs()
    print("dX err / bound", float((err / bound.clamp(min=1e-300)).max()))
    assert (err <= bound).all()
    assert not dX[259:299].any()


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "randn"])
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("dtype,W", CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_span_pool_matches_float64_loop(dtype, W, S, ties, monkeypatch):
    monkeypatch.delenv("SRX_SPAN_POOL", raising=False)
    starts, ends, X, dR, ref = case(dtype, W, S, ties)
    index = ops.span_index(starts, ends, T, "cuda")
    assert ops.span_pool_available(X.cuda(), index)
    x = X.cuda()
    _, which = ops.hip_ext().span_pool_fwd(x, index.starts, index.ends, S)
    assert torch.equal(which.cpu().long(), ref[1])
    R, dX = run(X, dR, index)
    assert R.shape == ((S + 63) // 64 * 64, 4 * W)
    check(dtype, X, starts, ends, R, dX, ref)
    R2, dX2 = run(X, dR, index)
    assert torch.equal(R, R2) and torch.equal(dX, dX2)


@pytest.mark.parametrize("how", ["env", "max_len"])
def test_composed_dispatch(how, monkeypatch):
    dtype, W, S = torch.bfloat16, 96, 65
    starts, ends, X, dR, ref = case(dtype, W, S, False)
    if how == "env":
        monkeypatch.setenv("SRX_SPAN_POOL", "composed")
    else:
        monkeypatch.delenv("SRX_SPAN_POOL", raising=False)
        starts, ends = starts + [0], ends + [256]
        ref = reference(X, starts, ends, dR[:S + 1])
        S += 1
    index = ops.span_index(starts, ends, T, "cuda")
    assert (how == "env") == ops.span_pool_available(X.cuda(), index)
    x = X.cuda().requires_grad_(True)
    R = ops.span_pool(x, index, pad_rows=64)
    assert R.grad_fn is not None and type(R.grad_fn).__name__ != "_SpanPoolBackward"
    R.backward(dR.cuda())
    check(dtype, X, starts, ends, R.detach().cpu(), x.grad.cpu(), ref)


def test_bad_env_raises(monkeypatch):
    monkeypatch.setenv("SRX_SPAN_POOL", "hip")
    index = ops.span_index([0], [1], T, "cuda")
    with pytest.raises(ValueError):
        ops.span_pool(torch.zeros(T, 96, device="cuda"), index)


def test_reducer_head_end_to_end(monkeypatch):
    """Fused route (span_pool + mixer_layer) and composed route on the same
    weights against a float64 evaluation of the head; ratio rule: kernel
    error <= 2 x composed-bf16 error + one bf16 ulp at max|ref|."""
    from spacy_ray_amd.pipeline.pipes import SpancatReducerHead

    monkeypatch.delenv("SRX_MIXER", raising=False)
    W, S = 96, 257
    starts, ends = make_spans(S)
    X = make_x(torch.bfloat16, W, False)
    torch.manual_seed(5)
    head = SpancatReducerHead(W, W, 3)
    head64 = SpancatReducerHead(W, W, 3).double()
    head = head.to(torch.bfloat16)
    head64.load_state_dict({k: v.double() for k, v in head.state_dict().items()})
    index = ops.span_index(starts, ends, T, "cuda")
    head = head.cuda()
    with torch.no_grad():
        ref = head64(X.double(), ops.span_index(starts, ends, T, "cpu"))
        monkeypatch.setenv("SRX_SPAN_POOL", "fused")
        fused = head(X.cuda(), index).double().cpu()
        monkeypatch.setenv("SRX_SPAN_POOL", "composed")
        monkeypatch.setenv("SRX_MIXER", "composed")
        composed = head(X.cuda(), index).double().cpu()
    monkeypatch.delenv("SRX_MIXER")
    monkeypatch.setenv("SRX_SPAN_POOL", "fused")
    e_fused = float((fused - ref).abs().max())
    e_comp = float((composed - ref).abs().max())
    ulp = float(ref.abs().max()) * 2.0 ** -8
    print("fused", e_fused, "composed", e_comp, "ulp", ulp)
    assert e_fused <= 2 * e_comp + ulp

    target = (torch.arange(S)[:, None] % 3 == torch.arange(3)[None, :]).float().cuda()
    opt = torch.optim.Adam(head.parameters(), lr=0.01)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            head(X.cuda(), index).float(), target)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
