"""vectors_most_similar (srx_vecsim.hip.h) against float64, its dispatch
through ops.vectors_most_similar, and Vectors.most_similar /
Vocab.prune_vectors on the GPU.

Inputs are built on the CPU from a seeded generator as randn * 0.5 rounded to
bf16; the float64 reference (normalise, matmul, sort by (-score, row)) is
computed from exactly those values.

The bound is derived, not tuned.  u = 2^-24, e = nM u.  Products of two bf16
values are exact in fp32, so q.t is an fp32 sum of nM exact terms: absolute
error e |q| |t| in any order (Cauchy-Schwarz); |q|^2 and |t|^2 are relative
e.  First order, with c = q.t / (|q| |t|), |c| <= 1:

  inv(x) = 1 / sqrt(ss)     relative e / 2 + 2u  (a square root, a division)
  s = dot * inv(t)          absolute (e + e / 2 + 3u) |q|
  score = s * inv(q)        absolute 2e + 6u;  the clip adds nothing

which is no more than the 2e + 10u of the cosine in test_gpu_vectors_loss.py
(same sums, fewer roundings), so the same form is used, doubled for the
second-order terms:  B = 2 (2 nM + 10) u."""
import numpy as np
import pytest
import torch

from spacy_ray_amd.ops import api as ops
from spacy_ray_amd.vocab.doc import Vocab
from spacy_ray_amd.vocab.vectors import Vectors

pytestmark = pytest.mark.gpu

NMS = (32, 50, 96, 300)
SHAPES = ((1, 1), (31, 127), (33, 129), (257, 321))  # (V, nQ)
NS = (1, 3, 8)
SPLITS = (0, 1, 2, 5, 1000)
U = 2.0 ** -24

_CASES = {}


def _vs():
    assert ops.hip_vecsim_ext() is not None
    return ops.hip_vecsim_ext()


def _pad(x):
    out = torch.zeros(x.shape[0], -(-x.shape[1] // 32) * 32, dtype=torch.bfloat16)
    out[:, :x.shape[1]] = x
    return out.cuda()


def _ref64(q, t):
    """float64 (scores, rows), every table row, best first, ties by row."""
    unit = lambda x: x.double() / x.double().norm(dim=1, keepdim=True).clamp(min=1e-300)
    sims = (unit(q) @ unit(t).t()).clamp(-1, 1)
    s, r = (-sims).sort(dim=1, stable=True)  # ascending -score, stable: low row first
    return -s, r


def _case(nM, V, nQ):
    """(queries, table: bf16 on the CPU; their padded GPU copies; float64
    sorted scores and rows).  Built once, never modified."""
    if (nM, V, nQ) not in _CASES:
        gen = torch.Generator().manual_seed(9000 + 1000 * nM + 10 * V + nQ)
        t = (torch.randn(V, nM, generator=gen) * 0.5).to(torch.bfloat16)
        q = (torch.randn(nQ, nM, generator=gen) * 0.5).to(torch.bfloat16)
        _CASES[(nM, V, nQ)] = (q, t, _pad(q), _pad(t)) + _ref64(q, t)
    return _CASES[(nM, V, nQ)]


def _check(rows, scores, q, t, want_s, want_r, n, B):
    V = t.shape[0]
    rows, scores = rows.cpu().long(), scores.cpu().double()
    assert rows.shape == scores.shape == (q.shape[0], n)
    assert ((rows >= 0) & (rows < V)).all()
    assert (rows.sort(dim=1).values.diff(dim=1) != 0).all(), "rows repeat"
    assert (scores.diff(dim=1) <= 0).all(), "scores increase"
    full = torch.empty_like(want_s).scatter_(1, want_r, want_s)  # by row
    err_row = (scores - full.gather(1, rows)).abs().max().item()
    err_rank = (scores - want_s[:, :n]).abs().max().item()
    # exact index wherever float64 separates the rank from both neighbours
    inf = torch.full((q.shape[0], 1), float("inf"), dtype=torch.float64)
    gaps = torch.cat([inf, -want_s.diff(dim=1), inf], dim=1)
    clear = (gaps[:, :n] > 2 * B) & (gaps[:, 1:n + 1] > 2 * B)
    exempt = 1.0 - clear.double().mean().item()
    print(f"most_similar nM={q.shape[1]} V={V} nQ={q.shape[0]} n={n}: score err "
          f"{err_row:.3e} / rank err {err_rank:.3e} (B {B:.3e}), exempt {exempt:.4f}")
    assert err_row <= B and err_rank <= B
    assert exempt <= 0.10
    assert (rows == want_r[:, :n])[clear].all()


@pytest.mark.parametrize("nM,V,nQ,n", [(nM, V, nQ, n) for nM in NMS
                                        for V, nQ in SHAPES for n in NS if n <= V])
def test_kernel_against_float64(nM, V, nQ, n):
    q, t, qd, td, want_s, want_r = _case(nM, V, nQ)
    B = 2 * (2 * nM + 10) * U
    first = None
    for splits in SPLITS if V == 257 else (0,):
        rows, scores = _vs().vectors_most_similar(qd, td, n, splits)
        _check(rows, scores, q, t, want_s, want_r, n, B)
        if first is None:
            first = (rows, scores)
        # bit-identical whatever the split
        assert torch.equal(rows, first[0])
        assert torch.equal(scores.view(torch.int32), first[1].view(torch.int32))


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("n", (1, 8))
def test_exact_cases(n, splits):
    """Row 200 duplicates row 10 (different 64-row tiles, so different splits
    at splits = 5), row 70 is all zero, query 0 equals row 10, query 1 is all
    zero, query 2 is arbitrary."""
    nM, V = 50, 257
    gen = torch.Generator().manual_seed(77)
    t = (torch.randn(V, nM, generator=gen) * 0.5).to(torch.bfloat16)
    t[200] = t[10]
    t[70] = 0
    q = (torch.randn(3, nM, generator=gen) * 0.5).to(torch.bfloat16)
    q[0] = t[10]
    q[1] = 0
    qd, td = _pad(q), _pad(t)
    rows, scores = _vs().vectors_most_similar(qd, td, n, splits)
    again = _vs().vectors_most_similar(qd, td, n, splits)
    base = _vs().vectors_most_similar(qd, td, n, 1)
    for other in (again, base):
        assert torch.equal(rows, other[0])
        assert torch.equal(scores.view(torch.int32), other[1].view(torch.int32))
    rows, scores = rows.cpu(), scores.cpu()
    assert rows[0, 0] == 10
    assert rows[1].tolist() == list(range(n))
    assert (scores[1] == 0).all()
    if n == 8:
        assert rows[0, 1] == 200 and scores[0, 0] == scores[0, 1]
        # the zero row scores exactly 0, between the positive and the negative:
        # all 8 rows of a table slice that holds it, for the arbitrary query
        r8, s8 = _vs().vectors_most_similar(qd[2:3], td[66:74].contiguous(), 8, splits)
        r8, s8 = r8.cpu()[0], s8.cpu()[0]
        at = int((r8 == 70 - 66).nonzero())
        assert s8[at] == 0 and (s8[:at] > 0).all() and (s8[at + 1:] < 0).all()
        assert 0 < at < 7, "the slice must hold both signs"


def test_dispatch_and_guards(monkeypatch):
    nM, V, nQ = 50, 257, 129
    q, t, qd, td, want_s, want_r = _case(nM, V, nQ)
    B = 2 * (2 * nM + 10) * U
    clear = (want_s[:, 0] - want_s[:, 1]) > 4 * B + 2 ** -7  # bf16 composed path
    assert clear.sum() > nQ // 2
    assert ops.vectors_most_similar_available(qd, td, 3)
    calls = []
    real = _vs().vectors_most_similar
    monkeypatch.setattr(_vs(), "vectors_most_similar",
                        lambda *a: calls.append(1) or real(*a))
    for mode, fused in (("fused", True), ("composed", False),
                        ("", ops.VECTORS_MOST_SIMILAR_FUSED_DEFAULT)):
        monkeypatch.setenv("SRX_MOST_SIMILAR", mode)
        del calls[:]
        rows, _ = ops.vectors_most_similar(qd, td, 1)
        assert bool(calls) == fused
        assert (rows.cpu()[:, 0] == want_r[:, 0])[clear].all()
    monkeypatch.setenv("SRX_MOST_SIMILAR", "bogus")
    with pytest.raises(ValueError, match="SRX_MOST_SIMILAR"):
        ops.vectors_most_similar(qd, td, 1)
    monkeypatch.undo()

    rows, scores = _vs().vectors_most_similar(qd[:0], td, 3, 0)
    assert rows.shape == scores.shape == (0, 3)
    assert rows.dtype == torch.int32 and scores.dtype == torch.float32
    bad = [
        (qd.float(), td, 1, 0),                    # dtype
        (qd, td.float(), 1, 0),
        (qd[:, :32], td, 1, 0),                    # layout: strided, width
        (qd[:, :32].contiguous(), td, 1, 0),
        (qd.cpu(), td, 1, 0),
        (_pad(q)[:, :48].contiguous(), _pad(t)[:, :48].contiguous(), 1, 0),  # % 32
        (torch.zeros(2, 352, dtype=torch.bfloat16).cuda(),
         torch.ones(9, 352, dtype=torch.bfloat16).cuda(), 1, 0),             # > 320
        (qd, td, 0, 0), (qd, td, 9, 0), (qd, td[:2].contiguous(), 3, 0),     # n
        (qd, td[:0], 1, 0),                        # V >= 1
        (qd, td, 1, -1),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            _vs().vectors_most_similar(*args)
    assert not ops.vectors_most_similar_available(qd, td, 9)
    rows, _ = ops.vectors_most_similar(qd, td, 9)  # composed: n > 8
    assert rows.shape == (nQ, 9)


def test_vectors_and_vocab_prune_on_gpu():
    """12 kept rows; dropped row 12 + i is kept row (5 i) % 12 plus a small
    perturbation, so its neighbour is known."""
    rng = np.random.default_rng(5)
    kept = rng.standard_normal((12, 50)).astype(np.float32)
    src = (5 * np.arange(30)) % 12
    data = np.concatenate([kept, kept[src] + 0.05 * rng.standard_normal(
        (30, 50)).astype(np.float32)])
    words = [f"w{i}" for i in range(42)]
    vocab = Vocab()
    vocab.strings.add_batch(words)
    vocab.vectors = Vectors.from_words(words, data)
    kept_only = Vectors.from_words(words[:12], data[:12])
    keys, rows, scores = kept_only.most_similar(data[12:], n=2, device="cuda")
    assert (rows[:, 0] == src).all() and (scores[:, 0] > 0.9).all()
    assert (kept_only.find_rows(keys[:, 0]) == src).all()
    assert scores.dtype == np.float32 and rows.dtype == np.int32
    remap = vocab.prune_vectors(12)
    assert vocab.vectors.shape == (12, 50) and len(vocab.vectors.keys) == 42
    assert (vocab.vectors.find_words(words) ==
            np.concatenate([np.arange(12), src])).all()
    assert set(remap) == set(words[12:])
    for i in range(30):
        syn, score = remap[words[12 + i]]
        assert syn == words[src[i]] and abs(score - scores[i, 0]) < 1e-6
