"""dpre_gather (srx_embed_parser.hip.h): the atomic-free dPre of the parser /
NER backward on doc-major arenas.

dSummed holds integers in [-8, 8] with the maxout zero pattern, so every fp32
sum of up to 256 rows is exact and the expected dPre is exactly index_add_ in
float64 cast once to the output dtype: the checks are bit equality, with no
tolerance.  dPre starts as NaN, so a row the kernel owns but does not write
shows up as a non-finite value."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# 1, 2, 20, 32, 33, 64, 128 mixed in one batch of 9 docs; 32 -> 33 crosses
# the 64-row chunk edge at cap_mult = 2.  Doc 7 has pad features only.
LENS = (20, 1, 33, 2, 128, 32, 64, 7, 20)
ALL_PAD_DOC = 7
TAIL = 5  # trailing batch-padding tokens


@functools.lru_cache(maxsize=None)
def _case(nF, cap_mult, HP):
    """CPU inputs and the float64 reference, built once per shape."""
    rng = np.random.default_rng(1000 * nF + 10 * cap_mult + HP)
    lens = np.asarray(LENS, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total = int(lens.sum())
    T = total + TAIL
    S = cap_mult * total
    H = HP // 2
    feats = np.full((S, nF), T, dtype=np.int64)
    dS = rng.integers(-8, 9, (S, HP)).astype(np.float64)
    # maxout backward: exactly one of each piece pair (h, H + h) is nonzero
    pick = rng.integers(0, 2, (S, H)).astype(bool)
    dS[:, :H][pick] = 0.0
    dS[:, H:][~pick] = 0.0
    for d, (o, n) in enumerate(zip(off, lens)):
        r0, rows = cap_mult * o, cap_mult * n
        # unused capacity rows at the end of each doc: zero dSummed, pad feats
        used = rows if d == ALL_PAD_DOC else max(1, rows - max(1, rows // 4))
        dS[r0 + used:r0 + rows] = 0.0
        if d == ALL_PAD_DOC:
            continue
        f = o + rng.integers(0, n, (used, nF))
        f[rng.random((used, nF)) < 0.25] = T
        feats[r0:r0 + used] = f
    ref_feats = feats.copy()
    # one feature of doc 0 points at a token of doc 2: it must be ignored
    feats[0, 1] = off[2] + 3
    ref_feats[0, 1] = -1
    ref = torch.zeros((T + 1) * nF, HP, dtype=torch.float64)
    dS64 = torch.from_numpy(dS)
    for q in range(nF):
        t = torch.from_numpy(ref_feats[:, q])
        keep = t >= 0
        ref.index_add_(0, t[keep] * nF + q, dS64[keep])
    ref = ref.view(T + 1, nF, HP)
    return {
        "feats": torch.from_numpy(feats), "dS": dS64, "T": T, "total": total,
        "off": torch.from_numpy(off.astype(np.int32)),
        "lens": torch.from_numpy(lens.astype(np.int32)),
        "dPre": ref[:T], "dPad": ref[T], "dBias": dS64.sum(0),
    }


def _bits(x):
    return x.contiguous().view(torch.int16 if x.dtype == torch.bfloat16
                               else torch.int32)


@need_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("HP", [64, 128])
@pytest.mark.parametrize("nF,cap_mult", [(13, 2), (6, 1)])
def test_dpre_gather_bit_exact(nF, cap_mult, HP, dtype):
    from spacy_ray_amd.ops.api import hip_ext

    hip = hip_ext()
    c = _case(nF, cap_mult, HP)
    T, dev = c["T"], "cuda"
    dS = c["dS"].to(dev).to(dtype)
    feats = c["feats"].to(dev)
    off, lens = c["off"].to(dev), c["lens"].to(dev)
    maxlen = max(LENS)

    def run():
        dPre = torch.full((T + 1, nF, HP), float("nan"), device=dev, dtype=dtype)
        dBias, dPad = hip.dpre_gather(dS, feats, dPre, off, lens, T, cap_mult,
                                      maxlen, c["total"])
        return dPre[:T].cpu(), dBias.cpu(), dPad.cpu()

    dPre, dBias, dPad = run()
    # every row the kernel owns is written: untouched destinations, the
    # all-pad doc and the batch-padding tokens included
    assert torch.isfinite(dPre.float()).all()
    assert dBias.dtype == torch.float32 and dBias.shape == (HP,)
    assert dPad.dtype == torch.float32 and dPad.shape == (nF, HP)
    assert torch.equal(_bits(dPre), _bits(c["dPre"].to(dtype)))
    assert torch.equal(_bits(dBias), _bits(c["dBias"].float()))
    assert torch.equal(_bits(dPad), _bits(c["dPad"].float()))
    o7, n7 = int(c["off"][ALL_PAD_DOC]), LENS[ALL_PAD_DOC]
    assert not dPre[o7:o7 + n7].any() and not dPre[c["total"]:].any()
    # no atomics: a second call gives identical bits
    for a, b in zip((dPre, dBias, dPad), run()):
        assert torch.equal(_bits(a), _bits(b))


def _bf16_ulp(x):
    """Spacing of bf16 (8 significant bits) at the magnitude of x."""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126))) - 7)


@need_gpu
def test_gather_path_matches_atomic_path_end_to_end(monkeypatch):
    """dPre out of transition_loop_loss_fused: gather path against
    SRX_DPRE=atomic (started at zero), within one bf16 ulp per element.

    Every (token, slot) destination gets at most 2 contributions here (each
    slot of a doc draws its 2 * len rows from two permutations of the doc's
    tokens, a quarter of them replaced by pad).  The atomic path's first add
    into zero is exact and its second add rounds once; the gather path adds
    in fp32 (exact for two bf16 terms up to fp32 rounding) and rounds once.
    The CPU pair (torch_ref.maxout_backward, then per-add bf16 rounding
    against one rounding) is checked against the bound first."""
    from spacy_ray_amd.ops import api
    from spacy_ray_amd.ops import torch_ref as ref

    rng = np.random.default_rng(5)
    n_docs, nF, H, A, cap = 64, 13, 64, 10, 2
    HP = 2 * H
    lens = np.maximum(2, rng.poisson(20, n_docs)).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    total = int(lens.sum())
    T, S = total + 3, cap * total
    feats = np.full((S, nF), T, dtype=np.int64)
    for o, n in zip(off, lens):
        for q in range(nF):
            feats[cap * o:cap * (o + n), q] = o + np.concatenate(
                [rng.permutation(n) for _ in range(cap)])
    feats[rng.random((S, nF)) < 0.25] = T
    g = torch.Generator().manual_seed(5)
    bf = torch.bfloat16
    dScores = (torch.randn(S, A, generator=g) * 0.1).to(bf)
    upperW = (torch.randn(A, H, generator=g) * 0.3).to(bf)
    which = torch.randint(0, 2, (S, H), generator=g, dtype=torch.uint8)
    hidden = torch.randn(S, H, generator=g).to(bf)
    feats_t = torch.from_numpy(feats)

    # the reference pair on the CPU
    dHidden = dScores.mm(upperW)
    dSummed = ref.maxout_backward(dHidden, which.bool(), 2).reshape(S, HP)
    once = torch.zeros((T + 1) * nF, HP)
    per_add = torch.zeros((T + 1) * nF, HP, dtype=bf)
    for q in range(nF):
        idx = feats_t[:, q] * nF + q
        once.index_add_(0, idx, dSummed.float())
        # two rounds of disjoint destinations: one rounding per add
        for k in range(cap):
            rows = torch.cat([torch.arange(cap * o + k * n, cap * o + (k + 1) * n)
                              for o, n in zip(off, lens)])
            per_add.index_add_(0, idx[rows], dSummed[rows])
    once = once.to(bf).view(T + 1, nF, HP)[:T].float()
    per_add = per_add.view(T + 1, nF, HP)[:T].float()
    bound = _bf16_ulp(torch.maximum(once.abs(), per_add.abs()))
    assert ((once - per_add).abs() <= bound).all()

    dev = "cuda"
    args = [x.to(dev) for x in (dScores, torch.zeros(A), torch.ones(2), feats_t,
                                which, hidden)]
    lay = dict(doc_off=torch.from_numpy(off.astype(np.int32)).to(dev),
               doc_lens=torch.from_numpy(lens.astype(np.int32)).to(dev),
               cap_mult=cap, maxlen=int(lens.max()), doc_total=total)

    def grad(mode):
        if mode is None:
            monkeypatch.delenv("SRX_DPRE", raising=False)
        else:
            monkeypatch.setenv("SRX_DPRE", mode)
        pre = torch.zeros(T + 1, nF, HP, device=dev, dtype=bf, requires_grad=True)
        lower_b = torch.zeros(HP, device=dev, dtype=bf, requires_grad=True)
        uW = upperW.to(dev).requires_grad_(True)
        uB = torch.zeros(A, device=dev, dtype=bf, requires_grad=True)
        loss = api.transition_loop_loss_fused(pre, lower_b, uW, uB, *args, **lay)
        loss.backward()
        return pre.grad[:T].float().cpu()

    gather, atomic = grad(None), grad("atomic")
    assert torch.isfinite(gather).all()
    bound = _bf16_ulp(torch.maximum(gather.abs(), atomic.abs()))
    assert ((gather - atomic).abs() <= bound).all()
