"""Fused MultiHashEmbed mixer (mixer_fwd / mixer_bwd_fused / ops.mixer_layer)
against float64.

Forward: Y = mask * LN(maxout_3(E @ Wm^T + bias)) with the composed bf16
chain linear -> maxout -> layer_norm -> * mask as the baseline of
ref64.check_parity (factor 2); mu / rstd to a relative 1e-4; `which` exact
where the float64 top-two gap is >= 1e-5.  For T <= 192 the seeds (SEEDS) are
chosen so that no gap is below 1e-5, asserted here from a CPU float64
product.  At T = 16448 there are 1.6M maxout elements and about 50 of them
are expected to have a gap below 1e-5 whatever the seed, so that size
compares `which` on the other elements only.

Backward: inputs as in test_gpu_mwe_bwd_fused (Mout / mu / rstd / which from
the float64 forward, a random dY).  dPre against ref64.mwe_stage1_ref64 (the
stage is the MWE one), dE against dPre64 @ Wm, baseline mwe_bwd_stage1 +
dPre.mm(Wm); the fp32 column sums to 1e-3 + 1e-3 |sum| (a fixed-order sum:
no accumulation allowance)."""
import functools
import math
import types

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
FACTOR = 2
FP32_TOL = dict(atol=1e-3, rtol=1e-3)
EPS = 1e-5
MIN_GAP = 1e-5

# (W, NS, T) -> a seed whose float64 pre-activations have no top-two gap
# below MIN_GAP (test_mixer_seeds_have_no_near_ties checks all of them)
SEEDS = {
    (96, 4, 64): 1, (96, 4, 128): 2, (96, 4, 192): 2,
    (96, 5, 64): 2, (96, 5, 128): 1, (96, 5, 192): 1,
    (128, 4, 64): 2, (128, 4, 128): 1, (128, 4, 192): 4,
    (128, 5, 64): 1, (128, 5, 128): 1, (128, 5, 192): 2,
}
SMALL_T = (64, 128, 192)   # half a tile; one tile; a tile + a 64-row tail
BIG_T = 16448              # 128 full tiles + a tail: two column-sum levels


def mixer_inputs(W, NS, T, seed):
    """CPU-generated inputs, already rounded to bf16: E, Wm, bias, g, b and
    a keep-0.9 mask."""
    gen = torch.Generator().manual_seed(seed)
    K = NS * W
    bf = torch.bfloat16
    E = (torch.randn(T, K, generator=gen) * 0.5).to(bf)
    Wm = (torch.randn(3 * W, K, generator=gen) / math.sqrt(K)).to(bf)
    bias = (torch.randn(3 * W, generator=gen) * 0.1).to(bf)
    g = (1 + 0.1 * torch.randn(W, generator=gen)).to(bf)
    b = (0.1 * torch.randn(W, generator=gen)).to(bf)
    mask = ((torch.rand(T, W, generator=gen) < 0.9).float() / 0.9).to(bf)
    return E, Wm, bias, g, b, mask


def mixer_ref64(E, Wm, bias, g, b, eps, mask=None):
    """Float64 mixer (pieces-major pre-activations, first index wins ties).
    Returns (Y, M, which, mu, rstd, pre [T, 3, W])."""
    E, Wm, bias, g, b = (t.double() for t in (E, Wm, bias, g, b))
    T, W = E.shape[0], g.shape[0]
    pre = (E @ Wm.t() + bias).view(T, 3, W)
    which = torch.zeros(T, W, dtype=torch.long, device=E.device)
    best = pre[:, 0].detach()
    for p in (1, 2):
        upd = pre[:, p].detach() > best
        which = torch.where(upd, torch.full_like(which, p), which)
        best = torch.where(upd, pre[:, p].detach(), best)
    M = pre.gather(1, which[:, None, :]).squeeze(1)
    mu = M.mean(-1)
    var = ((M - mu[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    Y = (M - mu[:, None]) * rstd[:, None] * g + b
    if mask is not None:
        Y = Y * mask.double()
    return Y, M, which, mu, rstd, pre


def _composed_bf16(E, Wm, bias, g, b, eps, mask=None, which=None):
    """Baseline: linear -> maxout -> layer_norm -> * mask in stock bf16 ops.
    With ``which`` the maxout takes the given pieces."""
    T, W = E.shape[0], g.shape[0]
    pre = torch.nn.functional.linear(E, Wm, bias).view(T, 3, W)
    if which is None:
        m = pre.max(dim=1).values
    else:
        m = pre.gather(1, which[:, None, :]).squeeze(1)
    y = torch.nn.functional.layer_norm(m, (W,), g, b, eps)
    if mask is not None:
        y = y * mask
    return y, m


def _seed(W, NS, T):
    return SEEDS.get((W, NS, T), 1)


@functools.lru_cache(maxsize=4)
def _case(W, NS, T):
    """Device inputs, the float64 forward (with the mask), and a dY."""
    ins = mixer_inputs(W, NS, T, _seed(W, NS, T))
    gap = None
    if T in SMALL_T:  # the CPU side: no near-tie in this seed's maxout
        gap = float(ref64.top2_gap(mixer_ref64(*ins[:5], EPS)[5]).min())
    E, Wm, bias, g, b, mask = (t.to(DEV) for t in ins)
    ref = mixer_ref64(E, Wm, bias, g, b, EPS, mask)
    dY = torch.randn(T, W, generator=torch.Generator().manual_seed(12)) \
        .to(torch.bfloat16).to(DEV)
    return (E, Wm, bias, g, b, mask), ref, dY, gap


def test_mixer_seeds_have_no_near_ties():
    for (W, NS, T), seed in sorted(SEEDS.items()):
        pre = mixer_ref64(*mixer_inputs(W, NS, T, seed)[:5], EPS)[5]
        assert float(ref64.top2_gap(pre).min()) >= MIN_GAP, (W, NS, T, seed)


def _check_fwd(tag, W, NS, T, with_mask):
    from spacy_ray_amd import _srx_hip

    (E, Wm, bias, g, b, mask), ref, _, gap = _case(W, NS, T)
    rY, rM, rwhich, rmu, rrstd, pre = ref
    if not with_mask:
        mask = None
        rY = mixer_ref64(E, Wm, bias, g, b, EPS)[0]
    valid = None
    if gap is not None:
        assert gap >= MIN_GAP, (tag, gap)
    else:
        valid = ref64.top2_gap(pre) >= MIN_GAP
    Y, Mout, which, mu, rstd = _srx_hip.mixer_fwd(E, Wm, bias, g, b, mask, EPS)
    assert Y.shape == (T, W) and Y.dtype == torch.bfloat16
    assert Mout.shape == (T, W) and which.dtype == torch.uint8
    bY, bM = _composed_bf16(E, Wm, bias, g, b, EPS, mask)
    ref64.check_parity("mixer Y " + tag, Y, bY, rY, None, FACTOR)
    ref64.check_parity("mixer Mout " + tag, Mout, bM, rM, None, FACTOR)
    for name, got, want in (("mu", mu, rmu), ("rstd", rstd, rrstd)):
        rel = ((got.double() - want).abs() / want.abs()).max()
        print("mixer %s %s max rel err %.3e" % (name, tag, float(rel)))
        assert float(rel) <= 1e-4, (tag, name, float(rel))
    same = which.long() == rwhich
    if valid is not None:
        same = same | ~valid
    assert bool(same.all()), (tag, int((~same).sum()))


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("T", SMALL_T)
@pytest.mark.parametrize("NS", [4, 5])
@pytest.mark.parametrize("W", [96, 128])
def test_mixer_fwd_matches_ref64(W, NS, T, with_mask):
    _check_fwd("W=%d NS=%d T=%d mask=%d" % (W, NS, T, with_mask), W, NS, T,
               with_mask)


@need_gpu
def test_mixer_fwd_many_tiles():
    _check_fwd("W=96 NS=4 T=%d mask=1" % BIG_T, 96, 4, BIG_T, True)


def _run_bwd(W, NS, T, with_mask):
    from spacy_ray_amd import _srx_hip

    (E, Wm, bias, g, b, mask), ref, dY, _ = _case(W, NS, T)
    _, rM, rwhich, rmu, rrstd, _ = ref
    if not with_mask:
        mask = None
    args = (dY, mask, rM.to(torch.bfloat16), g, rmu.float(), rrstd.float(),
            rwhich.to(torch.uint8))
    out = _srx_hip.mixer_bwd_fused(*args, Wm)
    base_dPre = _srx_hip.mwe_bwd_stage1(*args)[0]
    base_dE = base_dPre.mm(Wm)
    rdPre, rdg, rdb, rdbias, _ = ref64.mwe_stage1_ref64(*args)
    return args, out, base_dPre, base_dE, (rdPre, rdPre @ Wm.double(), rdg,
                                            rdb, rdbias)


def _check_bwd(tag, W, NS, T, with_mask, valid=None):
    args, out, base_dPre, base_dE, refs = _run_bwd(W, NS, T, with_mask)
    dPre, dE, dg32, db32, dbias32 = out
    rdPre, rdE, rdg, rdb, rdbias = refs
    which = args[6]
    assert dPre.shape == (T, 3 * W) and dPre.dtype == torch.bfloat16
    assert dE.shape == (T, NS * W) and dE.dtype == torch.bfloat16
    # exact zeros in the two non-argmax pieces
    onehot = torch.zeros(T, 3, W, dtype=torch.bool, device=DEV)
    onehot.scatter_(1, which.long()[:, None, :], True)
    assert float(dPre.view(T, 3, W)[~onehot].float().abs().max()) == 0.0
    ref64.check_parity("mixer dPre " + tag, dPre, base_dPre, rdPre, valid, FACTOR)
    ref64.check_parity("mixer dE " + tag, dE, base_dE, rdE, valid, FACTOR)
    for name, got, want, n in zip(("dg", "db", "dbias"), (dg32, db32, dbias32),
                                  (rdg, rdb, rdbias), (W, W, 3 * W)):
        assert got.dtype == torch.float32 and got.shape == (n,)
        err = (got.double() - want).abs()
        bound = FP32_TOL["atol"] + FP32_TOL["rtol"] * want.abs()
        print("mixer %s %s max err %.3e  worst err/bound %.3f" % (
            tag, name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (tag, name, float(err.max()))
    return out


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("T", SMALL_T)
@pytest.mark.parametrize("NS", [4, 5])
@pytest.mark.parametrize("W", [96, 128])
def test_mixer_bwd_fused_matches_ref64(W, NS, T, with_mask):
    _check_bwd("W=%d NS=%d T=%d mask=%d" % (W, NS, T, with_mask), W, NS, T,
               with_mask)


@need_gpu
def test_mixer_bwd_fused_many_tiles():
    """129 per-tile partial rows (two reduction levels) and a 64-row tail
    tile; dPre and dE also on the last tile alone."""
    W, NS, T = 96, 4, BIG_T
    _check_bwd("W=96 NS=4 T=%d mask=1" % T, W, NS, T, True)
    last = (torch.arange(T, device=DEV) >= T - 64)[:, None]
    _check_bwd("W=96 NS=4 last tile", W, NS, T, True, last)


@need_gpu
@pytest.mark.parametrize("W,NS", [(96, 4), (128, 5)])
def test_mixer_bit_reproducible(W, NS):
    """No atomics in either kernel: two calls agree bit for bit."""
    from spacy_ray_amd import _srx_hip

    T = BIG_T if W == 96 else 192
    (E, Wm, bias, g, b, mask), _, _, _ = _case(W, NS, T)
    f1 = _srx_hip.mixer_fwd(E, Wm, bias, g, b, mask, EPS)
    f2 = _srx_hip.mixer_fwd(E, Wm, bias, g, b, mask, EPS)
    args = _run_bwd(W, NS, T, True)[0]
    b1 = _srx_hip.mixer_bwd_fused(*args, Wm)
    b2 = _srx_hip.mixer_bwd_fused(*args, Wm)
    assert len(f1) == len(f2) == 5 and len(b1) == len(b2) == 5
    for x, y in zip(list(f1) + list(b1), list(f2) + list(b2)):
        assert torch.equal(x, y)


@need_gpu
@pytest.mark.parametrize("NS", [4, 5])
@pytest.mark.parametrize("W", [96, 128])
def test_mixer_layer_grads_match_ref64(W, NS):
    """ops.mixer_layer autograd (mask, keep 0.9) against float64 autograd;
    baselines: the composed bf16 chain, and the same chain with the maxout
    pieces pinned to the reference's `which` (rounding error only), as in
    test_mwe_layer_grads_match_ref64."""
    from spacy_ray_amd.ops.api import mixer_layer

    T = 192
    (E, Wm, bias, g, b, mask), ref, dY, gap = _case(W, NS, T)
    assert gap >= MIN_GAP
    rwhich = ref[2]

    def run(fn, ins, dy):
        leaves = [t.detach().clone().requires_grad_(True) for t in ins]
        fn(*leaves).backward(dy)
        return [t.grad for t in leaves]

    ins = (E, Wm, bias, g, b)
    got = run(lambda *a: mixer_layer(*a, mask, EPS), ins, dY)
    want = run(lambda *a: mixer_ref64(*a, EPS, mask)[0],
               [t.double() for t in ins], dY.double())
    base = run(lambda *a: _composed_bf16(*a, EPS, mask)[0], ins, dY)
    pinned = run(lambda *a: _composed_bf16(*a, EPS, mask, rwhich)[0], ins, dY)
    names = ("dE", "dW", "dbias", "dg", "db")
    for name, k, bl, r in zip(names, got, base, want):
        ref64.check_parity("mixer_layer %s W=%d NS=%d" % (name, W, NS), k, bl,
                           r, None, FACTOR)
    for name, k, bl, r in zip(names, got, pinned, want):
        ref64.check_parity("mixer_layer/pinned %s W=%d NS=%d" % (name, W, NS),
                           k, bl, r, None, FACTOR)


def _embed_and_batch(dtype):
    from spacy_ray_amd.models.tok2vec import MultiHashEmbed

    torch.manual_seed(3)
    embed = MultiHashEmbed(96).to(DEV).to(dtype)
    ids = torch.randint(0, 2 ** 40, (128, 4), dtype=torch.int64,
                        generator=torch.Generator().manual_seed(4)).to(DEV)
    return embed, types.SimpleNamespace(attr_ids=ids)


def _count_paths(monkeypatch, embed, batch, drop=0.0):
    from spacy_ray_amd.ops import api as ops

    calls = {"fused": 0, "composed": 0}
    fused, composed = ops.mixer_layer, ops.linear_cdw

    def spy_fused(*a, **k):
        calls["fused"] += 1
        return fused(*a, **k)

    def spy_composed(*a, **k):
        calls["composed"] += 1
        return composed(*a, **k)

    monkeypatch.setattr(ops, "mixer_layer", spy_fused)
    monkeypatch.setattr(ops, "linear_cdw", spy_composed)
    Y = embed(batch, drop=drop).detach()
    assert Y.shape == (128, 96)
    return calls, Y


@need_gpu
def test_multihashembed_dispatch(monkeypatch):
    monkeypatch.delenv("SRX_MIXER", raising=False)
    embed, batch = _embed_and_batch(torch.bfloat16)
    calls, Y = _count_paths(monkeypatch, embed, batch)
    assert calls == {"fused": 1, "composed": 0}
    monkeypatch.setenv("SRX_MIXER", "composed")
    calls, Yc = _count_paths(monkeypatch, embed, batch)
    assert calls == {"fused": 0, "composed": 1}
    # the two paths compute the same layer (bf16 rounding apart)
    assert float((Y.float() - Yc.float()).abs().max()) < 0.1
    monkeypatch.delenv("SRX_MIXER")
    embed32, batch = _embed_and_batch(torch.float32)
    calls, _ = _count_paths(monkeypatch, embed32, batch)
    assert calls == {"fused": 0, "composed": 1}
    monkeypatch.setenv("SRX_MIXER", "fused")
    with pytest.raises(ValueError):
        embed(batch)


@need_gpu
def test_mixer_launcher_guards():
    from spacy_ray_amd import _srx_hip

    def fwd_args(T, W, NS, dtype=torch.bfloat16):
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
        return [z(T, NS * W), z(3 * W, NS * W), z(3 * W), z(W), z(W), None, EPS]

    def bwd_args(T, W, NS, dtype=torch.bfloat16):
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
        f = torch.zeros(T, dtype=torch.float32, device=DEV)
        wh = torch.zeros(T, W, dtype=torch.uint8, device=DEV)
        return [z(T, W), None, z(T, W), z(W), f, f, wh, z(3 * W, NS * W)]

    strided = fwd_args(64, 96, 4)
    strided[0] = torch.zeros(64, 2 * 384, dtype=torch.bfloat16,
                             device=DEV)[:, ::2]
    for bad in (fwd_args(64, 96, 4, torch.float32),   # not bf16
                fwd_args(100, 96, 4),                 # T % 64 != 0
                fwd_args(64, 64, 4),                  # unsupported W
                fwd_args(64, 96, 3),                  # unsupported NS
                strided):                             # non-contiguous E
        with pytest.raises(RuntimeError):
            _srx_hip.mixer_fwd(*bad)
    strided = bwd_args(64, 96, 4)
    strided[0] = torch.zeros(64, 192, dtype=torch.bfloat16, device=DEV)[:, ::2]
    for bad in (bwd_args(64, 96, 4, torch.float32),
                bwd_args(100, 96, 4),
                bwd_args(64, 64, 4),
                bwd_args(64, 96, 6),
                strided):
        with pytest.raises(RuntimeError):
            _srx_hip.mixer_bwd_fused(*bad)
    Y, Mout, which, mu, rstd = _srx_hip.mixer_fwd(*fwd_args(0, 96, 4))
    assert Y.shape == (0, 96) and which.shape == (0, 96) and mu.shape == (0,)
    dPre, dE, dg32, db32, dbias32 = _srx_hip.mixer_bwd_fused(*bwd_args(0, 96, 4))
    assert dPre.shape == (0, 288) and dE.shape == (0, 384)
    assert float(dbias32.abs().max()) == 0.0
