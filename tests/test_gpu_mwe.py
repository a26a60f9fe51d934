"""Fused MWE-layer MFMA kernel vs the composed reference (GPU), and the
parity tests against the float64 reference of ref64.py (bf16 tolerances
follow ref64.check_parity's error-ratio rule; measured ratios are in
docs/KERNELS.md, "Parity margins")."""
import functools

import numpy as np
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"


def _composed_ref(X32, Wt32, bias32, g32, b32, lengths, eps, mask32=None):
    from spacy_ray_amd.ops import torch_ref as ref

    X3 = ref.seq2col(X32, lengths)
    pre = X3 @ Wt32.t() + bias32
    T, W = X32.shape
    m, which = pre.view(T, 3, W).max(dim=1)
    ln = torch.nn.functional.layer_norm(m, (W,), g32, b32, eps)
    if mask32 is not None:
        ln = ln * mask32
    return X32 + ln, m


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
@pytest.mark.parametrize("with_mask", [False, True])
def test_mwe_layer_fused_matches_composed(W, with_mask):
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8, mwe_layer

    torch.manual_seed(0)
    lengths = torch.tensor([30, 2, 64, 17, 15], device=DEV)
    T = 128
    assert int(lengths.sum()) == T
    X = (torch.randn(T, W, device=DEV) * 0.5).to(torch.bfloat16)
    Wt = (torch.randn(3 * W, 3 * W, device=DEV) * (1.0 / np.sqrt(3 * W))).to(torch.bfloat16)
    bias = torch.randn(3 * W, device=DEV).to(torch.bfloat16) * 0.1
    g = (1 + 0.1 * torch.randn(W, device=DEV)).to(torch.bfloat16)
    b = (0.1 * torch.randn(W, device=DEV)).to(torch.bfloat16)
    starts, ends = boundary_masks_u8(lengths, T)
    mask = None
    if with_mask:
        mask = ((torch.rand(T, W, device=DEV) < 0.9).to(torch.bfloat16) / 0.9)

    # fused forward (no grad path first)
    Y, Mout, which, mu, rstd = _srx_hip.mwe_layer_fwd(
        X, Wt, bias, g, b, starts, ends, mask, 1e-5
    )
    Yr, Mr = _composed_ref(
        X.float(), Wt.float(), bias.float(), g.float(), b.float(),
        lengths, 1e-5, mask.float() if mask is not None else None,
    )
    assert torch.allclose(Mout.float(), Mr, atol=5e-2, rtol=5e-2), (
        (Mout.float() - Mr).abs().max()
    )
    assert torch.allclose(Y.float(), Yr, atol=6e-2, rtol=6e-2), (
        (Y.float() - Yr).abs().max()
    )

    # autograd through the fused op vs composed fp32 autograd
    Xa = X.clone().requires_grad_(True)
    Wa = Wt.clone().requires_grad_(True)
    ba = bias.clone().requires_grad_(True)
    ga = g.clone().requires_grad_(True)
    bb = b.clone().requires_grad_(True)
    Yf = mwe_layer(Xa, Wa, ba, ga, bb, starts, ends, mask, 1e-5)
    dY = torch.randn_like(Yf)
    Yf.backward(dY)

    X2 = X.float().requires_grad_(True)
    W2 = Wt.float().requires_grad_(True)
    b2 = bias.float().requires_grad_(True)
    g2 = g.float().requires_grad_(True)
    bb2 = b.float().requires_grad_(True)
    Y2, _ = _composed_ref(X2, W2, b2, g2, bb2, lengths, 1e-5,
                          mask.float() if mask is not None else None)
    Y2.backward(dY.float())

    for got, want, name in [
        (Xa.grad, X2.grad, "dX"),
        (Wa.grad, W2.grad, "dW"),
        (ba.grad, b2.grad, "dbias"),
        (ga.grad, g2.grad, "dg"),
        (bb.grad, bb2.grad, "db"),
    ]:
        assert torch.allclose(got.float(), want, atol=2e-1, rtol=1e-1), (
            name, (got.float() - want).abs().max(), want.abs().max()
        )


@need_gpu
def test_srx_embedding_backward_matches_torch():
    from spacy_ray_amd.models.transformer import _SrxEmbedding

    torch.manual_seed(3)
    R, W, N = 500, 64, 4000
    emb = _SrxEmbedding(R, W, padding_idx=1).to(DEV).to(torch.bfloat16)
    ids = torch.randint(0, R, (N,), device=DEV)
    ids[::5] = 1    # padding rows must get no grad
    ids[::3] = 7    # hot row
    Y = emb(ids)
    dY = torch.randn_like(Y)
    Y.backward(dY)
    ref_emb = torch.nn.Embedding(R, W, padding_idx=1).to(DEV)
    with torch.no_grad():
        ref_emb.weight.copy_(emb.weight.float())
    Y2 = ref_emb(ids)
    Y2.backward(dY.float())
    assert torch.allclose(emb.weight.grad.float(), ref_emb.weight.grad,
                          atol=2e-1, rtol=5e-2)
    assert emb.weight.grad[1].abs().max() == 0  # padding_idx zeroed


@need_gpu
def test_srx_layernorm_module_matches_torch():
    from spacy_ray_amd.models.transformer import _SrxLayerNorm

    torch.manual_seed(4)
    ln = _SrxLayerNorm(768, eps=1e-5).to(DEV).to(torch.bfloat16)
    X = torch.randn(257, 768, device=DEV, dtype=torch.bfloat16, requires_grad=True)
    Y = ln(X)
    Yr = torch.nn.functional.layer_norm(X.float(), (768,), ln.weight.float(),
                                        ln.bias.float(), 1e-5)
    assert torch.allclose(Y.float(), Yr, atol=5e-2, rtol=5e-2)
    Y.sum().backward()
    assert torch.isfinite(X.grad.float()).all()


@need_gpu
def test_mwe_used_in_encoder_forward():
    """The CNN encoder must actually route through the fused kernel on GPU
    (bf16, W=96, padded T)."""
    from spacy_ray_amd.models.tok2vec import MaxoutWindowEncoder
    from spacy_ray_amd.ops import api

    enc = MaxoutWindowEncoder(96, depth=2).to(DEV).to(torch.bfloat16)
    T = 128
    X = torch.randn(T, 96, device=DEV, dtype=torch.bfloat16)
    lengths = torch.tensor([64, 64], device=DEV)
    assert api.mwe_layer_available(X, 96, 3)
    Y = enc(X, lengths)
    assert Y.shape == (T, 96)
    assert torch.isfinite(Y.float()).all()


# ===================================================== float64 parity tests
FP32_TOL = dict(atol=1e-3, rtol=1e-3)  # the layernorm-backward fp32 tolerance
# Error-ratio factors for ref64.check_parity (2 = equally many roundings).
FACTOR_FWD = 2
FACTOR_BWD = 2


def _composed_bf16(X, Wt, bias, g, b, lengths, eps, mask=None, which=None):
    """Baseline: the composed path in stock bf16 torch ops.  With ``which``
    the maxout takes the given pieces instead of its own bf16 argmax."""
    from spacy_ray_amd.ops import torch_ref as ref

    T, W = X.shape
    pre = ref.seq2col(X, lengths).mm(Wt.t()) + bias
    if which is None:
        m = pre.view(T, 3, W).max(dim=1).values
    else:
        m = pre.view(T, 3, W).gather(1, which[:, None, :]).squeeze(1)
    ln = torch.nn.functional.layer_norm(m, (W,), g, b, eps)
    if mask is not None:
        ln = ln * mask
    return X + ln, m


def _to_dev(ts):
    return [t.to(DEV) if t is not None else None for t in ts]


@need_gpu
@pytest.mark.parametrize("geom", sorted(ref64.MWE_GEOMETRIES))
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_layer_geometry(W, with_mask, geom):
    """Forward outputs AND the saved mu / rstd / which against float64 at
    the tile-geometry edges: boundary on the 64-row tile edge, a doc
    spanning it, single-token docs, a boundary-free interior tile, T=64."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    X, Wt, bias, g, b, lengths, mask = _to_dev(
        ref64.mwe_inputs(W, ref64.MWE_GEOMETRIES[geom], with_mask))
    T = X.shape[0]
    starts, ends = boundary_masks_u8(lengths, T)
    Y, Mout, which, mu, rstd = _srx_hip.mwe_layer_fwd(
        X, Wt, bias, g, b, starts, ends, mask, 1e-5)
    rY, rM, rwhich, rmu, rrstd, pre = ref64.mwe_ref64(
        X, Wt, bias, g, b, lengths, 1e-5, mask)
    bY, bM = _composed_bf16(X, Wt, bias, g, b, lengths, 1e-5, mask)
    tag = "W=%d %s mask=%d" % (W, geom, with_mask)
    ref64.check_parity("mwe Mout " + tag, Mout, bM, rM, None, FACTOR_FWD)
    ref64.check_parity("mwe Y " + tag, Y, bY, rY, None, FACTOR_FWD)
    # fp32 single-pass variance: relative error ~ W * 2^-24 * (1 + mu^2/var)
    var = rM.var(-1, unbiased=False)
    assert float((rmu ** 2 / var).max()) <= 10.0
    e_mu = float(((mu.double() - rmu).abs() / rmu.abs()).max())
    e_rstd = float(((rstd.double() - rrstd).abs() / rrstd).max())
    print("mwe %s rel err mu %.3e rstd %.3e" % (tag, e_mu, e_rstd))
    assert e_mu <= 1e-4 and e_rstd <= 1e-4
    # argmax: exact where the float64 top-two gap is clear, else either
    gap = ref64.top2_gap(pre)
    near = gap <= 1e-4
    assert float(near.double().mean()) < 0.01
    top2 = pre.topk(2, dim=1).indices
    got = which.long()
    assert torch.equal(got[~near], rwhich[~near])
    assert bool(((got == top2[:, 0]) | (got == top2[:, 1])).all())


STAGE1_CASES = [(torch.bfloat16, 96), (torch.bfloat16, 128),
                (torch.float32, 96), (torch.float32, 100), (torch.float32, 256)]


@functools.lru_cache(maxsize=4)
def _stage1_inputs(dtype, W, N):
    """Inputs produced by mwe_ref64 (Mout rounded to the compute dtype;
    mu / rstd / which from the reference), shared by the mask / DET cases."""
    X, Wt, bias, g, b, lengths, mask = _to_dev(
        ref64.mwe_inputs(W, [64] * (N // 64), True, seed=11, dtype=dtype))
    _, rM, rwhich, rmu, rrstd, _ = ref64.mwe_ref64(X, Wt, bias, g, b, lengths, 1e-5)
    gen = torch.Generator().manual_seed(12)
    dY = torch.randn(N, W, generator=gen).to(dtype).to(DEV)
    return (dY, mask, rM.to(dtype), g, rmu.float(), rrstd.float(),
            rwhich.to(torch.uint8))


@need_gpu
@pytest.mark.parametrize("det", [False, True], ids=["atomic", "det"])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("N", [64, 16448])  # 16448 rows > the 16384-wave grid
@pytest.mark.parametrize("dtype,W", STAGE1_CASES,
                         ids=["%s-%d" % (str(d)[6:], w) for d, w in STAGE1_CASES])
def test_mwe_bwd_stage1_direct(dtype, W, N, with_mask, det):
    from spacy_ray_amd import _srx_hip

    dY, mask, Mout, g, mu, rstd, which = _stage1_inputs(dtype, W, N)
    if not with_mask:
        mask = None
    dPre, dg32, db32, dbias32 = _srx_hip.mwe_bwd_stage1(
        dY, mask, Mout, g, mu, rstd, which, det)
    rdPre, rdg, rdb, rdbias, partials = ref64.mwe_stage1_ref64(
        dY, mask, Mout, g, mu, rstd, which)
    tag = "%s W=%d N=%d mask=%d det=%d" % (str(dtype)[6:], W, N, with_mask, det)
    # exact zeros in the two non-argmax pieces
    onehot = torch.zeros(N, 3, W, dtype=torch.bool, device=DEV)
    onehot.scatter_(1, which.long()[:, None, :], True)
    assert dPre.dtype == dtype and torch.isfinite(dPre.float()).all()
    assert float(dPre.view(N, 3, W)[~onehot].float().abs().max()) == 0.0
    if dtype == torch.float32:
        err = float((dPre.double() - rdPre).abs().max())
        print("stage1 %s dPre max err %.3e" % (tag, err))
        assert torch.allclose(dPre.double(), rdPre, **FP32_TOL)
    else:
        # baseline: stock bf16 LayerNorm backward (autograd) + scatter
        Mb = Mout.detach().clone().requires_grad_(True)
        ln = torch.nn.functional.layer_norm(Mb, (W,), g, torch.zeros_like(g), 1e-5)
        if mask is not None:
            ln = ln * mask
        ln.backward(dY)
        base = torch.zeros(N, 3, W, dtype=dtype, device=DEV)
        base.scatter_(1, which.long()[:, None, :], Mb.grad[:, None, :])
        ref64.check_parity("stage1 dPre " + tag, dPre, base.view(N, 3 * W),
                           rdPre, None, FACTOR_BWD)
    # the fp32 column sums, BEFORE any cast to the compute dtype, against
    # the float64 sums at the layernorm-backward fp32 tolerance
    # (1e-3 + 1e-3 * |sum|).  That literal bound holds for N = 64 and for
    # the DET fixed-point path at every N (its quantisation is at most
    # 2^-25 per atomic: 16384 * 2^-25 = 4.9e-4).
    # Deviation, float atomics at N = 16448 only: the launcher runs 16384
    # waves, each adds its register partial with ONE float atomic per
    # column, so a column is an fp32 accumulation of A = 16384 terms whose
    # running sum reaches P ~ 100-400.  Every add rounds the running sum
    # (<= 2^-24 * |partial|, zero mean, independent), a random walk with
    # std <= sqrt(A) * 2^-24 * P / sqrt(3) ~ 5e-4 — already at the 1e-3
    # atol wherever the final sum happens to cancel.  For that case the
    # bound gains 4 * sqrt(A) * 2^-24 * P (about 7 sigma; P is taken from
    # the float64 reference in row order, the slack covers the arbitrary
    # atomic order): ~6e-3 at P = 200.
    nwaves = min((N + 3) // 4, 4096) * 4
    n_atomics = min(N, nwaves)
    accumulates = (not det) and N > 64
    for name, got, ref, part in (("dg", dg32, rdg, partials[0]),
                                 ("db", db32, rdb, partials[1]),
                                 ("dbias", dbias32, rdbias, partials[2])):
        assert got.dtype == torch.float32
        err = (got.double() - ref).abs()
        bound = FP32_TOL["atol"] + FP32_TOL["rtol"] * ref.abs()
        if accumulates:
            bound = bound + 4 * (n_atomics ** 0.5) * 2.0 ** -24 * part
        print("stage1 %s %s max err %.3e  worst err/bound %.3f" % (
            tag, name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (tag, name, float(err.max()))


@need_gpu
def test_mwe_bwd_stage1_rejects_W_over_256():
    from spacy_ray_amd import _srx_hip

    N, W = 64, 257
    z = torch.zeros(N, W, device=DEV)
    with pytest.raises(RuntimeError):
        _srx_hip.mwe_bwd_stage1(z, None, z, torch.ones(W, device=DEV),
                                torch.zeros(N, device=DEV), torch.ones(N, device=DEV),
                                torch.zeros(N, W, dtype=torch.uint8, device=DEV), False)


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_layer_grads_match_ref64(W):
    """End-to-end mwe_layer autograd (dropout mask, keep 0.9) against
    float64 autograd under the error-ratio rule, with two baselines.  The
    composed bf16 path takes its maxout argmax over bf16-rounded
    pre-activations, and its flips dominate its dX / dW / dbias error (25-50x
    the kernel's), so that baseline alone would accept a large error there.
    The second baseline is the same bf16 chain with the maxout pieces pinned
    to the reference's ``which``: its error is rounding only.  The inputs
    (ref64.MWE_GRAD_SEED) have no float64 top-two gap below 1e-5 — ten times
    the fp32 accumulation error of a pre-activation — so the kernel's own
    fp32 argmax must agree with the reference everywhere."""
    from spacy_ray_amd.ops.api import boundary_masks_u8, mwe_layer

    X, Wt, bias, g, b, lengths, mask = _to_dev(ref64.mwe_inputs(
        W, ref64.MWE_GRAD_LENGTHS, True, seed=ref64.MWE_GRAD_SEED))
    T = X.shape[0]
    starts, ends = boundary_masks_u8(lengths, T)
    dY = torch.randn(T, W, generator=torch.Generator().manual_seed(22)) \
        .to(torch.bfloat16).to(DEV)

    def run(fn, ins, dy):
        leaves = [t.detach().clone().requires_grad_(True) for t in ins]
        fn(*leaves).backward(dy)
        return [t.grad for t in leaves]

    ins = (X, Wt, bias, g, b)
    _, _, rwhich, _, _, pre = ref64.mwe_ref64(*ins, lengths, 1e-5, mask)
    assert float(ref64.top2_gap(pre).min()) > 1e-5
    got = run(lambda *a: mwe_layer(*a, starts, ends, mask, 1e-5), ins, dY)
    ref = run(lambda *a: ref64.mwe_ref64(*a, lengths, 1e-5, mask)[0],
              [t.double() for t in ins], dY.double())
    base = run(lambda *a: _composed_bf16(*a, lengths, 1e-5, mask)[0], ins, dY)
    pinned = run(lambda *a: _composed_bf16(*a, lengths, 1e-5, mask, rwhich)[0],
                 ins, dY)
    names = ("dX", "dW", "dbias", "dg", "db")
    for name, k, bl, r in zip(names, got, base, ref):
        ref64.check_parity("mwe_layer %s W=%d" % (name, W), k, bl, r, None,
                           FACTOR_BWD)
    for name, k, bl, r in zip(names, got, pinned, ref):
        ref64.check_parity("mwe_layer/pinned %s W=%d" % (name, W), k, bl, r,
                           None, FACTOR_BWD)
