"""CPU self-test of the float64 references in ``ref64.py`` — the GPU parity
tests (test_gpu_attn.py, test_gpu_mwe.py) are only as good as these."""
import pytest
import torch

import ref64


def _attn_case(L, lens, H=3, D=64, seed=0):
    gen = torch.Generator().manual_seed(seed)
    B = len(lens)
    q, k, v = (torch.randn(B, H, L, D, generator=gen).to(torch.bfloat16)
               for _ in range(3))
    return q, k, v, torch.tensor(lens, dtype=torch.int32)


@pytest.mark.parametrize("L", [5, 32, 50, 96, 130])
def test_attn_ref64_matches_sdpa_float64(L):
    from torch.nn.attention import SDPBackend, sdpa_kernel

    lens_l = [L, 1, min(33, L), L - 1]  # SDPA cannot express len=0 rows
    q, k, v, lens = _attn_case(L, lens_l)
    scale = 64 ** -0.5
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    O, P, lse = ref64.attn_ref64(qd, kd, vd, lens, scale)
    valid_q = (torch.arange(L)[None, None, :, None] < lens[:, None, None, None])
    dO = torch.randn(O.shape, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(1))
    O.backward(dO)  # dense dO: the reference's padding rows are constant 0

    q2, k2, v2 = (t.double().requires_grad_(True) for t in (q, k, v))
    with sdpa_kernel([SDPBackend.MATH]):
        ref = torch.nn.functional.scaled_dot_product_attention(
            q2, k2, v2, attn_mask=ref64.sdpa_prefix_mask(lens, L), scale=scale)
    ref.backward(dO * valid_q)
    assert float(((O - ref).detach().abs() * valid_q).max()) < 1e-12
    for ours, theirs in ((qd.grad, q2.grad), (kd.grad, k2.grad), (vd.grad, v2.grad)):
        assert float((ours - theirs).abs().max()) < 1e-12
    # padding semantics: exact zeros, lse = 0
    pad = ~valid_q.expand_as(O)
    assert float(O.detach()[pad].abs().max()) == 0.0
    assert float(qd.grad[pad].abs().max()) == 0.0
    assert float(kd.grad[pad].abs().max()) == 0.0
    assert float(vd.grad[pad].abs().max()) == 0.0
    assert float(lse.detach()[~valid_q[..., 0].expand_as(lse)].abs().max()) == 0.0
    # lse is the log-normaliser: exp(scale*S - lse) == P on valid rows
    S = scale * qd.detach() @ kd.detach().transpose(-1, -2)
    kv = valid_q.transpose(-1, -2)
    P2 = torch.exp(S - lse[..., None]) * valid_q * kv
    assert float((P2 - P).abs().max()) < 1e-12
    assert float((P.sum(-1) - valid_q[..., 0].double()).abs().max()) < 1e-12


def test_attn_ref64_empty_window_and_explicit_mask():
    L = 20
    q, k, v, lens = _attn_case(L, [L, 0, 7], seed=2)
    keep = 0.7
    mask = (torch.rand(3, 3, L, L, generator=torch.Generator().manual_seed(3))
            < keep)
    qd = q.double().requires_grad_(True)
    O, P, lse = ref64.attn_ref64(qd, k, v, lens, 0.125, mask=mask, keep=keep)
    O.sum().backward()
    assert torch.isfinite(O).all() and torch.isfinite(qd.grad).all()
    assert float(O[1].abs().max()) == 0.0 and float(lse[1].abs().max()) == 0.0
    assert float(qd.grad[1].abs().max()) == 0.0
    # mask/keep is applied AFTER normalisation
    O0, P0, _ = ref64.attn_ref64(q, k, v, lens, 0.125)
    want = (P0 * mask / keep) @ v.double()
    assert float((O - want).abs().max()) < 1e-12
    assert float((P - P0).abs().max()) == 0.0


@pytest.mark.parametrize("W", [96, 128])
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("geom", sorted(ref64.MWE_GEOMETRIES))
def test_mwe_ref64_matches_composed_float64(W, with_mask, geom):
    from test_gpu_mwe import _composed_ref

    lengths_l = ref64.MWE_GEOMETRIES[geom]
    X, Wt, bias, g, b, lengths, mask = ref64.mwe_inputs(W, lengths_l, with_mask)
    ins = [t.double().requires_grad_(True) for t in (X, Wt, bias, g, b)]
    Y, M, which, mu, rstd, pre = ref64.mwe_ref64(*ins, lengths, 1e-5, mask)
    dY = torch.randn(Y.shape, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(5))
    Y.backward(dY)
    ins2 = [t.double().requires_grad_(True) for t in (X, Wt, bias, g, b)]
    Y2, M2 = _composed_ref(*ins2, lengths, 1e-5,
                           mask.double() if mask is not None else None)
    Y2.backward(dY)
    assert float((Y - Y2).abs().max()) < 1e-12
    assert float((M - M2).abs().max()) < 1e-12
    for a, c in zip(ins, ins2):
        assert float((a.grad - c.grad).abs().max()) < 1e-11
    # saved statistics describe M
    assert float((mu - M.mean(-1)).abs().max()) < 1e-14
    assert float((rstd - (M.var(-1, unbiased=False) + 1e-5).rsqrt()).abs().max()) < 1e-12
    assert float((pre.gather(1, which[:, None]).squeeze(1) - pre.max(1).values).abs().max()) == 0.0
    # preconditions the GPU test relies on (test_mwe_layer_geometry):
    # fp32 single-pass variance is well conditioned, and argmax near-ties
    # (top-two gap <= 1e-4) are rare
    var = M.var(-1, unbiased=False)
    assert float((mu ** 2 / var).max()) <= 10.0
    assert float(mu.abs().min()) > 0.05  # a relative bound on mu is meaningful
    assert float((ref64.top2_gap(pre) <= 1e-4).double().mean()) < 0.01


@pytest.mark.parametrize("W", [96, 128])
def test_mwe_grad_inputs_have_no_near_tie(W):
    """Precondition of test_mwe_layer_grads_match_ref64's pinned baseline."""
    X, Wt, bias, g, b, lengths, mask = ref64.mwe_inputs(
        W, ref64.MWE_GRAD_LENGTHS, True, seed=ref64.MWE_GRAD_SEED)
    pre = ref64.mwe_ref64(X, Wt, bias, g, b, lengths, 1e-5, mask)[5]
    assert float(ref64.top2_gap(pre).min()) > 1e-5


def test_mwe_ref64_first_index_wins_ties():
    W = 96
    X = torch.zeros(64, W)
    Wt = torch.zeros(3 * W, 3 * W)
    bias = torch.zeros(3 * W)
    bias[W:2 * W] = 1.0
    bias[2 * W:] = 1.0  # pieces 1 and 2 tie above piece 0
    _, M, which, *_ = ref64.mwe_ref64(X, Wt, bias, torch.ones(W), torch.zeros(W),
                                      torch.tensor([64]), 1e-5)
    assert int(which.min()) == 1 and int(which.max()) == 1
    assert float(M.min()) == 1.0


def test_mwe_stage1_ref64_matches_autograd():
    W = 100
    gen = torch.Generator().manual_seed(8)
    M = torch.randn(64, W, generator=gen, dtype=torch.float64).requires_grad_(True)
    gg = (1 + 0.1 * torch.randn(W, generator=gen, dtype=torch.float64)).requires_grad_(True)
    bb = torch.zeros(W, dtype=torch.float64, requires_grad=True)
    msk = (torch.rand(64, W, generator=gen) < 0.9).double() / 0.9
    dY = torch.randn(64, W, generator=gen, dtype=torch.float64)
    which = torch.randint(0, 3, (64, W), generator=gen)
    Y = torch.nn.functional.layer_norm(M, (W,), gg, bb, 1e-5) * msk
    Y.backward(dY)
    Md = M.detach()
    mu = Md.mean(-1)
    rstd = (Md.var(-1, unbiased=False) + 1e-5).rsqrt()
    dPre, dg, db, dbias, partials = ref64.mwe_stage1_ref64(dY, msk, Md, gg.detach(), mu, rstd, which)
    dPre3 = dPre.view(64, 3, W)
    assert float((dPre3.sum(1) - M.grad).abs().max()) < 1e-12
    assert float((dPre3.gather(1, which[:, None]).squeeze(1) - M.grad).abs().max()) < 1e-12
    assert float((dg - gg.grad).abs().max()) < 1e-12
    assert float((db - bb.grad).abs().max()) < 1e-12
    assert float((dbias - dPre.sum(0)).abs().max()) == 0.0
    assert float((partials[1] - (dY * msk).cumsum(0).abs().amax(0)).abs().max()) < 1e-12
    assert bool((partials[1] >= db.abs() - 1e-12).all())


def test_bf16_ulp():
    assert ref64.bf16_ulp(1.0) == 2.0 ** -7
    assert ref64.bf16_ulp(1.99) == 2.0 ** -7
    assert ref64.bf16_ulp(2.0) == 2.0 ** -6
    assert ref64.bf16_ulp(0.3) == 2.0 ** -9
    # the next bf16 after 1.0 is exactly one ulp away
    assert float(torch.tensor(1.0 + 2.0 ** -7).to(torch.bfloat16)) == 1.0 + 2.0 ** -7
    assert float(torch.tensor(1.0 + 2.0 ** -9).to(torch.bfloat16)) == 1.0
