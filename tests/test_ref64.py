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


# ----------------------- elementwise, CE and ragged references (ref64.py)
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _boundary_lengths():
    return [[1], [1, 1, 1], [5, 1, 9, 3], [40]]


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("lengths_l", _boundary_lengths(), ids=str)
def test_seq2col_bwd64_matches_autograd(lengths_l, with_residual):
    W, T = 12, sum(lengths_l)
    lengths = torch.tensor(lengths_l)
    X = torch.randn(T, W, generator=_gen(0), dtype=torch.float64).requires_grad_(True)
    dY = torch.randn(T, 3 * W, generator=_gen(1), dtype=torch.float64)
    res = torch.randn(T, W, generator=_gen(2), dtype=torch.float64) if with_residual else None
    ref64.seq2col64(X, lengths).backward(dY)
    want = X.grad if res is None else X.grad + res
    got = ref64.seq2col_bwd64(dY, lengths, res)
    assert float((got - want).abs().max()) < 1e-12


@pytest.mark.parametrize("P", [1, 2, 3])
def test_maxout64_matches_autograd_and_first_index_wins(P):
    X = torch.randn(17, P, 50, generator=_gen(3), dtype=torch.float64).requires_grad_(True)
    Y, which = ref64.maxout64(X)
    vals, idx = X.max(dim=1)
    assert torch.equal(Y, vals) and torch.equal(which, idx)
    dY = torch.randn(17, 50, generator=_gen(4), dtype=torch.float64)
    Y.backward(dY)
    dX = ref64.maxout_bwd64(dY, which, P)
    assert float((dX - X.grad).abs().max()) < 1e-12
    assert torch.equal(dX.gather(1, which[:, None])[:, 0], dY)
    assert int((dX != 0).sum()) <= dY.numel()
    tied = torch.ones(4, P, 8)
    assert int(ref64.maxout64(tied)[1].max()) == 0


@pytest.mark.parametrize("mean", [0.0, 30.0])
@pytest.mark.parametrize("W", [1, 65, 300])
def test_layernorm64_matches_autograd(W, mean):
    N = 9
    X = (mean + torch.randn(N, W, generator=_gen(5), dtype=torch.float64)).requires_grad_(True)
    g = (1 + 0.1 * torch.randn(W, generator=_gen(6), dtype=torch.float64)).requires_grad_(True)
    b = (0.1 * torch.randn(W, generator=_gen(7), dtype=torch.float64)).requires_grad_(True)
    dY = torch.randn(N, W, generator=_gen(8), dtype=torch.float64)
    want = torch.nn.functional.layer_norm(X, (W,), g, b, 1e-5)
    want.backward(dY)
    Y, mu, rstd = ref64.layernorm64(X.detach(), g.detach(), b.detach(), 1e-5)
    dX, dg, db = ref64.layernorm_bwd64(dY, X.detach(), g.detach(), 1e-5)
    Xd = X.detach()
    assert float((Y - want).abs().max()) < 1e-12
    assert float((mu - Xd.mean(-1)).abs().max()) < 1e-12
    assert float((rstd - (Xd.var(-1, unbiased=False) + 1e-5).rsqrt()).abs().max()) < 1e-12
    # W = 1 only: the true dX and dg are 0 and ours are exactly 0, but torch's
    # own x - mean is off by a rounding at mean 30, which rstd ~ 316 (var = 0)
    # multiplies (2.4e-12 in dg): there the bound is relative to rstd
    amp = float(rstd.max()) if W == 1 else 1.0
    assert float((dX - X.grad).abs().max()) < 1e-12 * amp
    assert float((dg - g.grad).abs().max()) < 1e-12 * amp
    assert float((db - b.grad).abs().max()) < 1e-12


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("C", [1, 2, 65])
def test_softmax_ce64_matches_autograd(C, scale):
    N = 33
    s = (scale * torch.randn(N, C, generator=_gen(9), dtype=torch.float64)).requires_grad_(True)
    gold = torch.randint(0, C, (N,), generator=_gen(10))
    gold[::5] = -1
    want = torch.nn.functional.cross_entropy(s, gold, ignore_index=-1, reduction="sum")
    want.backward()
    loss, count, d = ref64.softmax_ce64(s.detach(), gold)
    assert abs(float(loss - want)) < 1e-12
    assert count == int((gold >= 0).sum())
    assert float((d - s.grad).abs().max()) < 1e-12
    assert float(d[gold < 0].abs().max()) == 0.0
    loss, count, d = ref64.softmax_ce64(s.detach(), torch.full((N,), -1))
    assert float(loss) == 0.0 and count == 0 and not d.any()


def _ragged_loop(X, lengths_l, mode):
    """Per-document torch float64 composition under the empty-doc rule."""
    rows, off = [], 0
    for n in lengths_l:
        doc = X[off:off + n]
        if n == 0:
            rows.append(X.new_zeros(X.shape[1]) + 0 * X.sum())
        elif mode == 0:
            rows.append(doc.sum(0))
        elif mode == 1:
            rows.append(doc.mean(0))
        else:
            rows.append(doc.max(0).values)
        off += n
    return torch.stack(rows)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("geom", sorted(ref64.RAGGED_LENGTHS))
def test_reduce_ragged64_matches_autograd(geom, mode):
    lengths_l = ref64.RAGGED_LENGTHS[geom]
    lengths = torch.tensor(lengths_l)
    W, T = 65, sum(lengths_l)
    X = ref64.ragged_inputs(lengths, W, torch.float32).double().requires_grad_(True)
    dY = torch.randn(len(lengths_l), W, generator=_gen(11), dtype=torch.float64)
    want = _ragged_loop(X, lengths_l, mode)
    want.backward(dY)
    out, argmax = ref64.reduce_ragged64(X.detach(), lengths, mode)
    dX = ref64.reduce_ragged_bwd64(dY, lengths, mode, T, argmax)
    assert out.shape == want.shape and dX.shape == X.shape
    assert float((out - want).abs().max()) < 1e-12 if T else not out.any()
    if T:
        assert float((dX - X.grad).abs().max()) < 1e-12
    empty = lengths == 0
    assert not out[empty].any()
    if mode == 2:
        assert bool((argmax[empty] == -1).all())
        off = torch.cumsum(lengths, 0) - lengths
        live = argmax[~empty]
        assert bool((live >= off[~empty, None]).all())
        assert bool((live < (off + lengths)[~empty, None]).all())


def test_reduce_ragged64_first_row_wins_ties():
    X = torch.ones(6, 3)
    out, argmax = ref64.reduce_ragged64(X, torch.tensor([2, 0, 4]), 2)
    assert argmax.tolist() == [[0] * 3, [-1] * 3, [2] * 3]
    assert out.tolist() == [[1.0] * 3, [0.0] * 3, [1.0] * 3]


ACT_SETTINGS = [(0, 1.0, 0.0, float("-inf"), float("inf")),
                (1, 1.0, 0.0, float("-inf"), float("inf")),
                (2, 1.0, 0.0, float("-inf"), float("inf")),
                (3, 1.0, 0.0, 0.0, float("inf")),      # relu
                (3, 0.2, 0.5, 0.0, 1.0),               # hard_sigmoid
                (3, 1.0, 0.0, -1.0, 1.0)]              # hard_tanh


@pytest.mark.parametrize("setting", ACT_SETTINGS, ids=str)
def test_act64_matches_autograd(setting):
    op, slope, offset, lo, hi = setting
    # off the clip boundaries: autograd's clamp passes the gradient there
    x = torch.cat([torch.linspace(-30, 30, 997, dtype=torch.float64),
                   torch.tensor([-100.0, 100.0, 0.3], dtype=torch.float64)])
    x = x.requires_grad_(True)
    if op == 0:
        want = torch.nn.functional.mish(x)
    elif op == 1:
        want = torch.nn.functional.silu(x)
    elif op == 2:
        want = torch.nn.functional.gelu(x)
    else:
        want = torch.clamp(slope * x + offset, min=lo, max=hi)
    want.sum().backward()
    y = ref64.act64(x.detach(), *setting)
    dy = ref64.act_grad64(x.detach(), *setting)
    assert torch.isfinite(y).all() and torch.isfinite(dy).all()
    assert float((y - want).abs().max()) < 1e-12
    assert float((dy - x.grad).abs().max()) < 1e-12
    if op == 3:  # strict inequalities: zero gradient on a boundary
        edges = torch.tensor([(v - offset) / slope for v in (lo, hi)
                              if v not in (float("-inf"), float("inf"))],
                             dtype=torch.float64)
        assert not ref64.act_grad64(edges, *setting).any()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_step64_matches_torch_adamw(wd):
    n, lr, b1, b2, eps, clip = 101, 0.01, 0.9, 0.999, 1e-8, 0.5
    p = torch.randn(n, generator=_gen(12), dtype=torch.float64).requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    master = p.detach().clone()
    m = torch.zeros(n, dtype=torch.float64)
    v = torch.zeros(n, dtype=torch.float64)
    for step in (1, 2, 3):
        grad = torch.randn(n, generator=_gen(12 + step), dtype=torch.float64)
        p.grad = grad * clip
        opt.step()
        master, m, v = ref64.adam_step64(grad, master, m, v, clip, lr, b1, b2, eps,
                                         wd, 1 - b1 ** step, 1 - b2 ** step)
        # torch adds eps after dividing sqrt(v) by sqrt(bc2): the same formula
        assert float((master - p.detach()).abs().max()) < 1e-12
        st = opt.state[p]
        assert float((m - st["exp_avg"]).abs().max()) < 1e-12
        assert float((v - st["exp_avg_sq"]).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_argmax_inputs_have_no_near_tie(dtype):
    """Precondition of the exact ``which`` / ``argmax`` comparisons in
    test_gpu_elementwise_edges.py: nothing may be excluded there."""
    for N, P, W in ref64.MAXOUT_SHAPES:
        X = ref64.maxout_inputs(N, P, W, dtype)
        assert float(ref64.maxout_top2_gap(X).min()) > ref64.ARGMAX_MIN_GAP
    for lengths_l in ref64.RAGGED_LENGTHS.values():
        for W in ref64.RAGGED_WIDTHS:
            X = ref64.ragged_inputs(lengths_l, W, dtype)
            assert X.shape[0] == sum(lengths_l)
            gap = ref64.ragged_top2_gap(X, lengths_l)
            assert float(gap.min()) > ref64.ARGMAX_MIN_GAP
    X = ref64.maxout_inputs(*ref64.MAXOUT_TILE, dtype)
    assert float(ref64.maxout_top2_gap(X).min()) > ref64.ARGMAX_MIN_GAP
    lengths = ref64.ragged_lengths_many(ref64.ragged_many_docs())
    X = ref64.ragged_inputs(lengths, ref64.RAGGED_MANY_W, dtype)
    assert float(ref64.ragged_top2_gap(X, lengths).min()) > ref64.ARGMAX_MIN_GAP


def test_launch_caps_are_read_from_the_bindings():
    caps = ref64.launch_caps()
    assert caps["waves_per_block"] == 4
    assert all(v > 0 for v in caps.values())


def test_ulp_by_dtype_and_check_parity_dtype(capsys):
    assert ref64.fp32_ulp(1.0) == 2.0 ** -23
    assert ref64.fp32_ulp(1.99) == 2.0 ** -23
    assert ref64.fp32_ulp(0.3) == 2.0 ** -25
    assert ref64.fp32_ulp(0.0) == 0.0
    assert float(torch.tensor(1.0) + 2.0 ** -23) == 1.0 + 2.0 ** -23
    ref = torch.ones(4, dtype=torch.float64)
    got = ref + 2.0 ** -10
    ref64.check_parity("default bf16", got, ref, ref)       # within a bf16 ulp
    with pytest.raises(AssertionError):
        ref64.check_parity("fp32", got, ref, ref, dtype=torch.float32)
    ref64.check_parity("fp32", ref + 2.0 ** -23, ref, ref, dtype=torch.float32)
    assert "ulp 1.19e-07" in capsys.readouterr().out
