"""Every attn_fused_{fwd,bwd}<DROP,NT> and attn_softmax_{fwd,bwd}<T,DROP>
instantiation (srx_attn.hip.h) against the float64 reference in ref64.py.

bf16 outputs follow the error-ratio rule (ref64.check_parity): the
kernel's max-abs / RMS error against float64 may be at most FACTOR x the
error of the same operation in stock bf16 torch ops, plus one bf16 ulp at
max|ref|.  fp32 outputs use the project's attention tolerances (2e-4
forward, 3x that for gradients).  Measured ratios: docs/KERNELS.md,
"Parity margins"."""
import functools
import math

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"

D = 64
SCALE = D ** -0.5
P_DROP = 0.3
KEEP = 1.0 - P_DROP
SEED = 20240611
FP32_FWD_TOL = 2e-4          # test_window_attention_matches_sdpa's fp32 bound
FP32_BWD_TOL = 3 * FP32_FWD_TOL
FUSED_LS = [32, 20, 64, 50, 96, 70]   # NT = 1, 1, 2, 2, 3, 3
B_F, H_F = 5, 3
SOFTMAX_LS = [5, 64, 100, 130, 256]
# Error-ratio factor: 2 = "different but equally many rounding points".
# Every kernel holds it, so no kernel-specific allowance is named here.
FACTOR_FWD = 2
FACTOR_BWD = 2


def _hip():
    from spacy_ray_amd import _srx_hip

    return _srx_hip


def _fused_lens(L):
    return [L, 1, min(33, L), 0, L - 1]


def _valid_rows(lens, L):
    """[B, 1, L, 1] bool: row index < len."""
    return (torch.arange(L, device=lens.device)[None, None, :, None]
            < lens[:, None, None, None])


@functools.lru_cache(maxsize=None)
def _fused_inputs(L):
    gen = torch.Generator().manual_seed(100 + L)
    q, k, v, dO = (torch.randn(B_F, H_F, L, D, generator=gen)
                   .to(torch.bfloat16).to(DEV) for _ in range(4))
    lens = torch.tensor(_fused_lens(L), dtype=torch.int32, device=DEV)
    return q, k, v, dO, lens


def _flat(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1]).contiguous()


def _ref_fwd_bwd(q, k, v, dO, lens, mask=None, keep=1.0):
    qd, kd, vd = (t.double().requires_grad_(True) for t in (q, k, v))
    O, P, lse = ref64.attn_ref64(qd, kd, vd, lens, SCALE, mask=mask, keep=keep)
    O.backward(dO.double())
    return O.detach(), P.detach(), lse.detach(), qd.grad, kd.grad, vd.grad


def _sdpa_bf16(q, k, v, dO, lens):
    """Baseline without dropout: MATH-backend SDPA in bf16, same mask
    construction as test_window_attention_matches_sdpa."""
    from torch.nn.attention import SDPBackend, sdpa_kernel

    L = q.shape[-2]
    qb, kb, vb = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    with sdpa_kernel([SDPBackend.MATH]):
        O = torch.nn.functional.scaled_dot_product_attention(
            qb, kb, vb, attn_mask=ref64.sdpa_prefix_mask(lens, L), scale=SCALE)
    O.backward(dO * _valid_rows(lens, L))
    return O.detach(), qb.grad, kb.grad, vb.grad


def _composed_bf16(q, k, v, dO, lens, mask, keep):
    """Baseline with an explicit dropout mask: composed bf16
    softmax * M/keep @ V with autograd."""
    L = q.shape[-2]
    qb, kb, vb = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    S = (qb @ kb.transpose(-1, -2)) * SCALE
    S = S.masked_fill(~ref64.sdpa_prefix_mask(lens, L), -math.inf)
    P = torch.softmax(S, dim=-1)
    O = (P * (mask.to(torch.bfloat16) / keep)) @ vb
    O.backward(dO * _valid_rows(lens, L))
    return O.detach(), qb.grad, kb.grad, vb.grad


def _assert_padding_zero(lens, L, **tensors):
    pad = ~_valid_rows(lens, L)
    for name, t in tensors.items():
        t4 = t.view(lens.numel(), -1, L, t.shape[-1])
        assert torch.isfinite(t4.float()).all(), name
        assert float(t4[pad.expand_as(t4)].float().abs().max()) == 0.0, name
        empty = (lens == 0)
        if bool(empty.any()):
            assert float(t4[empty].float().abs().max()) == 0.0, name


# ====================================================== fused, no dropout
@need_gpu
@pytest.mark.parametrize("L", FUSED_LS)
def test_fused_matches_ref64(L):
    hip = _hip()
    q, k, v, dO, lens = _fused_inputs(L)
    qf, kf, vf, dOf = _flat(q), _flat(k), _flat(v), _flat(dO)  # dense dO
    O, lse = hip.attn_fused_fwd(qf, kf, vf, lens, H_F, SCALE, 0.0, 0)
    dQ, dK, dV = hip.attn_fused_bwd(qf, kf, vf, dOf, lse, lens, H_F, SCALE, 0.0, 0)
    rO, _, rlse, rdQ, rdK, rdV = _ref_fwd_bwd(q, k, v, dO, lens)
    bO, bdQ, bdK, bdV = _sdpa_bf16(q, k, v, dO, lens)
    valid = _valid_rows(lens, L)
    shp = q.shape
    d_lse = float((lse.view(B_F, H_F, L).double() - rlse).abs().max())
    print("fused L=%d lse max err %.3e" % (L, d_lse))
    assert d_lse < FP32_FWD_TOL
    ref64.check_parity("fused O L=%d" % L, O.view(shp), bO, rO, valid, FACTOR_FWD)
    for name, got, base, ref in (("dQ", dQ, bdQ, rdQ), ("dK", dK, bdK, rdK),
                                 ("dV", dV, bdV, rdV)):
        ref64.check_parity("fused %s L=%d" % (name, L), got.view(shp), base,
                           ref, valid, FACTOR_BWD)
    _assert_padding_zero(lens, L, O=O, dQ=dQ, dK=dK, dV=dV,
                         lse=lse.unsqueeze(-1))


# ========================================================= fused, dropout
def _recover_pt(L, p, seed):
    """The kernel's own staged bf16 P~ [B, H, L, L]: with V a selector
    (V[j, d] = [j == off + d]) O[i, d] is exactly P~[i, off + d]."""
    hip = _hip()
    q, k, _, _, lens = _fused_inputs(L)
    qf, kf = _flat(q), _flat(k)
    Pt = torch.zeros(B_F * H_F, L, L, device=DEV)
    seen = []
    for off in ([0] + ([32] if L > 64 else [])):
        sel = torch.zeros(L, D, device=DEV)
        n = min(D, L - off)
        sel[off + torch.arange(n), torch.arange(n)] = 1.0
        V = sel.to(torch.bfloat16).expand(B_F * H_F, L, D).contiguous()
        O, _ = hip.attn_fused_fwd(qf, kf, V, lens, H_F, SCALE, p, seed)
        O = O.float()
        assert float(O[:, :, n:].abs().max() if n < D else 0.0) == 0.0
        for lo, hi, old in seen:  # overlapping columns agree
            a, b = max(lo, off), min(hi, off + n)
            assert torch.equal(old[:, :, a - lo:b - lo], O[:, :, a - off:b - off])
        seen.append((off, off + n, O[:, :, :n]))
        Pt[:, :, off:off + n] = O[:, :, :n]
    assert max(hi for _, hi, _ in seen) == L
    return Pt.view(B_F, H_F, L, L)


@functools.lru_cache(maxsize=None)
def _fused_masks(L):
    P0 = _recover_pt(L, 0.0, 0)
    Pt = _recover_pt(L, P_DROP, SEED)
    return P0, Pt, Pt != 0


@need_gpu
@pytest.mark.parametrize("L", FUSED_LS)
def test_fused_dropout_mask(L):
    _, _, _, _, lens = _fused_inputs(L)
    P0, Pt, M = _fused_masks(L)
    vq = _valid_rows(lens, L)
    valid = (vq & vq.transpose(-1, -2)).expand_as(P0)
    # (a) undropped probabilities are > 0 on every valid entry, so
    # "P~ != 0" defines the mask; nothing outside the valid block
    assert bool((P0[valid] > 0).all())
    assert float(P0[~valid].abs().max()) == 0.0
    assert float(Pt[~valid].abs().max()) == 0.0
    # (b) kept entries are P0/keep within two bf16 roundings
    want = P0.double() / KEEP
    rel = ((Pt.double() - want).abs() / want.clamp_min(1e-300))[M]
    print("fused drop L=%d kept rel err %.3e" % (L, float(rel.max())))
    assert float(rel.max()) <= 2.0 ** -7
    # (c) keep fraction
    n = int(valid.sum())
    frac = float(M[valid].double().mean())
    print("fused drop L=%d keep frac %.4f n=%d" % (L, frac, n))
    assert abs(frac - KEEP) <= 4 * math.sqrt(KEEP * (1 - KEEP) / n)
    # (d) determinism / independence
    assert torch.equal(_recover_pt(L, P_DROP, SEED), Pt)
    M2 = _recover_pt(L, P_DROP, SEED + 1) != 0
    assert not torch.equal(M2, M)
    assert abs(float(M2[valid].double().mean()) - KEEP) <= \
        4 * math.sqrt(KEEP * (1 - KEEP) / n)
    assert not torch.equal(M[0, 0], M[0, 1])            # two heads
    a = L - 1                                           # window 4: len L-1
    assert not torch.equal(M[0, 0, :a, :a], M[4, 0, :a, :a])  # two windows
    for w, ln in enumerate(_fused_lens(L)):
        if ln < 64:
            continue
        for r0 in range(0, ln - 3, 4):  # aligned groups of 4 valid rows
            rows = M[w, :, r0:r0 + 4, :ln]
            for i in range(4):
                for j in range(i + 1, 4):
                    same = (rows[:, i] == rows[:, j]).all(-1)
                    assert not bool(same.any()), (w, r0, i, j)


@need_gpu
@pytest.mark.parametrize("L", FUSED_LS)
def test_fused_dropout_matches_ref64(L):
    """(e) forward with the recovered mask, (f) the backward regenerates the
    forward's mask and 1/keep scale."""
    hip = _hip()
    q, k, v, dO, lens = _fused_inputs(L)
    _, _, M = _fused_masks(L)
    qf, kf, vf, dOf = _flat(q), _flat(k), _flat(v), _flat(dO)
    O, lse = hip.attn_fused_fwd(qf, kf, vf, lens, H_F, SCALE, P_DROP, SEED)
    dQ, dK, dV = hip.attn_fused_bwd(qf, kf, vf, dOf, lse, lens, H_F, SCALE,
                                    P_DROP, SEED)
    rO, _, rlse, rdQ, rdK, rdV = _ref_fwd_bwd(q, k, v, dO, lens, M, KEEP)
    bO, bdQ, bdK, bdV = _composed_bf16(q, k, v, dO, lens, M, KEEP)
    valid = _valid_rows(lens, L)
    shp = q.shape
    assert float((lse.view(B_F, H_F, L).double() - rlse).abs().max()) < FP32_FWD_TOL
    ref64.check_parity("fused+drop O L=%d" % L, O.view(shp), bO, rO, valid,
                       FACTOR_FWD)
    for name, got, base, ref in (("dQ", dQ, bdQ, rdQ), ("dK", dK, bdK, rdK),
                                 ("dV", dV, bdV, rdV)):
        ref64.check_parity("fused+drop %s L=%d" % (name, L), got.view(shp),
                           base, ref, valid, FACTOR_BWD)
    _assert_padding_zero(lens, L, O=O, dQ=dQ, dK=dK, dV=dV)


# ===================================================== row-softmax kernels
B_S, H_S = 3, 2


@functools.lru_cache(maxsize=None)
def _softmax_inputs(L, dtype):
    gen = torch.Generator().manual_seed(200 + L)
    S = (torch.randn(B_S * H_S, L, L, generator=gen) / SCALE).to(dtype).to(DEV)
    dPt = torch.randn(B_S * H_S, L, L, generator=gen).to(dtype).to(DEV)
    lens = torch.tensor([L, 1, L // 2 + 1], dtype=torch.int32, device=DEV)
    return S, dPt, lens


def _softmax_ref(S, dPt, lens, heads, mask=None, keep=1.0):
    B = lens.numel()
    L = S.shape[-1]
    Sd = S.double().view(B, heads, L, L).requires_grad_(True)
    Pt, P, lse = ref64.softmax_ref64(Sd, lens, SCALE, mask, keep)
    (Pt * dPt.double().view_as(Pt)).sum().backward()
    return Pt.detach(), P.detach(), lse.detach(), Sd.grad


def _softmax_bf16(S, dPt, lens, heads, mask=None, keep=1.0):
    """Baseline: stock bf16 softmax (* M/keep) with autograd."""
    B = lens.numel()
    L = S.shape[-1]
    Sb = S.detach().clone().view(B, heads, L, L).requires_grad_(True)
    vq = _valid_rows(lens, L)
    Z = (Sb * SCALE).masked_fill(~ref64.sdpa_prefix_mask(lens, L), -math.inf)
    Pt = torch.softmax(Z, dim=-1)
    if mask is not None:
        Pt = Pt * (mask.to(S.dtype) / keep)
    (Pt * (dPt.view_as(Pt) * vq)).sum().backward()
    return Pt.detach(), Sb.grad


def _check_softmax(tag, dtype, got, base, ref, valid, tol):
    if dtype == torch.float32:
        err = float(((got.double() - ref).abs() * valid).max())
        print("softmax fp32 %s max err %.3e" % (tag, err))
        assert err < tol, (tag, err)
    else:
        ref64.check_parity("softmax bf16 " + tag, got, base, ref, valid, 2)


def _run_softmax_case(S, dPt, lens, heads, dtype, tag, p=0.0, seed=0):
    hip = _hip()
    B, L = lens.numel(), S.shape[-1]
    vq = _valid_rows(lens, L)
    valid = (vq & vq.transpose(-1, -2)).expand(B, heads, L, L)
    Pt, lse = hip.attn_softmax_fwd(S, lens, heads, SCALE, p, seed)
    assert Pt.dtype == dtype and lse.dtype == torch.float32
    Pt4 = Pt.view(B, heads, L, L)
    mask = None
    if p > 0:
        P0, _ = hip.attn_softmax_fwd(S, lens, heads, SCALE, 0.0, 0)
        P0 = P0.view_as(Pt4)
        assert bool((P0[valid] > 0).all())
        mask = Pt4 != 0
        want = P0.double() / (1 - p)
        rel = ((Pt4.double() - want).abs() / want.clamp_min(1e-300))[mask]
        print("softmax drop %s kept rel err %.3e" % (tag, float(rel.max())))
        # (b): bf16 two roundings; fp32 the same two roundings at 2^-24
        assert float(rel.max()) <= (2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -22)
        n = int(valid.sum())
        frac = float(mask[valid].double().mean())
        print("softmax drop %s keep frac %.4f n=%d" % (tag, frac, n))
        assert abs(frac - (1 - p)) <= 4 * math.sqrt(p * (1 - p) / n)
        again, _ = hip.attn_softmax_fwd(S, lens, heads, SCALE, p, seed)
        assert torch.equal(again, Pt)
        other, _ = hip.attn_softmax_fwd(S, lens, heads, SCALE, p, seed + 1)
        assert not torch.equal(other != 0, Pt != 0)
    dS = hip.attn_softmax_bwd(S, lse, dPt, lens, heads, SCALE, p, seed)
    rPt, _, rlse, rdS = _softmax_ref(S, dPt, lens, heads, mask, 1 - p)
    bPt, bdS = (None, None)
    if dtype == torch.bfloat16:
        bPt, bdS = _softmax_bf16(S, dPt, lens, heads, mask, 1 - p)
    d_lse = float((lse.view(B, heads, L).double() - rlse).abs().max())
    print("softmax %s lse max err %.3e" % (tag, d_lse))
    assert d_lse < FP32_FWD_TOL
    # dropped P~ is at most 1/keep: the forward bound scales with it
    _check_softmax(tag + " P", dtype, Pt4, bPt, rPt, valid, FP32_FWD_TOL)
    _check_softmax(tag + " dS", dtype, dS.view_as(Pt4), bdS, rdS, valid, FP32_BWD_TOL)
    # padding rows and columns are exactly zero
    assert float(Pt4[~valid].float().abs().max() if (~valid).any() else 0.0) == 0.0
    assert float(dS.view_as(Pt4)[~valid].float().abs().max() if (~valid).any() else 0.0) == 0.0
    assert torch.isfinite(Pt.float()).all() and torch.isfinite(dS.float()).all()


@need_gpu
@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L", SOFTMAX_LS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_row_softmax_matches_ref64(dtype, L, p):
    S, dPt, lens = _softmax_inputs(L, dtype)
    _run_softmax_case(S, dPt, lens, H_S, dtype, "L=%d p=%.1f" % (L, p), p, SEED)


@need_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_row_softmax_grid_stride(dtype):
    """66560 rows: more than the 16384-block x 4-wave grid covers at once."""
    NH, L, heads = 1040, 64, 2
    gen = torch.Generator().manual_seed(7)
    S = (torch.randn(NH, L, L, generator=gen) / SCALE).to(dtype).to(DEV)
    dPt = torch.randn(NH, L, L, generator=gen).to(dtype).to(DEV)
    lens = torch.randint(0, L + 1, (NH // heads,), generator=gen).to(torch.int32)
    lens[:3] = torch.tensor([L, 0, 1], dtype=torch.int32)
    lens[-1] = L  # the rows only the second grid-stride pass reaches
    _run_softmax_case(S, dPt, lens.to(DEV), heads, dtype, "grid-stride")


@need_gpu
def test_row_softmax_rejects_L_over_256():
    hip = _hip()
    S = torch.zeros(2, 257, 257, device=DEV)
    lens = torch.full((1,), 257, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        hip.attn_softmax_fwd(S, lens, 2, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):
        hip.attn_softmax_bwd(S, torch.zeros(2, 257, device=DEV), S, lens, 2,
                             SCALE, 0.0, 0)


@need_gpu
def test_launchers_reject_bad_inputs():
    """The launchers read raw pointers: wrong lens dtype/length, a strided
    operand or an L beyond the fused kernels' LDS layout must raise."""
    hip = _hip()
    q, k, v, dO, lens = _fused_inputs(32)
    qf, kf, vf, dOf = _flat(q), _flat(k), _flat(v), _flat(dO)
    _, lse = hip.attn_fused_fwd(qf, kf, vf, lens, H_F, SCALE, 0.0, 0)
    strided = qf.transpose(0, 1).contiguous().transpose(0, 1)
    assert not strided.is_contiguous()
    for bad in ((qf, strided, vf), (qf, kf, strided)):
        with pytest.raises(RuntimeError):
            hip.attn_fused_fwd(*bad, lens, H_F, SCALE, 0.0, 0)
        with pytest.raises(RuntimeError):
            hip.attn_fused_bwd(*bad, dOf, lse, lens, H_F, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):
        hip.attn_fused_bwd(qf, kf, vf, strided, lse, lens, H_F, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):
        hip.attn_fused_fwd(qf, kf, vf, lens.long(), H_F, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):  # one len per window
        hip.attn_fused_fwd(qf, kf, vf, lens[:-1].contiguous(), H_F, SCALE, 0.0, 0)
    big = torch.zeros(3, 128, D, device=DEV, dtype=torch.bfloat16)
    lens1 = torch.full((1,), 128, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        hip.attn_fused_fwd(big, big, big, lens1, 3, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):
        hip.attn_fused_bwd(big, big, big, big,
                           torch.zeros(3, 128, device=DEV), lens1, 3, SCALE, 0.0, 0)
    S, dPt, slens = _softmax_inputs(64, torch.float32)
    with pytest.raises(RuntimeError):
        hip.attn_softmax_fwd(S, slens.long(), H_S, SCALE, 0.0, 0)
    with pytest.raises(RuntimeError):
        hip.attn_softmax_fwd(S.transpose(1, 2), slens, H_S, SCALE, 0.0, 0)


# ================================================================ dispatch
def _dispatch_inputs(B, L, H=2, seed=300):
    gen = torch.Generator().manual_seed(seed + L + B)
    # [B, L, H, D] transposed to [B, H, L, D]: how the attention interface
    # delivers q/k/v (non-contiguous)
    q, k, v = (torch.randn(B, L, H, D, generator=gen).to(torch.bfloat16)
               .to(DEV).transpose(1, 2) for _ in range(3))
    dO = torch.randn(B, H, L, D, generator=gen).to(torch.bfloat16).to(DEV)
    lens = torch.tensor([L, 1, L // 2 + 1][:B], dtype=torch.int32, device=DEV)
    return q, k, v, dO, lens


def _api_fwd_bwd(q, k, v, dO, lens):
    from spacy_ray_amd.ops import api

    qa, ka, va = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = api.window_attention(qa, ka, va, lens, SCALE, 0.0)
    out.backward(dO)
    return out.detach(), qa.grad, ka.grad, va.grad


@need_gpu
@pytest.mark.parametrize("L", [64, 128], ids=["fused", "bmm"])
def test_window_attention_dispatch(L):
    hip = _hip()
    B, H = 3, 2
    q, k, v, dO, lens = _dispatch_inputs(B, L)
    assert not q.is_contiguous()
    out, gq, gk, gv = _api_fwd_bwd(q, k, v, dO, lens)
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    # the route taken: bit-identical to calling that path's kernels directly
    qf, kf, vf = _flat(qc), _flat(kc), _flat(vc)
    if L <= 96:
        want, _ = hip.attn_fused_fwd(qf, kf, vf, lens, H, SCALE, 0.0, 0)
    else:
        S = torch.bmm(qf, kf.transpose(1, 2))
        P, _ = hip.attn_softmax_fwd(S, lens, H, SCALE, 0.0, 0)
        want = torch.bmm(P, vf)
    assert torch.equal(out, want.view_as(out))
    # numerics, forward and backward
    rO, _, _, rdQ, rdK, rdV = _ref_fwd_bwd(qc, kc, vc, dO, lens)
    bO, bdQ, bdK, bdV = _sdpa_bf16(qc, kc, vc, dO, lens)
    valid = _valid_rows(lens, L)
    for name, got, base, ref, f in (
            ("O", out, bO, rO, FACTOR_FWD), ("dQ", gq, bdQ, rdQ, FACTOR_BWD),
            ("dK", gk, bdK, rdK, FACTOR_BWD), ("dV", gv, bdV, rdV, FACTOR_BWD)):
        ref64.check_parity("api %s L=%d" % (name, L), got, base, ref, valid, f)
    _assert_padding_zero(lens, L, O=_flat(out), dQ=_flat(gq), dK=_flat(gk),
                         dV=_flat(gv))


@need_gpu
@pytest.mark.parametrize("B", [3, 1])
@pytest.mark.parametrize("L", [64, 128], ids=["fused", "bmm"])
def test_window_attention_noncontiguous_inputs(L, B):
    """Transposed [B, L, H, D] inputs give the same result as contiguous
    copies.  B == 1 matters: there reshape(B*H, L, D) is a strided VIEW,
    not a copy."""
    q, k, v, dO, lens = _dispatch_inputs(B, L)
    assert not q.is_contiguous()
    got = _api_fwd_bwd(q, k, v, dO, lens)
    want = _api_fwd_bwd(q.contiguous(), k.contiguous(), v.contiguous(), dO, lens)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    # mixed: only one operand strided
    got = _api_fwd_bwd(q.contiguous(), k, v.contiguous(), dO, lens)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
