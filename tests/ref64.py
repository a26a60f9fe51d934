"""Float64 references for the hand-written MFMA kernel families, plus the
error-ratio rule the GPU parity tests use for bf16 outputs.

Plain torch, differentiable, device-agnostic.  Inputs are upcast from the
exact values a kernel sees (pass the bf16 tensors, not their fp32
originals).  Validated on the CPU by ``test_ref64.py``.
"""
import math

import torch


# ------------------------------------------------------------- attention
def softmax_ref64(S, lens, scale, mask=None, keep=1.0):
    """Prefix-masked row softmax of the RAW scores ``S`` [B, H, L, L].

    Query rows ``i >= len`` give P = 0 and lse = 0; key columns
    ``j >= len`` are excluded.  Returns ``(Pt, P, lse)`` where
    ``Pt = P * mask / keep`` (== P without a mask)."""
    S = S.double()
    L = S.shape[-1]
    j = torch.arange(L, device=S.device)
    inside = j[None, :] < lens.to(S.device).long()[:, None]          # [B, L]
    qv = inside[:, None, :, None]
    valid = qv & inside[:, None, None, :]                            # [B,1,L,L]
    z = torch.where(valid, scale * S, torch.zeros_like(S))
    m = torch.where(valid, z, torch.full_like(S, -math.inf)).amax(-1, keepdim=True)
    m = torch.where(qv, m, torch.zeros_like(m)).detach()
    e = torch.where(valid, torch.exp(z - m), torch.zeros_like(S))
    s = e.sum(-1, keepdim=True)
    s1 = torch.where(qv, s, torch.ones_like(s))
    P = e / s1
    lse = torch.where(qv, m + torch.log(s1), torch.zeros_like(s)).squeeze(-1)
    Pt = P if mask is None else P * mask.double() / keep
    return Pt, P, lse


def attn_ref64(q, k, v, lens, scale, mask=None, keep=1.0):
    """q/k/v [B, H, L, D], lens [B].  Returns ``(O, P, lse)``: P is the
    normalised (undropped) probability, the optional explicit dropout
    multiplier ``mask / keep`` is applied after normalisation."""
    q, k, v = q.double(), k.double(), v.double()
    Pt, P, lse = softmax_ref64(q @ k.transpose(-1, -2), lens, scale, mask, keep)
    return Pt @ v, P, lse


def sdpa_prefix_mask(lens, L):
    """The boolean mask of ``test_window_attention_matches_sdpa``: valid
    queries see the valid prefix, padding queries attend position 0 only
    (a well-defined softmax; those rows are excluded from comparisons)."""
    j = torch.arange(L, device=lens.device)
    qvalid = j[:, None] < lens[:, None, None]
    kvalid = j[None, None, :] < lens[:, None, None]
    return torch.where(qvalid, kvalid, (j[None, None, :] == 0)).unsqueeze(1)


# ------------------------------------------------------------------- MWE
def seq2col64(X, lengths):
    T, W = X.shape
    offs = torch.cumsum(lengths.long(), 0)
    is_start = torch.zeros(T, dtype=torch.bool, device=X.device)
    is_end = torch.zeros(T, dtype=torch.bool, device=X.device)
    is_start[offs - lengths.long()] = True
    is_end[offs - 1] = True
    zero = X.new_zeros(1, W)
    prev = torch.cat([zero, X[:-1]]).masked_fill(is_start[:, None], 0)
    nxt = torch.cat([X[1:], zero]).masked_fill(is_end[:, None], 0)
    return torch.cat([prev, X, nxt], dim=1)


def mwe_ref64(X, Wt, bias, g, b, lengths, eps, mask=None):
    """Y = X + mask * LayerNorm(maxout_3(seq2col(X) @ Wt^T + bias)) in
    float64 (pieces-major pre-activations, first index wins ties).
    Returns ``(Y, M, which, mu, rstd, pre)`` with pre [T, 3, W]."""
    X, Wt, bias, g, b = (t.double() for t in (X, Wt, bias, g, b))
    T, W = X.shape
    pre = (seq2col64(X, lengths) @ Wt.t() + bias).view(T, 3, W)
    which = torch.zeros(T, W, dtype=torch.long, device=X.device)
    best = pre[:, 0].detach()
    for p in (1, 2):
        upd = pre[:, p].detach() > best
        which = torch.where(upd, torch.full_like(which, p), which)
        best = torch.where(upd, pre[:, p].detach(), best)
    M = pre.gather(1, which[:, None, :]).squeeze(1)
    mu = M.mean(-1)
    var = ((M - mu[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    ln = (M - mu[:, None]) * rstd[:, None] * g + b
    if mask is not None:
        ln = ln * mask.double()
    return X + ln, M, which, mu, rstd, pre


def mwe_stage1_ref64(dY, mask, Mout, g, mu, rstd, which):
    """LayerNorm backward over the saved (Mout, mu, rstd) + maxout scatter
    and the dg/db/dbias column sums, in float64 from the given inputs.
    Returns ``(dPre [N, 3W], dg, db, dbias [3W], partials)``; ``partials``
    holds, per column and in the same order, the largest |running sum| when
    the rows are added in order — the magnitude at which an fp32
    accumulation of that column rounds."""
    dY, Mout, g = dY.double(), Mout.double(), g.double()
    mu, rstd = mu.double()[:, None], rstd.double()[:, None]
    d = dY if mask is None else dY * mask.double()
    xh = (Mout - mu) * rstd
    dxh = d * g
    dM = rstd * (dxh - dxh.mean(-1, keepdim=True)
                 - xh * (dxh * xh).mean(-1, keepdim=True))
    N, W = dY.shape
    dPre = dM.new_zeros(N, 3, W)
    dPre.scatter_(1, which.long()[:, None, :], dM[:, None, :])
    partials = tuple(t.cumsum(0).abs().amax(0).reshape(-1)
                     for t in (d * xh, d, dPre))
    return (dPre.view(N, 3 * W), (d * xh).sum(0), d.sum(0),
            dPre.sum(0).reshape(3 * W), partials)


# ------------------------------------------------- bf16 error-ratio rule
def bf16_ulp(x):
    """Spacing of bf16 (8 significand bits) at magnitude |x|."""
    x = abs(float(x))
    return 0.0 if x == 0.0 else 2.0 ** (math.floor(math.log2(x)) - 7)


def errs(got, ref, valid=None):
    """(max-abs, RMS) error of ``got`` against the float64 ``ref`` over the
    ``valid`` entries (broadcastable bool), plus max|ref| there."""
    d = (got.double() - ref).abs()
    r = ref.abs()
    if valid is not None:
        valid = valid.expand_as(d)
        d, r = d[valid], r[valid]
    if d.numel() == 0:
        return 0.0, 0.0, 0.0
    return float(d.max()), float(d.pow(2).mean().sqrt()), float(r.max())


def check_parity(name, got, base, ref, valid=None, factor=2):
    """kernel_err <= factor x baseline_err + one bf16 ulp at max|ref|, for
    both the max-abs and the RMS error.  ``base`` is the same operation done
    with stock torch ops in bf16.  Prints the figures before asserting."""
    k_max, k_rms, rmax = errs(got, ref, valid)
    b_max, b_rms, _ = errs(base, ref, valid)
    ulp = bf16_ulp(rmax)
    line = ("parity %-28s max %.3e / base %.3e (x%.2f)  rms %.3e / base %.3e "
            "(x%.2f)  ulp %.2e" % (
                name, k_max, b_max, k_max / b_max if b_max else float("nan"),
                k_rms, b_rms, k_rms / b_rms if b_rms else float("nan"), ulp))
    print(line)
    assert math.isfinite(k_max) and math.isfinite(k_rms), line
    assert k_max <= factor * b_max + ulp, line
    assert k_rms <= factor * b_rms + ulp, line


# ------------------------------------------- shared deterministic inputs
MWE_GEOMETRIES = {
    "edge": [64, 64],              # doc boundary exactly on the tile edge
    "span": [40, 50, 38],          # a doc spanning the tile edge
    "single": [1] * 64 + [64],     # single-token docs: start == end row
    "interior": [192],             # middle tile has no boundary at all
    "one_tile": [64],
}

# test_mwe_layer_grads_match_ref64: a seed whose float64 pre-activations have
# no top-two gap below 1e-5 at W = 96 and 128 (checked by test_ref64.py)
MWE_GRAD_LENGTHS = [30, 2, 64, 17, 15]
MWE_GRAD_SEED = 22


def mwe_inputs(W, lengths, with_mask, seed=0, dtype=torch.bfloat16):
    """CPU-generated (device-independent) MWE layer inputs, already rounded
    to ``dtype``: X, Wt, bias, g, b, lengths, mask (0 or 1/0.9, or None)."""
    gen = torch.Generator().manual_seed(seed)
    T = int(sum(lengths))
    X = (torch.randn(T, W, generator=gen) * 0.5).to(dtype)
    Wt = (torch.randn(3 * W, 3 * W, generator=gen) / math.sqrt(3 * W)).to(dtype)
    bias = (torch.randn(3 * W, generator=gen) * 0.1).to(dtype)
    g = (1 + 0.1 * torch.randn(W, generator=gen)).to(dtype)
    b = (0.1 * torch.randn(W, generator=gen)).to(dtype)
    mask = None
    if with_mask:
        mask = ((torch.rand(T, W, generator=gen) < 0.9).float() / 0.9).to(dtype)
    return X, Wt, bias, g, b, torch.tensor(lengths), mask


def top2_gap(pre):
    """Gap between the two largest of the 3 pre-activations, [T, W]."""
    top = pre.detach().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]
