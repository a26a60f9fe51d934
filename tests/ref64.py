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


# ------------------------------- elementwise, CE and ragged kernel family
def seq2col_bwd64(dY, lengths, residual=None):
    """Gradient of ``seq2col64``: dX[t] = dY[t, W:2W] + the prev-slot of row
    t+1 + the next-slot of row t-1, neither across a doc boundary
    (+ ``residual``)."""
    dY = dY.double()
    T, W = dY.shape[0], dY.shape[1] // 3
    offs = torch.cumsum(lengths.long(), 0)
    is_start = torch.zeros(T, dtype=torch.bool, device=dY.device)
    is_end = torch.zeros(T, dtype=torch.bool, device=dY.device)
    is_start[offs - lengths.long()] = True
    is_end[offs - 1] = True
    dX = dY[:, W:2 * W].clone()
    dX[:-1] += dY[1:, :W].masked_fill(is_start[1:, None], 0)
    dX[1:] += dY[:-1, 2 * W:].masked_fill(is_end[:-1, None], 0)
    return dX if residual is None else dX + residual.double()


def maxout64(X):
    """Pieces-major maxout [N, P, W] -> (Y [N, W], which [N, W] long), the
    first index winning ties."""
    X = X.double()
    best = X[:, 0].detach()
    which = torch.zeros(best.shape, dtype=torch.long, device=X.device)
    for p in range(1, X.shape[1]):
        upd = X[:, p].detach() > best
        which = torch.where(upd, torch.full_like(which, p), which)
        best = torch.where(upd, X[:, p].detach(), best)
    return X.gather(1, which[:, None, :]).squeeze(1), which


def maxout_bwd64(dY, which, P):
    """dX [N, P, W]: dY at piece ``which``, exact zeros elsewhere."""
    dY = dY.double()
    dX = dY.new_zeros(dY.shape[0], P, dY.shape[1])
    return dX.scatter_(1, which.long()[:, None, :], dY[:, None, :])


def layernorm64(X, g, b, eps):
    """(Y, mu [N], rstd [N]) with the biased variance about the mean."""
    X, g, b = X.double(), g.double(), b.double()
    mu = X.mean(-1)
    var = ((X - mu[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (X - mu[:, None]) * rstd[:, None] * g + b, mu, rstd


def layernorm_bwd64(dY, X, g, eps):
    """(dX, dg, db) of ``layernorm64`` at the float64 statistics of X."""
    dY, g = dY.double(), g.double()
    _, mu, rstd = layernorm64(X, g, torch.zeros_like(g), eps)
    xh = (X.double() - mu[:, None]) * rstd[:, None]
    dxh = dY * g
    dX = rstd[:, None] * (dxh - dxh.mean(-1, keepdim=True)
                          - xh * (dxh * xh).mean(-1, keepdim=True))
    return dX, (dY * xh).sum(0), dY.sum(0)


def softmax_ce64(scores, gold):
    """(summed loss, valid-row count, dScores = softmax - onehot) over the
    rows with ``gold >= 0``; an ignored row has a zero dScores row."""
    s = scores.double()
    live = gold >= 0
    m = s.amax(-1, keepdim=True)
    lse = m + torch.log(torch.exp(s - m).sum(-1, keepdim=True))
    logp = s - lse
    g = gold.long().clamp(min=0)[:, None]
    loss = -(logp.gather(1, g)[:, 0] * live).sum()
    d = torch.exp(logp)
    d = d.scatter_add(1, g, -torch.ones_like(g, dtype=d.dtype))
    return loss, int(live.sum()), d * live[:, None]


def _doc_of(lengths, device):
    lengths = lengths.long().to(device)
    return torch.repeat_interleave(
        torch.arange(lengths.numel(), device=device), lengths)


def reduce_ragged64(X, lengths, mode):
    """Ragged sum (0), mean (1) or max (2) of X [T, W] over docs of the given
    lengths -> (out [N, W], argmax [N, W] long for mode 2, else None).  An
    empty doc pools to a zero row in every mode and has argmax -1; the first
    row wins ties."""
    X = X.double()
    T, W = X.shape
    N = lengths.numel()
    lens = lengths.long().to(X.device)
    seg = _doc_of(lengths, X.device)
    if mode < 2:
        out = X.new_zeros(N, W).index_add_(0, seg, X)
        if mode == 1:
            out = out / lens.clamp(min=1)[:, None]
        return out, None
    idx = seg[:, None].expand(T, W)
    mx = X.new_full((N, W), -math.inf).scatter_reduce(
        0, idx, X.detach(), "amax", include_self=True)
    rows = torch.arange(T, device=X.device)[:, None].expand(T, W)
    at_max = X.detach() == mx[seg]
    first = torch.full((N, W), T, dtype=torch.long, device=X.device).scatter_reduce(
        0, idx, torch.where(at_max, rows, T), "amin", include_self=True)
    live = (lens > 0)[:, None].expand(N, W)
    # row T of the padded X is the empty doc's zero row
    out = torch.cat([X, X.new_zeros(1, W)]).gather(0, torch.where(live, first, T))
    return out, torch.where(live, first, -1)


def reduce_ragged_bwd64(dY, lengths, mode, T, argmax=None):
    """dX [T, W] of ``reduce_ragged64``; an empty doc's dY row goes nowhere."""
    dY = dY.double()
    lens = lengths.long().to(dY.device)
    if mode < 2:
        if mode == 1:
            dY = dY / lens.clamp(min=1)[:, None]
        return dY[_doc_of(lengths, dY.device)]
    # row T is a sink for the empty docs' entries
    dX = dY.new_zeros(T + 1, dY.shape[1])
    return dX.scatter_add_(0, torch.where(argmax >= 0, argmax, T), dY)[:T]


ACT_MISH, ACT_SWISH, ACT_GELU, ACT_CLIPPED_LINEAR = 0, 1, 2, 3


def act64(X, op, slope=1.0, offset=0.0, lo=-math.inf, hi=math.inf):
    """mish, swish, erf-gelu or clip(slope * x + offset, lo, hi)."""
    x = X.double()
    if op == ACT_MISH:
        return x * torch.tanh(torch.nn.functional.softplus(x, threshold=700.0))
    if op == ACT_SWISH:
        return x * torch.sigmoid(x)
    if op == ACT_GELU:
        return x * 0.5 * torch.erfc(-x / math.sqrt(2.0))
    return torch.clamp(slope * x + offset, min=lo, max=hi)


def act_grad64(X, op, slope=1.0, offset=0.0, lo=-math.inf, hi=math.inf):
    """d act64 / dx; a clipped-linear boundary point has gradient 0 (strict
    inequalities)."""
    x = X.double()
    if op == ACT_MISH:
        t = torch.tanh(torch.nn.functional.softplus(x, threshold=700.0))
        return t + x * torch.sigmoid(x) * (1 - t * t)
    if op == ACT_SWISH:
        sig = torch.sigmoid(x)
        return sig * (1 + x * (1 - sig))
    if op == ACT_GELU:
        return (0.5 * torch.erfc(-x / math.sqrt(2.0))
                + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi))
    y = slope * x + offset
    return torch.where((y > lo) & (y < hi), torch.full_like(x, slope),
                       torch.zeros_like(x))


def adam_step64(grad, master, m, v, clip, lr, beta1, beta2, eps, wd, bc1, bc2):
    """One Adam step with decoupled weight decay -> (master, m, v):
    g = clip * grad; p = master (1 - lr wd); m, v the usual moments;
    p -= (lr / bc1) m / (sqrt(v / bc2) + eps)."""
    g = grad.double() * clip
    p = master.double() * (1.0 - lr * wd)
    m = beta1 * m.double() + (1.0 - beta1) * g
    v = beta2 * v.double() + (1.0 - beta2) * g * g
    p = p - (lr / bc1) * (m / (torch.sqrt(v / bc2) + eps))
    return p, m, v


# ------------------------------------------------- bf16 error-ratio rule
def bf16_ulp(x):
    """Spacing of bf16 (8 significand bits) at magnitude |x|."""
    x = abs(float(x))
    return 0.0 if x == 0.0 else 2.0 ** (math.floor(math.log2(x)) - 7)


def fp32_ulp(x):
    """Spacing of fp32 (24 significand bits) at magnitude |x|."""
    x = abs(float(x))
    return 0.0 if x == 0.0 else 2.0 ** (math.floor(math.log2(x)) - 23)


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


def check_parity(name, got, base, ref, valid=None, factor=2,
                 dtype=torch.bfloat16):
    """kernel_err <= factor x baseline_err + one ulp of ``dtype`` (bf16 or
    fp32) at max|ref|, for both the max-abs and the RMS error.  ``base`` is
    the same operation done with stock torch ops in that dtype.  Prints the
    figures before asserting."""
    k_max, k_rms, rmax = errs(got, ref, valid)
    b_max, b_rms, _ = errs(base, ref, valid)
    ulp = {torch.bfloat16: bf16_ulp, torch.float32: fp32_ulp}[dtype](rmax)
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


# inputs for the exact argmax comparisons of the elementwise-family tests:
# distinct by construction, so no float64 top-two gap is below 1e-5 (checked
# by test_ref64.py for every shape the GPU tests use)
ARGMAX_MIN_GAP = 1e-5
MAXOUT_SHAPES = [(N, P, W) for N in (1, 17) for P in (1, 2, 3)
                 for W in (8, 50, 96, 128)]
RAGGED_LENGTHS = {
    "plain": [3, 1, 7, 5],
    "empties": [0, 4, 0, 0, 2],
    "trailing_empty": [4, 2, 0],
    "only_empty": [0],
}
RAGGED_WIDTHS = [1, 64, 65, 96]


def maxout_inputs(N, P, W, dtype, seed=0):
    """X [N, P, W] rounded to ``dtype``: a shared value per (n, w) plus
    0.75 x a random cyclic order of the pieces."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.randn(N, 1, W, generator=gen) * 0.5
    shift = torch.randint(0, P, (N, 1, W), generator=gen)
    order = (torch.arange(P)[None, :, None] + shift) % P
    return (r + 0.75 * order).to(dtype)


def maxout_top2_gap(X):
    if X.shape[1] == 1:
        return torch.full(X[:, 0].shape, math.inf, dtype=torch.float64)
    top = X.double().topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def ragged_lengths_many(n_docs, seed=0):
    """Doc lengths 0..3, the first and the last doc empty."""
    gen = torch.Generator().manual_seed(seed)
    lengths = torch.randint(0, 4, (n_docs,), generator=gen)
    lengths[0] = 0
    lengths[-1] = 0
    return lengths


def ragged_inputs(lengths, W, dtype, seed=0):
    """X [T, W] rounded to ``dtype`` for docs of at most 7 rows: 0.75 x
    ((t + a per-column shift) mod 8) plus noise within +-0.3, so the rows of
    one doc differ by at least 0.15 in every column."""
    gen = torch.Generator().manual_seed(seed)
    T = int(torch.as_tensor(lengths).sum())
    assert int(torch.as_tensor(lengths).max()) <= 7
    shift = torch.randint(0, 8, (1, W), generator=gen)
    noise = (torch.randn(T, W, generator=gen) * 0.1).clamp(-0.3, 0.3)
    level = (torch.arange(T)[:, None] + shift) % 8
    return (0.75 * level - 2.0 + noise).to(dtype)


def ragged_top2_gap(X, lengths):
    """Per (doc, column) gap between the two largest rows; inf where the doc
    has fewer than two rows."""
    X = X.double()
    T, W = X.shape
    N = torch.as_tensor(lengths).numel()
    seg = _doc_of(torch.as_tensor(lengths), X.device)
    idx = seg[:, None].expand(T, W)
    top, argmax = reduce_ragged64(X, torch.as_tensor(lengths), 2)
    rows = torch.arange(T)[:, None].expand(T, W)
    rest = X.masked_fill(rows == argmax[seg], -math.inf)
    second = X.new_full((N, W), -math.inf).scatter_reduce(
        0, idx, rest, "amax", include_self=True)
    return torch.where(second > -math.inf, top - second, math.inf)


MAXOUT_TILE = (4096, 2, 8)  # the past-the-cap maxout case repeats this block
RAGGED_MANY_W = 8


def launch_caps():
    """Launch geometry read from the binding sources: threads per block,
    wave size, the block caps of grid_for, layernorm_bwd and softmax_ce, and
    the widest layernorm_bwd row."""
    import os
    import re

    from spacy_ray_amd.ops import api

    kdir = os.path.join(os.path.dirname(api.__file__), "kernels")

    def grab(name, pattern):
        with open(os.path.join(kdir, name)) as f:
            return int(re.search(pattern, f.read()).group(1))

    caps = {
        "block": grab("srx_bind.hip.h", r"constexpr int kBlock = (\d+);"),
        "wave": grab("srx_common.hip.h", r"#define SRX_WAVE (\d+)"),
        "grid": grab("srx_bind.hip.h", r"std::min<long>\(blocks, (\d+)\)"),
        "layernorm_bwd": grab("srx_bind_elementwise.hip", r"long cap = (\d+);"),
        "softmax_ce": grab("srx_bind_elementwise.hip", r"\(N \+ 3\) / 4, (\d+)\)"),
        "adam_per_thread": grab("srx_bind_elementwise.hip",
                                r"adam_step_kernel<scalar_t>\), dim3\(grid_for\(n, (\d+)\)\)"),
        "ln_max_w": grab("srx_elementwise.hip.h", r"#define SRX_LN_MAX_W (\d+)"),
    }
    caps["waves_per_block"] = caps["block"] // caps["wave"]
    caps["threads"] = caps["grid"] * caps["block"]
    return caps


def ragged_many_docs():
    """Document count at which every wave of reduce_ragged's capped grid
    takes at least two documents."""
    caps = launch_caps()
    return 2 * caps["grid"] * caps["waves_per_block"] + 1
