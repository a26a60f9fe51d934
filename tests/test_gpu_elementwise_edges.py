"""Edge-shape parity of the elementwise, softmax-CE and ragged kernels (the
family bound in srx_bind_elementwise.hip) against the float64 references in
ref64.py.

Rule for every numeric comparison (ref64.check_parity): kernel error <= 2 x
the error of the same operation done with stock torch ops in the same dtype
on the same device, plus one ulp of that dtype at max|ref|, on both max-abs
and RMS.  Copies, maxima, argmax indices and zeroed rows are compared with
torch.equal; no index is excluded (test_ref64.py checks that the inputs
carry no near-tie).  Row counts of the grid-stride cases come from the block
caps read in the binding sources (ref64.launch_caps), so that every wave, or
every thread, takes at least two items.  Inputs are generated on the CPU,
rounded to the dtype, and valid by construction."""
import functools
import math

import pytest
import torch

import ref64
from spacy_ray_amd.ops import api
from spacy_ray_amd.ops import torch_ref as tref

if torch.cuda.is_available():
    from spacy_ray_amd import _srx_hip

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-5
INF = float("inf")
dt_id = lambda v: str(v).replace("torch.", "")  # noqa: E731


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, dtype, seed, scale=1.0):
    return (torch.randn(shape, generator=gen(seed)) * scale).to(dtype).to(DEV)


def parity(name, got, base, ref, dtype, valid=None):
    ref64.check_parity(name, got, base, ref, valid, 2, dtype)


@functools.lru_cache(maxsize=1)
def caps():
    return ref64.launch_caps()


def kvec(dtype):
    return 8 if dtype == torch.bfloat16 else 4


# --------------------------------------------------------------- seq2col
def seq2col_check(tag, X, dY, res, lengths, dtype):
    T, W = X.shape
    starts, ends = api.boundary_masks_u8(lengths, T)
    Y = _srx_hip.seq2col_fwd(X, starts, ends)
    assert torch.equal(Y, ref64.seq2col64(X, lengths).to(dtype)), tag
    for residual in (None, res):
        dX = _srx_hip.seq2col_bwd(dY, starts, ends, residual)
        base = tref.seq2col_backward(dY, lengths)
        if residual is not None:
            base = base + residual
        parity("seq2col_bwd %s res=%d" % (tag, residual is not None), dX, base,
               ref64.seq2col_bwd64(dY, lengths, residual), dtype)
    return Y


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", [8, 12, 96, 100])
@pytest.mark.parametrize("lengths_l", [[1], [1, 1, 1], [5, 1, 9, 3], [300]], ids=str)
def test_seq2col_edges(lengths_l, W, dtype):
    T = sum(lengths_l)
    lengths = torch.tensor(lengths_l, device=DEV)
    X = randn((T, W), dtype, 0)
    dY = randn((T, 3 * W), dtype, 1)
    res = randn((T, W), dtype, 2)
    tag = "%s W=%d %s" % (dt_id(dtype), W, lengths_l)
    seq2col_check(tag, X, dY, res, lengths, dtype)
    # through autograd
    x = X.clone().requires_grad_(True)
    y = api.seq2col(x, lengths)
    y.backward(dY)
    assert torch.equal(y, ref64.seq2col64(X, lengths).to(dtype))
    parity("api.seq2col grad " + tag, x.grad, tref.seq2col_backward(dY, lengths),
           ref64.seq2col_bwd64(dY, lengths), dtype)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_seq2col_past_the_grid_cap(dtype):
    """Backward items = T * W / kVec: twice the capped grid's threads, so
    every thread loops twice (the forward has three times as many)."""
    W = 8
    reps = 2 * caps()["threads"] // (W // kvec(dtype)) // 18 + 1
    lengths = torch.tensor([5, 1, 9, 3], device=DEV).repeat(reps)
    T = 18 * reps
    assert T * (W // kvec(dtype)) >= 2 * caps()["threads"]
    X = randn((18 * 64, W), dtype, 3).repeat(reps // 64 + 1, 1)[:T].contiguous()
    dY = randn((18 * 64, 3 * W), dtype, 4).repeat(reps // 64 + 1, 1)[:T].contiguous()
    res = randn((18 * 64, W), dtype, 5).repeat(reps // 64 + 1, 1)[:T].contiguous()
    seq2col_check("%s T=%d" % (dt_id(dtype), T), X, dY, res, lengths, dtype)


# ---------------------------------------------------------------- maxout
def maxout_check(tag, X, dY, dtype):
    N, P, W = X.shape
    Y, which = _srx_hip.maxout_fwd(X)
    rY, rwhich = ref64.maxout64(X)
    assert torch.equal(Y, rY.to(dtype)), tag
    assert torch.equal(which.long(), rwhich), tag
    dX = _srx_hip.maxout_bwd(dY, which, P)
    assert torch.equal(dX, ref64.maxout_bwd64(dY, rwhich, P).to(dtype)), tag


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("N,P,W", ref64.MAXOUT_SHAPES)
def test_maxout_edges(N, P, W, dtype):
    X = ref64.maxout_inputs(N, P, W, dtype).to(DEV)
    dY = randn((N, W), dtype, 6)
    tag = "%s N=%d P=%d W=%d" % (dt_id(dtype), N, P, W)
    maxout_check(tag, X, dY, dtype)
    x = X.clone().requires_grad_(True)
    y = api.maxout(x)
    y.backward(dY)
    rY, rwhich = ref64.maxout64(X)
    assert torch.equal(y, rY.to(dtype))
    assert torch.equal(x.grad, ref64.maxout_bwd64(dY, rwhich, P).to(dtype))


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_maxout_exact_ties_go_to_the_first_piece(dtype):
    X = (torch.randint(-2, 3, (17, 3, 96), generator=gen(7)) / 2).to(dtype).to(DEV)
    maxout_check("ties " + dt_id(dtype), X, randn((17, 96), dtype, 8), dtype)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_maxout_past_the_grid_cap(dtype):
    """Forward items = N * W / kVec: twice the capped grid's threads."""
    n0, P, W = ref64.MAXOUT_TILE
    N = 2 * caps()["threads"] // (W // kvec(dtype)) + 1
    block = ref64.maxout_inputs(n0, P, W, dtype).to(DEV)
    X = block.repeat(N // n0 + 1, 1, 1)[:N].contiguous()
    dY = randn((n0, W), dtype, 9).repeat(N // n0 + 1, 1)[:N].contiguous()
    maxout_check("%s N=%d" % (dt_id(dtype), N), X, dY, dtype)


# ------------------------------------------------------------- layernorm
LN_WIDTHS = [1, 63, 64, 65, 96, 128, 300, 768, 1000, 1024]


def ln_inputs(N, W, dtype, means, seed=10, const_row=None):
    """Rows of std 1 about the given means (cycled); row ``const_row`` is the
    constant 2.0, whose sums are exact in fp32."""
    X = torch.randn(N, W, generator=gen(seed))
    X = X + torch.tensor(means)[torch.arange(N) % len(means)][:, None]
    if const_row is not None:
        X[const_row] = 2.0
    g = 1 + 0.1 * torch.randn(W, generator=gen(seed + 1))
    b = 0.1 * torch.randn(W, generator=gen(seed + 2))
    dY = torch.randn(N, W, generator=gen(seed + 3))
    return tuple(t.to(dtype).to(DEV) for t in (X, g, b, dY))


def torch_layernorm(X, g, b, dY):
    """Stock torch in the inputs' dtype: (Y, mu, rstd, dX, dg, db)."""
    W = X.shape[-1]
    x, gg, bb = (t.clone().requires_grad_(True) for t in (X, g, b))
    torch.nn.functional.layer_norm(x, (W,), gg, bb, EPS).backward(dY)
    Y, mu, rstd = torch.native_layer_norm(X, (W,), g, b, EPS)
    return Y, mu.reshape(-1), rstd.reshape(-1), x.grad, gg.grad, bb.grad


def layernorm_check(tag, X, g, b, dY, dtype):
    bY, bmu, brstd, bdX, bdg, bdb = torch_layernorm(X, g, b, dY)
    rY, rmu, rrstd = ref64.layernorm64(X, g, b, EPS)
    rdX, rdg, rdb = ref64.layernorm_bwd64(dY, X, g, EPS)
    Y, mu, rstd = _srx_hip.layernorm_fwd(X, g, b, EPS)
    parity("ln Y " + tag, Y, bY, rY, dtype)
    # mu / rstd are held to the dtype of the row, as the rule says ("the same
    # operation in the same dtype"): for bf16 rows the check is only
    # bf16-tight on purpose.  The bf16 kernels keep the one-pass fp32
    # variance, whose rstd is off by ~6e-5 at mean 30: far inside what the
    # bf16 output shows, and outside an fp32 ulp.
    parity("ln mu " + tag, mu, bmu, rmu, dtype)
    parity("ln rstd " + tag, rstd, brstd, rrstd, dtype)
    for det in (False, True):
        dX, dg, db = _srx_hip.layernorm_bwd(dY, X, g, mu, rstd, det)
        mode = " det=%d " % det
        parity("ln dX" + mode + tag, dX, bdX, rdX, dtype)
        parity("ln dg" + mode + tag, dg, bdg, rdg, dtype)
        parity("ln db" + mode + tag, db, bdb, rdb, dtype)
        if det:
            again = _srx_hip.layernorm_bwd(dY, X, g, mu, rstd, True)
            assert all(torch.equal(a, c) for a, c in zip((dX, dg, db), again)), tag
    return Y


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", LN_WIDTHS)
def test_layernorm_edges(W, dtype):
    for N in (1, 257):
        for mean in (0.0, 8.0, 30.0):
            X, g, b, dY = ln_inputs(N, W, dtype, [mean])
            layernorm_check("%s N=%d W=%d mean=%g" % (dt_id(dtype), N, W, mean),
                            X, g, b, dY, dtype)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", [63, 96, 128, 1024])
def test_layernorm_constant_row_gives_b(W, dtype):
    X, g, b, dY = ln_inputs(9, W, dtype, [0.0, 8.0, 30.0], const_row=4)
    Y = layernorm_check("%s const W=%d" % (dt_id(dtype), W), X, g, b, dY, dtype)
    assert torch.equal(Y[4], b)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", [96, 128])
def test_layernorm_past_the_grid_caps(W, dtype):
    """Two rows or more for every wave of the forward's capped grid, and
    more still for the backward's smaller one: dg / db accumulate over
    several rows in each wave's registers."""
    c = caps()
    N = 2 * max(c["grid"], c["layernorm_bwd"]) * c["waves_per_block"] + 1
    X, g, b, dY = ln_inputs(N, W, dtype, [0.0, 8.0, 30.0])
    layernorm_check("%s N=%d W=%d" % (dt_id(dtype), N, W), X, g, b, dY, dtype)


@need_gpu
def test_layernorm_bwd_rejects_a_row_wider_than_its_registers():
    W = caps()["ln_max_w"] + 1
    X, g, b, dY = ln_inputs(2, W, torch.float32, [0.0])
    Y, mu, rstd = _srx_hip.layernorm_fwd(X, g, b, EPS)
    with pytest.raises(RuntimeError, match="layernorm width"):
        _srx_hip.layernorm_bwd(dY, X, g, mu, rstd)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", [96, 128])
def test_add_layernorm_autograd(W, dtype, monkeypatch):
    monkeypatch.delenv("SRX_DETERMINISTIC", raising=False)
    N = 257
    X, g, b, dY = ln_inputs(N, W, dtype, [0.0, 8.0, 30.0])
    R = randn((N, W), dtype, 20)
    S = X + R
    leaves = [t.clone().requires_grad_(True) for t in (X, R, g, b)]
    Y = api.add_layernorm(*leaves, EPS)
    Y.backward(dY)
    bY, _, _, bdS, bdg, bdb = torch_layernorm(S, g, b, dY)
    rY = ref64.layernorm64(S, g, b, EPS)[0]
    rdS, rdg, rdb = ref64.layernorm_bwd64(dY, S, g, EPS)
    tag = " add_layernorm %s W=%d" % (dt_id(dtype), W)
    parity("Y" + tag, Y.detach(), bY, rY, dtype)
    assert torch.equal(leaves[0].grad, leaves[1].grad)
    parity("dX" + tag, leaves[0].grad, bdS, rdS, dtype)
    parity("dg" + tag, leaves[2].grad, bdg, rdg, dtype)
    parity("db" + tag, leaves[3].grad, bdb, rdb, dtype)
    # and the plain wrapper
    leaves = [t.clone().requires_grad_(True) for t in (S, g, b)]
    api.layernorm(*leaves, EPS).backward(dY)
    parity("dX layernorm" + tag, leaves[0].grad, bdS, rdS, dtype)


# ------------------------------------------------------------ softmax_ce
def ce_inputs(N, C, dtype, scale, seed=30):
    """Every 7th row ignored; rows [N/2, N/2 + N/4) have a gold logit 30
    above the rest (an fp32 loss of exactly 0)."""
    s = torch.randn(N, C, generator=gen(seed)) * scale
    gold = torch.randint(0, C, (N,), generator=gen(seed + 1))
    sure = torch.arange(N // 2, N // 2 + N // 4)
    if C > 1:
        s[sure] = s[sure].clamp(-2, 2)
        s[sure, gold[sure]] = 32.0
    gold[::7] = -1 if N > 1 else gold[0]
    return s.to(dtype).to(DEV), gold.to(DEV)


def torch_ce(scores, gold):
    """Stock torch in the scores' dtype: (summed loss, dScores)."""
    live = gold >= 0
    g = gold.clamp(min=0)[:, None]
    logp = torch.log_softmax(scores, -1)
    loss = -(logp.gather(1, g)[:, 0] * live).sum()
    d = torch.softmax(scores, -1)
    d = d.scatter_add(1, g, -torch.ones_like(g, dtype=d.dtype))
    return loss, d * live[:, None]


def ce_check(tag, scores, gold, dtype):
    out, d = _srx_hip.softmax_ce(scores, gold)
    rloss, rcount, rd = ref64.softmax_ce64(scores, gold)
    bloss, bd = torch_ce(scores, gold)
    assert out.dtype == torch.float32
    assert float(out[1]) == rcount == int((gold >= 0).sum()), tag
    # the loss is an fp32 result whatever the scores' dtype
    bloss32 = torch_ce(scores.float(), gold)[0]
    parity("ce loss " + tag, out[0].reshape(1), bloss32.reshape(1),
           rloss.reshape(1), torch.float32)
    parity("ce dScores " + tag, d, bd, rd, dtype)
    assert not d[gold < 0].any(), tag
    assert torch.isfinite(d).all(), tag
    return out, d


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 300])
def test_softmax_ce_edges(C, scale, dtype):
    for N in (1, 513):
        scores, gold = ce_inputs(N, C, dtype, scale)
        tag = "%s N=%d C=%d x%g" % (dt_id(dtype), N, C, scale)
        ce_check(tag, scores, gold, dtype)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("C", [1, 64, 65])
def test_softmax_ce_counts_rows_whose_loss_is_exactly_zero(C, dtype):
    """Each of the rows below has an fp32 loss of exactly 0.0 (one class, or
    a gold logit 30 above the rest): with a wave per row the wave's summed
    loss is 0 and its row must still reach the valid count."""
    N = 64
    s = torch.randn(N, C, generator=gen(32)).clamp(-2, 2)
    gold = torch.randint(0, C, (N,), generator=gen(33))
    s[torch.arange(N), gold] = 32.0 if C > 1 else 0.5
    gold[::5] = -1
    scores, gold = s.to(dtype).to(DEV), gold.to(DEV)
    out, d = ce_check("zero-loss %s C=%d" % (dt_id(dtype), C), scores, gold, dtype)
    assert float(out[0]) == 0.0
    assert float(out[1]) == float((gold >= 0).sum())


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_softmax_ce_all_ignored(dtype):
    scores, gold = ce_inputs(513, 65, dtype, 1.0)
    gold = torch.full_like(gold, -1)
    out, d = _srx_hip.softmax_ce(scores, gold)
    assert out.tolist() == [0.0, 0.0]
    assert not d.any()


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_softmax_ce_past_the_grid_cap_and_autograd(dtype):
    c = caps()
    N = 2 * c["softmax_ce"] * c["waves_per_block"] + 1
    scores, gold = ce_inputs(N, 65, dtype, 1.0)
    tag = "%s N=%d C=65" % (dt_id(dtype), N)
    out, d = ce_check(tag, scores, gold, dtype)
    s = scores.clone().requires_grad_(True)
    loss = api.softmax_ce_loss(s, gold)
    loss.backward()
    # a second launch: the atomics may arrive in another order, so the
    # wrapper's loss is held to the rule, not to the first call's bits
    parity("api ce loss " + tag, loss.detach().reshape(1),
           torch_ce(scores.float(), gold)[0].reshape(1),
           ref64.softmax_ce64(scores, gold)[0].reshape(1), torch.float32)
    assert torch.equal(s.grad, d)


# --------------------------------------------------------- reduce_ragged
def ragged_check(tag, X, lengths, dtype):
    T, W = X.shape
    N = lengths.numel()
    offsets, doc_of = api._offsets_and_docof(lengths)
    dY = randn((N, W), dtype, 40)
    empty = (lengths == 0)
    for mode, base_fn in ((0, tref.reduce_sum_ragged), (1, tref.reduce_mean_ragged)):
        out, _ = _srx_hip.reduce_ragged(X, offsets, mode)
        rout, _ = ref64.reduce_ragged64(X, lengths, mode)
        parity("ragged mode=%d %s" % (mode, tag), out, base_fn(X, lengths), rout, dtype)
        assert not out[empty].any(), tag
        dX = _srx_hip.reduce_ragged_bwd(dY, doc_of, offsets, T, mode)
        rdX = ref64.reduce_ragged_bwd64(dY, lengths, mode, T)
        if mode == 0:
            assert torch.equal(dX, rdX.to(dtype)), tag
        else:
            base = (dY / lengths.clamp(min=1)[:, None].to(dtype))[doc_of.long()]
            parity("ragged_bwd mode=1 " + tag, dX, base, rdX, dtype)
    out, argmax = _srx_hip.reduce_ragged(X, offsets, 2)
    rout, rargmax = ref64.reduce_ragged64(X, lengths, 2)
    assert torch.equal(out, rout.to(dtype)), tag
    assert torch.equal(argmax.long(), rargmax), tag
    assert not out[empty].any() and bool((argmax[empty] == -1).all()), tag
    dX = _srx_hip.reduce_max_bwd(dY, argmax, T)
    assert torch.equal(dX, ref64.reduce_ragged_bwd64(dY, lengths, 2, T, rargmax).to(dtype)), tag
    return dY


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("W", ref64.RAGGED_WIDTHS)
@pytest.mark.parametrize("geom", sorted(ref64.RAGGED_LENGTHS))
def test_reduce_ragged_edges(geom, W, dtype):
    lengths_l = ref64.RAGGED_LENGTHS[geom]
    lengths = torch.tensor(lengths_l, device=DEV)
    X = ref64.ragged_inputs(lengths_l, W, dtype).to(DEV)
    tag = "%s W=%d %s" % (dt_id(dtype), W, lengths_l)
    dY = ragged_check(tag, X, lengths, dtype)
    T = X.shape[0]
    wrappers = (api.reduce_sum_ragged, api.reduce_mean_ragged, api.reduce_max_ragged)
    for mode, fn in enumerate(wrappers):
        x = X.clone().requires_grad_(True)
        out = fn(x, lengths)
        out.backward(dY)
        rout, rargmax = ref64.reduce_ragged64(X, lengths, mode)
        rdX = ref64.reduce_ragged_bwd64(dY, lengths, mode, T, rargmax)
        if mode == 1:
            base = (dY / lengths.clamp(min=1)[:, None].to(dtype))[
                api._offsets_and_docof(lengths)[1].long()]
            parity("api ragged_bwd mode=1 " + tag, x.grad, base, rdX, dtype)
        else:
            assert torch.equal(x.grad, rdX.to(dtype)), (tag, mode)
        if mode == 2:
            assert torch.equal(out.detach(), rout.to(dtype))


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_reduce_ragged_past_the_grid_cap(dtype):
    """Two documents or more, of 0 to 3 rows, for every wave."""
    lengths = ref64.ragged_lengths_many(ref64.ragged_many_docs())
    X = ref64.ragged_inputs(lengths, ref64.RAGGED_MANY_W, dtype).to(DEV)
    ragged_check("%s docs=%d" % (dt_id(dtype), lengths.numel()), X,
                 lengths.to(DEV), dtype)


# ----------------------------------------------------------- activations
ACT_SETTINGS = {
    "mish": (0, 1.0, 0.0, -INF, INF),
    "swish": (1, 1.0, 0.0, -INF, INF),
    "gelu": (2, 1.0, 0.0, -INF, INF),
    "relu": (3, 1.0, 0.0, 0.0, INF),
    "hard_sigmoid": (3, 0.2, 0.5, 0.0, 1.0),
    "hard_tanh": (3, 1.0, 0.0, -1.0, 1.0),
}


def act_edges(setting):
    """x where slope * x + offset meets a finite clip bound."""
    op, slope, offset, lo, hi = setting
    return [(v - offset) / slope for v in (lo, hi) if op == 3 and math.isfinite(v)]


def act_inputs(n, setting, dtype):
    """+-100, 0 and the setting's clip boundaries, then a sweep of [-30, 30];
    the single point of n = 1 is the exact 0."""
    special = [0.0, -100.0, 100.0] + act_edges(setting)
    sweep = torch.linspace(-30, 30, max(n - len(special), 2))
    x = torch.cat([torch.tensor(special), sweep])[:n]
    return x.to(dtype).to(DEV), len(special)


def act_check(tag, x, dY, setting, dtype, n_special):
    y = _srx_hip.act_fwd(x, *setting)
    dx = _srx_hip.act_bwd(dY, x, *setting)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all(), tag
    ry = ref64.act64(x, *setting)
    rdx = dY.double() * ref64.act_grad64(x, *setting)
    parity("act_fwd " + tag, y, tref.act_forward(x, *setting), ry, dtype)
    parity("act_bwd " + tag, dx, tref.act_backward(dY, x, *setting), rdx, dtype)
    if setting[0] == 3:
        k = min(n_special, x.numel())
        # the special points and their images are representable: exact
        assert torch.equal(y[:k], ry[:k].to(dtype)), tag
        edge = torch.tensor(act_edges(setting)).to(dtype).to(DEV)
        if edge.numel():
            one = torch.ones_like(edge)
            assert not _srx_hip.act_bwd(one, edge, *setting).any(), tag


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", sorted(ACT_SETTINGS))
def test_activation_edges(name, dtype):
    setting = ACT_SETTINGS[name]
    for n in (1, 7, 4096, 4099):
        x, n_special = act_inputs(n, setting, dtype)
        dY = randn((n,), dtype, 50)
        tag = "%s %s n=%d" % (name, dt_id(dtype), n)
        act_check(tag, x, dY, setting, dtype, n_special)
    xg = x.clone().requires_grad_(True)
    getattr(api, name)(xg).backward(dY)
    assert torch.equal(xg.grad, _srx_hip.act_bwd(dY, x, *setting))


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("name", ["mish", "hard_sigmoid"])
def test_activation_past_the_grid_cap(name, dtype):
    """Chunks of kVec elements: twice the capped grid's threads."""
    setting = ACT_SETTINGS[name]
    n = (2 * caps()["threads"] + 1) * kvec(dtype)
    x0, n_special = act_inputs(1 << 16, setting, dtype)
    x = x0.repeat(n // x0.numel() + 1)[:n].contiguous()
    dY = randn((1 << 16,), dtype, 51).repeat(n // x0.numel() + 1)[:n].contiguous()
    act_check("%s %s n=%d" % (name, dt_id(dtype), n), x, dY, setting, dtype, n_special)


# ------------------------------------------------------------------ adam
LR, B1, B2, ADAM_EPS, CLIP = 0.01, 0.9, 0.999, 1e-8, 0.5


def torch_adam(grad, master, m, v, wd, bc1, bc2):
    """The step in stock fp32 torch ops."""
    g = grad.float() * CLIP
    p = master * (1.0 - LR * wd)
    m = B1 * m + (1.0 - B1) * g
    v = B2 * v + (1.0 - B2) * g * g
    p = p - (LR / bc1) * (m / (torch.sqrt(v / bc2) + ADAM_EPS))
    return p, m, v


def adam_check(n, wd, dtype, steps):
    """``steps`` consecutive steps from a state as after three earlier ones."""
    master = randn((n,), torch.float32, 60)
    m = randn((n,), torch.float32, 61, 0.1)
    v = (torch.rand(n, generator=gen(62)) * 0.01).to(DEV)
    clip = torch.tensor([CLIP], device=DEV)
    param = torch.zeros(n, dtype=dtype, device=DEV)
    base = (master.clone(), m.clone(), v.clone())
    want = tuple(t.double() for t in base)
    for step in range(4, 4 + steps):
        grad = randn((n,), dtype, 62 + step)
        bc1, bc2 = 1 - B1 ** step, 1 - B2 ** step
        _srx_hip.adam_step(grad, master, m, v, param, clip, LR, B1, B2, ADAM_EPS,
                           wd, bc1, bc2)
        base = torch_adam(grad, *base, wd, bc1, bc2)
        want = ref64.adam_step64(grad, *want, CLIP, LR, B1, B2, ADAM_EPS, wd, bc1, bc2)
        tag = " adam %s n=%d wd=%g step=%d" % (dt_id(dtype), n, wd, step)
        for name, got, bs, rf in zip(("master", "m", "v"), (master, m, v), base, want):
            parity(name + tag, got, bs, rf, torch.float32)
        assert torch.equal(param, master.to(dtype)), tag


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 10_001])
def test_adam_three_steps(n, wd, dtype):
    adam_check(n, wd, dtype, 3)


@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
def test_adam_past_the_grid_cap(dtype):
    """adam_step sizes its grid for several elements per thread: one element
    more than the capped grid covers at that rate, so the grid is capped and
    every thread loops at least that many times."""
    c = caps()
    adam_check(c["threads"] * c["adam_per_thread"] + 1, 0.01, dtype, 1)


# --------------------------------------------------------------- dropout
@need_gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=dt_id)
@pytest.mark.parametrize("n", [1, 3, 5, 4099])
def test_dropout_mask_edges(n, dtype):
    like = torch.empty(n, dtype=dtype, device=DEV)
    assert torch.equal(_srx_hip.dropout_mask(like, 0.0, 11, 3), torch.ones_like(like))
    for p in (0.5, 0.3):
        m1 = _srx_hip.dropout_mask(like, p, 11, 3)
        assert torch.equal(m1, _srx_hip.dropout_mask(like, p, 11, 3))
        # 1 / (1 - p) as the kernel's fp32 arithmetic gives it
        keep = torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32)
        scale = (torch.tensor(1.0) / keep).to(dtype).to(DEV)
        assert bool(((m1 == 0) | (m1 == scale)).all()), (n, p)
        if n == 4099:
            assert 0 < int((m1 == 0).sum()) < n
            assert not torch.equal(m1, _srx_hip.dropout_mask(like, p, 11, 4))
