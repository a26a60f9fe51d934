"""The W = 256 MWE kernels (srx_mwe_wide.hip.h) against float64: forward
geometry, the fused backward called directly, autograd through
ops.mwe_layer, and the encoder's routing.  Same rules as test_gpu_mwe.py /
test_gpu_mwe_bwd_fused.py: ref64.check_parity with factor 2 (as many
roundings as the bf16 baseline), fixed-order fp32 column sums within
1e-3 + 1e-3 |sum|.  The forward tile is 64 rows, the backward tile 128."""
import functools

import pytest
import torch

import ref64
from test_gpu_mwe import _composed_bf16

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
W = 256
FACTOR = 2

LAYOUTS = dict(ref64.MWE_GEOMETRIES)
LAYOUTS.update({
    "edge128": [128, 64],   # doc boundary exactly on a 128-row tile edge
    "span128": [100, 92],   # a doc spanning the edge
    "T192": [192],          # 128 + a partial last tile of 64 rows
})


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_mwe_wide_forward_geometry(layout, with_mask):
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    X, Wt, bias, g, b, lengths, mask = (
        t.to(DEV) if t is not None else None
        for t in ref64.mwe_inputs(W, LAYOUTS[layout], with_mask))
    starts, ends = boundary_masks_u8(lengths, X.shape[0])
    Y, Mout, which, mu, rstd = _srx_hip.mwe_layer_fwd(
        X, Wt, bias, g, b, starts, ends, mask, 1e-5)
    rY, rM, rwhich, rmu, rrstd, pre = ref64.mwe_ref64(
        X, Wt, bias, g, b, lengths, 1e-5, mask)
    bY, bM = _composed_bf16(X, Wt, bias, g, b, lengths, 1e-5, mask)
    tag = "W=256 %s mask=%d" % (layout, with_mask)
    ref64.check_parity("wide Mout " + tag, Mout, bM, rM, None, FACTOR)
    ref64.check_parity("wide Y " + tag, Y, bY, rY, None, FACTOR)
    # fp32 single-pass variance: relative error ~ W * 2^-24 * (1 + mu^2/var)
    assert float((rmu ** 2 / rM.var(-1, unbiased=False)).max()) <= 10.0
    e_mu = float(((mu.double() - rmu).abs() / rmu.abs()).max())
    e_rstd = float(((rstd.double() - rrstd).abs() / rrstd).max())
    print("wide %s rel err mu %.3e rstd %.3e" % (tag, e_mu, e_rstd))
    assert e_mu <= 1e-4 and e_rstd <= 1e-4
    # argmax: exact where the float64 top-two gap is clear, else either
    near = ref64.top2_gap(pre) <= 1e-4
    assert float(near.double().mean()) < 0.01
    top2 = pre.topk(2, dim=1).indices
    got = which.long()
    assert torch.equal(got[~near], rwhich[~near])
    assert bool(((got == top2[:, 0]) | (got == top2[:, 1])).all())


@functools.lru_cache(maxsize=2)
def _bwd_inputs(layout):
    """As test_gpu_mwe_bwd_fused._inputs: saved tensors from the reference."""
    lengths = LAYOUTS[layout]
    X, Wt, bias, g, b, lens, mask = (
        t.to(DEV) for t in ref64.mwe_inputs(W, lengths, True, seed=11))
    _, rM, rwhich, rmu, rrstd, _ = ref64.mwe_ref64(X, Wt, bias, g, b, lens, 1e-5)
    gen = torch.Generator().manual_seed(12)
    dY = torch.randn(int(sum(lengths)), W, generator=gen).to(torch.bfloat16).to(DEV)
    return (dY, mask, rM.to(torch.bfloat16), g, rmu.float(), rrstd.float(),
            rwhich.to(torch.uint8), Wt, lens)


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_mwe_wide_bwd_fused_matches_ref64(layout, with_mask):
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    dY, mask, Mout, g, mu, rstd, which, weight, lens = _bwd_inputs(layout)
    if not with_mask:
        mask = None
    T = dY.shape[0]
    starts, ends = boundary_masks_u8(lens, T)
    dPre, dX, dg32, db32, dbias32 = _srx_hip.mwe_bwd_fused(
        dY, mask, Mout, g, mu, rstd, which, weight, starts, ends)
    base_dPre = _srx_hip.mwe_bwd_stage1(dY, mask, Mout, g, mu, rstd, which)[0]
    base_dX = _srx_hip.seq2col_bwd(base_dPre.mm(weight), starts, ends, dY)
    rdPre, rdg, rdb, rdbias, _ = ref64.mwe_stage1_ref64(
        dY, mask, Mout, g, mu, rstd, which)
    Xv = torch.zeros(T, W, dtype=torch.float64, device=DEV, requires_grad=True)
    ref64.seq2col64(Xv, lens).backward(rdPre @ weight.double())
    rdX = dY.double() + Xv.grad

    tag = "W=256 %s mask=%d" % (layout, with_mask)
    assert dPre.shape == (T, 3 * W) and dPre.dtype == torch.bfloat16
    assert dX.shape == (T, W) and dX.dtype == torch.bfloat16
    onehot = torch.zeros(T, 3, W, dtype=torch.bool, device=DEV)
    onehot.scatter_(1, which.long()[:, None, :], True)
    assert float(dPre.view(T, 3, W)[~onehot].float().abs().max()) == 0.0
    ref64.check_parity("wide dPre " + tag, dPre, base_dPre, rdPre, None, FACTOR)
    ref64.check_parity("wide dX " + tag, dX, base_dX, rdX, None, FACTOR)
    for name, got, ref, n in (("dg", dg32, rdg, W), ("db", db32, rdb, W),
                              ("dbias", dbias32, rdbias, 3 * W)):
        assert got.dtype == torch.float32 and got.shape == (n,)
        err = (got.double() - ref).abs()
        bound = 1e-3 + 1e-3 * ref.abs()
        print("wide %s %s max err %.3e  worst err/bound %.3f" % (
            tag, name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (tag, name, float(err.max()))


@need_gpu
def test_mwe_wide_layer_grads_match_ref64():
    """The scheme of test_mwe_layer_grads_match_ref64 at W = 256: dX / dW /
    dbias against the bf16 chain with the maxout pinned to the reference's
    `which`, dg / db against the plain bf16 chain.  Seed 13: the smallest
    float64 top-two gap at this width is 4.04e-5."""
    from spacy_ray_amd.ops.api import boundary_masks_u8, mwe_layer

    X, Wt, bias, g, b, lengths, mask = (t.to(DEV) for t in ref64.mwe_inputs(
        W, ref64.MWE_GRAD_LENGTHS, True, seed=13))
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
    for i, name in enumerate(("dX", "dW", "dbias", "dg", "db")):
        bl = pinned if i < 3 else base
        ref64.check_parity("wide mwe_layer %s" % name, got[i], bl[i], ref[i],
                           None, FACTOR)


@need_gpu
def test_mwe_wide_used_in_encoder():
    """MaxoutWindowEncoder(256) takes the fused kernel and agrees with its
    own composed route.  One block is held to atol = rtol = 6e-2
    (test_mwe_layer_fused_matches_composed); the second block carries the
    first one's difference through a residual block of gain about one, so
    two blocks get twice that."""
    from spacy_ray_amd.models.tok2vec import MaxoutWindowEncoder
    from spacy_ray_amd.ops import api

    torch.manual_seed(5)
    enc = MaxoutWindowEncoder(W, depth=2).to(DEV).to(torch.bfloat16)
    X = torch.randn(128, W, device=DEV, dtype=torch.bfloat16)
    lengths = torch.tensor([64, 64], device=DEV)
    assert api.mwe_layer_available(X, W, 3)
    Y = enc(X, lengths)
    starts, ends = api.boundary_masks_u8(lengths, X.shape[0])
    Yc = X
    for block in enc.blocks:
        Yc = Yc + block(api.seq2col(Yc, lengths, starts, ends))
    assert Y.shape == (128, W) and torch.isfinite(Y.float()).all()
    assert torch.allclose(Y.float(), Yc.float(), atol=0.12, rtol=0.12), (
        (Y.float() - Yc.float()).abs().max())
