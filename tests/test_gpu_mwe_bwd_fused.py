"""Fused MWE backward (mwe_bwd_fused = mwe_bwd_stage1 + mwe_bwd_dx in one
kernel) against float64.

Inputs are built the way test_gpu_mwe._stage1_inputs does: Mout / mu / rstd /
which from ref64.mwe_ref64, a random dY.  dPre and dX go through
ref64.check_parity with the two existing kernels as the baseline (factor 2);
the fp32 column sums are held to the stage-1 bound 1e-3 + 1e-3 |sum| with no
allowance for accumulation: they are a two-level fixed-order sum (at most
128 rows per thread group and tile, then the tiles in order in fp64), so
their rounding error is of order sqrt(rows) * 2^-24 * |partial sum| ~ 1e-4
at the largest size used here."""
import functools

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
FACTOR_BWD = 2
FP32_TOL = dict(atol=1e-3, rtol=1e-3)  # the layernorm-backward fp32 tolerance

LAYOUTS = dict(ref64.MWE_GEOMETRIES)
LAYOUTS.update({
    "T64": [64],                     # a single 64-row tail tile
    "T192": [192],                   # 128 + 64 rows
    "edges64": [64, 64, 64],
    "edge128": [128, 64],            # doc boundary exactly on a tile edge
    "span128": [100, 92],            # a doc spanning the edge
    "singles128": [1] * 128 + [64],  # one-token docs
    "tiles129": [64] * 257,          # T = 16448: 128 full tiles + a 64-row tail
})


@functools.lru_cache(maxsize=4)
def _inputs(W, layout):
    lengths = LAYOUTS[layout]
    X, Wt, bias, g, b, lens, mask = (
        t.to(DEV) for t in ref64.mwe_inputs(W, lengths, True, seed=11))
    _, rM, rwhich, rmu, rrstd, _ = ref64.mwe_ref64(X, Wt, bias, g, b, lens, 1e-5)
    T = int(sum(lengths))
    gen = torch.Generator().manual_seed(12)
    dY = torch.randn(T, W, generator=gen).to(torch.bfloat16).to(DEV)
    return (dY, mask, rM.to(torch.bfloat16), g, rmu.float(), rrstd.float(),
            rwhich.to(torch.uint8), Wt, lens)


def _ref64_dx(dPre64, weight, dY, lengths):
    T, W = dY.shape
    dX3 = dPre64 @ weight.double()
    Xv = torch.zeros(T, W, dtype=torch.float64, device=dY.device,
                     requires_grad=True)
    ref64.seq2col64(Xv, lengths).backward(dX3)
    return dY.double() + Xv.grad


def _run(W, layout, with_mask):
    """(fused outputs, baseline dPre, baseline dX, float64 references)."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    dY, mask, Mout, g, mu, rstd, which, weight, lens = _inputs(W, layout)
    if not with_mask:
        mask = None
    T = dY.shape[0]
    starts, ends = boundary_masks_u8(lens, T)
    out = _srx_hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, weight,
                                 starts, ends)
    base_dPre = _srx_hip.mwe_bwd_stage1(dY, mask, Mout, g, mu, rstd, which)[0]
    base_dX = _srx_hip.mwe_bwd_dx(base_dPre, weight, starts, ends, dY)
    rdPre, rdg, rdb, rdbias, _ = ref64.mwe_stage1_ref64(
        dY, mask, Mout, g, mu, rstd, which)
    rdX = _ref64_dx(rdPre, weight, dY, lens)
    return out, base_dPre, base_dX, (rdPre, rdX, rdg, rdb, rdbias)


def _check_outputs(tag, W, layout, out, base_dPre, base_dX, refs, valid=None):
    dPre, dX, dg32, db32, dbias32 = out
    rdPre, rdX, rdg, rdb, rdbias = refs
    which = _inputs(W, layout)[6]
    T = which.shape[0]
    assert dPre.shape == (T, 3 * W) and dPre.dtype == torch.bfloat16
    assert dX.shape == (T, W) and dX.dtype == torch.bfloat16
    # exact zeros in the two non-argmax pieces
    onehot = torch.zeros(T, 3, W, dtype=torch.bool, device=DEV)
    onehot.scatter_(1, which.long()[:, None, :], True)
    assert float(dPre.view(T, 3, W)[~onehot].float().abs().max()) == 0.0
    ref64.check_parity("fused dPre " + tag, dPre, base_dPre, rdPre, valid,
                       FACTOR_BWD)
    ref64.check_parity("fused dX " + tag, dX, base_dX, rdX, valid, FACTOR_BWD)
    _check_sums(tag, (dg32, db32, dbias32), (rdg, rdb, rdbias), W)


def _check_sums(tag, got3, ref3, W):
    for name, got, ref, n in zip(("dg", "db", "dbias"), got3, ref3,
                                 (W, W, 3 * W)):
        assert got.dtype == torch.float32 and got.shape == (n,)
        err = (got.double() - ref).abs()
        bound = FP32_TOL["atol"] + FP32_TOL["rtol"] * ref.abs()
        print("fused %s %s max err %.3e  worst err/bound %.3f" % (
            tag, name, float(err.max()), float((err / bound).max())))
        assert bool((err <= bound).all()), (tag, name, float(err.max()))


PARITY_LAYOUTS = sorted(k for k in LAYOUTS if k != "tiles129")


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("layout", PARITY_LAYOUTS)
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_bwd_fused_matches_ref64(W, layout, with_mask):
    out, base_dPre, base_dX, refs = _run(W, layout, with_mask)
    tag = "W=%d %s mask=%d" % (W, layout, with_mask)
    _check_outputs(tag, W, layout, out, base_dPre, base_dX, refs)


@need_gpu
def test_mwe_bwd_fused_many_tiles_halo_not_counted():
    """T = 16448: 129 per-tile partial rows (two reduction levels) and a
    64-row tail tile.  A halo row counted into the sums would be an error of
    order one in db.  dPre and dX are also checked on the last tile alone."""
    W, layout = 96, "tiles129"
    out, base_dPre, base_dX, refs = _run(W, layout, True)
    T = out[1].shape[0]
    assert T == 16448
    _check_outputs("W=96 T=16448 mask=1", W, layout, out, base_dPre, base_dX, refs)
    last = (torch.arange(T, device=DEV) >= T - 64)[:, None]
    ref64.check_parity("fused dPre last tile", out[0], base_dPre, refs[0], last,
                       FACTOR_BWD)
    ref64.check_parity("fused dX last tile", out[1], base_dX, refs[1], last,
                       FACTOR_BWD)


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_bwd_fused_bit_reproducible(W):
    """No atomics anywhere in this path: two calls agree bit for bit."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    dY, mask, Mout, g, mu, rstd, which, weight, lens = _inputs(W, "tiles129")
    starts, ends = boundary_masks_u8(lens, dY.shape[0])
    a = _srx_hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, weight,
                               starts, ends)
    b = _srx_hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, weight,
                               starts, ends)
    assert len(a) == len(b) == 5
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_bwd_fused_single_token_docs_exact(W):
    """Every doc one token long, g = 1, rstd = 1, mu = 0, no mask, and small
    integers arranged so that the LayerNorm step is exact: columns come in
    pairs (2k, 2k+1) with dY = (+a, -a) and Mout = (m, m), so the row sums of
    dY and of dY * Mout are exactly zero, s1 = s2 = 0 and dM == dY.  Then
      dPre == dY scattered to piece `which`,
      dX   == round(dY + dPre @ weight[:, W:2W])  (only section 1 survives),
    with the weight integers / 16: every product and partial sum is exact in
    fp32, so the rounded result is unique and any term from a neighbouring
    row, or any inexact LN step, changes it.  The column sums are sums of
    small integers and are exact too."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    T = 192
    gen = torch.Generator().manual_seed(33)
    a = torch.randint(-8, 9, (T, W // 2), generator=gen)
    m = torch.randint(-4, 5, (T, W // 2), generator=gen)
    dY = torch.stack([a, -a], dim=2).reshape(T, W).to(torch.bfloat16).to(DEV)
    Mout = torch.stack([m, m], dim=2).reshape(T, W).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, 3, (T, W), generator=gen).to(torch.uint8).to(DEV)
    weight = (torch.randint(-8, 9, (3 * W, 3 * W), generator=gen).float()
              / 16).to(torch.bfloat16).to(DEV)
    g = torch.ones(W, dtype=torch.bfloat16, device=DEV)
    mu = torch.zeros(T, dtype=torch.float32, device=DEV)
    rstd = torch.ones(T, dtype=torch.float32, device=DEV)
    lengths = torch.ones(T, dtype=torch.long, device=DEV)
    starts, ends = boundary_masks_u8(lengths, T)
    dPre, dX, dg32, db32, dbias32 = _srx_hip.mwe_bwd_fused(
        dY, None, Mout, g, mu, rstd, which, weight, starts, ends)
    want_dPre = torch.zeros(T, 3, W, dtype=torch.float64, device=DEV)
    want_dPre.scatter_(1, which.long()[:, None, :], dY.double()[:, None, :])
    want_dPre = want_dPre.view(T, 3 * W)
    assert torch.equal(dPre.double(), want_dPre)
    want_dX = (dY.double()
               + want_dPre @ weight.double()[:, W:2 * W]).to(torch.bfloat16)
    assert torch.equal(dX, want_dX)
    assert torch.equal(dg32.double(), (dY.double() * Mout.double()).sum(0))
    assert torch.equal(db32.double(), dY.double().sum(0))
    assert torch.equal(dbias32.double(), want_dPre.sum(0))


@need_gpu
def test_mwe_bwd_fused_guards():
    from spacy_ray_amd import _srx_hip

    def args(T, W, dtype=torch.bfloat16, wshape=None):
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
        f = torch.zeros(T, dtype=torch.float32, device=DEV)
        u8 = torch.zeros(T, dtype=torch.uint8, device=DEV)
        wh = torch.zeros(T, W, dtype=torch.uint8, device=DEV)
        return (z(T, W), None, z(T, W), z(W), f, f, wh,
                z(*(wshape or (3 * W, 3 * W))), u8, u8)

    for bad in (args(64, 64),                          # unsupported W
                args(100, 96),                         # T % 64 != 0
                args(64, 96, torch.float32),           # not bf16
                args(64, 96, wshape=(3 * 96, 96))):    # weight shape
        with pytest.raises(RuntimeError):
            _srx_hip.mwe_bwd_fused(*bad)
    dPre, dX, dg32, db32, dbias32 = _srx_hip.mwe_bwd_fused(*args(0, 96))
    assert dPre.shape == (0, 288) and dPre.dtype == torch.bfloat16
    assert dX.shape == (0, 96) and dX.dtype == torch.bfloat16
    for t, n in ((dg32, 96), (db32, 96), (dbias32, 288)):
        assert t.shape == (n,) and t.dtype == torch.float32
        assert float(t.abs().max()) == 0.0
