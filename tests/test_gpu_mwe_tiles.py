"""Fused MWE forward on the layouts its 128-row tiling can get wrong: a
half-filled last tile (T = 64 and T = 192 are 1 and 3 units of 64 rows),
and doc boundaries on and across the 64- and 128-row edges.  Same checks as
test_gpu_mwe.test_mwe_layer_geometry (float64 reference, ref64.check_parity
factor 2 against the composed bf16 baseline).  One workgroup handles one
tile and the grid is not capped, so there is no tile-loop case."""
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
FACTOR_FWD = 2

TILE_LAYOUTS = {
    "T64": [64],
    "T192": [192],
    "edges64": [64, 64, 64],
    "edge128": [128, 64],
    "span": [100, 92],
    "singles128": [1] * 128 + [64],
}


def _composed_bf16(X, Wt, bias, g, b, lengths, eps, mask=None):
    """Baseline: the composed path in stock bf16 torch ops."""
    from spacy_ray_amd.ops import torch_ref as ref

    T, W = X.shape
    pre = ref.seq2col(X, lengths).mm(Wt.t()) + bias
    m = pre.view(T, 3, W).max(dim=1).values
    ln = torch.nn.functional.layer_norm(m, (W,), g, b, eps)
    if mask is not None:
        ln = ln * mask
    return X + ln, m


@need_gpu
@pytest.mark.parametrize("layout", sorted(TILE_LAYOUTS))
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_layer_tile_layouts(W, with_mask, layout):
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    X, Wt, bias, g, b, lengths, mask = [
        t.to(DEV) if t is not None else None
        for t in ref64.mwe_inputs(W, TILE_LAYOUTS[layout], with_mask, seed=5)]
    T = X.shape[0]
    starts, ends = boundary_masks_u8(lengths, T)
    Y, Mout, which, mu, rstd = _srx_hip.mwe_layer_fwd(
        X, Wt, bias, g, b, starts, ends, mask, 1e-5)
    rY, rM, rwhich, rmu, rrstd, pre = ref64.mwe_ref64(
        X, Wt, bias, g, b, lengths, 1e-5, mask)
    bY, bM = _composed_bf16(X, Wt, bias, g, b, lengths, 1e-5, mask)
    tag = "W=%d %s mask=%d" % (W, layout, with_mask)
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
