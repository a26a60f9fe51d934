"""Fused MWE backward dX (mwe_bwd_dx) against float64:
    dX = dY + seq2col-backward(dPre @ weight)
under ref64.check_parity with the composed path itself as the baseline
(bf16 ``dPre.mm(weight)`` then ``seq2col_bwd(..., dY)``, factor 2).  The
fused kernel rounds once where the baseline rounds twice; measured ratios
are in docs/KERNELS.md, "Parity margins"."""
import functools

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
FACTOR_BWD = 2

LAYOUTS = dict(ref64.MWE_GEOMETRIES)
LAYOUTS.update({
    "T64": [64],
    "T192": [192],
    "edges64": [64, 64, 64],
    "edge128": [128, 64],
    "span128": [100, 92],
    "singles128": [1] * 128 + [64],
})


@functools.lru_cache(maxsize=None)
def _inputs(W, layout):
    """Dense random bf16 dPre (every piece column live, so a term leaking
    across a doc boundary shows), weight from ref64.mwe_inputs, random dY."""
    lengths = LAYOUTS[layout]
    _, Wt, _, _, _, lens, _ = ref64.mwe_inputs(W, lengths, False, seed=31)
    T = int(sum(lengths))
    gen = torch.Generator().manual_seed(32)
    dPre = torch.randn(T, 3 * W, generator=gen).to(torch.bfloat16)
    dY = torch.randn(T, W, generator=gen).to(torch.bfloat16)
    return dPre.to(DEV), Wt.to(DEV), dY.to(DEV), lens.to(DEV)


def _ref64_dx(dPre, weight, dY, lengths):
    T, W = dY.shape
    dX3 = dPre.double() @ weight.double()
    Xv = torch.zeros(T, W, dtype=torch.float64, device=dY.device,
                     requires_grad=True)
    ref64.seq2col64(Xv, lengths).backward(dX3)
    return dY.double() + Xv.grad


@need_gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_bwd_dx_matches_ref64(W, layout):
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    dPre, weight, dY, lengths = _inputs(W, layout)
    T = dY.shape[0]
    starts, ends = boundary_masks_u8(lengths, T)
    dX = _srx_hip.mwe_bwd_dx(dPre, weight, starts, ends, dY)
    assert dX.shape == (T, W) and dX.dtype == torch.bfloat16
    ref = _ref64_dx(dPre, weight, dY, lengths)
    base = _srx_hip.seq2col_bwd(dPre.mm(weight).contiguous(), starts, ends, dY)
    ref64.check_parity("mwe_bwd_dx W=%d %s" % (W, layout), dX, base, ref,
                       None, FACTOR_BWD)


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
def test_mwe_bwd_dx_single_token_docs_exact(W):
    """dY = 0 and every doc one token long: only the section-1 term may
    contribute, dX == round(dPre @ weight[:, W:2W]).  The operands are
    small dyadic values (integers, and integers / 16), so every product and
    partial sum is exact in fp32 and the rounded result is unique: any term
    from a neighbouring row changes it."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    T = 192
    gen = torch.Generator().manual_seed(33)
    dPre = torch.randint(-8, 9, (T, 3 * W), generator=gen).to(torch.bfloat16).to(DEV)
    weight = (torch.randint(-8, 9, (3 * W, 3 * W), generator=gen).float()
              / 16).to(torch.bfloat16).to(DEV)
    dY = torch.zeros(T, W, dtype=torch.bfloat16, device=DEV)
    lengths = torch.ones(T, dtype=torch.long, device=DEV)
    starts, ends = boundary_masks_u8(lengths, T)
    dX = _srx_hip.mwe_bwd_dx(dPre, weight, starts, ends, dY)
    want = (dPre.double() @ weight.double()[:, W:2 * W]).to(torch.bfloat16)
    assert torch.equal(dX, want)


@need_gpu
def test_mwe_bwd_dx_guards():
    from spacy_ray_amd import _srx_hip

    def args(T, W, dtype=torch.bfloat16, wshape=None):
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)  # noqa: E731
        u8 = torch.zeros(T, dtype=torch.uint8, device=DEV)
        return (z(T, 3 * W), z(*(wshape or (3 * W, 3 * W))), u8, u8, z(T, W))

    for bad in (args(64, 64),                          # unsupported W
                args(100, 96),                         # T % 64 != 0
                args(64, 96, torch.float32),           # not bf16
                args(64, 96, wshape=(3 * 96, 96))):    # weight shape
        with pytest.raises(RuntimeError):
            _srx_hip.mwe_bwd_dx(*bad)
    out = _srx_hip.mwe_bwd_dx(*args(0, 96))
    assert out.shape == (0, 96) and out.dtype == torch.bfloat16
