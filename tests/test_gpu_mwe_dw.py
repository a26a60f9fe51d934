"""MWE weight gradient without dPre / seq2col / the chunked GEMM
(mwe_bwd_dw, srx_mwe_dw.hip.h) and the compact output of mwe_bwd_fused.

Reference for dW: float64 dPre expanded from (dM, which), float64 seq2col of
X, dPre64^T @ X3_64 — from the same bf16 inputs.  Tolerance: the project's
ratio rule (ref64.check_parity, factor 2): max-abs and RMS error within
2 x baseline + one bf16 ulp at max|ref|, the baseline being
``dPre.t().mm(X3)`` in stock bf16 torch ops on the expanded inputs."""
import functools

import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
DEV = "cuda:0"
W = 96
FACTOR = 2

LAYOUTS = {
    "T64": [64],              # one half-filled tile
    "T192": [192],            # 128 + a 64-row tail, boundary-free inside
    "edge128": [128, 64],     # doc boundary exactly at rows 127 / 128
    "span": [100, 92],        # boundary inside a tile, docs across the edge
    "long": [448],            # one doc spanning several tiles
    "mixed": [30, 2, 1, 95, 1, 127],
}


def _expand(dM, which):
    T, w = dM.shape
    out = torch.zeros(T, 3, w, dtype=dM.dtype, device=dM.device)
    out.scatter_(1, which.long()[:, None, :], dM[:, None, :])
    return out.view(T, 3 * w)


@functools.lru_cache(maxsize=8)
def _case(layout):
    """(dM, which, X, lens, starts, ends, ref64 dW, bf16 baseline dW)."""
    from spacy_ray_amd.ops.api import boundary_masks_u8

    lengths = LAYOUTS[layout]
    T = int(sum(lengths))
    gen = torch.Generator().manual_seed(41 + T)
    dM = torch.randn(T, W, generator=gen).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, 3, (T, W), generator=gen).to(torch.uint8).to(DEV)
    X = (torch.randn(T, W, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    lens = torch.tensor(lengths, device=DEV)
    starts, ends = boundary_masks_u8(lens, T)
    ref, base = _refs(dM, which, X, lens)
    return dM, which, X, lens, starts, ends, ref, base


def _refs(dM, which, X, lens):
    dPre = _expand(dM, which)
    ref = dPre.double().t() @ ref64.seq2col64(X.double(), lens)
    X3 = ref64.seq2col64(X, lens)  # bf16: shifts and zeros only, exact
    base = dPre.t().mm(X3)
    return ref, base


@need_gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_mwe_bwd_dw_matches_ref64(layout):
    from spacy_ray_amd import _srx_hip

    dM, which, X, lens, starts, ends, ref, base = _case(layout)
    assert set(which.unique().tolist()) == {0, 1, 2}
    dW = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends)
    assert dW.shape == (3 * W, 3 * W) and dW.dtype == torch.bfloat16
    ref64.check_parity("mwe_bwd_dw " + layout, dW, base, ref, None, FACTOR)


@functools.lru_cache(maxsize=1)
def _case640():
    from spacy_ray_amd.ops.api import boundary_masks_u8

    lengths = [70, 58, 200, 1, 183, 128]
    T = 640
    gen = torch.Generator().manual_seed(43)
    dM = torch.randn(T, W, generator=gen).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, 3, (T, W), generator=gen).to(torch.uint8).to(DEV)
    X = (torch.randn(T, W, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    lens = torch.tensor(lengths, device=DEV)
    starts, ends = boundary_masks_u8(lens, T)
    ref, base = _refs(dM, which, X, lens)
    return dM, which, X, starts, ends, ref, base


@need_gpu
def test_mwe_bwd_dw_grid_stride():
    """T = 640 is five tiles.  With the cap at 2 one workgroup takes tiles 0,
    2, 4 and the other 1, 3; with the cap at 5 every tile has its own
    workgroup.  Both must meet the rule against float64, and they may differ
    from each other only by fp32 summation order: each is held to the rule
    with the other as `got`, i.e. the difference is at most the sum of the two
    allowed errors, checked directly below as well."""
    from spacy_ray_amd import _srx_hip

    dM, which, X, starts, ends, ref, base = _case640()
    a = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends, max_groups=2)
    b = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends, max_groups=5)
    ref64.check_parity("mwe_bwd_dw cap=2", a, base, ref, None, FACTOR)
    ref64.check_parity("mwe_bwd_dw cap=5", b, base, ref, None, FACTOR)
    b_max, _, rmax = ref64.errs(base, ref)
    diff = float((a.double() - b.double()).abs().max())
    print("cap 2 vs cap 5: max diff %.3e (bound %.3e)" % (
        diff, FACTOR * b_max + ref64.bf16_ulp(rmax)))
    assert diff <= FACTOR * b_max + ref64.bf16_ulp(rmax)


@need_gpu
def test_mwe_bwd_dw_single_token_docs():
    """Every row is both a doc start and a doc end: sections 0 and 2 are
    dropped everywhere, so those column blocks are exactly zero."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    T = 192
    gen = torch.Generator().manual_seed(44)
    dM = torch.randn(T, W, generator=gen).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, 3, (T, W), generator=gen).to(torch.uint8).to(DEV)
    X = (torch.randn(T, W, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    lens = torch.ones(T, dtype=torch.long, device=DEV)
    starts, ends = boundary_masks_u8(lens, T)
    assert bool(starts.all()) and bool(ends.all())
    dW = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends)
    assert float(dW[:, :W].float().abs().max()) == 0.0
    assert float(dW[:, 2 * W:].float().abs().max()) == 0.0
    ref, base = _refs(dM, which, X, lens)
    mid = torch.zeros(3 * W, dtype=torch.bool, device=DEV)
    mid[W:2 * W] = True
    ref64.check_parity("mwe_bwd_dw singles mid", dW, base, ref, mid[None, :],
                       FACTOR)


@need_gpu
def test_mwe_bwd_dw_small_integers_exact():
    """dM and X in {-1, 0, 1} over T = 256 rows: every product is -1, 0 or 1
    and every partial sum an integer of magnitude <= 256, exact in fp32 and in
    bf16, so dW equals the float64 reference exactly.  The operands are
    asymmetric and unrelated: a row/column swap, a shifted section or a
    wrong piece changes the result."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    lengths = [100, 1, 91, 64]
    T = int(sum(lengths))
    assert T == 256
    gen = torch.Generator().manual_seed(45)
    dM = torch.randint(-1, 2, (T, W), generator=gen).to(torch.bfloat16).to(DEV)
    X = torch.randint(-1, 2, (T, W), generator=gen).to(torch.bfloat16).to(DEV)
    which = torch.randint(0, 3, (T, W), generator=gen).to(torch.uint8).to(DEV)
    lens = torch.tensor(lengths, device=DEV)
    starts, ends = boundary_masks_u8(lens, T)
    ref, _ = _refs(dM, which, X, lens)
    for cap in (0, 1):  # one tile per workgroup; both tiles in one workgroup
        dW = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends, max_groups=cap)
        assert torch.equal(dW.double(), ref), cap


@need_gpu
def test_mwe_bwd_dw_bit_reproducible():
    from spacy_ray_amd import _srx_hip

    dM, which, X, starts, ends, _, _ = _case640()
    a = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends, max_groups=2)
    b = _srx_hip.mwe_bwd_dw(dM, which, X, starts, ends, max_groups=2)
    assert torch.equal(a, b)


@need_gpu
@pytest.mark.parametrize("with_mask", [False, True])
@pytest.mark.parametrize("Wc", [96, 128])
def test_mwe_bwd_fused_compact(Wc, with_mask):
    """compact=True stores dM [T, W] = dPre[t, which[t, c] W + c] of the full
    form, bit for bit; dX and the three column sums are bit-identical."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops.api import boundary_masks_u8

    lengths = [100, 92, 1, 63]
    Xi, Wt, bias, g, b, lens, mask = (
        t.to(DEV) if t is not None else None
        for t in ref64.mwe_inputs(Wc, lengths, True, seed=13))
    _, rM, rwhich, rmu, rrstd, _ = ref64.mwe_ref64(Xi, Wt, bias, g, b, lens, 1e-5)
    T = int(sum(lengths))
    gen = torch.Generator().manual_seed(14)
    dY = torch.randn(T, Wc, generator=gen).to(torch.bfloat16).to(DEV)
    args = (dY, mask if with_mask else None, rM.to(torch.bfloat16), g,
            rmu.float(), rrstd.float(), rwhich.to(torch.uint8), Wt,
            *boundary_masks_u8(lens, T))
    full = _srx_hip.mwe_bwd_fused(*args)
    comp = _srx_hip.mwe_bwd_fused(*args, compact=True)
    assert comp[0].shape == (T, Wc) and comp[0].dtype == torch.bfloat16
    want = full[0].view(T, 3, Wc).gather(
        1, rwhich.long()[:, None, :]).squeeze(1)
    assert torch.equal(comp[0].view(torch.int16), want.view(torch.int16))
    for x, y in zip(comp[1:], full[1:]):
        assert x.dtype == y.dtype and torch.equal(x, y)


@need_gpu
def test_mwe_layer_autograd_dw_paths(monkeypatch):
    """ops.mwe_layer under SRX_MWE_DW unset against `composed`, T = 256, two
    docs: dX, dbias, dg, db identical; dW within the rule against float64
    (reference from the dM the kernel path itself stores)."""
    from spacy_ray_amd import _srx_hip
    from spacy_ray_amd.ops import api

    lengths = [150, 106]
    X, Wt, bias, g, b, lens, mask = (
        t.to(DEV) for t in ref64.mwe_inputs(W, lengths, True, seed=15))
    T = 256
    starts, ends = api.boundary_masks_u8(lens, T)
    gen = torch.Generator().manual_seed(16)
    dY = torch.randn(T, W, generator=gen).to(torch.bfloat16).to(DEV)

    def grads():
        leaves = [t.clone().requires_grad_(True) for t in (X, Wt, bias, g, b)]
        Y = api.mwe_layer(*leaves, starts, ends, mask)
        Y.backward(dY)
        return [t.grad for t in leaves], leaves

    monkeypatch.delenv("SRX_MWE_DW", raising=False)
    new, _ = grads()
    monkeypatch.setenv("SRX_MWE_DW", "composed")
    old, _ = grads()
    for i in (0, 2, 3, 4):  # dX, dbias, dg, db
        assert torch.equal(new[i], old[i]), i
    # float64 dW from the stored forward state and the compact dM
    Yf, Mout, which, mu, rstd = _srx_hip.mwe_layer_fwd(
        X, Wt, bias, g, b, starts, ends, mask, 1e-5)
    dM = _srx_hip.mwe_bwd_fused(dY, mask, Mout, g, mu, rstd, which, Wt, starts,
                                ends, compact=True)[0]
    ref, base = _refs(dM, which, X, lens)
    ref64.check_parity("mwe_layer dW new", new[1], base, ref, None, FACTOR)
    ref64.check_parity("mwe_layer dW composed", old[1], base, ref, None, FACTOR)
    monkeypatch.setenv("SRX_MWE_DW", "bogus")
    with pytest.raises(ValueError):
        api.mwe_dw_available(W)


@need_gpu
def test_mwe_bwd_dw_guards():
    from spacy_ray_amd import _srx_hip

    def args(T, w, dtype=torch.bfloat16, dev=DEV, tx=None):
        z = lambda *s: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        u8 = torch.zeros(T, dtype=torch.uint8, device=dev)
        wh = torch.zeros(T, w, dtype=torch.uint8, device=dev)
        return [z(T, w), wh, z(tx or T, w), u8, u8]

    noncontig = args(64, 96)
    noncontig[0] = torch.zeros(64, 192, dtype=torch.bfloat16, device=DEV)[:, ::2]
    short_ends = args(64, 96)
    short_ends[4] = short_ends[4][:32]
    for bad in (args(64, 96, torch.float32),    # not bf16
                noncontig,                      # non-contiguous dM
                args(100, 96),                  # T % 64 != 0
                args(64, 128),                  # unsupported W
                args(64, 96, tx=128),           # X rows != dM rows
                short_ends,                     # ends too short
                args(64, 96, dev="cpu")):       # CPU tensors
        with pytest.raises(RuntimeError):
            _srx_hip.mwe_bwd_dw(*bad)
    dW = _srx_hip.mwe_bwd_dw(*args(0, 96))
    assert dW.shape == (288, 288) and float(dW.float().abs().max()) == 0.0
