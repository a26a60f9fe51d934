"""multi_hashembed_fwd and hashembed_bwd_merged (srx_embed_parser.hip.h).

Backward: the reference is a float64 index_add_ of dY.double() into [R, W]
over the 4T (row, token) pairs of the saved rows.  The fp32 accumulator must
lie within the sequential fp32 summation bound n_r * 2^-24 * S of it, element
by element (n_r = contributions to the row, S = float64 sum of the absolute
contributions to the element); a bf16 gradient within that bound plus
2^-8 * |ref|.  Nothing in the bounds is measured.

Forward: X, rows and the sort keys are bit-identical to per-table
hashembed_fwd calls writing the same column blocks.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

U32 = 2.0 ** -24
UBF = 2.0 ** -8
SEED = 11


def _hip():
    from spacy_ray_amd.ops.api import hip_ext

    hip = hip_ext()
    assert hip is not None
    return hip


def _rows_cpu(ids: torch.Tensor, seed: int, R: int) -> torch.Tensor:
    from spacy_ray_amd.ops import torch_ref as ref

    rows = ref.hashembed_rows_cpu(ids.numpy().view(np.uint64), seed, R)
    return torch.from_numpy(np.ascontiguousarray(rows)).to(torch.int32)


def _sort_key(rows: torch.Tensor, R: int) -> torch.Tensor:
    if R * R < 2 ** 31:
        return (rows[:, 0] * R + rows[:, 1]).to(torch.int32)
    return rows[:, 0].contiguous()


def _zipf_ids(T, n_types, gen):
    p = 1.0 / torch.arange(1, n_types + 1, dtype=torch.float64)
    types = torch.randint(-2 ** 62, 2 ** 62, (n_types,), generator=gen)
    return types[torch.multinomial(p / p.sum(), T, replacement=True, generator=gen)]


def _ids(kind, T, gen):
    if kind == "equal":
        return torch.full((T,), 0x1234567, dtype=torch.int64)
    if kind == "distinct":
        return torch.arange(T, dtype=torch.int64) * 0x9E3779B97F4A7C1 + 13
    if kind == "types500":
        types = torch.randint(-2 ** 62, 2 ** 62, (500,), generator=gen)
        return types[torch.randint(0, 500, (T,), generator=gen)]
    if kind == "zipf":
        return _zipf_ids(T, 5000, gen)
    raise AssertionError(kind)


def _reference(dY: torch.Tensor, rows: torch.Tensor, R: int):
    """(ref, bound) in float64 on the CPU: ref [R, W], bound = n_r 2^-24 S."""
    T, W = dY.shape
    dst = rows.reshape(-1).long()
    contrib = dY.double().repeat_interleave(4, dim=0)
    ref = torch.zeros(R, W, dtype=torch.float64).index_add_(0, dst, contrib)
    S = torch.zeros(R, W, dtype=torch.float64).index_add_(0, dst, contrib.abs())
    n_r = torch.bincount(dst, minlength=R).double()
    return ref, n_r[:, None] * U32 * S


def _check_acc(dT32: torch.Tensor, ref, bound, what):
    err = (dT32.double().cpu() - ref).abs()
    worst = (err - bound).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max (err - bound) {worst:.3e}")
    assert (err <= bound).all(), what


def _check_bf16(dT: torch.Tensor, ref, bound, what, factor=1.0):
    err = (dT.double().cpu() - ref).abs()
    lim = factor * (bound + UBF * ref.abs())
    print(f"{what}: bf16 max err {err.max().item():.3e}")
    assert (err <= lim).all(), what


def _run_merged(dY_dev, rows, R):
    """hashembed_bwd_merged on the device view dY_dev; returns dT32."""
    hip = _hip()
    rows_d = rows.cuda()
    order = torch.argsort(_sort_key(rows_d, R))
    assert order.dtype == torch.int64
    dT32 = torch.zeros(R, dY_dev.shape[1], dtype=torch.float32, device="cuda")
    hip.hashembed_bwd_merged(order, rows_d, dY_dev, dT32)
    torch.cuda.synchronize()
    return dT32


# (name, T, R, ids)
BWD_CASES = [
    ("T1", 1, 5000, "distinct"),
    ("T5", 5, 5000, "distinct"),
    ("T129", 129, 5000, "types500"),
    ("T4099_equal", 4099, 2500, "equal"),
    ("T4099_distinct", 4099, 2500, "distinct"),
    ("T5000_R1", 5000, 1, "zipf"),
    ("T5000_R3", 5000, 3, "types500"),
    ("T8192_zipf", 8192, 5000, "zipf"),
]


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
@pytest.mark.parametrize("case", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_bwd_merged_bf16(case, W):
    name, T, R, kind = case
    gen = torch.Generator().manual_seed(1000 * T + W + R)
    rows = _rows_cpu(_ids(kind, T, gen), SEED, R)
    if name == "T5000_R1":
        assert (rows == 0).all()
    if name == "T5000_R3":
        # equal keys with different (r2, r3) must exist for this case to
        # exercise the full-quadruple comparison
        key = _sort_key(rows, R)
        assert len(torch.unique(rows, dim=0)) > len(torch.unique(key))
    dY = (torch.randn(T, W, generator=gen) * 0.1).to(torch.bfloat16)
    ref, bound = _reference(dY, rows, R)
    dT32 = _run_merged(dY.cuda(), rows, R)
    _check_acc(dT32, ref, bound, f"{name} W={W}")
    _check_bf16(dT32.to(torch.bfloat16), ref, bound, f"{name} W={W}")


@need_gpu
def test_bwd_merged_fp32():
    T, R, W = 8192, 5000, 96
    gen = torch.Generator().manual_seed(5)
    rows = _rows_cpu(_ids("zipf", T, gen), SEED, R)
    dY = torch.randn(T, W, generator=gen) * 0.1
    ref, bound = _reference(dY, rows, R)
    _check_acc(_run_merged(dY.cuda(), rows, R), ref, bound, "fp32 dY")


@need_gpu
@pytest.mark.parametrize("W", [96, 128])
@pytest.mark.parametrize("blocks,block", [(4, 1), (5, 3)])
def test_bwd_merged_column_block(blocks, block, W):
    T, R = 1000, 2500
    gen = torch.Generator().manual_seed(77 + blocks + W)
    rows = _rows_cpu(_ids("types500", T, gen), SEED, R)
    dX = (torch.randn(T, blocks * W, generator=gen) * 0.1).to(torch.bfloat16)
    dY = dX[:, block * W:(block + 1) * W]
    ref, bound = _reference(dY, rows, R)
    dT32 = _run_merged(dX.cuda()[:, block * W:(block + 1) * W], rows, R)
    _check_acc(dT32, ref, bound, f"block {block}/{blocks} W={W}")


@need_gpu
def test_bwd_merged_generic_width():
    T, R, W = 1000, 2500, 64
    gen = torch.Generator().manual_seed(64)
    rows = _rows_cpu(_ids("types500", T, gen), SEED, R)
    dY = (torch.randn(T, W, generator=gen) * 0.1).to(torch.bfloat16)
    ref, bound = _reference(dY, rows, R)
    _check_acc(_run_merged(dY.cuda(), rows, R), ref, bound, "W=64")


@need_gpu
@pytest.mark.parametrize("W,dtype", [(200, torch.bfloat16), (1024, torch.bfloat16),
                                     (33, torch.float32)])
def test_bwd_merged_wide_and_odd(W, dtype):
    """The multi-pass (W > 128) and the unpaired (odd W) instantiations."""
    T, R = 300, 50
    gen = torch.Generator().manual_seed(W)
    rows = _rows_cpu(_ids("types500", T, gen), SEED, R)
    dY = (torch.randn(T, W, generator=gen) * 0.1).to(dtype)
    ref, bound = _reference(dY, rows, R)
    _check_acc(_run_merged(dY.cuda(), rows, R), ref, bound, f"W={W}")


# ------------------------------------------------------------ autograd
def _autograd_setup():
    T, W = 4099, 96
    nrows = (5000, 2500, 2500, 7)
    gen = torch.Generator().manual_seed(2024)
    ids4 = torch.stack([_zipf_ids(T, 1500, gen) for _ in nrows], dim=1).contiguous()
    tables = [(torch.randn(R, W, generator=gen) * 0.1).to(torch.bfloat16)
              for R in nrows]
    dX = (torch.randn(T, len(nrows) * W, generator=gen) * 0.1).to(torch.bfloat16)
    seeds = [8, 9, 10, 11]
    refs = []
    for i, R in enumerate(nrows):
        rows = _rows_cpu(ids4[:, i].contiguous(), seeds[i], R)
        refs.append(_reference(dX[:, i * W:(i + 1) * W], rows, R))
    return ids4, seeds, tables, dX, refs


def _autograd_grads(ids4, seeds, tables, dX):
    from spacy_ray_amd.ops.api import multi_hashembed

    params = [t.cuda().requires_grad_(True) for t in tables]
    X = multi_hashembed(ids4.cuda(), seeds, params)
    X.backward(dX.cuda())
    torch.cuda.synchronize()
    return X.detach(), [p.grad for p in params]


def _forbid(monkeypatch, name):
    def boom(*a, **k):
        raise AssertionError(f"{name} must not run in this mode")

    monkeypatch.setattr(_hip(), name, boom)


@need_gpu
def test_autograd_default_against_legacy(monkeypatch):
    ids4, seeds, tables, dX, refs = _autograd_setup()
    monkeypatch.delenv("SRX_DETERMINISTIC", raising=False)
    monkeypatch.delenv("SRX_HASHEMBED", raising=False)
    with monkeypatch.context() as m:
        _forbid(m, "seg_scatter_add")
        _forbid(m, "hashembed_fwd")
        X_new, g_new = _autograd_grads(ids4, seeds, tables, dX)
    monkeypatch.setenv("SRX_HASHEMBED", "legacy")
    with monkeypatch.context() as m:
        _forbid(m, "hashembed_bwd_merged")
        _forbid(m, "multi_hashembed_fwd")
        X_old, g_old = _autograd_grads(ids4, seeds, tables, dX)
    assert torch.equal(X_new.view(torch.int16), X_old.view(torch.int16))
    for i, (ref, bound) in enumerate(refs):
        _check_bf16(g_new[i], ref, bound, f"merged table {i}")
        _check_bf16(g_old[i], ref, bound, f"legacy table {i}")
        diff = (g_new[i].double() - g_old[i].double()).abs().cpu()
        assert (diff <= 2 * (bound + UBF * ref.abs())).all(), f"table {i}"


@need_gpu
def test_autograd_deterministic_is_bit_identical(monkeypatch):
    ids4, seeds, tables, dX, refs = _autograd_setup()
    monkeypatch.delenv("SRX_HASHEMBED", raising=False)
    monkeypatch.setenv("SRX_DETERMINISTIC", "1")
    _forbid(monkeypatch, "hashembed_bwd_merged")
    _, g1 = _autograd_grads(ids4, seeds, tables, dX)
    _, g2 = _autograd_grads(ids4, seeds, tables, dX)
    for i, (a, b) in enumerate(zip(g1, g2)):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"table {i}"
        ref, bound = refs[i]
        # fixed-point sink: one 2^-25 rounding per pushed partial sum on top
        _check_bf16(a, ref, bound + 4 * 4099 * 2.0 ** -25, f"deterministic table {i}")


@need_gpu
def test_single_table_autograd_large_T(monkeypatch):
    """_HashEmbed takes the merged backward at T >= 4096."""
    from spacy_ray_amd.ops.api import hashembed

    monkeypatch.delenv("SRX_DETERMINISTIC", raising=False)
    monkeypatch.delenv("SRX_HASHEMBED", raising=False)
    _forbid(monkeypatch, "seg_scatter_add")
    T, R, W = 4099, 2500, 128
    gen = torch.Generator().manual_seed(9)
    ids = _zipf_ids(T, 1500, gen)
    table = (torch.randn(R, W, generator=gen) * 0.1).to(torch.bfloat16)
    dY = (torch.randn(T, W, generator=gen) * 0.1).to(torch.bfloat16)
    ref, bound = _reference(dY, _rows_cpu(ids, SEED, R), R)
    p = table.cuda().requires_grad_(True)
    hashembed(p, ids.cuda(), SEED).backward(dY.cuda())
    _check_bf16(p.grad, ref, bound, "single table")


# ------------------------------------------------------------- forward
TABLE_SETS = [(5000,), (7,), (50000,), (5000, 2500, 2500, 7)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@need_gpu
@pytest.mark.parametrize("nrows", TABLE_SETS, ids=lambda s: "R" + "_".join(map(str, s)))
@pytest.mark.parametrize("W", [96, 128])
@pytest.mark.parametrize("T", [1, 63, 4099])
def test_multi_fwd_bit_identical(T, W, nrows, dtype=torch.bfloat16):
    hip = _hip()
    n = len(nrows)
    gen = torch.Generator().manual_seed(T + W + sum(nrows))
    ids4 = torch.randint(-2 ** 62, 2 ** 62, (T, n), generator=gen).cuda()
    tables = [torch.randn(R, W, generator=gen).to(dtype).cuda() for R in nrows]
    seeds = list(range(3, 3 + n))
    fill = torch.randn(T, 5 * W, generator=gen).to(dtype).cuda()
    X_new, X_old = fill.clone(), fill.clone()
    rows, keys = hip.multi_hashembed_fwd(ids4, tables, seeds, X_new, 0)
    assert rows.shape == (n, T, 4) and rows.dtype == torch.int32
    assert keys.shape == (n, T) and keys.dtype == torch.int32
    for i, table in enumerate(tables):
        _, rows_i = hip.hashembed_fwd(table, ids4[:, i].contiguous(), seeds[i],
                                      X_old, i * W)
        assert torch.equal(rows[i], rows_i), f"rows of table {i}"
        assert torch.equal(keys[i], _sort_key(rows_i, nrows[i])), f"keys of table {i}"
    torch.cuda.synchronize()
    assert torch.equal(_bits(X_new), _bits(X_old))
    # the blocks past the n tables keep their pre-filled contents
    assert torch.equal(_bits(X_new[:, n * W:]), _bits(fill[:, n * W:]))
    assert not torch.equal(_bits(X_new[:, :n * W]), _bits(fill[:, :n * W]))


@need_gpu
def test_multi_fwd_bit_identical_fp32():
    test_multi_fwd_bit_identical(4099, 96, (5000, 2500, 2500, 7), dtype=torch.float32)
