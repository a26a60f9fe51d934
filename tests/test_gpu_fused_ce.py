"""Transition CE fused into the GPU state machines (gpu_arceager /
gpu_biluo with fuse_ce=True, srx_gpustate.hip) against the two-kernel path
it replaces: the same entry point with fuse_ce=False followed by
hip.transition_ce on the arenas it returns.

The scorer has no atomics, so both runs take the same trajectory; the
trajectory tensors are compared bit for bit first, then dScores, the loss,
the supervised-row count and the column sums over ALL capacity rows."""
import os

import numpy as np
import pytest
import torch

import ref64

pytestmark = pytest.mark.gpu
need_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

# single-token docs, the 64-bit stack-bitmap boundary and GPU_STATE_MAXLEN
LENS = [1, 2, 3, 5, 20, 63, 64, 65, 127, 128]


def _hip():
    from spacy_ray_amd.ops.api import hip_ext

    hip = hip_ext()
    assert hip is not None
    return hip


def _layout(lens):
    lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    return lens, off, int(lens.sum())


def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def _weights(total, nF, H, A, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    pre = (torch.randn(total + 1, nF, 2 * H, generator=g) * 0.5)
    lowerB = torch.randn(2 * H, generator=g) * 0.5
    upperW = torch.randn(A, H, generator=g) * 0.3
    upperB = torch.randn(A, generator=g) * 0.3
    return [t.to(dtype).cuda().contiguous() for t in (pre, lowerB, upperW, upperB)]


def _parser_gold(lens, off, total, L, rng):
    """Random in-range gold heads (about one in six -1), random labels and
    the gold-children CSR built as ParserPipe._gold_to_device builds it."""
    tok_off = np.repeat(off, lens)
    tok_len = np.repeat(lens, lens)
    heads = (rng.random(total) * tok_len).astype(np.int64)
    heads[rng.random(total) < 1.0 / 6.0] = -1
    labs = rng.integers(0, L, size=total)
    local = np.arange(total, dtype=np.int64) - tok_off
    ok = (heads >= 0) & (heads < tok_len)
    parent = tok_off[ok] + heads[ok]
    order = np.argsort(parent, kind="stable")
    kids = local[ok][order]
    kids_off = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(np.bincount(parent, minlength=total), out=kids_off[1:])
    return heads, labs, kids_off, kids


def _check_ce(dtype, ref_outs, fused_outs, n_traj, cap, A, used_rows):
    """ref_outs / fused_outs: the entry point's tuples; n_traj = number of
    leading tensors after the three CE slots that must be bit-equal."""
    hip = _hip()
    scores, gold, valid = ref_outs[0], ref_outs[1], ref_outs[2]
    # same trajectory, or nothing below means anything
    for k in range(3, 3 + n_traj):
        assert torch.equal(ref_outs[k], fused_outs[k]), k
    ref_lc, ref_d, ref_colsum = hip.transition_ce(scores, gold, valid)
    d, lc, colsum = fused_outs[0], fused_outs[-2], fused_outs[-1]
    assert d.shape == (cap, A) and d.dtype == dtype
    assert tuple(fused_outs[1].shape) == (0, A)
    assert tuple(fused_outs[2].shape) == (0, A)
    assert lc.shape == (2,) and lc.dtype == torch.float32
    assert colsum.shape == (A,) and colsum.dtype == torch.float32
    # unused capacity rows stay exactly zero
    unused = torch.ones(cap, dtype=torch.bool, device="cuda")
    unused[used_rows] = False
    assert int(unused.sum()) > 0
    assert not d[unused].any()
    # dScores over every capacity row
    df, rf = d.float(), ref_d.float()
    err = (df - rf).abs()
    print("max |dScores - ref| = %.3e, differing entries = %d, loss %.6f vs "
          "%.6f, count %d vs %d, max |colsum - ref| = %.3e"
          % (float(err.max()), int((df != rf).sum()), float(lc[0]),
             float(ref_lc[0]), int(lc[1]), int(ref_lc[1]),
             float((colsum - ref_colsum).abs().max())))
    if dtype == torch.float32:
        assert float(err.max()) <= 1e-5
    else:
        bad = (df != rf).nonzero(as_tuple=False).cpu().tolist()
        for r, c in bad:
            ulp = ref64.bf16_ulp(float(rf[r, c]))
            assert abs(float(df[r, c]) - float(rf[r, c])) <= ulp, (r, c)
    assert float(lc[1]) == float(ref_lc[1])
    assert torch.allclose(lc[0], ref_lc[0], rtol=1e-3, atol=1e-3)
    assert torch.allclose(colsum, ref_colsum, rtol=1e-3, atol=1e-3)
    return ref_lc


@need_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("H", [64, 32])
@pytest.mark.parametrize("L", [3, 40, 70])
def test_arceager_fused_ce_matches_transition_ce(L, H, dtype):
    hip = _hip()
    lens, off, total = _layout(LENS)
    A = 2 + 2 * L  # 8, 82, 142: one, two, three 64-column chunks
    rng = np.random.default_rng(100 + L)
    heads, labs, kids_off, kids = _parser_gold(lens, off, total, L, rng)
    pre, lowerB, upperW, upperB = _weights(total, 13, H, A, dtype, 7 + L + H)
    args = (pre, _dev(off, np.int32), _dev(lens, np.int32),
            _dev(heads, np.int32), _dev(labs, np.int32),
            _dev(kids_off, np.int32), _dev(kids, np.int32), lowerB, upperW,
            upperB, total, L, True)
    ref = hip.gpu_arceager(*args, fuse_ce=False)
    fused = hip.gpu_arceager(*args, fuse_ce=True)
    assert len(ref) == 9 and len(fused) == 11
    cap = 2 * total
    # rows in use: feats differ from the pad-row fill (slot 3 is the buffer
    # front or s0 on every real step, never both missing)
    used = (ref[3] != total).any(dim=1)
    assert int(used.sum()) == int(ref[8][0])
    ref_lc = _check_ce(dtype, ref, fused, 6, cap, A, used)
    assert float(ref_lc[1]) > 0


@need_gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("NT", [1, 4])
def test_biluo_fused_ce_matches_transition_ce(NT, dtype):
    hip = _hip()
    # the NER arena has one row per token, so unused capacity rows exist
    # only past the last doc: `total` is passed `spare` rows larger
    lens, off, total = _layout(LENS)
    A = 1 + 4 * NT  # 5, 17
    H = 64
    rng = np.random.default_rng(200 + NT)
    gold = rng.integers(0, A, size=total)
    gold[rng.random(total) < 0.2] = -1
    spare = 7  # capacity rows past the last doc: must stay zero
    pre, lowerB, upperW, upperB = _weights(total + spare, 6, H, A, dtype,
                                           11 + NT)
    gold_d = _dev(np.concatenate([gold, np.zeros(spare, np.int64)]), np.int32)
    args = (pre, _dev(off, np.int32), _dev(lens, np.int32), gold_d, lowerB,
            upperW, upperB, total + spare, NT, True)
    ref = hip.gpu_biluo(*args, fuse_ce=False)
    fused = hip.gpu_biluo(*args, fuse_ce=True)
    assert len(ref) == 8 and len(fused) == 10
    cap = total + spare
    used = torch.zeros(cap, dtype=torch.bool, device="cuda")
    used[:total] = True
    # tags past `total` are never written: compare the docs' part
    assert torch.equal(ref[6][:total], fused[6][:total])
    assert torch.equal(ref[7], fused[7])
    ref_lc = _check_ce(dtype, ref, fused, 3, cap, A, used)
    # by construction four in five rows carry supervision
    assert float(ref_lc[1]) >= 0.5 * total
    assert float(ref_lc[1]) < total  # and unsupervised rows do occur


@need_gpu
def test_fused_ce_end_to_end_matches_unfused(monkeypatch):
    """The default (fused) training path against SRX_FUSED_CE=0 on the
    setup of test_gpu_state_machine_parity, with that test's tolerances."""
    from spacy_ray_amd.config.config import Config, resolve
    from spacy_ray_amd.parallel.comm import LocalComm
    from spacy_ray_amd.parallel.engine import ZeRO1Engine
    from spacy_ray_amd.pipeline.language import init_nlp
    from spacy_ray_amd.data.corpus import make_synthetic_docs
    from spacy_ray_amd.vocab.doc import Example

    monkeypatch.setenv("SRX_GPU_STATES", "1")
    cfg = Config.from_disk(os.path.join(os.path.dirname(__file__), "..",
                                        "examples", "configs", "en_core_cnn.cfg"))

    def run(fused):
        monkeypatch.setenv("SRX_FUSED_CE", "1" if fused else "0")
        torch.manual_seed(0)
        np.random.seed(0)
        nlp = init_nlp(cfg, device="cuda:0", sample_size=32)
        T = resolve(cfg.interpolate()["training"], validate=False)
        engine = ZeRO1Engine(nlp, T["optimizer"], LocalComm())
        docs = make_synthetic_docs(nlp.vocab, n_docs=64, words_per_doc=14,
                                   vocab_size=400, n_tags=50, n_deps=40,
                                   n_ent_types=4, seed=13)
        examples = [Example.from_doc(d) for d in docs]
        losses = {}
        engine.accumulate(examples, drop=0.0, losses=losses)
        torch.cuda.synchronize()
        return dict(losses), engine.grad_shard.float().clone()

    losses_ref, grad_ref = run(False)
    losses_new, grad_new = run(True)
    assert "parser" in losses_ref and "ner" in losses_ref
    for k in losses_ref:
        assert abs(losses_new[k] - losses_ref[k]) <= 1e-3 + 0.02 * abs(losses_ref[k]), (
            k, losses_ref[k], losses_new[k])
    denom = grad_ref.abs().mean().clamp(min=1e-8)
    rel = (grad_new - grad_ref).abs().mean() / denom
    assert float(rel) < 0.05, float(rel)
